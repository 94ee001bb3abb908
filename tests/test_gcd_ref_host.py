"""CPU tests of tests/gcd_ref.py (the exact references the GPU tests of ecfft_poly_gcd / ecfft_poly_xgcd compare with), pinned
against themselves and against known answers, and of the two entry points' argument checks, which are made before a device is
touched."""
import math
import os

import numpy as np
import pytest

import gcd_ref as G
import poly_ref as R
from conftest import ROOT

FIELDS = ["secp256k1", "m31"]
P = R.P


@pytest.mark.parametrize("field", FIELDS)
def test_eea_matches_from_quotients(field):
    """Euclid on a pair built backwards from a quotient sequence returns that pair's gcd and cofactors, abnormal quotients included"""
    for seed, degs, dg in ((1, [1, 1, 1, 1, 1], 0), (2, [3, 1, 2, 5, 1], 2), (3, [0, 2, 1, 7], 3), (4, [4], 1), (5, [1, 9, 1, 1, 2, 1], 0)):
        qs = [G.rand_poly(field, d + 1, 100 * seed + i) for i, d in enumerate(degs)]
        g = G.rand_poly(field, dg + 1, 7 * seed, monic=True)
        r0, r1, s, t = G.from_quotients(field, g, qs)
        assert G.deg(r0) == sum(degs) + dg and G.deg(r1) == sum(degs[1:]) + dg
        assert G.eea(field, r0, r1) == (s, t, g)
        assert G.gcd(field, r0, r1) == g and G.gcd(field, r1, r0) == g
        n0, n1 = len(r0) + 2, len(r1) + 1
        assert G.check_xgcd(field, G.arr(field, r0, n0), G.arr(field, r1, n1), G.arr(field, s, n1), G.arr(field, t, n0), G.arr(field, g, n0)) == ""
        wrong = G.arr(field, [(t[0] + 1) % P[field]] + t[1:], n0)
        assert G.check_xgcd(field, G.arr(field, r0, n0), G.arr(field, r1, n1), G.arr(field, s, n1), wrong, G.arr(field, g, n0)) != ""


def test_reference_crate_xgcd_tests_on_m31():
    """the three xgcd tests of the reference (src/utils.rs:416-456) on Fp31, with seeded operands of the same shapes"""
    f, p = "m31", P["m31"]
    a, b = G.rand_poly(f, 6, 0), G.rand_poly(f, 6, 1)                     # DensePolynomial::rand(5, ..)
    s, t, g = G.eea(f, a, b)
    assert G._add(G.mul(f, a, s), G.mul(f, b, t), p) == g
    a, b = [p - 1, 0, 1], [1, 1, 1]                                        # x^2 - 1 and x^2 + x + 1
    s, t, g = G.eea(f, a, b)
    assert G._add(G.mul(f, a, s), G.mul(f, b, t), p) == g and g == [1]
    s, t, g = G.eea(f, [], b)                                              # xgcd(0, b)
    assert s == [] and G.mul(f, b, t) == g and g and g[-1] == 1
    assert t == [pow(b[-1], p - 2, p)]
    s, t, g = G.eea(f, b, [])                                              # b = 0: s = 1/lc(a), t = 0
    assert s == [pow(b[-1], p - 2, p)] and t == [] and g == G._scale(b, s[0], p)
    assert G.eea(f, [], []) == ([1], [], [])                               # the reference's own value; the GPU call returns zeros here


def test_gcd_steps_of_finds_roots_of_cubic():
    """finds_roots_of_cubic (src/utils.rs:400-414): f = x^3 - 4x splits completely, so gcd(f, x^p - x mod f) = f and the equal-degree
    splits gcd(h^((p-1)/2) - 1, f) divide it"""
    f, p = "m31", P["m31"]
    cubic = [0, p - 4, 0, 1]

    def pow_mod(base, e):
        res, acc = [1], base
        while e:
            if e & 1:
                res = G.divmod_school(G.mul(f, res, acc), cubic, p)[1]
            acc = G.divmod_school(G.mul(f, acc, acc), cubic, p)[1]
            e >>= 1
        return res
    xp = pow_mod([0, 1], p)
    assert G.gcd(f, cubic, G._sub(xp, [0, 1], p)) == cubic
    h = [5, 1]
    w = G._sub(pow_mod(h, (p - 1) // 2), [1], p)
    d = G.gcd(f, w, cubic)
    assert not G.divmod_school(cubic, d, p)[1] if d else True
    roots = [r for r in (0, 2, p - 2) if sum(c * pow(r, i, p) for i, c in enumerate(d)) % p == 0]
    assert len(roots) == G.deg(d)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n,m", [(12, 18), (7, 5), (30, 12), (1, 9)])
def test_gcd_of_cyclotomic_binomials(field, n, m):
    """gcd(x^n - 1, x^m - 1) = x^gcd(n, m) - 1"""
    p = P[field]
    binom = lambda k: [p - 1] + [0] * (k - 1) + [1]
    assert G.gcd(field, binom(n), binom(m)) == binom(math.gcd(n, m))
    s, t, g = G.eea(field, binom(n), binom(m))
    assert g == binom(math.gcd(n, m)) and G._add(G.mul(field, binom(n), s), G.mul(field, binom(m), t), p) == g


def test_both_symbols_are_exported_and_check_their_arguments_without_a_gpu():
    import ecfft_amd
    from ecfft_amd import fftree as FT
    ecfft_amd.build.build()
    L = FT.lib()
    assert "ecfft_poly_gcd" in FT.EXPORTS and "ecfft_poly_xgcd" in FT.EXPORTS
    assert hasattr(L, "ecfft_poly_gcd") and hasattr(L, "ecfft_poly_xgcd")
    assert FT.GCD_SMALL_MAX >= 64
    header = open(os.path.join(ROOT, "include", "ecfft_hip.h")).read()
    assert f"#define ECFFT_GCD_SMALL_MAX {FT.GCD_SMALL_MAX}\n" in header
    buf = np.zeros(8, np.uint32)
    deg = np.zeros(1, np.int64)
    ptr = buf.ctypes.data
    # a NULL context, then zero lengths and count (checked before the context is looked at)
    assert L.ecfft_poly_gcd(None, ptr, 2, ptr, 2, ptr, deg.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_xgcd(None, ptr, 2, ptr, 2, ptr, ptr, ptr, deg.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    for na, nb, count in ((0, 2, 1), (2, 0, 1), (2, 2, 0)):
        assert L.ecfft_poly_gcd(None, ptr, na, ptr, nb, ptr, None, count, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert L.ecfft_poly_xgcd(None, ptr, na, ptr, nb, None, None, ptr, None, count, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert deg[0] == 0 and not buf.any()
