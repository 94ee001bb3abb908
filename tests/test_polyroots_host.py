"""CPU tests of tests/roots_ref.py (the restatement of ecfft_poly_find_roots' scheme that the GPU tests lean on), against known
answers and against brute-force evaluation at a small prime, and of the entry point's argument checks, which are made before a
device is touched."""
import os

import numpy as np
import pytest

import poly_ref as R
import roots_ref as RR
from conftest import ROOT

P = R.P
M31 = P["m31"]


def brute(f, p):
    return [a for a in range(p) if sum(c * pow(a, i, p) for i, c in enumerate(f)) % p == 0]


def test_finds_roots_of_cubic():
    """finds_roots_of_cubic (src/utils.rs:400-414) on Fp31: x^3 - 4x has the roots 0, 2 and p - 2"""
    roots, attempts = RR.find_roots([0, M31 - 4, 0, 1], M31)
    assert roots == [0, 2, 2147483645] and attempts >= 2


@pytest.mark.parametrize("field", ["m31", "secp256k1"])
def test_degree_36_with_a_double_root_and_rootless_quadratics(field):
    p = P[field]
    assert p % 4 == 3                                      # x^2 + c^2 is irreducible
    rm = [(3 + 7 * i, 2 if i == 0 else 1) for i in range(25)]
    f = RR.product(p, rm, [1, 2, 3, 4, 5], 9)
    assert len(f) - 1 == 36 and f[-1] == 9
    assert RR.linear_part(f, p) == RR.product(p, [(r, 1) for r, _ in rm], [])
    roots, attempts = RR.find_roots(f, p)
    assert roots == sorted(r for r, _ in rm) and 24 <= attempts < 24 + RR.CAP


@pytest.mark.parametrize("p", [103, 107, 131])
def test_against_brute_force_at_a_small_prime(p):
    """every element tried: all, some and no roots, multiplicities, the roots 0, 1, p - 1 .. p - 3 (w = 0 for the first shifts),
    constants and x itself; p = 3 mod 4"""
    assert p % 4 == 3
    cases = [RR.product(p, [(r, 1) for r in (0, 1, p - 1, p - 2, p - 3)], [], 5),
             RR.product(p, [(r, 1 + r % 3) for r in range(2, 40, 3)], [2, 9], 7),
             RR.product(p, [], [1, 2, 3]),
             RR.product(p, [(17, 3)], [4]),
             RR.product(p, [(r, 1) for r in range(p)], []),      # x^p - x: every element
             [5], [0, 1], [3, 1, 0, 0]]
    for f in cases:
        roots, _ = RR.find_roots(f, p)
        assert roots == brute(f, p), f
        assert len(set(roots)) == len(roots)
    assert RR.find_roots([0, 0, 0], p) is None


def test_the_quadratic_whose_first_four_shifts_fail():
    """equal Legendre symbols of r + c and s + c for c = 1 .. 4 put both roots on the same side of the split; c = 5 parts them"""
    assert RR.legendre_pair(M31) == (2, 50)
    for field in ("m31", "secp256k1"):
        p = P[field]
        r, s = RR.legendre_pair(p)
        h = RR.product(p, [(r, 1), (s, 1)], [])
        for c in range(1, 5):
            u, v = RR.split(h, c, p)
            assert len(u) - 1 in (0, 2)
        u, v = RR.split(h, 5, p)
        assert len(u) == 2 and len(v) == 2
        roots, attempts = RR.find_roots(h, p)
        assert roots == [r, s] and attempts == 5


def test_the_root_minus_c_lands_in_v():
    p = M31
    h = RR.product(p, [(p - 1, 1), (10, 1), (11, 1), (12, 1)], [])
    u, v = RR.split(h, 1, p)                               # the root -1: w = 0 there, so it is no root of w - 1
    assert sum(c * pow(p - 1, i, p) for i, c in enumerate(v)) % p == 0


def test_the_symbol_is_exported_and_checks_its_arguments_without_a_gpu():
    import ecfft_amd
    from ecfft_amd import fftree as FT
    ecfft_amd.build.build()
    L = FT.lib()
    assert "ecfft_poly_find_roots" in FT.EXPORTS and hasattr(L, "ecfft_poly_find_roots")
    assert FT.ROOTS_SMALL_MAX == 65
    header = open(os.path.join(ROOT, "include", "ecfft_hip.h")).read()
    assert f"#define ECFFT_ROOTS_SMALL_MAX {FT.ROOTS_SMALL_MAX} " in header
    assert hasattr(FT.FFTree, "poly_find_roots")
    buf = np.zeros(8, np.uint32)
    n = np.zeros(1, np.int64)
    ptr = buf.ctypes.data
    # a NULL context, then zero nf and count (checked before the context is looked at)
    assert L.ecfft_poly_find_roots(None, ptr, 2, ptr, n.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    for nf, count in ((0, 1), (2, 0)):
        assert L.ecfft_poly_find_roots(None, ptr, nf, ptr, n.ctypes.data, count, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert n[0] == 0 and not buf.any()
