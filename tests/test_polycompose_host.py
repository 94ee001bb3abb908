"""CPU tests of tests/compose_ref.py, the exact reference of tests/test_gpu_polycompose.py, and of what ecfft_poly_compose_mod decides
without a device: the Brent-Kung list model against Horner with long division at small primes, the Barrett Horner against the same
for both fields, the closed form at a linear modulus, the split-modulus identity the large GPU cases rest on, and the export, the
regime constant and the argument checks of the C ABI."""
import os

import numpy as np
import pytest

import compose_ref as C
import poly_ref as R
import powmod_ref as W

FIELDS = ["secp256k1", "m31"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def modulus(field, nm, seed):
    return R.set_nonzero(field, R.rand_std(field, nm, seed), nm - 1)


def eval_int(c, x, p):
    r = 0
    for v in reversed(c):
        r = (r * x + v) % p
    return r


def test_chunking():
    for nf, want in ((1, (1, 1)), (2, (2, 1)), (3, (2, 2)), (4, (2, 2)), (5, (3, 2)), (13, (4, 4)), (16, (4, 4)), (17, (5, 4)), (26, (6, 5)),
                     (100, (10, 10)), (101, (11, 10)), (145, (13, 12))):
        assert C.chunking(nf) == want
        k, kp = want
        assert k * kp >= nf > k * (kp - 1) and (k - 1) ** 2 < nf <= k * k


@pytest.mark.parametrize("p", [7, 97, 65537])
@pytest.mark.parametrize("d", [1, 2, 3, 8, 9, 33])
def test_brent_kung_model_matches_horner(p, d):
    rng = np.random.default_rng(1000 * p + d)
    for nf in (1, 2, 3, 4, 5, 13, 16, 17, 26):
        for ng in (1, max(1, d // 2), d, d + 1, 2 * d + 3):
            h = [int(v) for v in rng.integers(0, p, d)] + [int(rng.integers(1, p))]
            f, g = [int(v) for v in rng.integers(0, p, nf)], [int(v) for v in rng.integers(0, p, ng)]
            stats = {}
            assert C.brent_kung_model(f, g, h, p, stats) == C.horner_long_division(f, g, h, p), (nf, ng)
            k, kp = C.chunking(nf)
            assert stats["products"] == (0 if nf <= 2 else (k - 1) + (kp - 1))
    # zero coefficients in every position of the ragged chunk and a zero g
    h = [int(v) for v in rng.integers(0, p, d)] + [1]
    assert C.brent_kung_model([0] * 5, [3 % p], h, p) == [0] * d
    assert C.brent_kung_model([2, 1, 4, 0, 5], [0], h, p) == [2 % p] + [0] * (d - 1)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d,nf,ng", [(1, 1, 1), (1, 5, 3), (2, 2, 2), (3, 7, 9), (7, 3, 2), (17, 17, 17), (17, 30, 18), (40, 9, 100), (65, 13, 64)])
def test_compose_mod_matches_long_division(field, d, nf, ng):
    p = R.P[field]
    h, f, g = modulus(field, d + 1, 10 * d + nf), R.rand_std(field, nf, 3 * d + nf), R.rand_std(field, ng, 5 * d + ng)
    got = C.compose_mod(field, f, g, h)
    assert got.shape == R.shape(field, d) and R.canonical(field, got).all()
    assert R.to_ints(field, got) == C.horner_long_division(R.to_ints(field, f), R.to_ints(field, g), R.to_ints(field, h), p)


@pytest.mark.parametrize("field", FIELDS)
def test_linear_modulus_is_evaluation(field):
    """h = x - r: f(g) mod h = f(g(r))"""
    p = R.P[field]
    r = R.to_ints(field, R.rand_std(field, 1, 5, specials=False))[0]
    h = R.from_ints(field, [(-r) % p, 1])
    for nf, ng in ((1, 1), (2, 5), (9, 4), (30, 30)):
        f, g = R.rand_std(field, nf, nf), R.rand_std(field, ng, 100 + ng)
        want = eval_int(R.to_ints(field, f), eval_int(R.to_ints(field, g), r, p), p)
        assert R.to_ints(field, C.compose_mod(field, f, g, h)) == [want]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d,nf,ng", [(5, 5, 4), (33, 70, 33), (65, 30, 140)])
def test_split_modulus_identity(field, d, nf, ng):
    """h = prod (x - r_i), the r_i distinct: out = f(g) mod h has out(r_i) = f(g(r_i)) at every root, and fewer than d coefficients"""
    p = R.P[field]
    roots = R.rand_std(field, d, 7 * d, specials=False)
    ri = R.to_ints(field, roots)
    assert len(set(ri)) == d
    h = W.from_roots(field, roots)
    f, g = R.rand_std(field, nf, d + nf), R.rand_std(field, ng, d + ng + 1)
    out = R.to_ints(field, C.compose_mod(field, f, g, h))
    fi, gi = R.to_ints(field, f), R.to_ints(field, g)
    assert len(out) == d
    assert [eval_int(out, r, p) for r in ri] == [eval_int(fi, eval_int(gi, r, p), p) for r in ri]


def test_symbol_is_exported_and_checks_its_arguments_without_a_gpu():
    import ecfft_amd
    from ecfft_amd import fftree as FT
    ecfft_amd.build.build()
    L = FT.lib()
    assert "ecfft_poly_compose_mod" in FT.EXPORTS and hasattr(L, "ecfft_poly_compose_mod")
    header = open(os.path.join(ROOT, "include", "ecfft_hip.h")).read()
    assert f"#define ECFFT_COMPOSE_SMALL_MAX {FT.COMPOSE_SMALL_MAX} " in header
    assert FT.COMPOSE_SMALL_MAX == 65
    assert hasattr(FT.FFTree, "poly_compose_mod")
    buf = np.zeros(8, np.uint32)
    ptr = buf.ctypes.data
    cm = L.ecfft_poly_compose_mod
    # a NULL context; then zero lengths, a modulus without a residue, count = 0 and NULL pointers: all decided before the context
    # is looked at, so before a device is touched
    assert cm(None, ptr, 2, ptr, 2, ptr, 2, ptr, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    for nf, ng, nm, count in ((0, 2, 2, 1), (2, 0, 2, 1), (2, 2, 1, 1), (2, 2, 0, 1), (2, 2, 2, 0)):
        assert cm(None, ptr, nf, ptr, ng, ptr, nm, ptr, count, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    for args in ((None, ptr, ptr, ptr), (ptr, None, ptr, ptr), (ptr, ptr, None, ptr), (ptr, ptr, ptr, None)):
        assert cm(None, args[0], 2, args[1], 2, args[2], 2, args[3], 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert not buf.any()
