"""CPU tests of tests/factor_ref.py, the exact model that tests/test_gpu_polyfactor.py compares ecfft_poly_squarefree_decompose and
ecfft_poly_factor with: the model returns the constructed factors of every spec it can afford, they multiply back to f, the inputs
stay away from the attempt cap, the packing is the C ABI's, and the surface (header macro, exports, Python wrappers) exists.

What the model cannot afford here: L3 over secp256k1 (179 coefficients of 256 bits through schoolbook powers); it is skipped by name
below and its GPU test compares with the construction, which needs no model.

Time: S1, S2, S3, S4, S6 take at most 2 s each; S5 and L2 over secp256k1 take 6 s and 8 s."""
import os

import numpy as np
import pytest

import ddf_ref as D
import edf_ref as E
import factor_ref as FR
import poly_ref as R

P = R.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["secp256k1", "m31"]

SMALL = [(f, name) for f in FIELDS for name in FR.SMALL]
LARGE = [(f, name) for f in ("m31", "secp256k1") for name in FR.LARGE if (f, name) != ("secp256k1", "L3")]


def run_spec(spec, p, k):
    f, want = FR.case(spec, p, k)
    assert len(f) - 1 == FR.degree(spec)
    got, lead, worst = FR.factor(f, p)
    assert got == want and lead == k
    assert FR.multiply_back(got, lead, p) == f
    assert worst < E.CAP // 4, worst                                          # a condition on the inputs: a quarter of the cap
    parts, lead2, iterations = FR.yun(f, p)
    assert parts == FR.parts_of(want, p) and lead2 == k
    assert iterations == max(e for _, _, e in spec)                          # a squarefree input costs one iteration
    return f, want


@pytest.mark.parametrize("field,name", SMALL)
def test_model_equals_the_construction_small(field, name):
    f, want = run_spec(FR.SMALL[name], P[field], 7)
    assert len(f) <= 65


@pytest.mark.parametrize("field,name", LARGE)
def test_model_equals_the_construction_large(field, name):
    spec, leaves = FR.LARGE[name]
    f, want = run_spec(spec, P[field], 5)
    assert len(f) > 65 and leaves // 2 < 2 * len(f) - 1 <= leaves


def test_yun_on_small_primes_and_written_out_inputs():
    """x^9; (x - 0)(x - 1)^2 (x + 1)^3 (x - 5) with two quadratics squared and a cubic: the decomposition collects by multiplicity"""
    for p in (P["m31"], P["secp256k1"], 103):
        assert FR.yun([0] * 9 + [4], p) == ({9: [0, 1]}, 4, 9)
        lin = lambda a: [-a % p, 1]
        quad = D.irreducible_binomials(2, 2, p)
        cub = D.irreducible_binomials(3, 1, p)[0]
        f = D.product([lin(0), lin(5), cub] + [lin(1)] * 2 + quad * 2 + [lin(p - 1)] * 3, p)
        assert len(f) - 1 == 18
        parts, lead, it = FR.yun([3 * v % p for v in f], p)
        assert lead == 3 and it == 3
        assert parts == {1: D.product([lin(0), lin(5), cub], p), 2: D.product([lin(1)] + quad, p), 3: lin(p - 1)}
    assert FR.yun([0, 0], 101) is None and FR.yun([7, 0], 101) == ({}, 7, 0) and FR.factor([0], 101) is None
    assert FR.factor([9], 101) == ([], 9, 0)


def test_packing_is_the_layout_of_the_c_abi():
    p = 101
    q1, q2, q3 = [3, 1], [5, 1], [2, 0, 1]
    want = FR.order([(q3, 1), (q2, 2), (q1, 2), ([7, 1], 1)])
    assert want == [([7, 1], 1), (q3, 1), (q1, 2), (q2, 2)]                   # (e, degree, coefficients)
    row, fdeg, fmult, n = FR.pack_factor(want, 8)
    assert (row, fdeg, fmult, n) == ([7, 2, 0, 3, 5, 0, 0, 0], [1, 2, 1, 1, 0, 0, 0, 0], [1, 1, 2, 2, 0, 0, 0, 0], 4)
    assert FR.unpack_factor(row, fdeg, fmult, n) == want
    assert FR.pack_factor(None, 3) == ([0, 0, 0], [0, 0, 0], [0, 0, 0], -1) and FR.pack_factor([], 1) == ([0], [0], [0], 0)
    parts = {1: D.product([[7, 1], q3], p), 2: D.product([q1, q2], p)}
    prow, pdeg = FR.pack_decompose(parts, 8)
    assert pdeg == [3, 2, 0, 0, 0, 0, 0, 0] and prow == parts[1][:-1] + parts[2][:-1] + [0, 0, 0]
    assert FR.pack_decompose(None, 2) == ([0, 0], [-1, 0]) and FR.pack_decompose({}, 1) == ([0], [0])
    assert FR.pack_decompose({1: [4, 1], 3: [9, 1]}, 4) == ([4, 9, 0, 0], [1, 0, 1, 0])   # a gap at multiplicity 2


def test_symbols_are_exported_and_check_their_arguments_without_a_gpu():
    import ecfft_amd
    from ecfft_amd import fftree as FT
    ecfft_amd.build.build()
    L = FT.lib()
    for sym in ("ecfft_poly_squarefree_decompose", "ecfft_poly_factor"):
        assert sym in FT.EXPORTS and hasattr(L, sym)
    header = open(os.path.join(ROOT, "include", "ecfft_hip.h")).read()
    assert f"#define ECFFT_FACTOR_SMALL_MAX {FT.FACTOR_SMALL_MAX} " in header
    assert FT.FACTOR_SMALL_MAX == 65
    for name in ("poly_squarefree_decompose", "poly_factor", "factor_unpack", "poly_irreducible_factors"):
        assert hasattr(FT.FFTree, name)
    buf = np.zeros(8, np.uint32)
    n = np.zeros(4, np.int64)
    ptr, pn = buf.ctypes.data, n.ctypes.data
    sd, fa = L.ecfft_poly_squarefree_decompose, L.ecfft_poly_factor
    # a NULL context; then nf and count of zero and NULL pointers: all decided before a device is touched
    assert sd(None, ptr, 3, ptr, pn, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert fa(None, ptr, 3, ptr, pn, pn, pn, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    for nf, count in ((0, 1), (3, 0)):
        assert sd(None, ptr, nf, ptr, pn, ptr, count, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert fa(None, ptr, nf, ptr, pn, pn, pn, ptr, count, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert not buf.any() and not n.any()
