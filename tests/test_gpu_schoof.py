"""GPU tests of ecfft_division_polynomial (the memoised driver on the products of ecfft_poly_mul), ecfft_curve_trace_mod and
ecfft_curve_cardinality.  Small regime: k_schoof_small, one workgroup per curve — psi_l from the recurrence, pi, pi^2 by the
composition or by the powers, the group law with its infinity case, and the restart on a proper factor of the modulus where a
denominator is not invertible.  Large regime (l >= 13): the host driver on the kept modulus, a split that hands a factor to the
kernel, both forms of pi^2, the tree rule.  The count: every row of the table of known orders with its residues.  Every
comparison is an equality of ints: with the exact model tests/schoof_ref.py, whose residues for the small-regime curves are
recorded in tests/golden/schoof_residues.json (tests/test_schoof_ref_host.py recomputes every entry and pins the branches they
reach), and with the known orders, each of which the host test checks by N P = O.

The small-regime calls run on a tree of 2 leaves: the regime needs no transform.  Time on one MI355X: 8 s for the file (31 cases)."""
import json
import os

import numpy as np
import pytest

import poly_ref as R
import schoof_ref as S
from conftest import GOLDEN, std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
LS = [2, 3, 5, 7, 11]

_trees = {}
_golden = {}


def golden(field):
    if not _golden:
        with open(os.path.join(GOLDEN, "schoof_residues.json")) as f:
            _golden.update(json.load(f))
    return _golden[field]


def tree(field, n=2):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def elems(F, field, vals):
    return std_to_field(F, R.from_ints(field, [v % S.P[field] for v in vals]))


def curves(F, field, rows):
    return elems(F, field, [r["A"] for r in rows]), elems(F, field, [r["B"] for r in rows])


@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("field", FIELDS)
def test_eight_mixed_curves_in_one_call(oracle_mod, field, l):
    """count = 8 in ONE launch: curves without a split, curves whose modulus splits (once, and down to degree 1), supersingular
    curves (pi^2 + [p] = O, the infinity branch) and a singular curve (-1), so that divergent workgroups share the launch"""
    F, t = oracle_mod.field(field), tree(field)
    rows = golden(field)
    assert len(rows) == 8
    A, B = curves(F, field, rows)
    got = t.curve_trace_mod(A, B, l)
    assert got.dtype == np.int64 and got.shape == (8,)
    want = [r["t"][str(l)] for r in rows]
    assert got.tolist() == want
    assert -1 in want and (l == 2 or any(r["splits_infinity_deg1"][str(l)][1] for r in rows))
    if l in (3, 7):
        assert any(r["splits_infinity_deg1"][str(l)][0] for r in rows)


def test_secp256k1_residues_of_the_published_order(oracle_mod):
    field = "secp256k1"
    F, t = oracle_mod.field(field), tree(field)
    tr = S.P[field] + 1 - S.SECP256K1_ORDER
    for l in LS:
        assert t.curve_trace_mod(elems(F, field, [0]), elems(F, field, [7]), l).tolist() == [tr % l]


def test_m31_table_rows_by_the_known_orders(oracle_mod):
    """the orders of the issue's table (each satisfies N P = O in tests/test_schoof_ref_host.py): t = p + 1 - N modulo l"""
    field = "m31"
    F, t = oracle_mod.field(field), tree(field)
    table = {(8, 81): 2147489041, (1, 1): 2147423272, (2, 3): 2147477024, (5, 7): 2147430114, (0, 7): 2147444533,
             (11, 19): 2147429416, (3, 0): 2147483648, (1, 0): 2147483648}
    A, B = elems(F, field, [k[0] for k in table]), elems(F, field, [k[1] for k in table])
    for l in LS:
        assert t.curve_trace_mod(A, B, l).tolist() == [(S.P[field] + 1 - n) % l for n in table.values()]


@pytest.mark.parametrize("field", FIELDS)
def test_batch_against_single_calls_and_device_memory(oracle_mod, field):
    import torch
    F, t = oracle_mod.field(field), tree(field)
    rows = golden(field)
    A, B = curves(F, field, rows)
    l = 7
    got = t.curve_trace_mod(A, B, l)
    for b in range(len(rows)):
        assert t.curve_trace_mod(A[b:b + 1], B[b:b + 1], l).tolist() == [got[b]]
    as_int = lambda a: a.view(np.int64) if field == "secp256k1" else a.view(np.int32)
    dev = t.curve_trace_mod(torch.from_numpy(as_int(A)).cuda(), torch.from_numpy(as_int(B)).cuda(), l)
    assert np.array_equal(dev, got)
    assert np.array_equal(t.curve_trace_mod(A, B, l), got)                    # again on the same context


@pytest.mark.parametrize("field", FIELDS)
def test_both_forms_of_pi_squared_agree(oracle_mod, hooks_lib, field):
    """the powers (1) and the composition (2), forced by ecfft_test_schoof_pi2, and the shipped rule (0): the same residues"""
    import ecfft_amd
    F = oracle_mod.field(field)
    t = ecfft_amd.FIELDS[field].build_fftree(2)
    rows = golden(field)
    A, B = curves(F, field, rows)
    try:
        for l in (3, 7, 11):
            want = [r["t"][str(l)] for r in rows]
            for mode in (1, 2, 0):
                assert hooks_lib.ecfft_test_schoof_pi2(mode) == 0
                assert t.curve_trace_mod(A, B, l).tolist() == want, (l, mode)
    finally:
        assert hooks_lib.ecfft_test_schoof_pi2(0) == 0
    assert hooks_lib.ecfft_test_schoof_pi2(3) != 0


@pytest.mark.parametrize("field", FIELDS)
def test_errors(oracle_mod, field):
    from ecfft_amd import fftree as FT
    F, t = oracle_mod.field(field), tree(field)
    L = FT.lib()
    rows = golden(field)
    A, B = curves(F, field, rows)
    out = np.zeros(8, np.int64)
    tm = L.ecfft_curve_trace_mod
    ok = lambda: t.curve_trace_mod(A, B, 3).tolist() == [r["t"]["3"] for r in rows]
    for l in (0, 1, 4, 9, 201, 2**40):
        assert tm(t._h, A.ctypes.data, B.ctypes.data, l, out.ctypes.data, 8, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert ok()                                                           # the context works after each error
    assert tm(t._h, None, B.ctypes.data, 3, out.ctypes.data, 8, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert tm(t._h, A.ctypes.data, None, 3, out.ctypes.data, 8, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert tm(t._h, A.ctypes.data, B.ctypes.data, 3, None, 8, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert tm(t._h, A.ctypes.data, B.ctypes.data, 3, out.ctypes.data, 0, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert tm(None, A.ctypes.data, B.ctypes.data, 3, out.ctypes.data, 8, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert tm(t._h, A.ctypes.data, B.ctypes.data, 3, out.ctypes.data, 8, 7, None) == FT.ERR_BAD_ARG      # no such memory kind
    assert ok()
    with pytest.raises(ValueError):
        t.curve_trace_mod(A, B, 9)
    assert FT.SCHOOF_MAX_L == 199 and FT.SCHOOF_SMALL_MAX == 65 and FT.ORDER_BYTES == 40


# ---- ecfft_division_polynomial -------------------------------------------------------------------------------------------------------------
DIVPOLY_N = {"m31": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 17], "secp256k1": [3, 4, 5, 11, 13]}
DIVPOLY_CURVES = [(8, 81), (0, 7), (-3, 2)]                                  # distinct curves; the last one is singular


def to_std(F, x):
    import ctypes
    x = np.ascontiguousarray(x, F.dtype)
    out = np.empty_like(x)
    F._to_std(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0])
    return out


@pytest.mark.parametrize("field", FIELDS)
def test_division_polynomials_against_the_model(oracle_mod, field):
    """count = 3 distinct curves per call; every n of the list; the length L(n) and the leading coefficient n (odd) or n / 2 (even)"""
    F, p = oracle_mod.field(field), S.P[field]
    t = tree(field, 256 if field == "m31" else 128)
    A, B = elems(F, field, [c[0] for c in DIVPOLY_CURVES]), elems(F, field, [c[1] for c in DIVPOLY_CURVES])
    for n in DIVPOLY_N[field]:
        ln = S.L(n)
        assert t.division_polynomial_len(n) == ln
        out = t.division_polynomial(A, B, n)
        assert out.shape[0] == 3 * ln
        got = R.to_ints(field, to_std(F, out))
        for b, (a_, b_) in enumerate(DIVPOLY_CURVES):
            want = S.divpoly(n, a_, b_, p)
            row = got[b * ln:(b + 1) * ln]
            assert row == want + [0] * (ln - len(want)), (n, b)
            if n:
                assert row[-1] == (n if n & 1 else n // 2 if n > 2 else 1)
    small = tree(field, 2)                                                    # the closed forms need no transform
    for n in range(5):
        assert small.division_polynomial(A, B, n).tobytes() == t.division_polynomial(A, B, n).tobytes()


@pytest.mark.parametrize("field", FIELDS)
def test_division_polynomial_errors_and_the_tree_rule(oracle_mod, field):
    from ecfft_amd import fftree as FT
    F = oracle_mod.field(field)
    L = FT.lib()
    A, B = elems(F, field, [8]), elems(F, field, [81])
    dp = L.ecfft_division_polynomial
    t8, t16 = tree(field, 8), tree(field, 16)
    out = elems(F, field, [0] * 64)
    want5 = S.divpoly(5, 8, 81, S.P[field])
    ok = lambda t: R.to_ints(field, to_std(F, t.division_polynomial(A, B, 5))) == want5
    assert S.L(5) == 13
    assert dp(t8._h, A.ctypes.data, B.ctypes.data, 5, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_TREE_TOO_SMALL   # one size below the rule
    assert ok(t16)
    for bad in (200, 2**40):
        assert dp(t16._h, A.ctypes.data, B.ctypes.data, bad, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert ok(t16)
    assert dp(t16._h, None, B.ctypes.data, 5, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert dp(t16._h, A.ctypes.data, None, 5, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert dp(t16._h, A.ctypes.data, B.ctypes.data, 5, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert dp(t16._h, A.ctypes.data, B.ctypes.data, 5, out.ctypes.data, 0, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert ok(t16)
    with pytest.raises(ValueError):
        t16.division_polynomial(A, B, 200)
    with pytest.raises(ValueError, match="FFTree is too small"):
        t8.division_polynomial(A, B, 5)
    assert FT.SCHOOF_MAX_L == 199


# ---- the large regime: psi_l above 65 coefficients ------------------------------------------------------------------------------------------
# (A, B): #E over M31, the issue's table (each satisfies N P = O in tests/test_schoof_ref_host.py)
TABLE = {(8, 81): 2147489041, (1, 1): 2147423272, (2, 3): 2147477024, (5, 7): 2147430114, (0, 7): 2147444533,
         (11, 19): 2147429416, (3, 0): 2147483648, (1, 0): 2147483648}
SPLIT_13 = (1, 4, 12)       # M31: the model splits psi_13 (degree 84) once and finishes on a factor of degree 6; t mod 13 = 12


def leaves(l):
    n = 1
    while n < 2 * S.L(l) - 1:
        n *= 2
    return n


@pytest.mark.parametrize("l", [13, 17])
def test_large_regime_m31_table_rows(oracle_mod, l):
    """every table row plus a singular curve in one call; l = 13 (85 coefficients) and 17 (145) on the tree of the rule"""
    field = "m31"
    F, p = oracle_mod.field(field), S.P[field]
    assert leaves(13) == 256 and leaves(17) == 512
    t = tree(field, leaves(l))
    cs = list(TABLE) + [(-3, 2)]
    A, B = elems(F, field, [c[0] for c in cs]), elems(F, field, [c[1] for c in cs])
    assert t.curve_trace_mod(A, B, l).tolist() == [(p + 1 - n) % l for n in TABLE.values()] + [-1]


def test_large_regime_secp256k1_l13_of_the_published_order(oracle_mod):
    field = "secp256k1"
    F, t = oracle_mod.field(field), tree(field, leaves(13))
    assert t.curve_trace_mod(elems(F, field, [0]), elems(F, field, [7]), 13).tolist() == [(S.P[field] + 1 - S.SECP256K1_ORDER) % 13]


def test_large_regime_split_hands_a_factor_to_the_small_kernel_with_both_forms_of_pi_squared(oracle_mod, hooks_lib):
    """M31, l = 13: (1, 4) splits psi_13 down to degree 6, which k_schoof_small finishes; (8, 81) never splits.  The shipped rule
    (0), the powers (1) and the kept composition (2) give the same residues."""
    import ecfft_amd
    field = "m31"
    F, p = oracle_mod.field(field), S.P[field]
    t = ecfft_amd.FIELDS[field].build_fftree(leaves(13))
    a, b, r = SPLIT_13
    A, B = elems(F, field, [a, 8]), elems(F, field, [b, 81])
    want = [r, (p + 1 - TABLE[(8, 81)]) % 13]
    try:
        for mode in (0, 1, 2):
            assert hooks_lib.ecfft_test_schoof_pi2(mode) == 0
            assert t.curve_trace_mod(A, B, 13).tolist() == want, mode
    finally:
        assert hooks_lib.ecfft_test_schoof_pi2(0) == 0


@pytest.mark.parametrize("field", FIELDS)
def test_large_regime_tree_rule(oracle_mod, field):
    from ecfft_amd import fftree as FT
    F = oracle_mod.field(field)
    A, B = elems(F, field, [8]), elems(F, field, [81])
    out = np.zeros(1, np.int64)
    small = tree(field, leaves(13) // 2)                                       # one size below the rule
    tm = FT.lib().ecfft_curve_trace_mod
    assert tm(small._h, A.ctypes.data, B.ctypes.data, 13, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_TREE_TOO_SMALL
    assert tm(small._h, A.ctypes.data, B.ctypes.data, 15, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert small.curve_trace_mod(A, B, 11).shape == (1,)                       # the context works, and l <= 11 needs no tree
    with pytest.raises(ValueError, match="FFTree is too small"):
        small.curve_trace_mod(A, B, 13)


# ---- ecfft_curve_cardinality ------------------------------------------------------------------------------------------------------------------
def test_cardinality_of_every_m31_table_row(oracle_mod):
    field = "m31"
    F, p, t = oracle_mod.field(field), S.P[field], tree(field, 512)
    primes = S.primes_for(p)
    assert t.schoof_primes() == primes == [2, 3, 5, 7, 11, 13, 17]
    cs = list(TABLE) + [(-3, 2)]
    A, B = elems(F, field, [c[0] for c in cs]), elems(F, field, [c[1] for c in cs])
    orders, tr = t.curve_cardinality(A, B, traces=True)
    assert orders == list(TABLE.values()) + [0]
    assert tr.tolist() == [[(p + 1 - n) % l for l in primes] for n in TABLE.values()] + [[-1] * len(primes)]
    assert t.curve_cardinality(A[:1], B[:1]) == [TABLE[(8, 81)]]               # without traces


def test_cardinality_errors(oracle_mod):
    from ecfft_amd import fftree as FT
    field = "m31"
    F = oracle_mod.field(field)
    A, B = elems(F, field, [8]), elems(F, field, [81])
    order = np.zeros(FT.ORDER_BYTES, np.uint8)
    cc = FT.lib().ecfft_curve_cardinality
    t256, t512 = tree(field, 256), tree(field, 512)
    assert cc(t256._h, A.ctypes.data, B.ctypes.data, order.ctypes.data, None, 1, FT.MEM_HOST, None) == FT.ERR_TREE_TOO_SMALL
    assert cc(t512._h, None, B.ctypes.data, order.ctypes.data, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert cc(t512._h, A.ctypes.data, None, order.ctypes.data, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert cc(t512._h, A.ctypes.data, B.ctypes.data, None, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert cc(t512._h, A.ctypes.data, B.ctypes.data, order.ctypes.data, None, 0, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert cc(t512._h, A.ctypes.data, B.ctypes.data, order.ctypes.data, None, 1, FT.MEM_HOST, None) == FT.OK
    assert int.from_bytes(order.tobytes(), "little") == TABLE[(8, 81)]


def test_a_found_curve_through_the_short_weierstrass_helper(oracle_mod):
    """M31, k = 4: find_curve's y^2 = x (x^2 + a x + bb) as (A, B); its order is divisible by the 2^n that curve_two_sylow reports"""
    import ecfft_amd
    field = "m31"
    fld, t, p = ecfft_amd.FIELDS[field], tree(field, 512), S.P[field]
    r = fld.find_curve(4, 1)
    assert r is not None and r["n"] >= 4
    n2, _ = fld.curve_two_sylow(r["a"], r["bb"])
    assert int(n2[0]) == r["n"]
    A, B = fld.short_weierstrass(r["a"], r["bb"])
    (a,), (bb,) = fld.to_ints(r["a"]), fld.to_ints(r["bb"])
    assert (fld.to_ints(A), fld.to_ints(B)) == tuple([v] for v in S.from_find_curve(a, bb, p))
    (order,) = t.curve_cardinality(A, B)
    assert order % (1 << r["n"]) == 0 and (order - (p + 1)) ** 2 <= 4 * p          # Hasse
