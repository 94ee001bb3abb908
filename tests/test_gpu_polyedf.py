"""GPU tests of ecfft_poly_equal_degree: k_edf_small (a polynomial of at most EDF_SMALL_MAX coefficients finished by one workgroup,
all rows in one launch, on any tree), k_edf_rank (the canonical order) and the large regime (the modulus kept once per row, the
Frobenius iterates taken as a kept composition or as fresh powers, rounds of one norm and one grouped modular power, leaves handed
to the kernel).  Every comparison is an equality of bytes or ints through the oracle's standard-form converters.  The expected
outputs are known by CONSTRUCTION (tests/edf_ref.case): g = k prod q over distinct irreducibles q of degree d, the binomials
x^d - a of tests/ddf_ref and their shifts (x + s)^d - a; the expected row is sorted(q[:-1] for q).

Time on one MI355X: 21 s for the file (49 cases); the slowest case, (3, 100) for secp256k1 with both iterate methods forced, 3.4 s."""
import ctypes

import numpy as np
import pytest

import ddf_ref as D
import edf_ref as E
import poly_ref as R
import roots_ref as RR
from conftest import std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P

_trees = {}
_cases = {}


def small_max():
    from ecfft_amd import fftree as FT
    return FT.EDF_SMALL_MAX


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def rule_leaves(ng):
    n = 1
    while n < 2 * ng - 1:
        n *= 2
    return n


def to_std(F, x):
    x = np.ascontiguousarray(x, F.dtype)
    out = np.empty_like(x)
    if x.shape[0]:
        F._to_std(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0])
    return out


def mem_rows(F, field, rows, ng):
    """int-list rows, each zero-padded to ng coefficients, laid end to end in the crate's form"""
    flat = []
    for r in rows:
        assert len(r) <= ng
        flat += [v % P[field] for v in r] + [0] * (ng - len(r))
    return std_to_field(F, R.from_ints(field, flat))


def case(field, d, r, k=3):
    """(g, want): computed once and shared"""
    key = (field, d, r, k)
    if key not in _cases:
        _cases[key] = E.case(d, r, P[field], k)
    return _cases[key]


def check(F, field, t, d, rows, wants, ng=None):
    """poly_equal_degree of the rows (int lists; wants: the list of factors, None for a zero row, -2 for a degree d does not divide)
    in ONE call"""
    count = len(rows)
    ng = ng or max(len(r) for r in rows)
    nd = max(ng - 1, 1)
    fac, n = t.poly_equal_degree(mem_rows(F, field, rows, ng), d, count=count)
    assert fac.shape[0] == count * nd and n.dtype == np.int64 and n.shape == (count,)
    got = R.to_ints(field, to_std(F, fac))
    for b, want in enumerate(wants):
        row, nb = E.pack(want, nd, d)
        assert n[b] == nb, (b, n[b], nb)
        assert got[b * nd:(b + 1) * nd] == row, b
    return fac, n


# ---- the small regime: one workgroup per polynomial, a 4-leaf tree ------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d,r", E.GPU_ONE_FACTOR)
def test_small_one_factor_comes_back_as_is(oracle_mod, field, d, r):
    F, t = oracle_mod.field(field), tree(field, 4)
    g, want = case(field, d, r, k=5)
    assert len(want) == 1
    check(F, field, t, d, [g], [want])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d,r", E.GPU_LINEAR)
def test_small_linear_factors_are_the_roots(oracle_mod, field, d, r):
    F, t, p = oracle_mod.field(field), tree(field, 4), P[field]
    g, want = case(field, d, r)
    fac, n = check(F, field, t, 1, [g], [want])
    roots, nr = t.poly_find_roots(mem_rows(F, field, [g], r + 1))
    rho = R.to_ints(field, to_std(F, roots))[:nr[0]]
    assert nr[0] == n[0] == r
    assert sorted(-v % p for v in R.to_ints(field, to_std(F, fac))[:r]) == rho


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d,r", E.GPU_SMALL_SPLITS)
def test_small_splits(oracle_mod, field, d, r):
    """(2, 2) is the smallest split, (2, 32) the limit of 65 coefficients"""
    F, t = oracle_mod.field(field), tree(field, 4)
    g, want = case(field, d, r)
    assert len(g) == d * r + 1 <= small_max()
    check(F, field, t, d, [g], [want])


@pytest.mark.parametrize("field", FIELDS)
def test_small_mixed_rows_batch_against_single_and_device_memory(oracle_mod, field):
    """k = 3, untrimmed rows, three true degrees, a zero row (-1), a constant (0) and a degree d does not divide (-2) in one call;
    the batch against single calls; device against host memory"""
    import torch
    F, t = oracle_mod.field(field), tree(field, 4)
    (d, _), (d2, r2) = E.GPU_MIXED_ROWS[0], E.GPU_MIXED_ROWS[3]
    rows, wants = [], []
    for d_, r in E.GPU_MIXED_ROWS[:3]:
        assert d_ == d == 3
        g, want = case(field, d, r)
        rows.append(g + [0, 0])
        wants.append(want)
    odd, _ = case(field, d2, r2)                                             # degree 8: 3 does not divide it
    rows += [[0], [12345], odd]
    wants += [None, [], -2]
    ng = 30
    fac, n = check(F, field, t, d, rows, wants, ng=ng)
    assert n.tolist() == [5, 2, 9, -1, 0, -2]
    nd = ng - 1
    for b in range(len(rows)):
        one, n1 = check(F, field, t, d, [rows[b]], [wants[b]], ng=ng)
        assert n1[0] == n[b] and one.tobytes() == fac[b * nd:(b + 1) * nd].tobytes()
    fm = mem_rows(F, field, rows, ng)
    as_int = lambda a: a.view(np.int64) if field == "secp256k1" else a.view(np.int32)
    dfac, dn = t.poly_equal_degree(torch.from_numpy(as_int(fm)).cuda(), d, count=len(rows))
    assert np.array_equal(dn, n) and np.array_equal(dfac.cpu().numpy().view(fac.dtype).reshape(fac.shape), fac)
    fac1, n1 = t.poly_equal_degree(mem_rows(F, field, [[0], [7], [0]], 1), 1, count=3)      # ng = 1: one entry per row all the same
    assert n1.tolist() == [-1, 0, -1] and not np.ascontiguousarray(fac1).view(np.uint8).any()


# ---- the large regime, on exactly the rule's tree ----------------------------------------------------------------------------------------
def large(F, field, d, r, hooks_lib=None, ng=None):
    import ecfft_amd
    g, want = case(field, d, r)
    ng = ng or len(g)
    if hooks_lib is None:
        return check(F, field, tree(field, rule_leaves(ng)), d, [g], [want], ng=ng)
    th = ecfft_amd.FIELDS[field].build_fftree(rule_leaves(ng))                # made inside the hooks library, never from the cache
    outs = []
    try:
        for mode in (1, 2):
            assert hooks_lib.ecfft_test_ddf_iterate(mode) == 0
            outs.append(check(F, field, th, d, [g], [want], ng=ng))
    finally:
        assert hooks_lib.ecfft_test_ddf_iterate(0) == 0
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d,r", E.GPU_LARGE_FIRST)
def test_large_first_lengths_above_the_limit(oracle_mod, field, d, r):
    F = oracle_mod.field(field)
    assert d * r + 1 == 67
    large(F, field, d, r)


# the forced fresh power stays at d <= 9 for secp256k1 and d <= 21 for M31: 504 products per iterate for secp256k1
BOTH = [(f, d, r) for f in FIELDS for d, r in E.GPU_LARGE_BOTH[f]]
SHIPPED = [(f, d, r) for f in FIELDS for d, r in E.GPU_LARGE_SHIPPED[f]]


@pytest.mark.parametrize("field,d,r", BOTH)
def test_large_regime_with_both_iterate_methods(oracle_mod, hooks_lib, field, d, r):
    """the kept composition (1) and the fresh power (2), forced by ecfft_test_ddf_iterate: the constructed factors, and the same
    bytes; (3, 100) takes several rounds with unequal pending factors padded into one group and leaves handed to the kernel"""
    large(oracle_mod.field(field), field, d, r, hooks_lib=hooks_lib)


@pytest.mark.parametrize("field,d,r", SHIPPED)
def test_large_regime_shipped_rule(oracle_mod, field, d, r):
    """(2, 160): several rounds, no iterate at all; (63, 2) and (21, 4): the iterates dominate"""
    large(oracle_mod.field(field), field, d, r)


@pytest.mark.parametrize("field", FIELDS)
def test_linear_factors_and_find_roots_run_the_same_rounds(oracle_mod, field):
    """200 distinct roots, 120 with r + 1 a square and 80 with r + 1 a non-square (chosen as test_gpu_polyroots.py's
    test_unequal_splits_pad_a_group chooses them): 201 coefficients on the 512-leaf tree are the large regime of both calls.  The
    first shift splits 200 = 120 + 80, both still pending and both of 256 leaves, so the second round is ONE group whose shorter
    modulus is padded by x^40.  poly_equal_degree(g, 1) and poly_find_roots(g) run the one splitting loop: the negated constant
    terms of the 200 factors, sorted, are exactly the roots array, and both are the constructed roots."""
    F, p = oracle_mod.field(field), P[field]
    a = 0x9E3779B1 if field == "m31" else 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95
    sq, nsq = [], []
    for i in range(2000):
        x = (a * (i + 1) + 9000) % p
        s = RR.legendre(x + 1, p)
        if s == 1 and len(sq) < 120:
            sq.append(x)
        if s == -1 and len(nsq) < 80:
            nsq.append(x)
    roots = sq + nsq
    assert len(sq) == 120 and len(nsq) == 80 and len(set(roots)) == 200
    g = D.product([[-x % p, 1] for x in roots], p)
    assert len(g) == 201 > small_max() and rule_leaves(201) == 512
    t = tree(field, 512)
    fac, n = check(F, field, t, 1, [g], [[[-x % p, 1] for x in roots]])
    rho, nr = t.poly_find_roots(mem_rows(F, field, [g], 201))
    assert n[0] == nr[0] == 200 and fac.shape[0] == rho.shape[0] == 200
    assert sorted(-v % p for v in R.to_ints(field, to_std(F, fac))) == R.to_ints(field, to_std(F, rho)) == sorted(roots)


@pytest.mark.parametrize("field", FIELDS)
def test_large_short_polynomial_in_a_long_row_and_degenerate_rows(oracle_mod, field):
    F = oracle_mod.field(field)
    t = tree(field, rule_leaves(300))
    g, want = case(field, 3, 21)                                              # true degree 63 in a row of 300
    wide, wwant = case(field, 7, 10)                                          # degree 70: 3 does not divide it
    check(F, field, t, 3, [g, [0], [9], wide + [0], g], [want, None, [], -2, want], ng=300)
    check(F, field, t, 7, [wide, [0]], [wwant, None], ng=300)                 # a long polynomial next to a zero row


@pytest.mark.parametrize("field", FIELDS)
def test_repeated_use_and_trim(oracle_mod, field):
    """the pool after 2 and after 6 large-regime calls is the same size, and ecfft_ctx_trim gives it back"""
    import ecfft_amd
    F = oracle_mod.field(field)
    g, want = case(field, 7, 10)
    t = ecfft_amd.FIELDS[field].build_fftree(rule_leaves(len(g)))
    fm = mem_rows(F, field, [g], len(g))
    t.poly_equal_degree(fm, 7)                                                # the transform scratch (grow-only, not a temporary) reaches its size
    t.trim()
    before = t.device_bytes
    first = t.poly_equal_degree(fm, 7)
    t.poly_equal_degree(fm, 7)
    held = t.device_bytes
    for _ in range(4):
        again = t.poly_equal_degree(fm, 7)
    assert t.device_bytes == held
    assert first[0].tobytes() == again[0].tobytes() and first[1][0] == again[1][0] == 10
    assert R.to_ints(field, to_std(F, first[0])) == E.pack(want, len(g) - 1, 7)[0]
    t.trim()
    assert t.device_bytes == before


@pytest.mark.parametrize("field", FIELDS)
def test_errors_and_the_tree_rule(oracle_mod, field):
    from ecfft_amd import fftree as FT
    F = oracle_mod.field(field)
    L = FT.lib()
    g, want = case(field, 2, 33)
    ng = len(g)
    assert ng == 67 and rule_leaves(ng) == 256
    t = tree(field, 128)                                                      # one tree size below the rule
    fm = mem_rows(F, field, [g], ng)
    out = np.zeros_like(fm)
    n = np.zeros(1, np.int64)
    ed = L.ecfft_poly_equal_degree
    assert ed(t._h, fm.ctypes.data, ng, 2, out.ctypes.data, n.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_TREE_TOO_SMALL
    g65, want65 = case(field, 2, 32)
    check(F, field, t, 2, [g65], [want65])                                    # 65 coefficients work on any tree
    assert ed(t._h, fm.ctypes.data, ng, 0, out.ctypes.data, n.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert ed(t._h, fm.ctypes.data, 0, 2, out.ctypes.data, n.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert ed(t._h, fm.ctypes.data, ng, 2, out.ctypes.data, n.ctypes.data, 0, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert ed(t._h, None, ng, 2, out.ctypes.data, n.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert ed(t._h, fm.ctypes.data, ng, 2, None, n.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert ed(t._h, fm.ctypes.data, ng, 2, out.ctypes.data, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert ed(t._h, fm.ctypes.data, 65, 2, out.ctypes.data, n.ctypes.data, 1, 7, None) == FT.ERR_BAD_ARG    # no such memory kind
    with pytest.raises(ValueError):
        t.poly_equal_degree(fm, 0)
    with pytest.raises(ValueError, match="FFTree is too small"):
        t.poly_equal_degree(fm, 2)


# ---- the pipeline and the cap -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_pipeline_irreducible_factors(oracle_mod, field):
    """f = k (linear factors)(x^2 - a_i)..(x^3 - b_i).. with multiplicities: poly_irreducible_factors returns the constructed sets"""
    F, p = oracle_mod.field(field), P[field]
    lin = E.irreducibles(1, 5, p)
    quad = D.irreducible_binomials(2, 3, p)
    cub = D.irreducible_binomials(3, 2, p)
    parts = [lin[0]] * 3 + lin[1:] + [quad[0]] * 2 + quad[1:] + cub + [cub[1]]
    f = [v * 7 % p for v in D.product(parts, p)]
    t = tree(field, 4)
    assert len(f) <= small_max()
    got = t.poly_irreducible_factors(mem_rows(F, field, [f], len(f)))
    assert sorted(got) == [1, 2, 3]
    for d, qs in ((1, lin), (2, quad), (3, cub)):
        assert [R.to_ints(field, to_std(F, q)) for q in got[d]] == sorted(qs)


def test_cap_is_an_error_return_and_the_context_survives(oracle_mod):
    """M31, small regime: the irreducible x^6 - a passed with d = 3 violates the precondition and every shift fails: ECFFT_ERR_HIP,
    not a device fault, and the next call on the same context succeeds"""
    from ecfft_amd import fftree as FT
    field = "m31"
    F, t = oracle_mod.field(field), tree(field, 4)
    L = FT.lib()
    q = D.irreducible_binomials(6, 1, P[field])[0]
    fm = mem_rows(F, field, [q], 7)
    out = np.zeros(6, fm.dtype)
    n = np.zeros(1, np.int64)
    assert L.ecfft_poly_equal_degree(t._h, fm.ctypes.data, 7, 3, out.ctypes.data, n.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_HIP
    g, want = case(field, 3, 2)
    check(F, field, t, 3, [g], [want])
    check(F, field, t, 6, [q], [[q]])
