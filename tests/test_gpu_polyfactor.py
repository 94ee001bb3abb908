"""GPU tests of ecfft_poly_squarefree_decompose and ecfft_poly_factor: k_yun_small (Yun's loop of a row of at most FACTOR_SMALL_MAX
coefficients in one workgroup), the shared launches of the small regime (one k_ddf_small over all parts of all rows, one k_edf_small
per distinct degree, the ranking, one scatter) and the large regime (Yun's loop on the gcd and division bodies, long parts through
the large regimes of distinct-degree and equal-degree splitting, short parts of all rows queued for the shared launches).  Every
comparison is an equality of bytes or ints through the oracle's standard-form converters.  The expected outputs are known by
CONSTRUCTION (tests/factor_ref.case): f = k prod q^e over distinct irreducibles; the expected list is sorted by (e, deg q, q).

Time on one MI355X: 6 s for the file (28 cases); the slowest case, S1 for secp256k1 with the first launches of the process, 1.7 s."""
import ctypes

import numpy as np
import pytest

import factor_ref as FR
import poly_ref as R
from conftest import std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P

_trees = {}
_cases = {}


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def rule_leaves(nf):
    n = 1
    while n < 2 * nf - 1:
        n *= 2
    return n


def to_std(F, x):
    x = np.ascontiguousarray(x, F.dtype)
    out = np.empty_like(x)
    if x.shape[0]:
        F._to_std(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0])
    return out


def mem_rows(F, field, rows, nf):
    """int-list rows, each zero-padded to nf coefficients, laid end to end in the crate's form"""
    flat = []
    for r in rows:
        assert len(r) <= nf
        flat += [v % P[field] for v in r] + [0] * (nf - len(r))
    return std_to_field(F, R.from_ints(field, flat))


def case(field, name, k=3):
    """(f, want): computed once and shared"""
    key = (field, name, k)
    if key not in _cases:
        spec = FR.SMALL[name] if name in FR.SMALL else FR.LARGE[name][0]
        _cases[key] = FR.case(spec, P[field], k)
    return _cases[key]


def check(F, field, t, rows, wants, leads, nf=None, fm=None):
    """poly_factor and poly_squarefree_decompose of the rows (int lists; wants: the expected [(q, e), ...], None for a zero row; leads:
    the leading coefficients) in ONE call each"""
    p = P[field]
    count = len(rows)
    nf = nf or max(len(r) for r in rows)
    nd = max(nf - 1, 1)
    fm = mem_rows(F, field, rows, nf) if fm is None else fm
    fac, fdeg, fmult, n, lead = t.poly_factor(fm, count=count)
    assert fac.shape[0] == count * nd and lead.shape[0] == count
    for a in (fdeg, fmult):
        assert a.dtype == np.int64 and a.shape == (count, nd)
    assert n.dtype == np.int64 and n.shape == (count,)
    got = R.to_ints(field, to_std(F, fac))
    assert R.to_ints(field, to_std(F, lead)) == [v % p for v in leads]
    for b, want in enumerate(wants):
        row, wdeg, wmult, wn = FR.pack_factor(want, nd)
        assert n[b] == wn, (b, n[b], wn)
        assert fdeg[b].tolist() == wdeg and fmult[b].tolist() == wmult, b
        assert got[b * nd:(b + 1) * nd] == row, b
    parts, deg, lead2 = t.poly_squarefree_decompose(fm, count=count)
    assert parts.shape[0] == count * nd and deg.dtype == np.int64 and deg.shape == (count, nd)
    assert lead2.tobytes() == lead.tobytes()
    gotp = R.to_ints(field, to_std(F, parts))
    for b, want in enumerate(wants):
        prow, pdeg = FR.pack_decompose(None if want is None else FR.parts_of(want, p), nd)
        assert deg[b].tolist() == pdeg, b
        assert gotp[b * nd:(b + 1) * nd] == prow, b
    return fac, fdeg, fmult, n, lead


# ---- the small regime: workgroup kernels alone, a 4-leaf tree ----------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", list(FR.SMALL))
def test_small_specs(oracle_mod, field, name):
    F, t = oracle_mod.field(field), tree(field, 4)
    f, want = case(field, name, k=7)
    from ecfft_amd import fftree as FT
    assert len(f) <= FT.FACTOR_SMALL_MAX
    fac, fdeg, fmult, n, lead = check(F, field, t, [f], [want], [7])
    unpacked = t.factor_unpack(fac, fdeg[0], fmult[0], n[0])
    assert [(R.to_ints(field, to_std(F, q)), e) for q, e in unpacked] == want


@pytest.mark.parametrize("field", FIELDS)
def test_small_mixed_rows_batch_against_single_and_device_memory(oracle_mod, field):
    """the zero row, a constant, a linear row, an untrimmed row and non-monic rows in one call, with `lead`; the yun model on the same
    inputs; the batch against single calls; device against host memory; lead = NULL"""
    import torch
    from ecfft_amd import fftree as FT
    F, t, p = oracle_mod.field(field), tree(field, 4), P[field]
    f1, w1 = case(field, "S1", k=p - 2)
    f4, w4 = case(field, "S4", k=1)
    rows = [[0], [12345], [9, 4], f1 + [0, 0, 0], f4, [0, 0, 0, 5]]
    lin = [9 * pow(4, p - 2, p) % p, 1]
    wants = [None, [], [(lin, 1)], w1, w4, [([0, 1], 3)]]
    leads = [0, 12345, 4, p - 2, 1, 5]
    nf = 30
    for b, r in enumerate(rows):                                             # the model agrees with the construction on these inputs
        y = FR.yun(r, p)
        assert (y is None) == (wants[b] is None)
        if y is not None:
            assert y[0] == FR.parts_of(wants[b], p) and y[1] == leads[b]
    fac, fdeg, fmult, n, lead = check(F, field, t, rows, wants, leads, nf=nf)
    assert n.tolist() == [-1, 0, 1, len(w1), 2, 1]
    nd = nf - 1
    for b in range(len(rows)):
        one = check(F, field, t, [rows[b]], [wants[b]], [leads[b]], nf=nf)
        assert one[0].tobytes() == fac[b * nd:(b + 1) * nd].tobytes() and one[3][0] == n[b]
    fm = mem_rows(F, field, rows, nf)
    as_int = lambda a: a.view(np.int64) if field == "secp256k1" else a.view(np.int32)
    dev = torch.from_numpy(as_int(fm)).cuda()
    dfac, dfdeg, dfmult, dn, dlead = t.poly_factor(dev, count=len(rows))
    assert np.array_equal(dn, n) and np.array_equal(dfdeg, fdeg) and np.array_equal(dfmult, fmult)
    assert np.array_equal(dfac.cpu().numpy().view(fac.dtype).reshape(fac.shape), fac)
    assert np.array_equal(dlead.cpu().numpy().view(lead.dtype).reshape(lead.shape), lead)
    parts, deg, _ = t.poly_squarefree_decompose(fm, count=len(rows))
    dparts, ddeg, dlead2 = t.poly_squarefree_decompose(dev, count=len(rows))
    assert np.array_equal(ddeg, deg) and np.array_equal(dparts.cpu().numpy().view(parts.dtype).reshape(parts.shape), parts)
    assert np.array_equal(dlead2.cpu().numpy().view(lead.dtype).reshape(lead.shape), lead)
    # lead = NULL: the same outputs
    L = FT.lib()
    out = np.zeros_like(fac)
    a, b_, c = np.zeros_like(fdeg), np.zeros_like(fmult), np.zeros_like(n)
    assert L.ecfft_poly_factor(t._h, fm.ctypes.data, nf, out.ctypes.data, a.ctypes.data, b_.ctypes.data, c.ctypes.data, None, len(rows),
                               FT.MEM_HOST, None) == 0
    assert out.tobytes() == fac.tobytes() and np.array_equal(a, fdeg) and np.array_equal(b_, fmult) and np.array_equal(c, n)
    fac1 = t.poly_factor(mem_rows(F, field, [[0], [7], [0]], 1), count=3)    # nf = 1: one entry per row all the same
    assert fac1[3].tolist() == [-1, 0, -1] and not np.ascontiguousarray(fac1[0]).view(np.uint8).any()
    assert R.to_ints(field, to_std(F, fac1[4])) == [0, 7, 0]


@pytest.mark.parametrize("field", FIELDS)
def test_small_launch_count_does_not_depend_on_count(oracle_mod, field):
    """S1 alone and six copies of S1 in one call take the same number of launches, and every copy gives the bytes of the single call"""
    F, t = oracle_mod.field(field), tree(field, 4)
    f, want = case(field, "S1", k=7)
    nf = len(f)

    def launches(fm, count):
        t.profile(True)
        out = t.poly_factor(fm, count=count)
        n = sum(c["launches"] for c in t.profile_read())
        t.profile(False)
        return n, out
    n1, one = launches(mem_rows(F, field, [f], nf), 1)
    n6, six = launches(mem_rows(F, field, [f] * 6, nf), 6)
    assert n1 == n6 and n1 > 0, (n1, n6)
    assert six[0].tobytes() == one[0].tobytes() * 6 and six[3].tolist() == [len(want)] * 6


# ---- the large regime, on exactly the rule's tree ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", list(FR.LARGE))
def test_large_specs(oracle_mod, field, name):
    F = oracle_mod.field(field)
    f, want = case(field, name, k=5)
    leaves = FR.LARGE[name][1]
    assert rule_leaves(len(f)) == leaves
    check(F, field, tree(field, leaves), [f], [want], [5])


@pytest.mark.parametrize("field", FIELDS)
def test_large_short_polynomial_in_a_long_row_and_degenerate_rows(oracle_mod, field):
    """rows of 100 coefficients on the 256-leaf tree: S1 (true degree 23), a zero row, a constant, S4 and S1 again go to the workgroup
    kernels on their true length and share their launches"""
    F = oracle_mod.field(field)
    f1, w1 = case(field, "S1", k=7)
    f4, w4 = case(field, "S4", k=1)
    assert rule_leaves(100) == 256
    check(F, field, tree(field, 256), [f1, [0], [9], f4, f1], [w1, None, [], w4, w1], [7, 0, 9, 1, 7], nf=100)


@pytest.mark.parametrize("field", FIELDS)
def test_large_rows_share_the_launches_of_their_small_parts(oracle_mod, field):
    """L1 and L2 in one call, padded to one nf: the queued small parts of the two rows share their launches; the bytes of each row are
    those of its own call"""
    F = oracle_mod.field(field)
    (f1, w1), (f2, w2) = case(field, "L1", k=5), case(field, "L2", k=5)
    nf = max(len(f1), len(f2))
    assert rule_leaves(nf) == 256
    t = tree(field, 256)
    both = check(F, field, t, [f1, f2], [w1, w2], [5, 5], nf=nf)
    nd = nf - 1
    for b, (f, w) in enumerate(((f1, w1), (f2, w2))):
        one = check(F, field, t, [f], [w], [5], nf=nf)
        assert one[0].tobytes() == both[0][b * nd:(b + 1) * nd].tobytes()


# ---- errors: decided before any GPU work --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_errors_and_the_tree_rule(oracle_mod, field):
    from ecfft_amd import fftree as FT
    F = oracle_mod.field(field)
    L = FT.lib()
    t = tree(field, 64)
    nf = 66
    assert rule_leaves(nf) == 256
    fm = mem_rows(F, field, [[1] * nf], nf)
    out, lead = np.zeros_like(fm[:nf - 1]), np.zeros_like(fm[:1])
    a, b, n = np.zeros(nf - 1, np.int64), np.zeros(nf - 1, np.int64), np.zeros(1, np.int64)
    pf, po, pl, pa, pb, pn = fm.ctypes.data, out.ctypes.data, lead.ctypes.data, a.ctypes.data, b.ctypes.data, n.ctypes.data
    fa, sd = L.ecfft_poly_factor, L.ecfft_poly_squarefree_decompose
    assert fa(t._h, pf, nf, po, pa, pb, pn, pl, 1, FT.MEM_HOST, None) == FT.ERR_TREE_TOO_SMALL
    assert sd(t._h, pf, nf, po, pa, pl, 1, FT.MEM_HOST, None) == FT.ERR_TREE_TOO_SMALL
    for args in ((None, po, pa, pb, pn), (pf, None, pa, pb, pn), (pf, po, None, pb, pn), (pf, po, pa, None, pn), (pf, po, pa, pb, None)):
        assert fa(t._h, args[0], 65, args[1], args[2], args[3], args[4], pl, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    for args in ((None, po, pa), (pf, None, pa), (pf, po, None)):
        assert sd(t._h, args[0], 65, args[1], args[2], pl, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    for nf_, count in ((0, 1), (65, 0)):
        assert fa(t._h, pf, nf_, po, pa, pb, pn, pl, count, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert sd(t._h, pf, nf_, po, pa, pl, count, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert fa(t._h, pf, 65, po, pa, pb, pn, pl, 1, 7, None) == FT.ERR_BAD_ARG            # no such memory kind
    with pytest.raises(ValueError, match="FFTree is too small"):
        t.poly_factor(fm)
    with pytest.raises(ValueError, match="FFTree is too small"):
        t.poly_squarefree_decompose(fm)
    assert not out.view(np.uint8).any() and not a.any() and not b.any() and not n.any()
