"""GPU tests of ecfft_poly_find_roots (utils::find_roots, src/utils.rs:25-44): k_roots_small (a polynomial of at most
ROOTS_SMALL_MAX coefficients finished by one workgroup, all rows in one launch), the large regime (g = gcd(f, x^p - x mod f), then
rounds that share one modular power among the pending factors and end in the same kernel) and k_roots_rank (the order).  Every
comparison is an equality of bytes or ints through the oracle's standard-form converters.  The expected roots are known by
construction: f = k prod (x - r_i)^m_i prod (x^2 + c_j^2), whose quadratics are irreducible because p = 3 mod 4 in both fields.
The returned roots are also fed to ecfft_poly_eval_points, which must give zeros.  The large cases run on exactly the tree the
header's rule asks for."""
import ctypes

import numpy as np
import pytest

import poly_ref as R
import powmod_ref as W
import roots_ref as RR
from conftest import std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P

_trees = {}


def small_max():
    from ecfft_amd import fftree as FT
    return FT.ROOTS_SMALL_MAX


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def rule_leaves(nf):
    """include/ecfft_hip.h: any tree up to ROOTS_SMALL_MAX coefficients, next_pow2(2 nf - 1) leaves above"""
    if nf <= small_max():
        return 4
    n = 1
    while n < 2 * nf - 1:
        n <<= 1
    return n


def to_std(F, x):
    x = np.ascontiguousarray(x, F.dtype)
    out = np.empty_like(x)
    if x.shape[0]:
        F._to_std(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0])
    return out


def to_mem(F, x):
    return std_to_field(F, x) if x.shape[0] else np.ascontiguousarray(x)


def pad(field, x, n):
    return W._pad(field, x, n)


def tree_product(field, polys):
    level = list(polys)
    while len(level) > 1:
        nxt = [R.mul_exact(field, level[i], level[i + 1]) for i in range(0, len(level) - 1, 2)]
        if len(level) & 1:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def build(field, roots_mult, nquad, k=3):
    """standard-form f = k prod (x - r)^m prod_{c = 1 .. nquad} (x^2 + c^2)"""
    p = P[field]
    parts = [R.from_ints(field, [k % p])]
    lin = [r % p for r, m in roots_mult for _ in range(m)]
    if lin:
        parts.append(W.from_roots(field, R.from_ints(field, lin)))
    if nquad:
        parts.append(tree_product(field, [R.from_ints(field, [c * c % p, 0, 1]) for c in range(1, nquad + 1)]))
    return tree_product(field, parts)


def spread_roots(field, r, seed):
    """r distinct elements spread over the field (i -> a i + b with an invertible a)"""
    p = P[field]
    a = 0x9E3779B1 if field == "m31" else 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95
    return [(a * (i + 1) + 1000 * seed) % p for i in range(r)]


def with_degree(field, deg, r, seed):
    """(f, sorted roots): degree exactly deg with r distinct roots; an odd rest makes the first root double"""
    roots = spread_roots(field, r, seed)
    rest = deg - r
    assert rest >= 0 and (r or rest % 2 == 0)
    rm = [(x, 1 + (rest % 2 if i == 0 else 0)) for i, x in enumerate(roots)]
    f = build(field, rm, rest // 2, k=5 + seed)
    assert f.shape[0] == deg + 1
    return f, sorted(roots)


def check(F, field, t, f, want, count=1, eval_tree=None):
    """poly_find_roots(f) == want: per row the sorted ints (None: the zero polynomial, -1), zeros above, and f(roots) = 0"""
    fm = to_mem(F, f)
    roots, n = t.poly_find_roots(fm, count=count)
    nf = f.shape[0] // count
    assert roots.shape[0] == count * (nf - 1) and n.dtype == np.int64 and n.shape == (count,)
    std = to_std(F, roots)
    for b in range(count):
        w = want[b]
        assert n[b] == (-1 if w is None else len(w)), (b, n[b])
        k = 0 if w is None else len(w)
        row = std[b * (nf - 1):(b + 1) * (nf - 1)]
        assert R.to_ints(field, row[:k]) == (w or []) if k else True, b
        assert not np.ascontiguousarray(roots[b * (nf - 1) + k:(b + 1) * (nf - 1)]).view(np.uint8).any()
        if k:
            et = eval_tree or (tree(field, 128) if nf == small_max() else t)     # poly_eval_points: next_pow2(nf) leaves above 64
            vals = et.poly_eval_points(np.ascontiguousarray(fm[b * nf:(b + 1) * nf]), np.ascontiguousarray(roots[b * (nf - 1):b * (nf - 1) + k]))
            assert not np.ascontiguousarray(vals).view(np.uint8).any(), b
    return roots, n


# ---- the small regime: one workgroup per polynomial, any tree --------------------------------------------------------------------------
SMALL = [(d, k) for d in (1, 2, 3, 63, 64) for k in ("all", "some", "one", "none") if not (k == "none" and d % 2)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("deg,kind", SMALL)
def test_small_regime_on_a_four_leaf_tree(oracle_mod, field, deg, kind):
    """all roots, some, one (double when the rest of the degree is odd) and none (even degrees: a product of quadratics)"""
    F, t = oracle_mod.field(field), tree(field, 4)
    r = {"all": deg, "some": deg - 2 * (deg // 4), "one": 1, "none": 0}[kind]
    f, want = with_degree(field, deg, r, deg)
    check(F, field, t, f, [want], eval_tree=tree(field, 128))


@pytest.mark.parametrize("field", FIELDS)
def test_the_reference_cubic_and_special_roots(oracle_mod, field):
    """finds_roots_of_cubic (x^3 - 4x: 0, 2, p - 2), and root sets with 0, 1, p - 1, p - 2, p - 3: the root -c makes w = 0 for the
    first shifts and must land in v"""
    F, t, p = oracle_mod.field(field), tree(field, 4), P[field]
    check(F, field, t, R.from_ints(field, [0, p - 4, 0, 1]), [[0, 2, p - 2]])
    sp = [0, 1, p - 1, p - 2, p - 3]
    check(F, field, t, build(field, [(x, 1) for x in sp], 0), [sorted(sp)])
    check(F, field, t, build(field, [(x, 1) for x in sp] + [(x, 1) for x in spread_roots(field, 40, 2)], 3, k=11),
          [sorted(sp + spread_roots(field, 40, 2))], eval_tree=tree(field, 128))
    for x in sp:
        check(F, field, t, build(field, [(x, 1)], 2), [[x]])


@pytest.mark.parametrize("field", FIELDS)
def test_multiplicities_and_untrimmed_rows(oracle_mod, field):
    F, t = oracle_mod.field(field), tree(field, 4)
    roots = spread_roots(field, 9, 4)
    f = build(field, [(x, 1 + i % 3) for i, x in enumerate(roots)], 4)       # multiplicities 1, 2 and 3
    assert f.shape[0] - 1 == 9 + 9 + 8
    got = check(F, field, t, f, [sorted(roots)])
    for n in (f.shape[0] + 1, small_max()):                                 # the same polynomial in longer rows
        padded = check(F, field, t, pad(field, f, n), [sorted(roots)])
        assert np.array_equal(padded[0][:9], got[0][:9])
    check(F, field, t, build(field, [(roots[0], 3)], 0), [[roots[0]]])


@pytest.mark.parametrize("field", FIELDS)
def test_the_quadratic_whose_first_four_shifts_fail(oracle_mod, field):
    """the shifts are 1, 2, 3, ... (documented): both roots stay together for c = 1 .. 4 and c = 5 parts them; alone, and with
    one of them double beside rootless quadratics"""
    F, t, p = oracle_mod.field(field), tree(field, 4), P[field]
    r, s = RR.legendre_pair(p)
    if field == "m31":
        assert (r, s) == (2, 50)
    check(F, field, t, build(field, [(r, 1), (s, 1)], 0, k=1), [[r, s]])
    check(F, field, t, build(field, [(r, 2), (s, 1)], 3), [[r, s]])


@pytest.mark.parametrize("field", FIELDS)
def test_a_batch_of_six_rows_in_one_call(oracle_mod, field):
    F, t, p = oracle_mod.field(field), tree(field, 4), P[field]
    nf = small_max()
    a, wa = with_degree(field, 64, 64, 1)
    b, wb = with_degree(field, 40, 11, 2)
    c, wc = R.from_ints(field, [0, p - 4, 0, 1]), [0, 2, p - 2]
    rows = [a, pad(field, b, nf), pad(field, c, nf), np.zeros(R.shape(field, nf), R.dtype(field)),
            pad(field, R.from_ints(field, [12345]), nf), pad(field, build(field, [], 20), nf)]
    want = [wa, wb, wc, None, [], []]
    f = np.concatenate(rows)
    roots, n = check(F, field, t, f, want, count=6, eval_tree=tree(field, 128))
    for i in (0, 1, 2):                                                      # count x rows == the same rows called singly
        r1, n1 = t.poly_find_roots(to_mem(F, rows[i]))
        assert n1[0] == n[i] and np.array_equal(r1, roots[i * (nf - 1):(i + 1) * (nf - 1)])
    # nf == 1: no roots array at all
    r0, n0 = t.poly_find_roots(to_mem(F, R.from_ints(field, [0, 5, 0])), count=3)
    assert r0.shape[0] == 0 and list(n0) == [-1, 0, -1]


# ---- the large regime on exactly the rule's tree -------------------------------------------------------------------------------------
LARGE = {"secp256k1": [65, 130, 300, 1030], "m31": [65, 300, 1030, 4100, (1 << 14) + 3]}
CASES = [(f, d, k) for f in FIELDS for d in LARGE[f] for k in ("all", "r65", "one", "half") if not (d == 65 and k == "r65")]


@pytest.mark.parametrize("field,deg,kind", CASES)
def test_large_regime_on_the_minimum_tree(oracle_mod, field, deg, kind):
    """r = deg (g = f), r = 65 (one split above the leaves), r = 1 inside a large rootless part, and about half"""
    F, t = oracle_mod.field(field), tree(field, rule_leaves(deg + 1))
    r = {"all": deg, "r65": 65, "one": 1, "half": deg // 2}[kind]
    f, want = with_degree(field, deg, r, deg % 97)
    check(F, field, t, f, [want])


@pytest.mark.parametrize("field", FIELDS)
def test_unequal_splits_pad_a_group(oracle_mod, field):
    """250 roots with r + 1 a square and 130 with r + 1 a non-square: the first shift splits 380 = 250 + 130, both of which take
    512 leaves, so the second round is ONE group whose shorter modulus is padded by x^120"""
    F, p = oracle_mod.field(field), P[field]
    sq, nsq = [], []
    for x in spread_roots(field, 2000, 9):
        s = RR.legendre(x + 1, p)
        if s == 1 and len(sq) < 250:
            sq.append(x)
        if s == -1 and len(nsq) < 130:
            nsq.append(x)
    assert len(sq) == 250 and len(nsq) == 130
    f = build(field, [(x, 1) for x in sq + nsq], 5)
    check(F, field, tree(field, rule_leaves(f.shape[0])), f, [sorted(sq + nsq)])


@pytest.mark.parametrize("field", FIELDS)
def test_two_different_polynomials_and_untrimmed_long_rows(oracle_mod, field):
    F = oracle_mod.field(field)
    nf = 301
    t = tree(field, rule_leaves(nf))
    a, wa = with_degree(field, 300, 140, 3)
    b, wb = with_degree(field, 200, 90, 4)                                  # true degree 200 in a row of 301
    roots, n = check(F, field, t, np.concatenate([a, pad(field, b, nf)]), [wa, wb], count=2)
    c, wc = with_degree(field, 40, 17, 5)                                   # a short polynomial in a long row: the leaf kernel on its true length
    z = np.zeros(R.shape(field, nf), R.dtype(field))
    check(F, field, t, np.concatenate([pad(field, c, nf), z, pad(field, R.from_ints(field, [9]), nf)]), [wc, None, []], count=3)


# ---- memory kinds, repeated calls and the pool -----------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("deg", [40, 200])
def test_device_memory_equals_host_memory_and_calls_repeat(oracle_mod, field, deg):
    import torch
    F, t = oracle_mod.field(field), tree(field, rule_leaves(deg + 1))
    f, want = with_degree(field, deg, deg // 2, 6)
    fm = to_mem(F, np.concatenate([f, f[::-1].copy()]))
    roots, n = t.poly_find_roots(fm, count=2)
    again, n2 = t.poly_find_roots(fm, count=2)
    assert roots.tobytes() == again.tobytes() and np.array_equal(n, n2) and n[0] == len(want)
    df = torch.from_numpy(fm.view(np.int64) if field == "secp256k1" else fm.view(np.int32)).cuda()
    droots, dn = t.poly_find_roots(df, count=2)
    assert np.array_equal(dn, n)
    assert np.array_equal(droots.cpu().numpy().view(roots.dtype).reshape(roots.shape), roots)


@pytest.mark.parametrize("field", FIELDS)
def test_repeated_use_and_trim(oracle_mod, field):
    """the pool after 2 and after 6 large-regime calls is the same size, and ecfft_ctx_trim gives it back"""
    import ecfft_amd
    deg = 200
    t = ecfft_amd.FIELDS[field].build_fftree(rule_leaves(deg + 1))
    F = oracle_mod.field(field)
    f, want = with_degree(field, deg, 150, 8)
    fm = to_mem(F, f)
    t.poly_find_roots(fm)                                                   # the transform scratch (grow-only, not a temporary) reaches its size
    t.trim()
    before = t.device_bytes
    first = t.poly_find_roots(fm)
    t.poly_find_roots(fm)
    held = t.device_bytes
    for _ in range(4):
        again = t.poly_find_roots(fm)
    assert t.device_bytes == held
    assert first[0].tobytes() == again[0].tobytes() and first[1][0] == again[1][0] == 150
    t.trim()
    assert t.device_bytes == before


# ---- errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_errors(oracle_mod, field):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    F = oracle_mod.field(field)
    nf = small_max() + 1                                                    # the first size that needs a tree: next_pow2(2 nf - 1) leaves
    need = rule_leaves(nf)
    f, want = with_degree(field, nf - 1, 30, 1)
    fm = to_mem(F, f)
    out = np.zeros_like(fm[:nf - 1])
    n = np.zeros(2, np.int64)
    small, enough = tree(field, need // 2), tree(field, need)
    L = small._L
    args = lambda t, pf, nf_, pr, pn, count=1, mem=FT.MEM_HOST: (t._h, pf, nf_, pr, pn, count, mem, None)
    assert L.ecfft_poly_find_roots(*args(small, fm.ctypes.data, nf, out.ctypes.data, n.ctypes.data)) == FT.ERR_TREE_TOO_SMALL
    assert not out.view(np.uint8).any() and n[0] == 0
    # the small regime needs no tree at all, and the context keeps working after the error
    r1, n1 = small.poly_find_roots(pad(field, fm[:nf - 1], nf - 1))
    assert n1[0] >= 0
    r2, n2 = enough.poly_find_roots(fm)
    assert n2[0] == 30 and R.to_ints(field, to_std(F, r2)[:30]) == want
    t = enough
    ok = (fm.ctypes.data, nf, out.ctypes.data, n.ctypes.data)
    assert L.ecfft_poly_find_roots(*args(t, None, nf, out.ctypes.data, n.ctypes.data)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_find_roots(*args(t, fm.ctypes.data, nf, out.ctypes.data, None)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_find_roots(*args(t, fm.ctypes.data, nf, None, n.ctypes.data)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_find_roots(*args(t, fm.ctypes.data, 1, None, n.ctypes.data)) == FT.OK and n[0] == 0
    assert L.ecfft_poly_find_roots(*args(t, fm.ctypes.data, 0, out.ctypes.data, n.ctypes.data)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_find_roots(*args(t, *ok, count=0)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_find_roots(*args(t, *ok, count=(1 << 62))) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_find_roots(*args(t, *ok, mem=7)) == FT.ERR_BAD_ARG
    shard = ecfft_amd.FIELDS[field].build_extend_shard(1024, 1, 0)         # EXTEND-only context: holds no full tree
    assert L.ecfft_poly_find_roots(*args(shard, fm.ctypes.data, 8, out.ctypes.data, n.ctypes.data)) == FT.ERR_BAD_ARG
    with pytest.raises(ValueError):
        t.poly_find_roots(fm[:0])
    r3, n3 = t.poly_find_roots(fm)
    assert n3[0] == 30 and r3.tobytes() == r2.tobytes()
