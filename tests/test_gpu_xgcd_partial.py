"""GPU tests of ecfft_poly_xgcd_partial: k_xgcd_partial_small (pairs of at most XGCD_PARTIAL_SMALL_MAX coefficients, one workgroup
per pair) and the large regime (gcd_pair stopped at the straddle point: half-GCD steps, one half-GCD of the truncated operands, the
leaf kernel with bound = stop).  Every output is compared byte for byte, through the oracle's standard-form converters, with the
exact model of tests/rs_ref.py: the first row of the classical sequence below `stop`, made monic in t."""
import ctypes
import functools

import numpy as np
import pytest

import gcd_ref as G
import poly_ref as R
import rs_ref as S
from conftest import std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P
SMALL = [(2, 1), (9, 9), (65, 40), (256, 256)]
LARGE = {"secp256k1": 600, "m31": 1100}               # just above the leaf kernel (512 / 1024 coefficients)

_trees = {}


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def tree_for(field, nmax):
    """the smallest tree the rule allows: next_pow2(2 nmax - 1) leaves, or a tiny tree for the small regime"""
    from ecfft_amd import fftree as FT
    n = 4
    if nmax > FT.XGCD_PARTIAL_SMALL_MAX:
        while n < 2 * nmax - 1:
            n <<= 1
    return tree(field, n)


def to_std(F, x):
    x = np.ascontiguousarray(x, F.dtype)
    out = np.empty_like(x)
    if x.shape[0]:
        F._to_std(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0])
    return out


def stops_for(da, db):
    m = (da + 1) // 2
    return sorted({0, 1, max(da // 3, 0), max(m - 1, 0), m, m + 1, max(db, 0), da + 1})


def rand_poly(field, n, seed):
    return G.rand_poly(field, n, seed) if n else []


def common_factor_pair(field, na, nb, dg, seed):
    """a = g u, b = g v of na and nb coefficients with g monic of degree dg"""
    dg = max(0, min(dg, na - 1, nb - 1))
    g = G.rand_poly(field, dg + 1, seed, monic=True)
    return G.mul(field, g, rand_poly(field, na - dg, seed + 1)), G.mul(field, g, rand_poly(field, nb - dg, seed + 2))


def abnormal_pair(field, na, nb, seed):
    """(r0, r1) with deg r0 = na - 1 built backwards from quotients of degree 2 to 5 (the first one at least na - nb, so that r1 has
    at most nb coefficients, the last one cut to fit) and a gcd of degree 1"""
    total, degs, i = na - 2, [min(max(na - nb, 0), max(na - 2, 0))], 1
    while sum(degs) < total:
        degs.append(min(2 + (i * 3 + seed) % 4, total - sum(degs)))
        i += 1
    degs = [d for d in degs if d > 0] or [0]
    qs = [G.rand_poly(field, d + 1, seed + 17 * j) for j, d in enumerate(degs)]
    r0, r1, _, _ = G.from_quotients(field, G.rand_poly(field, 2 if na > 1 else 1, seed + 5, monic=True), qs)
    return r0, r1


@functools.lru_cache(maxsize=None)
def cases(field, na, nb, large=False):
    """[(name, a, b)]: int lists of at most na and nb coefficients.  Rows shorter than na / nb are untrimmed rows of the call"""
    da = na - 1
    out = [("random", rand_poly(field, na, 1), rand_poly(field, nb, 2)),
           ("common_factor_high", *common_factor_pair(field, na, nb, 2 * da // 3, 10)),
           ("common_factor_low", *common_factor_pair(field, na, nb, 2, 20))]
    r0, r1 = abnormal_pair(field, na, nb, 30)
    if len(r1) <= nb:
        out.append(("abnormal", r0, r1))
    if nb >= 2:
        out.append(("deg_a_below_deg_b", rand_poly(field, max(1, min(na, nb) // 2), 40), rand_poly(field, nb, 41)))
    if not large:
        out += [("untrimmed", rand_poly(field, max(1, na - na // 4), 50), rand_poly(field, max(1, nb // 2), 51)),
                ("b_zero", rand_poly(field, na, 60), []), ("a_zero", [], rand_poly(field, nb, 61)), ("both_zero", [], [])]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def model(field, na, nb, large=False):
    """{name: {stop: (r, s, t, prev)}} over the stops of the shape, one pass over each sequence"""
    return {name: S.partial_rows(P[field], a, b, stops_for(na - 1, nb - 1)) for name, a, b in cases(field, na, nb, large)}


def run(F, t, field, a_rows, b_rows, na, nb, stop, device=False):
    """poly_xgcd_partial on int-list rows padded to na / nb; standard-form (r, s, t) and the degrees"""
    count = len(a_rows)
    a = std_to_field(F, np.concatenate([G.arr(field, v, na) for v in a_rows]))
    b = std_to_field(F, np.concatenate([G.arr(field, v, nb) for v in b_rows]))
    r, s, tt, deg = t.poly_xgcd_partial(a, b, stop, count=count)
    assert r.shape[0] == count * max(na, nb) and s.shape[0] == count * nb and tt.shape[0] == count * na and deg.shape == (count, 3)
    return to_std(F, r), to_std(F, s), to_std(F, tt), deg, (a, b, r, s, tt)


def check(field, na, nb, i, count, got, want, what):
    r, s, tt, deg = got
    er, es, et, _ = want
    ng = max(na, nb)
    assert np.array_equal(r[i * ng:(i + 1) * ng], G.arr(field, er, ng)), what
    assert np.array_equal(s[i * nb:(i + 1) * nb], G.arr(field, es, nb)), what
    assert np.array_equal(tt[i * na:(i + 1) * na], G.arr(field, et, na)), what
    assert list(deg[i]) == [S.deg(er), S.deg(es), S.deg(et)], what


def check_identity(F, t, field, na, nb, count, mem):
    """r = s a + t b through the library's own poly_mul (on a tree that holds the products), row by row"""
    a, b, r, s, tt = mem
    size = 4
    while size < na + nb - 1:
        size <<= 1
    t = tree(field, max(size, t.n))
    sa = to_std(F, t.poly_mul(s, a, count=count))
    tb = to_std(F, t.poly_mul(tt, b, count=count))
    rs = to_std(F, r)
    n, ng, p = na + nb - 1, max(na, nb), P[field]
    for i in range(count):
        x, y = R.to_ints(field, sa[i * n:(i + 1) * n]), R.to_ints(field, tb[i * n:(i + 1) * n])
        assert G.trim([(u + v) % p for u, v in zip(x, y)]) == G.ints(field, rs[i * ng:(i + 1) * ng])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", SMALL)
def test_small_regime(oracle_mod, field, na, nb):
    """all the rows of a shape in ONE call per stop, on a tree of four leaves"""
    F, t = oracle_mod.field(field), tree_for(field, max(na, nb))
    cs, want = cases(field, na, nb), model(field, na, nb)
    for stop in stops_for(na - 1, nb - 1):
        r, s, tt, deg, mem = run(F, t, field, [c[1] for c in cs], [c[2] for c in cs], na, nb, stop)
        for i, (name, _, _) in enumerate(cs):
            check(field, na, nb, i, len(cs), (r, s, tt, deg), want[name][stop], (name, stop))
        check_identity(F, t, field, na, nb, len(cs), mem)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", ["random", "common_factor_high", "common_factor_low", "abnormal", "deg_a_below_deg_b"])
def test_large_regime(oracle_mod, field, kind):
    """just above the leaf kernel on the smallest tree the rule allows: the leaf, one half-GCD node and one division step"""
    n = LARGE[field]
    F, t = oracle_mod.field(field), tree_for(field, n)
    assert t.n == (2048 if field == "secp256k1" else 4096)
    name, a, b = next(c for c in cases(field, n, n - 3, True) if c[0] == kind)
    want = model(field, n, n - 3, True)[kind]
    for stop in stops_for(n - 1, n - 4):
        r, s, tt, deg, mem = run(F, t, field, [a], [b], n, n - 3, stop)
        check(field, n, n - 3, 0, 1, (r, s, tt, deg), want[stop], (kind, stop))
    check_identity(F, t, field, n, n - 3, 1, mem)


@pytest.mark.parametrize("field", FIELDS)
def test_large_regime_rows_and_zero_operands(oracle_mod, field):
    """several pairs in one large-regime call (they run one after another), untrimmed and zero rows among them, and a device call"""
    import torch
    n = LARGE[field]
    F, t = oracle_mod.field(field), tree_for(field, n)
    p = P[field]
    a_rows = [rand_poly(field, n - 40, 70), [], rand_poly(field, n, 71), [], rand_poly(field, 3, 72)]
    b_rows = [rand_poly(field, n // 2, 73), rand_poly(field, n, 74), [], [], rand_poly(field, n, 75)]
    for stop in (0, n // 3, n):
        r, s, tt, deg, mem = run(F, t, field, a_rows, b_rows, n, n, stop)
        for i, (a, b) in enumerate(zip(a_rows, b_rows)):
            check(field, n, n, i, len(a_rows), (r, s, tt, deg), S.partial_row(p, a, b, stop), (i, stop))
    dev = [torch.from_numpy(x).cuda() for x in mem[:2]]
    r2, s2, t2, deg2 = t.poly_xgcd_partial(dev[0], dev[1], n, count=len(a_rows))
    assert r2.is_cuda and np.array_equal(r2.cpu().numpy(), mem[2]) and np.array_equal(s2.cpu().numpy(), mem[3])
    assert np.array_equal(t2.cpu().numpy(), mem[4]) and np.array_equal(deg2, deg)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [65, 256, "large"])
def test_stop_zero_agrees_with_xgcd(oracle_mod, field, n):
    """stop = 0 runs the sequence to its end like poly_xgcd: r = 0 and t = +-(a / g) / lc, so t g = a / lc(a) — and poly_gcd /
    poly_xgcd still give the bytes of the model on the same inputs (the kernels share their remainder loop)"""
    n = LARGE[field] if n == "large" else n
    F, t = oracle_mod.field(field), tree_for(field, n)
    p = P[field]
    a, b = common_factor_pair(field, n, n - 1, 5, 80)
    am, bm = std_to_field(F, G.arr(field, a, n)), std_to_field(F, G.arr(field, b, n - 1))
    r, s, tt, deg = t.poly_xgcd_partial(am, bm, 0)
    xs, xt, xg, xdeg = t.poly_xgcd(am, bm)
    g2, deg2 = t.poly_gcd(am, bm)
    g = G.ints(field, to_std(F, xg))
    assert not to_std(F, r).any() and deg[0][0] == -1 and xdeg[0] == deg2[0] == len(g) - 1 >= 5
    tg = G.mul(field, G.ints(field, to_std(F, tt)), g)
    assert tg == G._scale(a, pow(a[-1], p - 2, p), p)
    assert np.array_equal(xg, g2)
    assert g == G.gcd(field, a, b)
    assert G.check_xgcd(field, G.arr(field, a, n), G.arr(field, b, n - 1), to_std(F, xs), to_std(F, xt), to_std(F, xg)) == ""
    if n <= 256:
        es, et, eg = G.eea(field, a, b)
        assert G.ints(field, to_std(F, xs)) == es and G.ints(field, to_std(F, xt)) == et and g == eg


def test_argument_errors(oracle_mod):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    assert FT.XGCD_PARTIAL_SMALL_MAX == FT.GCD_SMALL_MAX == 256
    field = "m31"
    F, t = oracle_mod.field(field), tree(field, 4)
    one = std_to_field(F, G.arr(field, [1, 2, 3]))
    with pytest.raises(ValueError):
        t.poly_xgcd_partial(one, one[:0], 1)
    big = std_to_field(F, G.arr(field, [1] * 300))
    with pytest.raises(ValueError, match="too small"):                 # the large regime needs next_pow2(2 n - 1) leaves
        tree(field, 512).poly_xgcd_partial(big, big, 1)
    r, s, tt, deg = t.poly_xgcd_partial(one, one, 1)                    # the context keeps working
    assert list(deg[0]) == [-1, 0, 0]
