"""GPU tests of ecfft_poly_gcd / ecfft_poly_xgcd (utils::gcd / utils::xgcd, src/utils.rs:132-182): k_gcd_small (pairs of at most
GCD_SMALL_MAX coefficients, the whole remainder sequence in one workgroup) and the large regime (a half-GCD on the poly_mul and
division bodies whose recursion ends in the same kernel).  Every comparison is an equality of bytes or ints through the oracle's
standard-form converters (so the crate's Montgomery representation of secp256k1 is exercised): against gcds known by construction,
against pairs built backwards from a prescribed quotient sequence (tests/gcd_ref.py), against the sparse identity
gcd(x^n - 1, x^m - 1) = x^gcd(n, m) - 1, and against the root-finding step gcd(f, x^p - x mod f), which needs no reference."""
import ctypes
import math

import numpy as np
import pytest

import gcd_ref as G
import poly_ref as R
import powmod_ref as W
from conftest import std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P

_trees = {}


def small_max():
    from ecfft_amd import fftree as FT
    return FT.GCD_SMALL_MAX


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def tree_for(field, nmax):
    """next_pow2(2 nmax) leaves, or a tiny tree for the small regime"""
    n = 4
    if nmax > small_max():
        while n < 2 * nmax:
            n <<= 1
    return tree(field, n)


def to_std(F, x):
    x = np.ascontiguousarray(x, F.dtype)
    out = np.empty_like(x)
    if x.shape[0]:
        F._to_std(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0])
    return out


def to_mem(F, x):
    return std_to_field(F, x) if x.shape[0] else np.ascontiguousarray(x)


def rows(x, count, i):
    n = x.shape[0] // count
    return x[i * n:(i + 1) * n]


def pad(field, x, n):
    return W._pad(field, x, n)


def scaled(field, x, c):
    return R.mul_exact(field, x, R.from_ints(field, [c % P[field]]))


def known_pair(field, na, nb, kind, seed):
    """(a, b, g): standard-form a = g u of na and b = g v of nb coefficients (neither monic), u and v products of linear factors
    over DISJOINT root sets — coprime by construction — and g random monic of the degree `kind` asks for"""
    da, db = na - 1, nb - 1
    dg = {"zero": 0, "one": 1, "half": min(da, db) // 2, "all": min(da, db)}[kind]
    dg = min(dg, da, db)
    g = R.rand_std(field, dg + 1, seed, specials=False)
    g[dg] = R.from_ints(field, [1])[0]
    ru = R.from_ints(field, [1 + i for i in range(da - dg)])
    rv = R.from_ints(field, [1_000_003 + 7 * i for i in range(db - dg)])
    u = scaled(field, W.from_roots(field, ru), 3 + seed) if da > dg else R.from_ints(field, [3 + seed])
    v = scaled(field, W.from_roots(field, rv), 5 + seed) if db > dg else R.from_ints(field, [5 + seed])
    return R.mul_exact(field, g, u), R.mul_exact(field, g, v), g


def run_xgcd(F, field, t, a, b, count=1):
    """poly_xgcd and poly_gcd on standard-form rows; returns standard-form (s, t, g, degrees) after checking that both calls agree"""
    am, bm = to_mem(F, a), to_mem(F, b)
    s, tt, g, deg = t.poly_xgcd(am, bm, count=count)
    g2, deg2 = t.poly_gcd(am, bm, count=count)
    assert np.array_equal(g, g2) and np.array_equal(deg, deg2)
    return to_std(F, s), to_std(F, tt), to_std(F, g), deg


def lengths(nmax, order):
    return {"lt": (max(1, nmax // 2), nmax), "eq": (nmax, nmax), "gt": (nmax, max(1, 2 * nmax // 3))}[order]


# ---- a gcd known by construction ---------------------------------------------------------------------------------------------------
def known_sizes():
    g = small_max()
    return [1, 2, 3, 63, 64, 65, g - 1, g, g + 1, 2 * g + 1, 4 * g + 3, 16 * g + 5]


ORDERS = ["lt", "eq", "gt"]
KINDS = ["zero", "one", "half", "all"]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("idx", range(12))
def test_known_gcd(oracle_mod, field, idx):
    """a = g u, b = g v with coprime u, v: poly_gcd == g byte for byte, poly_xgcd passes check_xgcd (whose degree bounds make the
    cofactors unique); deg g in {0, 1, about half, deg b (b | a)}, na <, = and > nb in turn, one pair and three"""
    nmax = known_sizes()[idx]
    F, t = oracle_mod.field(field), tree_for(field, nmax)
    for count, order, kinds in ((1, ORDERS[idx % 3], [KINDS[idx % 4]]), (3, ORDERS[(idx + 1) % 3], [KINDS[(idx + 1 + i) % 4] for i in range(3)])):
        na, nb = lengths(nmax, order)
        pairs = [known_pair(field, na, nb, k, 10 * idx + i) for i, k in enumerate(kinds)]
        a, b = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
        s, tt, g, deg = run_xgcd(F, field, t, a, b, count)
        assert g.shape[0] == count * nmax and s.shape[0] == count * max(nb - 1, 1) and tt.shape[0] == count * max(na - 1, 1)
        for i, (ai, bi, gi) in enumerate(pairs):
            assert deg[i] == gi.shape[0] - 1, (nmax, order, kinds[i])
            assert np.array_equal(rows(g, count, i), pad(field, gi, nmax)), (nmax, order, kinds[i])
            assert G.check_xgcd(field, ai, bi, rows(s, count, i), rows(tt, count, i), rows(g, count, i)) == "", (nmax, order, kinds[i])


# ---- abnormal remainder sequences --------------------------------------------------------------------------------------------------
def fill(pattern, total):
    """quotient degrees from the pattern, cut so that they sum to `total`"""
    out, i = [], 0
    while sum(out) < total:
        out.append(min(pattern[i % len(pattern)], total - sum(out)))
        i += 1
    return out


def quotient_cases():
    g = small_max()
    big = g + 7
    half = 2 * g + 90
    return {
        "all_one": (fill([1], g + 3), 0),
        "mixed_above_small": (fill([2, 1, 40, 3, 1, 1, 2, 1], g + 11), 2),
        "mixed_4g": (fill([1, 2, big, 1, 3, 40, 1, 1, 2, 3, 1], 4 * g + 5), 1),
        # deg r0 = 2 half, m = half: the quotients before the big one sum to half, so the remainder it divides by has degree exactly m
        "split_point": (fill([1, 3, 2, 1, 40, 1], half) + [big] + fill([2, 1, 1, 3], half - big), 0),
        "equal_degrees": ([0] + fill([1, 2, 1, 40, 3], 2 * g), 3),
    }


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("case", ["all_one", "mixed_above_small", "mixed_4g", "split_point", "equal_degrees"])
def test_prescribed_quotient_sequences(oracle_mod, field, case):
    """pairs built backwards from their quotient sequence (degrees over {1, 2, 3, 40, G + 7}): g, s and t byte for byte"""
    degs, dg = quotient_cases()[case]
    qs = [G.rand_poly(field, d + 1, 1000 + 13 * i + d) for i, d in enumerate(degs)]
    g = G.rand_poly(field, dg + 1, 99, monic=True)
    r0, r1, s, tt = G.from_quotients(field, g, qs)
    na, nb = len(r0), len(r1)
    assert na - 1 == sum(degs) + dg
    if case == "split_point":
        assert (na - 1 + 1) // 2 == sum(degs[:degs.index(small_max() + 7)]) == na - 1 - sum(degs[:degs.index(small_max() + 7)])
    F, t = oracle_mod.field(field), tree_for(field, max(na, nb))
    for swap in (False, True):
        a, b, es, et = (r1, r0, tt, s) if swap else (r0, r1, s, tt)
        gs, gt, gg, deg = run_xgcd(F, field, t, G.arr(field, a), G.arr(field, b))
        assert deg[0] == dg
        assert np.array_equal(gg, G.arr(field, g, max(na, nb)))
        assert np.array_equal(gs, G.arr(field, es, max(len(b) - 1, 1))) and np.array_equal(gt, G.arr(field, et, max(len(a) - 1, 1)))


# ---- sparse known answers ----------------------------------------------------------------------------------------------------------
def binomial(field, n):
    """x^n - 1"""
    out = np.zeros(R.shape(field, n + 1), R.dtype(field))
    out[0] = R.from_ints(field, [P[field] - 1])[0]
    out[n] = R.from_ints(field, [1])[0]
    return out


@pytest.mark.parametrize("field,n,m", [("secp256k1", 3 << 12, (1 << 13) + (1 << 12)), ("secp256k1", 3 << 12, (1 << 13) + (1 << 11)),
                                       ("m31", 3 << 12, (1 << 13) + (1 << 11)), ("secp256k1", 4099, 3000), ("m31", 4099, 3000),
                                       ("m31", 1 << 16, (1 << 15) + (1 << 13))])
def test_gcd_of_binomials(oracle_mod, field, n, m):
    """gcd(x^n - 1, x^m - 1) = x^gcd(n, m) - 1: few, very long quotients"""
    F, t = oracle_mod.field(field), tree_for(field, max(n, m) + 1)
    a, b = binomial(field, n), binomial(field, m)
    s, tt, g, deg = run_xgcd(F, field, t, a, b)
    k = math.gcd(n, m)
    assert deg[0] == k and np.array_equal(g, pad(field, binomial(field, k), max(n, m) + 1))
    if max(n, m) <= 3 << 12:
        assert G.check_xgcd(field, a, b, s, tt, g) == ""


# ---- untrimmed and zero operands ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [40, "above"])
def test_untrimmed_and_zero_operands(oracle_mod, field, n):
    n = small_max() + 50 if n == "above" else n
    F, t = oracle_mod.field(field), tree_for(field, 2 * n)
    a, b, g = known_pair(field, n, n - 7, "half", n)
    z = lambda k: np.zeros(R.shape(field, k), R.dtype(field))
    s0, t0, g0, d0 = run_xgcd(F, field, t, a, b)
    assert d0[0] == g.shape[0] - 1 and np.array_equal(g0, pad(field, g, n))
    # high zero coefficients on either side or both: the same answer in longer rows
    for ea, eb in ((3, 0), (0, 9), (n // 2, n), (n, 1)):
        s1, t1, g1, d1 = run_xgcd(F, field, t, pad(field, a, n + ea), pad(field, b, n - 7 + eb))
        assert d1[0] == d0[0]
        assert np.array_equal(g1, pad(field, g0, g1.shape[0])) and np.array_equal(s1, pad(field, s0, s1.shape[0]))
        assert np.array_equal(t1, pad(field, t0, t1.shape[0]))
    # zero operands, constants, a = b
    inv = lambda x: R.from_ints(field, [pow(G.ints(field, x)[-1], P[field] - 2, P[field])])
    monic = lambda x: scaled(field, x, G.ints(field, inv(x))[0])
    for nz in (1, n):
        s1, t1, g1, d1 = run_xgcd(F, field, t, a, z(nz))
        assert d1[0] == n - 1 and np.array_equal(g1, monic(a)) and np.array_equal(s1, pad(field, inv(a), s1.shape[0])) and not t1.any()
        s1, t1, g1, d1 = run_xgcd(F, field, t, z(nz), b)
        assert d1[0] == n - 8 and np.array_equal(g1, pad(field, monic(b), g1.shape[0])) and not s1.any()
        assert np.array_equal(t1, pad(field, inv(b), t1.shape[0]))
        s1, t1, g1, d1 = run_xgcd(F, field, t, z(nz), z(n))
        assert d1[0] == -1 and not (s1.any() or t1.any() or g1.any())
    c5, c9 = R.from_ints(field, [5]), R.from_ints(field, [9])
    s1, t1, g1, d1 = run_xgcd(F, field, t, c5, c9)                     # xgcd of two constants: the first division leaves s = 0
    assert d1[0] == 0 and G.ints(field, g1) == [1] and G.check_xgcd(field, c5, c9, s1, t1, g1) == ""
    s1, t1, g1, d1 = run_xgcd(F, field, t, a, c9)
    assert d1[0] == 0 and np.array_equal(g1, pad(field, R.from_ints(field, [1]), n)) and G.check_xgcd(field, a, c9, s1, t1, g1) == ""
    s1, t1, g1, d1 = run_xgcd(F, field, t, a, a)
    assert d1[0] == n - 1 and np.array_equal(g1, monic(a)) and G.check_xgcd(field, a, a, s1, t1, g1) == ""


# ---- the step the feature exists for -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nr,nq", [(30, 15), (100, 100)])
def test_distinct_linear_factors_by_frobenius(oracle_mod, field, nr, nq):
    """f = prod (x - r_i) prod (x^2 + c_j^2) with p = 3 mod 4, so every quadratic is irreducible: gcd(f, x^p - x mod f) is exactly
    prod (x - r_i).  Needs no reference: pow_mod and gcd are both the GPU's."""
    assert P[field] % 4 == 3
    F, t = oracle_mod.field(field), tree(field, 4096)
    lin = W.from_roots(field, R.from_ints(field, [11 + 3 * i for i in range(nr)]))
    f = lin
    for c in range(1, nq + 1):
        f = R.mul_exact(field, f, R.from_ints(field, [c * c, 0, 1]))
    d = f.shape[0] - 1
    assert d == nr + 2 * nq and (d <= 64 or d > small_max())
    x = R.from_ints(field, [0, 1])
    w = to_std(F, t.poly_pow_mod(to_mem(F, x), P[field], to_mem(F, f)))
    wx = W._sub(field, w, pad(field, x, d))
    g, deg = t.poly_gcd(to_mem(F, f), to_mem(F, wx))
    assert deg[0] == nr and np.array_equal(to_std(F, g), pad(field, lin, d + 1))


# ---- the two regimes against each other and against the Euclidean algorithm -----------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_cross_path(oracle_mod, field):
    """one pair in rows of GCD_SMALL_MAX coefficients (the batched launch of the small regime) and zero-padded to rows above it (the
    host's path, which finds the true lengths and finishes a pair that fits the leaf in the same kernel, one launch per pair): the
    same bytes; and both against the quadratic reference at <= 65 coefficients.  The host recursion itself is compared with known
    answers in the tests around the leaf, not here: no input takes both the kernel and the recursion."""
    gm = small_max()
    F, t = oracle_mod.field(field), tree_for(field, 2 * gm)
    a, b = R.rand_std(field, gm - 1, 5), R.rand_std(field, gm - 4, 6)
    s0, t0, g0, d0 = run_xgcd(F, field, t, pad(field, a, gm), pad(field, b, gm))
    s1, t1, g1, d1 = run_xgcd(F, field, t, pad(field, a, gm + 1), pad(field, b, gm + 9))
    assert d0[0] == d1[0] and np.array_equal(pad(field, g0, g1.shape[0]), g1)
    assert np.array_equal(pad(field, s0, s1.shape[0]), s1) and np.array_equal(pad(field, t0, t1.shape[0]), t1)
    assert G.check_xgcd(field, a, b, s0, t0, g0) == ""
    for na, nb, seed in ((65, 65, 1), (40, 65, 2), (65, 3, 3), (5, 4, 4)):
        a, b = R.rand_std(field, na, seed), R.rand_std(field, nb, seed + 50)
        es, et, eg = G.eea(field, G.ints(field, a), G.ints(field, b))
        for extra in (0, gm + 1):                                          # in place, and in rows above the small regime
            s, tt, g, d = run_xgcd(F, field, t, pad(field, a, na + extra), pad(field, b, nb + extra))
            assert d[0] == len(eg) - 1 and np.array_equal(g, G.arr(field, eg, g.shape[0]))
            assert np.array_equal(s, G.arr(field, es, s.shape[0])) and np.array_equal(tt, G.arr(field, et, tt.shape[0]))


# ---- memory kinds, batching and the pool -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_mem_batching_and_null_outputs(oracle_mod, field):
    import torch
    from ecfft_amd import fftree as FT
    gm = small_max()
    F = oracle_mod.field(field)
    for n in (50, 2 * gm + 3):
        t = tree_for(field, n)
        pairs = [known_pair(field, n, n - 3, k, 7 + i) for i, k in enumerate(["half", "one", "zero"])]
        a, b = to_mem(F, np.concatenate([p[0] for p in pairs])), to_mem(F, np.concatenate([p[1] for p in pairs]))
        s, tt, g, deg = t.poly_xgcd(a, b, count=3)
        assert list(deg) == [p[2].shape[0] - 1 for p in pairs]
        for i in range(3):                                                 # count x rows == the same rows called singly
            s1, t1, g1, d1 = t.poly_xgcd(rows(a, 3, i), rows(b, 3, i))
            assert d1[0] == deg[i] and np.array_equal(g1, rows(g, 3, i)) and np.array_equal(s1, rows(s, 3, i)) and np.array_equal(t1, rows(tt, 3, i))
        da = torch.from_numpy(a.view(np.int64) if field == "secp256k1" else a.view(np.int32)).cuda()
        db = torch.from_numpy(b.view(np.int64) if field == "secp256k1" else b.view(np.int32)).cuda()
        ds, dt, dg, ddeg = t.poly_xgcd(da, db, count=3)                    # MEM_DEVICE == MEM_HOST
        assert np.array_equal(ddeg, deg)
        for dev, host in ((ds, s), (dt, tt), (dg, g)):
            assert np.array_equal(dev.cpu().numpy().view(host.dtype).reshape(host.shape), host)
        # degrees = NULL, s or t NULL, through the C ABI
        L, h = t._L, t._h
        for ps, pt in ((None, None), (1, None), (None, 1)):
            os_, ot, og = np.zeros_like(s), np.zeros_like(tt), np.zeros_like(g)
            rc = L.ecfft_poly_xgcd(h, a.ctypes.data, n, b.ctypes.data, n - 3, os_.ctypes.data if ps else None, ot.ctypes.data if pt else None,
                                   og.ctypes.data, None, 3, FT.MEM_HOST, None)
            assert rc == FT.OK and np.array_equal(og, g)
            assert np.array_equal(os_, s) if ps else not os_.any()
            assert np.array_equal(ot, tt) if pt else not ot.any()
        og = np.zeros_like(g)
        assert L.ecfft_poly_gcd(h, a.ctypes.data, n, b.ctypes.data, n - 3, og.ctypes.data, None, 3, FT.MEM_HOST, None) == FT.OK
        assert np.array_equal(og, g)


@pytest.mark.parametrize("field", FIELDS)
def test_repeated_use_and_trim(oracle_mod, field):
    """the pool after 2 and after 10 large-regime calls is the same size, and ecfft_ctx_trim gives it back"""
    import ecfft_amd
    n = 4 * small_max() + 3
    t = ecfft_amd.FIELDS[field].build_fftree(4096)
    F = oracle_mod.field(field)
    a, b, g = known_pair(field, n, n - 1, "one", 3)
    am, bm = to_mem(F, a), to_mem(F, b)
    t.poly_xgcd(am, bm)                                                    # the transform scratch (grow-only, not a temporary) reaches its size:
                                                                           # the eight products of a matrix product are one batch
    t.trim()
    before = t.device_bytes
    first = t.poly_xgcd(am, bm)
    t.poly_xgcd(am, bm)
    held = t.device_bytes
    for _ in range(8):
        again = t.poly_xgcd(am, bm)
    assert t.device_bytes == held
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    t.trim()
    assert t.device_bytes == before
    assert np.array_equal(t.poly_gcd(am, bm)[0], first[2])


# ---- around the hand-over of the half-GCD to the kernel ----------------------------------------------------------------------------
def leaf_max(field):
    """kGcdLeaf of ecfft_amd/csrc/device_tree.h: a node, or what is left of a pair, of at most this many coefficients is one launch of
    k_gcd_small (1024 threads for M31, 512 for secp256k1); read from the source so that the sizes below follow it"""
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "ecfft_amd", "csrc", "device_tree.h")).read()
    m = re.search(r"kGcdLeaf = sizeof\(E\) == 4 \? (\d+) : (\d+);", src)
    return int(m.group(1)) if field == "m31" else int(m.group(2))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("idx", range(6))
def test_known_gcd_around_the_leaf(oracle_mod, field, idx):
    """the sizes at which the host recursion takes over from the kernel, per field: L - 1 and L finish in one launch, L + 1 is one
    node with two leaves, 2L + 1 and 4L + 3 recurse twice and more; gcd byte for byte, cofactors unique by check_xgcd"""
    L = leaf_max(field)
    assert L >= small_max()
    nmax = [L - 1, L, L + 1, L + 2, 2 * L + 1, 4 * L + 3][idx]
    F, t = oracle_mod.field(field), tree_for(field, nmax)
    for order, kind in ((ORDERS[idx % 3], KINDS[idx % 4]), (ORDERS[(idx + 1) % 3], KINDS[(idx + 2) % 4])):
        na, nb = lengths(nmax, order)
        a, b, g0 = known_pair(field, na, nb, kind, 300 + idx)
        s, tt, g, deg = run_xgcd(F, field, t, a, b)
        assert deg[0] == g0.shape[0] - 1 and np.array_equal(g, pad(field, g0, nmax)), (nmax, order, kind)
        assert G.check_xgcd(field, a, b, s, tt, g) == "", (nmax, order, kind)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("case", ["above_leaf", "big_quotient_2l", "split_point_4l"])
def test_prescribed_quotient_sequences_around_the_leaf(oracle_mod, field, case):
    """abnormal sequences sized from the leaf: total degree just above L, a quotient of L + 7 inside 2L, and at 4L one large quotient
    exactly on the top split point (the remainder it divides by has degree m); g, s and t byte for byte"""
    L = leaf_max(field)
    big = L + 7
    degs = {"above_leaf": fill([2, 1, 40, 3, 1, 1, 2, 1], L + 11),
            "big_quotient_2l": fill([1, 2, 1, 3], L // 2) + [big] + fill([1, 1, 2, 40, 1], L // 2 - 7),
            "split_point_4l": fill([1, 3, 2, 1, 40, 1], 2 * L) + [big] + fill([2, 1, 1, 3], 2 * L - big)}[case]
    qs = [G.rand_poly(field, d + 1, 2000 + 11 * i + d) for i, d in enumerate(degs)]
    g = G.rand_poly(field, 2, 97, monic=True)
    r0, r1, s, tt = G.from_quotients(field, g, qs)
    if case == "split_point_4l":
        assert len(r0) - 1 == 4 * L + 1 and sum(degs[:degs.index(big)]) == 2 * L       # m = ceil((4L + 1) / 2) = 2L + 1 = deg of the divisor
    F, t = oracle_mod.field(field), tree_for(field, len(r0))
    gs, gt, gg, deg = run_xgcd(F, field, t, G.arr(field, r0), G.arr(field, r1))
    assert deg[0] == 1 and np.array_equal(gg, G.arr(field, g, len(r0)))
    assert np.array_equal(gs, G.arr(field, s, max(len(r1) - 1, 1))) and np.array_equal(gt, G.arr(field, tt, len(r0) - 1))


# ---- the tree rule at its minimum ------------------------------------------------------------------------------------------------
def rule_leaves(nmax):
    """include/ecfft_hip.h: next_pow2(2 nmax - 1) leaves above GCD_SMALL_MAX"""
    n = 1
    while n < 2 * nmax - 1:
        n <<= 1
    return n


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", [(300, 3), (300, 2), (512, 2), (512, 3), (1366, 3), (1025, 40), (683, 1)])
def test_short_second_operand_on_the_minimum_tree(oracle_mod, field, na, nb):
    """a second operand of low degree makes the first division a quotient of almost na coefficients: the largest transforms the call
    runs.  On exactly the rule's tree, one size below it ECFFT_ERR_TREE_TOO_SMALL; the cofactors are unique by their degree bounds"""
    from ecfft_amd import fftree as FT
    F, need = oracle_mod.field(field), rule_leaves(na)
    t, small = tree(field, need), tree(field, need // 2)
    a, b = R.rand_std(field, na, na + nb, specials=False), R.rand_std(field, nb, na - nb, specials=False)
    R.set_nonzero(field, a, na - 1)
    R.set_nonzero(field, b, nb - 1)
    for x, y in ((a, b), (b, a), (pad(field, a, na), pad(field, b, na))):   # either order, and b in a row as long as a's
        s, tt, g, deg = run_xgcd(F, field, t, x, y)
        eg = G.gcd(field, G.ints(field, a), G.ints(field, b))
        assert deg[0] == len(eg) - 1 and np.array_equal(g, G.arr(field, eg, g.shape[0]))
        assert G.check_xgcd(field, x, y, s, tt, g) == ""
    am, bm = to_mem(F, a), to_mem(F, b)
    out = np.zeros_like(am)
    assert small._L.ecfft_poly_gcd(small._h, am.ctypes.data, na, bm.ctypes.data, nb, out.ctypes.data, None, 1, FT.MEM_HOST, None) == FT.ERR_TREE_TOO_SMALL


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("first,rest", [(290, 9), (500, 11), (380, 300)])
def test_huge_first_quotient_on_the_minimum_tree(oracle_mod, field, first, rest):
    """one quotient of `first` coefficients' degree before a normal tail, on exactly the rule's tree: g, s and t byte for byte"""
    degs = [first] + fill([1, 2, 1, 3], rest)
    qs = [G.rand_poly(field, d + 1, 500 + 7 * i + d) for i, d in enumerate(degs)]
    g = G.rand_poly(field, 3, 98, monic=True)
    r0, r1, s, tt = G.from_quotients(field, g, qs)
    F, t = oracle_mod.field(field), tree(field, rule_leaves(len(r0)))
    gs, gt, gg, deg = run_xgcd(F, field, t, G.arr(field, r0), G.arr(field, r1))
    assert deg[0] == 2 and np.array_equal(gg, G.arr(field, g, len(r0)))
    assert np.array_equal(gs, G.arr(field, s, max(len(r1) - 1, 1))) and np.array_equal(gt, G.arr(field, tt, len(r0) - 1))


# ---- errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_errors(oracle_mod, field):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    gm = small_max()
    F = oracle_mod.field(field)
    n = gm + 1                                                             # the header's rule: next_pow2(2 n - 1) leaves
    need = rule_leaves(n)
    a, b, g = known_pair(field, n, n - 2, "half", 1)
    am, bm = to_mem(F, a), to_mem(F, b)
    out, st = np.zeros_like(am), np.zeros_like(am)
    deg = np.zeros(1, np.int64)
    small, enough = tree(field, need // 2), tree(field, need)
    args = lambda t, pa, na, pb, nb, pg, count=1: (t._h, pa, na, pb, nb, pg, deg.ctypes.data, count, FT.MEM_HOST, None)
    L = small._L
    assert L.ecfft_poly_gcd(*args(small, am.ctypes.data, n, bm.ctypes.data, n - 2, out.ctypes.data)) == FT.ERR_TREE_TOO_SMALL
    assert L.ecfft_poly_xgcd(small._h, am.ctypes.data, n, bm.ctypes.data, n - 2, st.ctypes.data, st.ctypes.data, out.ctypes.data, None, 1,
                             FT.MEM_HOST, None) == FT.ERR_TREE_TOO_SMALL
    # the small regime needs no tree at all, and the context keeps working after the error
    g1, d1 = small.poly_gcd(am[:gm], bm[:gm])
    assert d1[0] >= 0
    g2, d2 = enough.poly_gcd(am, bm)
    assert d2[0] == g.shape[0] - 1 and np.array_equal(to_std(F, g2), pad(field, g, n))
    for n2 in (gm + 1, 3 * gm, 4 * gm + 1):                                # next_pow2(2 nmax) leaves are always enough
        a2, b2, _ = known_pair(field, n2, n2, "zero", n2)
        assert tree_for(field, n2).poly_gcd(to_mem(F, a2), to_mem(F, b2))[1][0] == 0
    t = enough
    assert L.ecfft_poly_gcd(*args(t, None, n, bm.ctypes.data, n, out.ctypes.data)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_gcd(*args(t, am.ctypes.data, n, None, n, out.ctypes.data)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_gcd(*args(t, am.ctypes.data, n, bm.ctypes.data, n - 2, None)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_gcd(*args(t, am.ctypes.data, 0, bm.ctypes.data, n - 2, out.ctypes.data)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_gcd(*args(t, am.ctypes.data, n, bm.ctypes.data, 0, out.ctypes.data)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_gcd(*args(t, am.ctypes.data, n, bm.ctypes.data, n - 2, out.ctypes.data, count=0)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_gcd(*args(t, am.ctypes.data, n, bm.ctypes.data, n - 2, out.ctypes.data, count=(1 << 62))) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_gcd(t._h, am.ctypes.data, n, bm.ctypes.data, n - 2, out.ctypes.data, None, 1, 7, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_xgcd(t._h, am.ctypes.data, n, bm.ctypes.data, n - 2, st.ctypes.data, st.ctypes.data, None, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    shard = ecfft_amd.FIELDS[field].build_extend_shard(1024, 1, 0)         # EXTEND-only context: holds no full tree
    assert L.ecfft_poly_gcd(*args(shard, am.ctypes.data, 8, bm.ctypes.data, 8, out.ctypes.data)) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_xgcd(shard._h, am.ctypes.data, 8, bm.ctypes.data, 8, st.ctypes.data, st.ctypes.data, out.ctypes.data, None, 1,
                             FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    with pytest.raises(ValueError):
        t.poly_gcd(am[:0], bm)
    g3, d3 = t.poly_gcd(am, bm)
    assert np.array_equal(g3, g2) and d3[0] == d2[0]
