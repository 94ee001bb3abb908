"""GPU tests of the polynomial operations (ecfft_poly_mul, ecfft_poly_divrem, ecfft_poly_inv_series, ecfft_poly_eval_points) in every
dispatch regime of device_tree.h, against exact references (tests/poly_ref.py: the Kronecker product on Python ints, the division and
series identities built on it) and, above the sizes where the exact product is affordable, Schwartz-Zippel (SZ) identities at seeded
points of [0, p) evaluated with the oracle's Horner.  Inputs are full-range (secp256k1: uniform below p, [2^255, p) included) with
0, 1, p - 1 and runs of zero coefficients mixed in.

The regimes (T = the elements of one launch; N = next_pow2 of the product a case forms):

  row  rule                                     where                   secp256k1 (32-byte elements)          M31
  A    small tiles (256)                        small_launch,           one stream, 2^8 <= T < 2^19           never
                                                log_low_for             (< 2^18 inside the two-halves form)
  B    large tiles (+ 32x32 int8 matrix-core    use_blk16, low16        T >= 2^19 on one stream               column passes once an EXTEND
       phases on secp256k1)                                                                                   spans more than one 2^13 tile
  C    two half-batches on two streams          batch_ways              count even and T/2 >= 2^19            same
  D    two-halves schedule of one transform     exit / enter,           count = 1, N >= 2^19                  same
                                                kSplitMinLog = 19
  E    lifts                                    lift_operands           one EXTEND per doubling from each operand's own size up to N/2

A call spans several rows: its lifts run at every size from the operand size up to N/2 (row E always), its ENTERs at the operand sizes
and its EXIT at N, on count (or 2 count, when both operands are lifted together) vectors.  The rows each case reaches, derived from
those rules, are in its label (the test id).  On M31 the profiler confirms row B: a case with N >= 2^15 records k_stages_col launches,
one with N <= 2^13 records none.

Checks (coverage conditions): every pair of a case whose largest product (poly_mul: na + nb - 1, poly_divrem: b q, that is na,
poly_inv_series: (f mod x^k) g) has at most 2^15 (secp256k1) / 2^17 (M31) coefficients is checked exactly; above that every pair gets
SZ and the pairs 0, count/2 - 1, count/2, count - 1 are also checked exactly while their product has at most 2^16 / 2^18 coefficients.
A pair with a short operand (<= 64 coefficients) is always checked exactly: its product costs (long / short) short products.
poly_eval_points is compared with Horner at every point while m nf <= 2^28 per polynomial; above that at one point of every 64-point
leaf block (nf <= 2^17) plus a seeded spread of >= 1024 points with the first and last point of every group and every special point.

The exact references run in a process pool (spawn, at most 8 workers, started with the first test of the module): Python-int
multiplication holds the GIL.  The jobs are poly_ref functions: the workers never import torch or the GPU library."""
import ctypes
import os
from concurrent.futures import ProcessPoolExecutor
import multiprocessing

import numpy as np
import pytest

import poly_ref as R
from conftest import horner_mt, spread_indices, std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
EXACT = {"secp256k1": 1 << 15, "m31": 1 << 17}          # every pair exact up to this product size
EXACT_EDGE = {"secp256k1": 1 << 16, "m31": 1 << 18}     # the boundary pairs exact up to this product size
SHORT = 64                                              # a product with an operand this short is always checked exactly
TREE = {"secp256k1": 1 << 20, "m31": 1 << 23}

_trees = {}


def tree(field):
    import ecfft_amd
    if field not in _trees:
        _trees[field] = ecfft_amd.FIELDS[field].build_fftree(TREE[field])
    return _trees[field]


@pytest.fixture(scope="module", autouse=True)
def pool():
    """the reference workers, started with the first test of the module and warm by the time the first GPU result is back"""
    ex = ProcessPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1)), mp_context=multiprocessing.get_context("spawn"))
    warm = [ex.submit(R.sz_count, "m31", 2) for _ in range(8)]
    yield ex
    for w in warm:
        w.result()
    ex.shutdown()


# ---- conversions -----------------------------------------------------------------------------------------------------------------------
def to_std(F, x):
    """in-memory (Montgomery for secp256k1) -> standard form, the oracle's converter on the whole array"""
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


def oracle_horner(F):
    """poly_ref's horner interface (standard form in, Python ints out) on the oracle's C Horner, points split over host threads"""
    def h(c, zs):
        return R.to_ints(F.name, to_std(F, horner_mt(F, to_mem(F, c), to_mem(F, zs), threads=len(zs))))
    return h


def edges(count):
    return sorted({i for i in (0, count // 2 - 1, count // 2, count - 1) if 0 <= i < count})


def exact_pairs(field, count, size, short):
    """the pairs checked exactly: all, the boundary pairs or none (see the module docstring)"""
    if size <= EXACT[field] or short <= SHORT:
        return list(range(count))
    return edges(count) if size <= EXACT_EDGE[field] else []


def gather(jobs):
    """wait for every reference job; assert each reported nothing"""
    bad = [f"{label}: {msg}" for label, fut in jobs for msg in [fut.result()] if msg]
    assert not bad, "\n".join(bad)


def assert_canonical(field, *xs):
    for x in xs:
        assert R.canonical(field, x).all(), "an output coefficient is >= p"


# ---- poly_mul ---------------------------------------------------------------------------------------------------------------------------
# (field, na, nb, count, rows reached)
MUL_CASES = [
    ("secp256k1", 100003, 150001, 1, "A-E"),             # N = 2^18: a lifted from 2^17, b entered at N; every launch < 2^19
    ("secp256k1", 3, (1 << 19) - 2, 1, "A-D-E"),         # N = 2^19: b entered at N on the two-halves schedule, a lifted alone 4 -> 2^18
    ("secp256k1", (1 << 17) - 1, (1 << 17) - 2, 3, "B-E"),   # N = 2^18, odd count: one stream, joint ENTER of 6 x 2^17
    ("secp256k1", (1 << 16) - 7, (1 << 16) + 5, 4, "A-B-E"),  # N = 2^17: b entered at N on 2^19 elements, T/2 < 2^19: one stream
    ("secp256k1", 1 << 16, (1 << 16) - 1, 8, "B-C-E"),   # N = 2^17: 8 x 2^17, two half-batches
    ("secp256k1", (1 << 19) + 3, (1 << 19) - 5, 2, "B-C-E"),   # N = 2^20
    ("secp256k1", (1 << 14) - 1, (1 << 14) - 2, 16, "B-E"),    # N = 2^15 x 16 pairs = 2^19 on one stream: large tiles, exact
    ("secp256k1", (1 << 14) - 1, 301, 32, "B-C-E"),      # N = 2^15 x 32 pairs: two half-batches, exact
    ("m31", 5000, 3000, 1, "E"),                          # N = 2^13: one tile, no column pass
    ("m31", 9000, 7001, 1, "B-E"),                        # N = 2^14
    ("m31", 9000, 7001, 3, "B-E"),
    ("m31", 40000, 25000, 1, "B-E"),                      # N = 2^16
    ("m31", 40000, 25000, 3, "B-E"),
    ("m31", 150000, 100000, 1, "B-E"),                    # N = 2^18
    ("m31", 150000, 100000, 3, "B-E"),
    ("m31", 1 << 17, (1 << 17) - 1, 4, "B-C-E"),          # N = 2^18 x 4: two half-batches
    ("m31", 600000, 448577, 1, "B-D-E"),                  # N = 2^20: two-halves schedule
    ("m31", 600000, 448577, 2, "B-C-E"),
]


def _id(c):
    return "-".join(str(x) for x in c)


@pytest.mark.parametrize("case", MUL_CASES, ids=_id)
def test_poly_mul_regimes(oracle_mod, pool, case):
    field, na, nb, count, _ = case
    F, t = oracle_mod.field(field), tree(field)
    a = R.rand_std(field, count * na, na * 3 + count)
    b = R.rand_std(field, count * nb, nb * 5 + count)
    nc = na + nb - 1
    N = 1 << (nc - 1).bit_length()
    if field == "m31":
        t.profile(True)
    c = t.poly_mul(to_mem(F, a), to_mem(F, b), count=count)
    if field == "m31":
        cols = sum(r["launches"] for r in t.profile_read() if r["name"] == "k_stages_col")
        t.profile(False)
        if N <= 1 << 13:                                              # row B on M31: column passes once an EXTEND spans > 2^13
            assert cols == 0, cols
        if N >= 1 << 15:
            assert cols > 0
    assert c.shape[0] == count * nc
    assert_canonical(field, c)
    cs = to_std(F, c)
    ex = exact_pairs(field, count, nc, min(na, nb))
    jobs = [(f"pair {i} exact", pool.submit(R.check_mul, field, rows(a, count, i), rows(b, count, i), rows(cs, count, i))) for i in ex]
    if nc > EXACT[field] and min(na, nb) > SHORT:
        h = oracle_horner(F)
        for i in range(count):
            zs = R.sz_points(field, R.sz_count(field, nc), 1000 + i)
            msg = R.sz_mul(field, rows(a, count, i), rows(b, count, i), rows(cs, count, i), zs, h)
            assert msg == "", f"pair {i} SZ: {msg}"
    gather(jobs)


# ---- poly_divrem ------------------------------------------------------------------------------------------------------------------------
# (field, na, nb, count, rows): tree rule N = next_pow2(max(2 nq - 1, nr + min(nq, nr) - 1))
DIV_CASES = [
    # long quotient, short divisor: the reciprocal's Newton steps up to N = next_pow2(2 nq - 1)
    ("secp256k1", (1 << 17) + 1000, 7, 1, "A-D-E"),       # N = 2^19
    ("secp256k1", 40000, 5, 3, "A-B-E"),                  # N = 2^17 x 3
    ("secp256k1", (1 << 18) + 100, 3, 2, "A-B-C-E"),      # N = 2^20 x 2
    # nq ~ nr, both large
    ("secp256k1", 40000, 20001, 1, "A-E"),                # N = 2^16
    ("secp256k1", 1 << 16, (1 << 15) + 1, 5, "A-B-E"),    # N = 2^17 x 5: one stream
    ("secp256k1", 1 << 18, (1 << 17) + 1, 4, "A-B-C-E"),  # N = 2^18 x 4: two half-batches
    ("secp256k1", 300000, 150001, 1, "A-D-E"),            # N = 2^19
    # short quotient, long remainder product: N = next_pow2(nr + nq - 1)
    ("secp256k1", (1 << 18) + 40, 1 << 18, 1, "A-D-E"),   # N = 2^19
    ("secp256k1", 70030, 70000, 3, "A-B-E"),              # N = 2^17 x 3
    ("secp256k1", (1 << 18) + 20, (1 << 18) - 10, 2, "A-B-C-E"),   # N = 2^19 x 2
    ("m31", (1 << 18) + 1000, 7, 1, "B-D-E"),             # N = 2^20
    ("m31", 150000, 5, 3, "B-E"),                         # N = 2^19 x 3
    ("m31", (1 << 19) + 100, 3, 2, "B-C-E"),              # N = 2^21 x 2
    ("m31", 1 << 17, (1 << 16) + 1, 1, "B-E"),            # N = 2^17
    ("m31", 1 << 18, (1 << 17) + 1, 3, "B-E"),            # N = 2^18 x 3
    ("m31", 1 << 19, (1 << 18) + 1, 4, "B-C-E"),          # N = 2^19 x 4
    ("m31", (1 << 19) + 40, 1 << 19, 1, "B-D-E"),         # N = 2^20
    ("m31", 100030, 100000, 3, "B-E"),                    # N = 2^17 x 3
    ("m31", (1 << 18) + 20, (1 << 18) - 10, 2, "B-C-E"),  # N = 2^19 x 2
]


def divrem_inputs(field, na, nb, count, seed):
    a = R.rand_std(field, count * na, seed)
    b = R.set_nonzero(field, R.rand_std(field, count * nb, seed + 1), np.arange(count) * nb + nb - 1)
    return a, b


def check_divrem_case(F, field, pool, a, b, q, r, count, label=""):
    na, nb = a.shape[0] // count, b.shape[0] // count
    nq = max(na - nb + 1, 0)
    assert q.shape[0] == count * nq and r.shape[0] == count * (nb - 1)
    assert_canonical(field, q, r)
    qs, rs = to_std(F, q), to_std(F, r)
    ex = exact_pairs(field, count, na, min(nb, nq))
    jobs = [(f"{label}pair {i} exact", pool.submit(R.check_divrem, field, rows(a, count, i), rows(b, count, i),
                                                   rows(qs, count, i) if nq else qs[:0], rows(rs, count, i) if nb > 1 else rs[:0])) for i in ex]
    if set(ex) != set(range(count)):
        h = oracle_horner(F)
        for i in range(count):
            zs = R.sz_points(field, R.sz_count(field, na), 2000 + i)
            msg = R.sz_divrem(field, rows(a, count, i), rows(b, count, i), rows(qs, count, i), rows(rs, count, i), zs, h)
            assert msg == "", f"{label}pair {i} SZ: {msg}"
    gather(jobs)


@pytest.mark.parametrize("case", DIV_CASES, ids=_id)
def test_poly_divrem_regimes(oracle_mod, pool, case):
    field, na, nb, count, _ = case
    F, t = oracle_mod.field(field), tree(field)
    a, b = divrem_inputs(field, na, nb, count, na + 7 * nb + count)
    q, r = t.poly_divrem(to_mem(F, a), to_mem(F, b), count=count)
    check_divrem_case(F, field, pool, a, b, q, r, count)


# ---- poly_inv_series --------------------------------------------------------------------------------------------------------------------
# (field, nf, k, count, rows): the last Newton step runs on N = next_pow2(2k - 1)
INV_CASES = [
    ("secp256k1", 5000, 8191, 1, "A-E"),                  # N = 2^14
    ("secp256k1", 10000, 8193, 3, "A-E"),                 # N = 2^15 x 3
    ("secp256k1", 1000, (1 << 16) - 1, 1, "A-E"),         # N = 2^17
    ("secp256k1", 70000, (1 << 16) + 1, 8, "A-B-C-E"),    # N = 2^18 x 8: two half-batches
    ("secp256k1", 300000, 1 << 18, 1, "A-D-E"),           # N = 2^19
    ("secp256k1", 1 << 17, (1 << 18) + 1, 2, "A-B-C-E"),  # N = 2^20 x 2
    ("m31", 5000, 8192, 1, "B-E"),                        # N = 2^14
    ("m31", 20000, 8193, 3, "B-E"),                       # N = 2^15 x 3
    ("m31", 70000, 1 << 16, 2, "B-E"),                    # N = 2^17 x 2
    ("m31", 1000, (1 << 18) - 1, 3, "B-E"),               # N = 2^19 x 3
    ("m31", 1 << 21, (1 << 18) + 1, 4, "B-C-E"),          # N = 2^20 x 4
    ("m31", 1 << 19, 1 << 20, 1, "B-D-E"),                # N = 2^21
    ("m31", 100, (1 << 20) - 3, 2, "B-C-E"),              # N = 2^21 x 2
]


def check_inv_case(F, field, pool, f, g, k, count, label=""):
    nf = f.shape[0] // count
    assert g.shape[0] == count * k
    assert_canonical(field, g)
    gs = to_std(F, g)
    size = min(nf, k) + k - 1
    ex = exact_pairs(field, count, size, min(nf, k))
    jobs = [(f"{label}pair {i} exact", pool.submit(R.check_inv_series, field, rows(f, count, i), rows(gs, count, i))) for i in ex]
    if set(ex) != set(range(count)):
        for i in range(count):
            zs = R.sz_points(field, R.sz_count(field, k), 3000 + i)
            jobs.append((f"{label}pair {i} SZ", pool.submit(R.sz_inv_series, field, rows(f, count, i), rows(gs, count, i), zs)))
    gather(jobs)


@pytest.mark.parametrize("case", INV_CASES, ids=_id)
def test_poly_inv_series_regimes(oracle_mod, pool, case):
    field, nf, k, count, _ = case
    F, t = oracle_mod.field(field), tree(field)
    f = R.set_nonzero(field, R.rand_std(field, count * nf, nf + k + count), np.arange(count) * nf)
    g = t.poly_inv_series(to_mem(F, f), k, count=count)
    check_inv_case(F, field, pool, f, g, k, count)


# ---- the second grid chunk of series_base (more than 2^16 pairs) ----------------------------------------------------------------------
CHUNKED = (1 << 16) + 3


def _chunked_jobs(pool, kind, field, count, *arrays):
    """exact checks of every pair, in 8 slices of whole pairs"""
    bounds = np.linspace(0, count, 9).astype(int)
    jobs = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        sl = [x[lo * (x.shape[0] // count):hi * (x.shape[0] // count)] for x in arrays]
        jobs.append((f"pairs {lo}..{hi - 1}", pool.submit(R.check_many, kind, field, int(hi - lo), int(lo), *sl)))
    return jobs


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nf,k", [(40, 64), (100, 37), (1, 64)])
def test_inv_series_chunked(oracle_mod, pool, field, nf, k):
    """count = 2^16 + 3 series with k <= 64: k_series_base alone, in two grid chunks; a zero f_0 in a pair of the second chunk is
    reported"""
    F, t = oracle_mod.field(field), tree(field)
    f = R.set_nonzero(field, R.rand_std(field, CHUNKED * nf, nf * 17 + k), np.arange(CHUNKED) * nf)
    g = t.poly_inv_series(to_mem(F, f), k, count=CHUNKED)
    assert g.shape[0] == CHUNKED * k
    assert_canonical(field, g)
    jobs = _chunked_jobs(pool, "inv_series", field, CHUNKED, f, to_std(F, g))
    z = f.copy()
    z[(CHUNKED - 2) * nf] = 0
    with pytest.raises(ValueError, match="constant coefficient"):
        t.poly_inv_series(to_mem(F, z), k, count=CHUNKED)
    gather(jobs)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", [(37, 1), (5, 9)])
def test_divrem_chunked(oracle_mod, pool, field, na, nb):
    """count = 2^16 + 3 pairs with nb = 1 (q = a / b_0) and with na < nb (r = a): the divisors' leading coefficients are inverted by
    k_series_base in two grid chunks; a zero one in a pair of the second chunk is reported"""
    F, t = oracle_mod.field(field), tree(field)
    a, b = divrem_inputs(field, na, nb, CHUNKED, na * 19 + nb)
    q, r = t.poly_divrem(to_mem(F, a), to_mem(F, b), count=CHUNKED)
    nq = max(na - nb + 1, 0)
    assert q.shape[0] == CHUNKED * nq and r.shape[0] == CHUNKED * (nb - 1)
    assert_canonical(field, q, r)
    if nq:                                                                    # nb = 1: r is empty and b_0 q == a
        jobs = _chunked_jobs(pool, "mul", field, CHUNKED, b, to_std(F, q), a)
    else:                                                                     # na < nb: q is empty and r == a, zero-padded
        jobs = []
        rs = to_std(F, r)
        want = np.zeros(R.shape(field, CHUNKED * (nb - 1)), R.dtype(field)).reshape((CHUNKED, nb - 1) + a.shape[1:])
        want[:, :na] = a.reshape((CHUNKED, na) + a.shape[1:])
        assert np.array_equal(rs, want.reshape(rs.shape))
    z = b.copy()
    z[(CHUNKED - 2) * nb + nb - 1] = 0
    with pytest.raises(ValueError, match="leading coefficient"):
        t.poly_divrem(to_mem(F, a), to_mem(F, z), count=CHUNKED)
    gather(jobs)


# ---- poly_eval_points -------------------------------------------------------------------------------------------------------------------
# (field, nf, m, count, rows): G = next_pow2(nf) points per group; the tree's levels run EXITs of 2d on P / d nodes, the descent
# EXITs of 2d on count P / d rows and lifts of d on count P / 2d rows, d = 64 .. G/2 (P = m rounded up to groups)
EVAL_CASES = [
    ("secp256k1", 9000, (1 << 14) + (1 << 13) + 777, 3, "A-E"),      # m nf <= 2^28: Horner at every point
    ("secp256k1", (1 << 17) - 5, (1 << 17) + (1 << 16) + 11, 2, "A-B-C-E"),
    ("secp256k1", (1 << 20) - 100, (1 << 20) + 3000, 1, "A-B-C-E"),
    ("m31", 12000, 3 * (1 << 14) + 5, 1, "B-E"),
    ("m31", 100000, 2 * (1 << 17) + 999, 3, "B-C-E"),
    ("m31", (1 << 20) - 7, (1 << 20) + (1 << 19) + 1, 2, "B-C-E"),
    # more than 2^22 points: the lowest level of the subproduct tree has > 2^16 nodes of 64 points (chunked k_series_base)
    ("secp256k1", 8193, (1 << 22) + (1 << 14) + 3, 1, "A-B-C-E"),
    ("m31", 8193, (1 << 22) + (1 << 14) + 3, 2, "B-C-E"),
]


def eval_points(F, field, t, m, G, seed):
    """full-range random points with repeats, 0, 1, p - 1 and a permuted subset of T_G's leaves with repeats (in-memory form);
    returns (points, positions of the special points)"""
    rng = np.random.default_rng(seed)
    x = to_mem(F, R.rand_std(field, m, seed, specials=False))
    n_sp = min(m // 8, 4096)
    pos = rng.choice(m, 4 * n_sp, replace=False)
    sp = np.split(pos, 4)
    x[sp[0]] = x[rng.integers(0, m, n_sp)]                                  # repeats
    x[sp[1]] = to_mem(F, R.from_ints(field, [0, 1, R.P[field] - 1]))[np.arange(n_sp) % 3]     # sp[1][:3] holds 0, 1, p - 1
    leaves = t.leaves(G)
    x[sp[2]] = leaves[rng.permutation(max(G, n_sp))[:n_sp] % G]
    x[sp[3]] = leaves[rng.integers(0, G, n_sp)]                            # leaves again, with repeats
    return x, np.concatenate([sp[1][:3], sp[1][3::64], sp[2][::16], sp[3][::16], sp[0][::16]])


def eval_indices(nf, m, G, special, seed):
    """the points compared with Horner (module docstring): `special` holds one position of each special value and a sample of
    the other special positions"""
    if m * nf <= 1 << 28:
        return np.arange(m)
    idx = [spread_indices(m, 1024, seed), special, np.arange(0, m, G), np.arange(G - 1, m, G), [m - 1]]
    if nf <= 1 << 17:
        rng = np.random.default_rng(seed + 1)
        blocks = np.arange(0, m, 64)
        idx.append(np.minimum(blocks + rng.integers(0, 64, blocks.shape[0]), m - 1))
    return np.unique(np.concatenate([np.asarray(i, dtype=np.int64) for i in idx]))


@pytest.mark.parametrize("case", EVAL_CASES, ids=_id)
def test_poly_eval_points_regimes(oracle_mod, case):
    field, nf, m, count, _ = case
    F, t = oracle_mod.field(field), tree(field)
    G = 1 << (nf - 1).bit_length()
    f = to_mem(F, R.rand_std(field, count * nf, nf + m))
    x, special = eval_points(F, field, t, m, G, m + count)
    got = t.poly_eval_points(f, x, count=count)
    assert got.shape[0] == count * m
    assert_canonical(field, got)
    for b in range(count):
        idx = eval_indices(nf, m, G, special, 77 + b)
        want = horner_mt(F, f[b * nf:(b + 1) * nf], x[idx])
        bad = np.flatnonzero((got[b * m:(b + 1) * m][idx] != want).reshape(len(idx), -1).any(axis=1))
        assert bad.size == 0, f"polynomial {b}: {bad.size} of {len(idx)} points differ, first point {idx[bad[0]]}"


# ---- forced regimes at small sizes (hooks build) --------------------------------------------------------------------------------------
FORCED = [("ECFFT_NO_SMALL_TILES",), ("ECFFT_NO_SMALL_TILES", "ECFFT_NO_MFMA"), ("ECFFT_NO_SMALL_TILES", "ECFFT_NO_LOW16"),
          ("ECFFT_NO_MFMA",), ("ECFFT_NO_LOW16",), ("ECFFT_NO_ROW256", "ECFFT_NO_COL256")]


def test_forced_regimes_small_sizes(oracle_mod, pool, hooks_lib, monkeypatch):
    """secp256k1 products of 2^11 .. 2^14 coefficients on contexts built with the A/B switches of the hooks build (read when a context
    is built): the large-tile and matrix-core forms (ECFFT_NO_SMALL_TILES), their VALU forms, and the generic small kernels.  The
    default form is checked against the exact reference and every other form must equal it bit for bit, so each matches the reference"""
    import ecfft_amd
    field = "secp256k1"
    F = oracle_mod.field(field)
    P = ecfft_amd.FIELDS[field]
    mul_shapes = [(1000, 900, 1), (1500, 700, 1), (5000, 3000, 3), (9000, 7000, 1), (2048, 2048, 2)]      # N = 2^11 .. 2^14
    ins = [(R.rand_std(field, c * na, na + 1), R.rand_std(field, c * nb, nb + 2), c) for na, nb, c in mul_shapes]
    da, db = divrem_inputs(field, 6000, 2500, 2, 91)
    fs = R.set_nonzero(field, R.rand_std(field, 2 * 3000, 92), np.array([0, 3000]))
    mem = [(to_mem(F, a), to_mem(F, b), c) for a, b, c in ins]
    mda, mdb, mfs = to_mem(F, da), to_mem(F, db), to_mem(F, fs)

    def run(t):
        return [t.poly_mul(a, b, count=c) for a, b, c in mem] + list(t.poly_divrem(mda, mdb, count=2)) + [t.poly_inv_series(mfs, 4000, count=2)]

    base = run(P.build_fftree(1 << 14))
    assert_canonical(field, *base)
    jobs = []
    for (a, b, c), out in zip(ins, base):
        cs = to_std(F, out)
        jobs += [(f"mul {a.shape[0] // c}x{b.shape[0] // c} pair {i}", pool.submit(R.check_mul, field, rows(a, c, i), rows(b, c, i), rows(cs, c, i))) for i in range(c)]
    q, r, g = to_std(F, base[-3]), to_std(F, base[-2]), to_std(F, base[-1])
    jobs += [(f"divrem pair {i}", pool.submit(R.check_divrem, field, rows(da, 2, i), rows(db, 2, i), rows(q, 2, i), rows(r, 2, i))) for i in range(2)]
    jobs += [(f"inv_series pair {i}", pool.submit(R.check_inv_series, field, rows(fs, 2, i), rows(g, 2, i))) for i in range(2)]
    for keys in FORCED:
        for k in keys:
            monkeypatch.setenv(k, "1")
        outs = run(P.build_fftree(1 << 14))
        for k in keys:
            monkeypatch.delenv(k)
        for j, (want, got) in enumerate(zip(base, outs)):
            assert np.array_equal(got, want), (keys, j)
    gather(jobs)


# ---- M31 element-aligned device buffers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [14, 18, 23])
def test_m31_element_aligned_buffers(oracle_mod, pool, log_n):
    """inputs and outputs of poly_mul and poly_divrem as int32 tensor slices at an odd element offset (4-byte aligned only).
    poly_mul (N, 1): the long operand is entered at N straight from the user's buffer and EXIT writes the user's output (na + nb - 1
    = N); from 2^23 elements per launch the column passes pair spans, which needs 16-byte alignment (pair_spans).  The reference is
    a scalar multiple, exact in numpy; (N - 3, 4) and the division are checked exactly (short operands)."""
    import torch
    from ecfft_amd import fftree as FT
    field = "m31"
    F, t = oracle_mod.field(field), tree(field)
    L, p = t._L, R.P[field]
    N = 1 << log_n

    def dev(x, off=1):
        buf = torch.zeros(x.shape[0] + off + 1, dtype=torch.int32, device="cuda")
        v = buf[off:off + x.shape[0]]
        v.copy_(torch.from_numpy(x.view(np.int32)))
        return v

    def out_slice(n):
        return torch.zeros(n + 2, dtype=torch.int32, device="cuda")[1:1 + n]

    stream = torch.cuda.current_stream().cuda_stream
    jobs = []
    for na, nb in [(N, 1), (N - 3, 4)]:
        a, b = R.rand_std(field, na, log_n + na), R.rand_std(field, nb, log_n + nb + 1)
        b[-1] = b[-1] or 1
        ta, tb, tc = dev(a), dev(b), out_slice(na + nb - 1)
        assert ta.data_ptr() % 8 == 4 and tc.data_ptr() % 8 == 4
        assert L.ecfft_poly_mul(t._h, ta.data_ptr(), na, tb.data_ptr(), nb, tc.data_ptr(), 1, FT.MEM_DEVICE, stream) == FT.OK
        torch.cuda.synchronize()
        c = tc.cpu().numpy().view(np.uint32)
        assert np.array_equal(c, t.poly_mul(a, b)), (na, nb)                        # the aligned call
        if nb == 1:
            assert np.array_equal(c, (a.astype(np.uint64) * np.uint64(int(b[0])) % np.uint64(p)).astype(np.uint32))
        else:
            jobs.append((f"mul {na}x{nb}", pool.submit(R.check_mul, field, a, b, c)))
    na, nb = (N // 2 + 5, 7) if log_n < 23 else ((1 << 22) + 5, 7)               # the quotient's Newton steps up to N
    a, b = divrem_inputs(field, na, nb, 1, log_n)
    ta, tb, tq, tr = dev(a), dev(b), out_slice(na - nb + 1), out_slice(nb - 1)                # held across the call
    assert L.ecfft_poly_divrem(t._h, ta.data_ptr(), na, tb.data_ptr(), nb, tq.data_ptr(), tr.data_ptr(), 1, FT.MEM_DEVICE, stream) == FT.OK
    torch.cuda.synchronize()
    q, r = tq.cpu().numpy().view(np.uint32), tr.cpu().numpy().view(np.uint32)
    wq, wr = t.poly_divrem(a, b)
    assert np.array_equal(q, wq) and np.array_equal(r, wr)
    jobs.append(("divrem", pool.submit(R.check_divrem, field, a, b, q, r)))
    gather(jobs)
