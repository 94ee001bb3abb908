"""GPU tests of the polynomial operations (ecfft_poly_mul, ecfft_poly_divrem, ecfft_poly_inv_series, ecfft_poly_eval_points,
ecfft_poly_interpolate, ecfft_poly_pow_mod, ecfft_poly_mul_mod) in every dispatch regime of device_tree.h, against exact references
(tests/poly_ref.py: the Kronecker product on Python ints, the division and series identities built on it; tests/powmod_ref.py: the
Barrett modular power on the same product) and, above the sizes where the exact product is affordable, Schwartz-Zippel (SZ) identities at seeded
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

The launches of the composed operations (rows of n x T: that many vectors in a launch of T elements):
  poly_interpolate  m points, P = next_pow2(m), count vectors.  The subproduct tree and the weights do not see count: per level d = 64 ..
                    P/2 one EXIT_2d, the Newton steps of 1/rev(M) up to N = 2d and one lift on P/d nodes (T = 2P, an even number of rows: row
                    C once P >= 2^19, else one stream, row B from 2P >= 2^19); the weights' EXIT_P of the two top nodes (2 x P), their
                    product and its EXIT_P with count = 1 (row D once P >= 2^19) and one remainder descent of M' (T <= 2P).  The ascent
                    runs per level one EXTEND of count P/4d rows of 2d (T = count P / 2) and the final EXIT_P on count rows (T = count P:
                    row C when count is even and count P / 2 >= 2^19, row D when count = 1 and P >= 2^19).  Row E: the lift of the leaves'
                    numerators and the lifts of the tree.  On M31 nothing spans more than one 2^13 tile while P <= 2^13.
  poly_pow_mod      d = nm - 1, N = next_pow2(2d - 1), count pairs.  Once per call the reciprocal's Newton steps (count rows, up to N) and
                    ONE lift of g | f | base from next_pow2(d) to N/2 as 3 count rows (T = 3 count next_pow2(d) at its ENTER: the kept lift of
                    9 x 2^16 is on row B where the steps' 3 x 2^17 stay on row A).  Per modular product three lifts of count rows and three
                    EXIT_N on count rows (T = count N: row C when count is even and count N / 2 >= 2^19, row D when count = 1 and N >= 2^19).
                    na >= nm: the remainder half of poly_divrem(na, nm) first.  d <= 64: k_powmod_small, one workgroup per pair.
  poly_mul_mod      poly_mul(na, nb) on N = next_pow2(na + nb - 1), then the remainder half of poly_divrem(na + nb - 1, nm), both on count rows.

Checks (coverage conditions): every pair of a case whose largest product (poly_mul: na + nb - 1, poly_divrem: b q, that is na,
poly_inv_series: (f mod x^k) g) has at most 2^15 (secp256k1) / 2^17 (M31) coefficients is checked exactly; above that every pair gets
SZ and the pairs 0, count/2 - 1, count/2, count - 1 are also checked exactly while their product has at most 2^16 / 2^18 coefficients.
A pair with a short operand (<= 64 coefficients) is always checked exactly: its product costs (long / short) short products.
poly_eval_points is compared with Horner at every point while m nf <= 2^28 per polynomial; above that at one point of every 64-point
leaf block (nf <= 2^17) plus a seeded spread of >= 1024 points with the first and last point of every group and every special point.
poly_interpolate: every vector but one holds the values of a known polynomial and the interpolant must equal it byte for byte (the
interpolant is unique, so this also proves every value right; the values are Horner's at every point while count m^2 <= 2^32, above
that poly_eval_points', compared with Horner at a spread of >= 1024 positions, the first, the last and every special one); one vector
holds arbitrary values and its interpolant is evaluated back at all m points by poly_eval_points, with Horner at the same sample.
poly_pow_mod / poly_mul_mod: every pair exactly against powmod_ref (Barrett on the Kronecker product) while the product has at most
2^15 / 2^17 coefficients; above that every modular product of the scan is proved by poly_ref.sz_mul_mod: for r = x y mod f a witness
quotient q = poly_divrem(poly_mul(x, y), f)[0] from the GPU and x(z) y(z) == f(z) q(z) + r(z) at seeded points.  r has deg f
coefficients by shape, so it is the remainder whatever produced q.  The scan is walked through the exponent's prefixes (each a GPU
output of its own); a squaring that is followed by a product with the base is taken from poly_mul_mod and proved the same way.

The exact references run in a process pool (spawn, at most 8 workers, started with the first test of the module): Python-int
multiplication holds the GIL.  The jobs are poly_ref and powmod_ref functions: the workers never import torch or the GPU library; the
witness quotients are computed in the test process."""
import ctypes
import os
from concurrent.futures import ProcessPoolExecutor
import multiprocessing

import numpy as np
import pytest

import poly_ref as R
import powmod_ref as W
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


# ---- poly_interpolate -------------------------------------------------------------------------------------------------------------------
# (field, m, count, rows): P = next_pow2(m); the rows by the rules of the module docstring
INTERP_CASES = [
    ("secp256k1", (1 << 15) + 233, 1, "A-E"),             # P = 2^16: the tree's launches are 2^17, the ascent's 2^16; Horner at every point
    ("secp256k1", (1 << 16) + 4099, 3, "A-E"),            # P = 2^17: tree 2^18, ascent and EXIT 3 x 2^17 < 2^19
    ("secp256k1", (1 << 18) - 3001, 2, "A-B-E"),          # P = 2^18: tree and final EXIT 2^19 with halves of 2^18: one stream, large tiles
    ("secp256k1", 1 << 17, 8, "A-B-C-E"),                 # P = m = 2^17 (k = 0): tree 2^18 (A), final EXIT 8 x 2^17 as two half-batches
    ("secp256k1", (1 << 18) + 77, 1, "A-B-C-D-E"),        # P = 2^19: tree EXITs 2^20 in two half-batches, weights' product and final EXIT D
    ("secp256k1", (1 << 20) - 12345, 2, "A-B-C-D-E"),     # P = 2^20: tree 2^21 (C), weights' product D, final EXIT 2 x 2^20 (C)
    ("m31", 5001, 1, "E"),                                # P = 2^13: no column pass
    ("m31", (1 << 13) + 5, 3, "B-E"),                     # P = 2^14
    ("m31", 100003, 3, "B-E"),                            # P = 2^17: 3 x 2^17 < 2^19, odd count
    ("m31", 1 << 19, 4, "B-C-D-E"),                       # P = m = 2^19 (k = 0): tree 2^20 (C), weights' product D, final EXIT 4 x 2^19 (C)
    ("m31", (1 << 19) + 9, 1, "B-C-D-E"),                 # P = 2^20: final EXIT D
    ("m31", (1 << 22) - 4097, 2, "B-C-D-E"),              # P = 2^22: tree 2^23
]
N_LEAVES = 61                                             # leaves of T_P among the points, next to 0, 1 and p - 1


def interp_points(F, field, t, m, P, seed):
    """m pairwise distinct points (in-memory form) with 0, 1, p - 1 and a permuted sample of T_P's leaves at seeded positions; M31: the
    affine progression of test_gpu_polyinterp.distinct_points without the special values, then patched.  Returns (points, positions
    of the special points)"""
    from test_gpu_polyinterp import distinct_points
    rng = np.random.default_rng(seed)
    sp = np.concatenate([to_mem(F, R.from_ints(field, [0, 1, R.P[field] - 1])), t.leaves(P)[rng.permutation(P)[:N_LEAVES]]])
    pos = rng.choice(m, sp.shape[0], replace=False)
    if field == "m31":
        x = distinct_points(F, field, m + 2 * sp.shape[0], seed)
        x = x[~np.isin(x, sp)][:m].copy()
    else:
        x = to_mem(F, R.rand_std(field, m, seed, specials=False))
    x[pos] = sp
    assert x.shape[0] == m and np.unique(x, axis=0).shape[0] == m
    return x, pos


def m31_columns(t, call):
    """call() under the profiler: (its result, the k_stages_col launches it made)"""
    t.profile(True)
    out = call()
    cols = sum(r["launches"] for r in t.profile_read() if r["name"] == "k_stages_col")
    t.profile(False)
    return out, cols


def assert_row_b_m31(size, cols):
    """row B on M31: column passes once a transform spans more than one 2^13 tile"""
    if size <= 1 << 13:
        assert cols == 0, cols
    if size >= 1 << 15:
        assert cols > 0


@pytest.mark.parametrize("case", INTERP_CASES, ids=_id)
def test_poly_interpolate_regimes(oracle_mod, case):
    """every vector of the batch: count - 1 known polynomials (the first with a zero top coefficient, all with runs of zeros) recovered
    byte for byte, and one vector of arbitrary values (count = 3: also an all-zero vector) whose interpolant is evaluated back at every
    point; count = 1: the known polynomial and the arbitrary vector in one call each"""
    field, m, count, _ = case
    F, t = oracle_mod.field(field), tree(field)
    P = 1 << (m - 1).bit_length()
    x, special = interp_points(F, field, t, m, P, 7 * m + count)
    idx = np.union1d(spread_indices(m, 1024, seed=m + count), np.concatenate([[0, m - 1], special]))
    assert idx.shape[0] >= 1024
    n_arb = 2 if count == 3 else 1
    nk = max(count - n_arb, 1)
    f = to_mem(F, R.rand_std(field, nk * m, 3 * m + count))
    f[m - 1] = 0                                                              # vector 0: a zero top coefficient
    if count * m * m <= 1 << 32:
        y = np.concatenate([horner_mt(F, rows(f, nk, b), x) for b in range(nk)])
    else:
        y = t.poly_eval_points(f, x, count=nk)
        assert_canonical(field, y)
        for b in range(nk):
            assert np.array_equal(rows(y, nk, b)[idx], horner_mt(F, rows(f, nk, b), x[idx])), f"values of polynomial {b}"
    arb = [to_mem(F, R.rand_std(field, m, 5 * m + count))] + [np.zeros_like(x)] * (n_arb - 1)
    vecs = [("known", rows(y, nk, b), rows(f, nk, b)) for b in range(nk)] + [("arbitrary", v, None) for v in arb]
    calls = [vecs] if count > 1 else [[v] for v in vecs]
    assert sum(len(c) for c in calls) == max(count, 2)
    for ci, call in enumerate(calls):
        vals = np.concatenate([v for _, v, _ in call])
        if field == "m31" and ci == 0:
            got, cols = m31_columns(t, lambda: t.poly_interpolate(x, vals, count=len(call)))
            assert_row_b_m31(P, cols)
        else:
            got = t.poly_interpolate(x, vals, count=len(call))
        assert got.shape[0] == len(call) * m
        assert_canonical(field, got)
        for b, (kind, v, want) in enumerate(call):
            g = rows(got, len(call), b)
            if kind == "known":
                assert np.array_equal(g, want), f"vector {b}: the interpolant is not the polynomial whose values were given"
                continue
            back = t.poly_eval_points(g, x)
            assert np.array_equal(back, v), f"vector {b}: the interpolant does not take the given values"
            assert np.array_equal(horner_mt(F, g, x[idx]), v[idx]), f"vector {b}: Horner at the sample"
            if not v.any():
                assert not g.any()


# ---- poly_pow_mod -----------------------------------------------------------------------------------------------------------------------
MIXED = 0b101101
POW_EXPS = [0, 1, 2, 3, MIXED]
# (field, d, na, count, rows): nm = d + 1, N = next_pow2(2d - 1); na below, at and above nm in turn, so that the remainder that
# comes first when na >= nm runs in rows A, B, C and D of both fields; in such a batch every third pair keeps a base of full length
POW_CASES = [
    ("secp256k1", (1 << 15) + 1, 2 * (1 << 15) + 7, 1, "A-E"),          # N = 2^17; na = 2 nm + 3: the division's N = 2^17
    ("secp256k1", 1 << 16, 40000, 3, "A-B-E"),                         # N = 2^17: the kept lift's ENTER is 9 x 2^16 >= 2^19 on one stream
    ("secp256k1", (1 << 16) + 1, (1 << 16) + 2, 4, "A-B-C-E"),          # N = 2^18: every EXIT of the scan 4 x 2^18 in two half-batches
    ("secp256k1", 1 << 18, (1 << 18) + 1001, 1, "A-B-D-E"),             # N = 2^19: EXITs on the two-halves schedule, kept lift 3 x 2^18
    ("secp256k1", (1 << 18) + 1, 100001, 2, "A-B-C-E"),                 # N = 2^20 x 2
    ("m31", 3000, 3001, 1, "E"),                                        # N = 2^13: one tile
    ("m31", 40000, 80005, 3, "B-E"),                                    # N = 2^17, exact
    ("m31", (1 << 17) + 1, 70001, 4, "B-C-E"),                          # N = 2^19 x 4
    ("m31", (1 << 19) + 5, (1 << 19) + 1006, 1, "B-D-E"),               # N = 2^21
    ("m31", 1 << 20, (1 << 20) + 1, 2, "B-C-E"),                        # N = 2^21 x 2
]


def moduli_std(field, nm, count, seed):
    """count non-monic moduli laid end to end: pair 0 with the leading coefficient p - 1, the last pair with f(0) = 0"""
    f = R.set_nonzero(field, R.rand_std(field, count * nm, seed), np.arange(count) * nm + nm - 1)
    f[nm - 1] = R.from_ints(field, [R.P[field] - 1])[0]
    f[(count - 1) * nm] = 0
    return f


def bases_std(field, na, nm, count, seed):
    """count bases of na coefficients; with na >= nm only the pairs 0, 3, .. are that long, the others are zero above half the modulus"""
    a = R.rand_std(field, count * na, seed)
    if na >= nm:
        for i in range(count):
            if i % 3:
                a[i * na + nm // 2:(i + 1) * na] = 0
    return a


def scan_steps(e):
    """the steps (prefix, bit) of the left-to-right scan of e: prefix -> 2 prefix + bit"""
    out, cur = [], 1
    for ch in bin(e)[3:]:
        out.append((cur, int(ch)))
        cur = 2 * cur + int(ch)
    return out


def witness_mul_mod(F, field, t, x, y, fm, fs, r, count, seed, label):
    """r == x y mod f for every pair (x, y, r, fm: in-memory form; fs: f in standard form): poly_ref.sz_mul_mod with the GPU's quotient
    of the GPU's product as the witness"""
    nm = fm.shape[0] // count
    q = t.poly_divrem(t.poly_mul(x, y, count=count), fm, count=count)[0]
    assert r.shape[0] == count * (nm - 1)
    assert_canonical(field, r)
    xs, qs, rs = to_std(F, x), to_std(F, q), to_std(F, r)
    ys = xs if y is x else to_std(F, y)
    h = oracle_horner(F)
    nc = x.shape[0] // count + y.shape[0] // count - 1
    for i in range(count):
        zs = R.sz_points(field, R.sz_count(field, nc + 1), seed + i)
        msg = R.sz_mul_mod(field, rows(xs, count, i), rows(ys, count, i), rows(fs, count, i), rows(qs, count, i) if qs.shape[0] else qs[:0],
                           rows(rs, count, i), zs, h)
        assert msg == "", f"{label} pair {i}: {msg}"


@pytest.mark.parametrize("case", POW_CASES, ids=_id)
def test_poly_pow_mod_regimes(oracle_mod, pool, case):
    """the exponents 0, 1, 2, 3 and 0b101101 and every prefix of the last; see the module docstring for the checks"""
    field, d, na, count, _ = case
    F, t = oracle_mod.field(field), tree(field)
    nm = d + 1
    N = 1 << (2 * d - 2).bit_length()
    a, fs = bases_std(field, na, nm, count, 11 * d + count), moduli_std(field, nm, count, 13 * d + count)
    am, fm = to_mem(F, a), to_mem(F, fs)
    exps = sorted(set(POW_EXPS) | {2 * c + b for c, b in scan_steps(MIXED)})
    pw = {}
    for e in exps:
        if field == "m31" and e == MIXED:
            pw[e], cols = m31_columns(t, lambda: t.poly_pow_mod(am, e, fm, count=count))
            assert_row_b_m31(N, cols)
        else:
            pw[e] = t.poly_pow_mod(am, e, fm, count=count)
        assert pw[e].shape[0] == count * d
        assert_canonical(field, pw[e])
    if 2 * d - 1 <= EXACT[field]:
        std = {e: to_std(F, v) for e, v in pw.items()}
        gather([(f"pair {i}", pool.submit(W.check_pow_mod, field, rows(a, count, i), rows(fs, count, i), exps, [rows(std[e], count, i) for e in exps]))
                for i in range(count)])
        return
    one = np.zeros_like(pw[0])
    one[::d] = to_mem(F, R.from_ints(field, [1]))[0]
    assert np.array_equal(pw[0], one)
    if na < nm:                                                               # a^1 mod f: a itself, zero-padded
        want = np.zeros_like(pw[1]).reshape((count, d) + am.shape[1:])
        want[:, :na] = am.reshape((count, na) + am.shape[1:])
        assert np.array_equal(pw[1], want.reshape(pw[1].shape))
    else:                                                                     # a == f q + r with the GPU's quotient as the witness
        q = to_std(F, t.poly_divrem(am, fm, count=count)[0])
        r1, h = to_std(F, pw[1]), oracle_horner(F)
        for i in range(count):
            zs = R.sz_points(field, R.sz_count(field, na), 4000 + i)
            msg = R.sz_divrem(field, rows(a, count, i), rows(fs, count, i), rows(q, count, i), rows(r1, count, i), zs, h)
            assert msg == "", f"a mod f pair {i}: {msg}"
    done = set()
    for e in (2, 3, MIXED):
        for cur, bit in scan_steps(e):
            if (cur, bit) in done:
                continue
            done.add((cur, bit))
            x = pw[cur]
            if bit == 0:
                witness_mul_mod(F, field, t, x, x, fm, fs, pw[2 * cur], count, 5000 + 8 * cur, f"a^{cur} squared")
            else:
                sq = t.poly_mul_mod(x, x, fm, count=count)
                witness_mul_mod(F, field, t, x, x, fm, fs, sq, count, 5000 + 8 * cur, f"a^{cur} squared (poly_mul_mod)")
                witness_mul_mod(F, field, t, sq, pw[1], fm, fs, pw[2 * cur + 1], count, 5004 + 8 * cur, f"a^{2 * cur} times a")


# ---- poly_mul_mod -----------------------------------------------------------------------------------------------------------------------
# (field, na, nb, nm, count, rows): the product on N = next_pow2(na + nb - 1), then the division of its na + nb - 1 coefficients by f
MULMOD_CASES = [
    ("secp256k1", 3000, 2500, 2000, 3, "A-E"),                          # N = 2^13, exact
    ("secp256k1", 40000, 30000, 35001, 1, "A-E"),                       # N = 2^17
    ("secp256k1", (1 << 16) - 7, (1 << 16) + 5, (1 << 16) + 1, 4, "A-B-E"),      # N = 2^17 x 4 = 2^19 with halves of 2^18: one stream
    ("secp256k1", 1 << 16, (1 << 16) - 1, 40000, 8, "A-B-C-E"),         # N = 2^17 x 8: two half-batches
    ("secp256k1", 1 << 18, (1 << 18) - 50, (1 << 19) - 100, 1, "A-B-D-E"),       # N = 2^19: a quotient of 50 under a long modulus
    ("secp256k1", 1 << 17, (1 << 17) + 1000, 7, 2, "A-B-C-E"),          # product 2^19 x 2, a long quotient over a short modulus: 2^20 x 2
    ("m31", 3000, 2500, 2000, 3, "E"),                                  # N = 2^13, exact
    ("m31", 40000, 30000, 35001, 3, "B-E"),                             # N = 2^17, exact
    ("m31", 150000, 100000, 120001, 3, "B-E"),                          # N = 2^18 x 3
    ("m31", 1 << 17, (1 << 17) - 1, (1 << 17) + 1, 4, "B-C-E"),         # N = 2^18 x 4
    ("m31", 1 << 19, (1 << 19) - 50, (1 << 20) - 100, 1, "B-D-E"),      # N = 2^20: a quotient of 50 under a long modulus
    ("m31", 1 << 18, (1 << 18) + 1000, 7, 2, "B-C-E"),                  # product 2^20 x 2, a long quotient over a short modulus: 2^21 x 2
]


@pytest.mark.parametrize("case", MULMOD_CASES, ids=_id)
def test_poly_mul_mod_regimes(oracle_mod, pool, case):
    field, na, nb, nm, count, _ = case
    F, t = oracle_mod.field(field), tree(field)
    a, b = R.rand_std(field, count * na, na + 3 * nb + count), R.rand_std(field, count * nb, nb + 5 * nm + count)
    fs = moduli_std(field, nm, count, nm + 7 * na + count)
    am, bm, fm = to_mem(F, a), to_mem(F, b), to_mem(F, fs)
    nc = na + nb - 1
    if field == "m31":
        out, cols = m31_columns(t, lambda: t.poly_mul_mod(am, bm, fm, count=count))
        assert_row_b_m31(1 << (nc - 1).bit_length(), cols)
    else:
        out = t.poly_mul_mod(am, bm, fm, count=count)
    assert out.shape[0] == count * (nm - 1)
    assert_canonical(field, out)
    if nc <= EXACT[field]:
        os_ = to_std(F, out)
        gather([(f"pair {i}", pool.submit(W.check_mul_mod, field, rows(a, count, i), rows(b, count, i), rows(fs, count, i), rows(os_, count, i)))
                for i in range(count)])
    else:
        witness_mul_mod(F, field, t, am, bm, fm, fs, out, count, 6000, "a b mod f")


@pytest.mark.parametrize("field,log_d,rows_", [("secp256k1", 17, "A-B-E"), ("m31", 19, "B-C-E")])
def test_frobenius_batched(oracle_mod, field, log_d, rows_):
    """two pairs whose moduli split into distinct linear factors over different roots, the full exponent p: a^p mod f == a mod f for
    both (secp256k1: N = 2^18 x 2 on one stream, M31: N = 2^20 x 2 in two half-batches); a pair that used the other's modulus fails"""
    from test_gpu_polypowmod import distinct_mem, gpu_from_roots, rand_mem
    F, t = oracle_mod.field(field), tree(field)
    d = 1 << log_d
    roots = distinct_mem(field, 2 * d, 700 + log_d)
    f = np.concatenate([gpu_from_roots(F, t, roots[:d]), gpu_from_roots(F, t, roots[d:])])
    a = rand_mem(field, 2 * d, 800 + log_d)
    got = t.poly_pow_mod(a, R.P[field], f, count=2)
    assert_canonical(field, got)
    for i in range(2):
        assert np.array_equal(rows(got, 2, i), rows(a, 2, i)), i


# ---- the second grid chunk of k_powmod_small (more than 2^16 pairs) -------------------------------------------------------------------
N_PATTERNS = 16


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d,na", [(64, 64), (17, 40), (1, 5)])
def test_pow_mod_chunked(oracle_mod, pool, field, d, na):
    """count = 2^16 + 3 pairs of d <= 64 with the full exponent p: k_powmod_small in two grid chunks (na >= nm: the remainder before it
    chunked too).  The batch is a seeded random map of 16 (a, f) patterns, so EVERY pair is compared with powmod_ref.pow_mod of its
    pattern and a pair that read a neighbour's base or modulus fails with probability 15/16.  A zero leading coefficient in a pair
    of the second chunk is reported, and the context then reproduces the good result"""
    F, t = oracle_mod.field(field), tree(field)
    nm, e = d + 1, R.P[field]
    rng = np.random.default_rng(131 * d + na)
    A = R.rand_std(field, N_PATTERNS * na, 17 * d + na)
    Fm = R.set_nonzero(field, R.rand_std(field, N_PATTERNS * nm, 19 * d + na), np.arange(N_PATTERNS) * nm + nm - 1)
    jobs = [pool.submit(W.pow_mod, field, rows(A, N_PATTERNS, k), e, rows(Fm, N_PATTERNS, k)) for k in range(N_PATTERNS)]
    pat = rng.integers(0, N_PATTERNS, CHUNKED)
    tail = A.shape[1:]
    a = A.reshape((N_PATTERNS, na) + tail)[pat].reshape((CHUNKED * na,) + tail)
    f = Fm.reshape((N_PATTERNS, nm) + tail)[pat].reshape((CHUNKED * nm,) + tail)
    am, fm = to_mem(F, a), to_mem(F, f)
    got = t.poly_pow_mod(am, e, fm, count=CHUNKED)
    assert got.shape[0] == CHUNKED * d
    assert_canonical(field, got)
    want = np.stack([j.result() for j in jobs])[pat].reshape(got.shape)
    bad = np.flatnonzero((to_std(F, got) != want).reshape(CHUNKED, -1).any(axis=1))
    assert bad.size == 0, f"{bad.size} pairs differ, the first is pair {bad[0]}"
    z = fm.copy()
    z[(CHUNKED - 2) * nm + nm - 1] = 0
    with pytest.raises(ValueError, match="leading coefficient"):
        t.poly_pow_mod(am, e, z, count=CHUNKED)
    assert np.array_equal(t.poly_pow_mod(am, e, fm, count=CHUNKED), got)


# ---- forced regimes at small sizes (hooks build) --------------------------------------------------------------------------------------
FORCED = [("ECFFT_NO_SMALL_TILES",), ("ECFFT_NO_SMALL_TILES", "ECFFT_NO_MFMA"), ("ECFFT_NO_SMALL_TILES", "ECFFT_NO_LOW16"),
          ("ECFFT_NO_MFMA",), ("ECFFT_NO_LOW16",), ("ECFFT_NO_ROW256", "ECFFT_NO_COL256")]


def test_forced_regimes_small_sizes(oracle_mod, pool, hooks_lib, monkeypatch):
    """secp256k1 products of 2^11 .. 2^14 coefficients, a division, a series, a multipoint evaluation, an interpolation, a modular power
    and a modular product on contexts built with the A/B switches of the hooks build (read when a context is built): the large-tile and
    matrix-core forms (ECFFT_NO_SMALL_TILES), their VALU forms, and the generic small kernels.  The default form is checked against
    the references (the exact product, Horner at every point, the known polynomial, powmod_ref) and every other form must equal it
    bit for bit, so each matches the reference"""
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
    ef, ex = to_mem(F, R.rand_std(field, 2 * 3000, 93)), to_mem(F, R.rand_std(field, 5000, 94))          # eval: nf = 3000, m = 5000
    ix = to_mem(F, R.rand_std(field, 3001, 95, specials=False))                                           # interpolate: m = 3001
    assert np.unique(ix, axis=0).shape[0] == 3001
    ig = to_mem(F, R.rand_std(field, 2 * 3001, 96))
    iy = np.concatenate([horner_mt(F, rows(ig, 2, i), ix) for i in range(2)])
    pa, pf = bases_std(field, 3500, 3001, 2, 97), moduli_std(field, 3001, 2, 98)                          # pow_mod: d = 3000, na > nm
    ma, mb = R.rand_std(field, 2 * 2500, 99), R.rand_std(field, 2 * 2000, 100)                            # mul_mod: 2500 x 2000 mod 3001
    mpa, mpf, mma, mmb = to_mem(F, pa), to_mem(F, pf), to_mem(F, ma), to_mem(F, mb)
    n_mul = len(mul_shapes)

    def run(t):
        return ([t.poly_mul(a, b, count=c) for a, b, c in mem] + list(t.poly_divrem(mda, mdb, count=2)) + [t.poly_inv_series(mfs, 4000, count=2)]
                + [t.poly_eval_points(ef, ex, count=2), t.poly_interpolate(ix, iy, count=2), t.poly_pow_mod(mpa, MIXED, mpf, count=2),
                   t.poly_mul_mod(mma, mmb, mpf, count=2)])

    base = run(P.build_fftree(1 << 14))
    assert_canonical(field, *base)
    jobs = []
    for (a, b, c), out in zip(ins, base):
        cs = to_std(F, out)
        jobs += [(f"mul {a.shape[0] // c}x{b.shape[0] // c} pair {i}", pool.submit(R.check_mul, field, rows(a, c, i), rows(b, c, i), rows(cs, c, i))) for i in range(c)]
    q, r, g = (to_std(F, x) for x in base[n_mul:n_mul + 3])
    ev, it, pw, mm = base[n_mul + 3:]
    pws, mms = to_std(F, pw), to_std(F, mm)
    jobs += [(f"pow_mod pair {i}", pool.submit(W.check_pow_mod, field, rows(pa, 2, i), rows(pf, 2, i), [MIXED], [rows(pws, 2, i)])) for i in range(2)]
    jobs += [(f"mul_mod pair {i}", pool.submit(W.check_mul_mod, field, rows(ma, 2, i), rows(mb, 2, i), rows(pf, 2, i), rows(mms, 2, i))) for i in range(2)]
    for i in range(2):
        assert np.array_equal(rows(ev, 2, i), horner_mt(F, rows(ef, 2, i), ex)), f"eval_points polynomial {i}"
    assert np.array_equal(it, ig), "interpolate"
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


# ---- one context, two host threads: the pooled temporaries across calls on two streams --------------------------------------------
def test_polynomial_calls_from_two_threads_and_streams(oracle_mod):
    """two host threads drive ONE secp256k1 context on two torch streams with device tensors: one loops the asynchronous poly_mul and
    poly_eval_points (which hand the temporaries pool back while their work is still in flight), the other the synchronous
    poly_interpolate and poly_pow_mod that take the pool over on another stream (ecfft_hip.h: threading as for ecfft_poly_mul).  Ten
    rounds each; every result equals the one computed beforehand from one thread"""
    import threading
    import ecfft_amd
    import torch
    field = "secp256k1"
    F = oracle_mod.field(field)
    t = ecfft_amd.FIELDS[field].build_fftree(1 << 13)
    ma, mb = to_mem(F, R.rand_std(field, 2 * 3000, 201)), to_mem(F, R.rand_std(field, 2 * 2500, 202))
    ef, ex = to_mem(F, R.rand_std(field, 2 * 3000, 203)), to_mem(F, R.rand_std(field, 4000, 204))
    ix = to_mem(F, R.rand_std(field, 3000, 205, specials=False))
    assert np.unique(ix, axis=0).shape[0] == 3000
    iy = to_mem(F, R.rand_std(field, 2 * 3000, 206))
    pa, pf = to_mem(F, bases_std(field, 2500, 2001, 2, 207)), to_mem(F, moduli_std(field, 2001, 2, 208))
    want = {"mul": t.poly_mul(ma, mb, count=2), "eval": t.poly_eval_points(ef, ex, count=2),
            "interp": t.poly_interpolate(ix, iy, count=2), "pow": t.poly_pow_mod(pa, MIXED, pf, count=2)}
    for i in range(2):                                                        # the single-threaded results are right
        assert np.array_equal(rows(want["eval"], 2, i), horner_mt(F, rows(ef, 2, i), ex)), f"eval_points polynomial {i}"
        assert np.array_equal(horner_mt(F, rows(want["interp"], 2, i), ix), rows(iy, 2, i)), f"interpolate vector {i}"
    got = {k: [] for k in want}
    errs = []
    start = threading.Barrier(2)

    def worker(names, calls, arrays):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                dev = [torch.from_numpy(x.view(np.int64)).cuda() for x in arrays]
                start.wait(timeout=60)
                outs = []
                for _ in range(10):
                    outs.append([c(*dev) for c in calls])
                st.synchronize()
            for round_ in outs:
                for name, o in zip(names, round_):
                    got[name].append(o.cpu().numpy().view(np.uint64))
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=worker, args=(("mul", "eval"), (lambda a, b, f, x: t.poly_mul(a, b, count=2),
                                                                 lambda a, b, f, x: t.poly_eval_points(f, x, count=2)), (ma, mb, ef, ex))),
          threading.Thread(target=worker, args=(("interp", "pow"), (lambda x, y, a, f: t.poly_interpolate(x, y, count=2),
                                                                   lambda x, y, a, f: t.poly_pow_mod(a, MIXED, f, count=2)), (ix, iy, pa, pf)))]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errs, errs
    for name, outs in got.items():
        assert len(outs) == 10, name
        for rnd, o in enumerate(outs):
            assert np.array_equal(o, want[name]), (name, rnd)
