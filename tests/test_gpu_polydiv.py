"""GPU tests of ecfft_poly_divrem / ecfft_poly_inv_series (division with remainder: the schoolbook base case k_series_base, Newton steps
g' = g (2 - f g) on T_N with k_newton_pointwise, the quotient and remainder products on ecfft_poly_mul's lifts) against Python-integer
long division mod p — through the oracle's standard-form converters, so the crate's Montgomery representation of secp256k1 is
exercised — and, at the largest sizes, by Schwartz-Zippel a(x) = b(x) q(x) + r(x) at random points with the oracle's Horner."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}
K0 = 64                                  # coefficients of the reciprocal from k_series_base (device_tree.h kSeriesBase)
# (na, nb): nb = 1, na < nb, na = nb, nq around K0 and around 128 / 256 / 1024 / 2048, nr > nq, nr < nq
SHAPES = [(1, 1), (50, 1), (1, 2), (3, 10), (2, 2), (100, 100), (72, 10), (73, 10), (74, 10), (130, 4), (131, 4), (132, 4),
          (257, 3), (258, 3), (259, 3), (1046, 24), (1047, 24), (1048, 24), (2050, 4), (2051, 4), (364, 300), (1019, 20), (2048, 1025)]

_trees = {}


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def rand_ints(field, n, rng):
    p = P[field]
    return [int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)]


def rand_divisor(field, n, rng):
    b = rand_ints(field, n, rng)
    b[-1] = b[-1] or 1                   # a trimmed polynomial, as ark's DensePolynomial always is
    return b


def rand_elems_fast(field, n, seed):
    """n elements in the in-memory form without a per-element Python loop (secp256k1: any value < 2^255 is a reduced residue)"""
    rng = np.random.default_rng(seed)
    if field == "m31":
        return rng.integers(1, 2**31 - 1, n, dtype=np.uint32)
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)
    a[:, 0] |= np.uint64(1)              # nonzero: divisors stay trimmed and series stay invertible
    return a


def long_division(a, b, p):
    """ark-poly divide_with_q_and_r restated on Python ints: a = b q + r, deg r < deg b; r zero-padded to len(b) - 1"""
    nb, nq = len(b), max(len(a) - len(b) + 1, 0)
    r = np.array(a, dtype=object)
    bb = np.array(b, dtype=object)
    q = [0] * nq
    inv = pow(b[-1], p - 2, p)
    for i in range(nq - 1, -1, -1):
        c = int(r[i + nb - 1]) * inv % p
        q[i] = c
        if c:
            r[i:i + nb] = (r[i:i + nb] - c * bb) % p
    rem = [int(x) % p for x in r[:nb - 1]] + [0] * max(nb - 1 - len(a), 0)
    return q, rem[:nb - 1]


def reciprocal(f, k, p):
    """1/f mod x^k by the schoolbook recurrence on Python ints"""
    g = [pow(f[0], p - 2, p)]
    fa = np.array(f[1:k], dtype=object)
    ga = np.zeros(k, dtype=object)
    ga[0] = g[0]
    for j in range(1, k):
        m = min(j, len(f) - 1)
        s = int(np.dot(fa[:m], ga[j - 1::-1][:m])) if m else 0
        ga[j] = (-g[0] * s) % p
    return [int(x) for x in ga]


def _divide(t, F, ai, bi, count=1):
    q, r = t.poly_divrem(F.from_ints(ai), F.from_ints(bi), count=count)
    return F.to_ints(q) if q.shape[0] else [], F.to_ints(r) if r.shape[0] else []


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", SHAPES)
def test_matches_long_division(oracle_mod, field, na, nb):
    F = oracle_mod.field(field)
    rng = np.random.default_rng(na * 7919 + nb)
    ai, bi = rand_ints(field, na, rng), rand_divisor(field, nb, rng)
    q, r = _divide(tree(field, 4096), F, ai, bi)
    wq, wr = long_division(ai, bi, P[field])
    assert len(q) == max(na - nb + 1, 0) and len(r) == nb - 1
    assert q == wq
    assert r == wr


@pytest.mark.parametrize("field", FIELDS)
def test_special_divisors(oracle_mod, field):
    """an exact division (r = 0), a monic and a non-monic divisor, a divisor with zero middle coefficients (x^200 - 3)"""
    F, p, t = oracle_mod.field(field), P[field], tree(field, 4096)
    rng = np.random.default_rng(5)
    bi, qi = rand_divisor(field, 37, rng), rand_ints(field, 300, rng)
    ai = [int(x) % p for x in np.convolve(np.array(bi, dtype=object), np.array(qi, dtype=object))]
    q, r = _divide(t, F, ai, bi)
    assert q == qi and r == [0] * 36
    for lead in (1, 12345):
        b2 = bi[:-1] + [lead]
        assert _divide(t, F, ai, b2) == long_division(ai, b2, p)
    sparse = [p - 3] + [0] * 199 + [1]
    a3 = rand_ints(field, 1500, rng)
    assert _divide(t, F, a3, sparse) == long_division(a3, sparse, p)
    assert _divide(t, F, a3, [7] + [0] * 99 + [5]) == long_division(a3, [7] + [0] * 99 + [5], p)


KS = sorted(set(list(range(1, 131)) + [(1 << i) + d for i in range(8, 12) for d in (-1, 0, 1)]))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nf", [1, 5, 100, 2100])
def test_inv_series_matches_python(oracle_mod, field, nf):
    """k in 1..130 and powers of two +-1 up to 2049, with nf < k and nf > k"""
    F, p = oracle_mod.field(field), P[field]
    fi = rand_ints(field, nf, np.random.default_rng(nf))
    fi[0] = fi[0] or 1
    want = reciprocal(fi, max(KS), p)
    t = tree(field, 8192)
    f = F.from_ints(fi)
    for k in KS:
        g = t.poly_inv_series(f, k)
        assert g.shape[0] == k
        assert F.to_ints(g) == want[:k], k


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", [(200, 60), (60, 200), (100, 1), (300, 150), (700, 3)])
@pytest.mark.parametrize("count", [1, 2, 3, 8])
def test_batch_equals_separate_calls(field, na, nb, count):
    t = tree(field, 4096)
    a = rand_elems_fast(field, count * na, 1 + count)
    b = rand_elems_fast(field, count * nb, 2 + count)
    q, r = t.poly_divrem(a, b, count=count)
    nq, nr = max(na - nb + 1, 0), nb - 1
    assert q.shape[0] == count * nq and r.shape[0] == count * nr
    for i in range(count):
        qi, ri = t.poly_divrem(a[i * na:(i + 1) * na], b[i * nb:(i + 1) * nb])
        assert np.array_equal(q[i * nq:(i + 1) * nq], qi), i
        assert np.array_equal(r[i * nr:(i + 1) * nr], ri), i
    g = t.poly_inv_series(a, 300, count=count)
    for i in range(count):
        assert np.array_equal(g[i * 300:(i + 1) * 300], t.poly_inv_series(a[i * na:(i + 1) * na], 300)), i


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", [(200, 70), (134, 70), (200, 1), (70, 200)])
def test_outputs_do_not_depend_on_which_are_asked_for(oracle_mod, field, na, nb):
    """q of a q-only call and r of an r-only call are byte for byte those of the call that asks for both, and that call matches
    long division: 3 pairs on a 512-leaf tree with nq = 131 > K0 (a Newton step) > nr, nq = 65 (the first size past the base
    case) < nr, nb = 1 (scaling) and na < nb (copy)"""
    from ecfft_amd import fftree as FT
    F, p, t, count = oracle_mod.field(field), P[field], tree(field, 512), 3
    rng = np.random.default_rng(na * 31 + nb)
    ai = [rand_ints(field, na, rng) for _ in range(count)]
    bi = [rand_divisor(field, nb, rng) for _ in range(count)]
    a, b = F.from_ints(sum(ai, [])), F.from_ints(sum(bi, []))
    nq, nr = max(na - nb + 1, 0), nb - 1

    def call(want_q, want_r):
        # one element more than the output, so that an empty output still has an address; all-ones bytes are no field element
        q = np.full((count * nq + 1,) + a.shape[1:], np.iinfo(a.dtype).max, a.dtype)
        r = np.full((count * nr + 1,) + a.shape[1:], np.iinfo(a.dtype).max, a.dtype)
        rc = t._L.ecfft_poly_divrem(t._h, a.ctypes.data, na, b.ctypes.data, nb, q.ctypes.data if want_q else None,
                                    r.ctypes.data if want_r else None, count, FT.MEM_HOST, None)
        assert rc == FT.OK, (want_q, want_r)
        return q[:count * nq], r[:count * nr]

    q, r = call(True, True)
    for i in range(count):
        wq, wr = long_division(ai[i], bi[i], p)
        assert (F.to_ints(q[i * nq:(i + 1) * nq]) if nq else []) == wq, i
        assert (F.to_ints(r[i * nr:(i + 1) * nr]) if nr else []) == wr, i
    assert np.array_equal(call(True, False)[0], q)
    assert np.array_equal(call(False, True)[1], r)


@pytest.mark.parametrize("field", FIELDS)
def test_device_tensors_match_host(field):
    import torch
    t = tree(field, 4096)
    a = rand_elems_fast(field, 3 * 500, 11)
    b = rand_elems_fast(field, 3 * 130, 12)
    wq, wr = t.poly_divrem(a, b, count=3)
    wg = t.poly_inv_series(b, 700, count=3)
    v = np.int64 if field != "m31" else np.int32           # torch has no unsigned 64-bit tensors: same bytes, signed view
    ta, tb = torch.from_numpy(a.view(v)).cuda(), torch.from_numpy(b.view(v)).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # the calls run on the tensor's current stream
        tq, tr = t.poly_divrem(ta, tb, count=3)
        tg = t.poly_inv_series(tb, 700, count=3)
    s.synchronize()
    assert np.array_equal(tq.cpu().numpy().view(wq.dtype), wq)
    assert np.array_equal(tr.cpu().numpy().view(wr.dtype), wr)
    assert np.array_equal(tg.cpu().numpy().view(wg.dtype), wg)


def _schwartz_zippel(F, field, a, b, q, r, seed):
    x = F.from_ints(rand_ints(field, 4, np.random.default_rng(seed)))
    assert np.array_equal(F.horner(a, x), F.add(F.mul(F.horner(b, x), F.horner(q, x)), F.horner(r, x)))


@pytest.mark.parametrize("field,log_a,log_b,log_tree", [("secp256k1", 20, 19, 20), ("m31", 24, 23, 24)])
def test_at_scale_schwartz_zippel(oracle_mod, field, log_a, log_b, log_tree):
    """na = 2^a, nb = 2^b + 1: nq = nr = 2^b, N = 2^a, the largest the tree allows"""
    F = oracle_mod.field(field)
    t = tree(field, 1 << log_tree)
    na, nb = 1 << log_a, (1 << log_b) + 1
    a, b = rand_elems_fast(field, na, 31 + log_a), rand_elems_fast(field, nb, 32 + log_a)
    q, r = t.poly_divrem(a, b)
    assert q.shape[0] == na - nb + 1 and r.shape[0] == nb - 1
    _schwartz_zippel(F, field, a, b, q, r, log_a)


def test_long_quotient(oracle_mod):
    """na = 2^18, nb = 3 on a 2^19 tree: nq = 2^18 - 2, the reciprocal's Newton steps run up to N = 2^19"""
    F = oracle_mod.field("secp256k1")
    t = tree("secp256k1", 1 << 19)
    a, b = rand_elems_fast("secp256k1", 1 << 18, 41), rand_elems_fast("secp256k1", 3, 42)
    q, r = t.poly_divrem(a, b)
    assert q.shape[0] == (1 << 18) - 2 and r.shape[0] == 2
    _schwartz_zippel(F, "secp256k1", a, b, q, r, 43)


def test_batched_large_two_streams(oracle_mod):
    """2 pairs of na = 2^19, nb = 2^18 + 1 (N = 2^19): the batched transforms of 2 x 2^19 run as two half-batches on two streams"""
    F = oracle_mod.field("secp256k1")
    t = tree("secp256k1", 1 << 20)
    na, nb = 1 << 19, (1 << 18) + 1
    a, b = rand_elems_fast("secp256k1", 2 * na, 51), rand_elems_fast("secp256k1", 2 * nb, 52)
    q, r = t.poly_divrem(a, b, count=2)
    nq, nr = na - nb + 1, nb - 1
    for i in range(2):
        ai, bi, qi, ri = a[i * na:(i + 1) * na], b[i * nb:(i + 1) * nb], q[i * nq:(i + 1) * nq], r[i * nr:(i + 1) * nr]
        _schwartz_zippel(F, "secp256k1", ai, bi, qi, ri, 53 + i)
        sq, sr = t.poly_divrem(ai, bi)
        assert np.array_equal(qi, sq) and np.array_equal(ri, sr), i


@pytest.mark.parametrize("field", FIELDS)
def test_tree_rule_boundary(oracle_mod, field):
    """N = next_pow2(max(2 nq - 1, nr + min(nq, nr) - 1)) on a 4096-leaf tree, one shape on each side of each term; the series
    needs next_pow2(2k - 1)"""
    F, p, t = oracle_mod.field(field), P[field], tree(field, 4096)
    rng = np.random.default_rng(61)
    for (na, nb), fits in [((2050, 3), True), ((2051, 3), False), ((4097, 4088), True), ((4098, 4089), False)]:
        ai, bi = rand_ints(field, na, rng), rand_divisor(field, nb, rng)
        if fits:
            assert _divide(t, F, ai, bi) == long_division(ai, bi, p), (na, nb)
        else:
            with pytest.raises(ValueError, match="too small"):
                t.poly_divrem(F.from_ints(ai), F.from_ints(bi))
    f = rand_elems_fast(field, 10, 62)
    assert t.poly_inv_series(f, 2048).shape[0] == 2048
    with pytest.raises(ValueError, match="too small"):
        t.poly_inv_series(f, 2049)
    # nb == 1 and na < nb need no transform: any length on any tree
    a = rand_elems_fast(field, 10000, 63)
    assert t.poly_divrem(a, a[:1])[0].shape[0] == 10000
    assert np.array_equal(t.poly_divrem(a[:5], a)[1][:5], a[:5])


@pytest.mark.parametrize("field", FIELDS)
def test_bad_args(field):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    t = tree(field, 4096)
    L = t._L
    a = rand_elems_fast(field, 3 * 300, 71)
    b = rand_elems_fast(field, 3 * 100, 72)
    out = np.zeros_like(a)
    pa, pb, po = a.ctypes.data, b.ctypes.data, out.ctypes.data
    H = FT.MEM_HOST
    assert L.ecfft_poly_divrem(t._h, None, 300, pb, 100, po, po, 1, H, None) == FT.ERR_BAD_ARG       # NULL input
    assert L.ecfft_poly_divrem(t._h, pa, 300, None, 100, po, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_divrem(t._h, pa, 300, pb, 100, None, None, 1, H, None) == FT.ERR_BAD_ARG     # both outputs NULL
    assert L.ecfft_poly_divrem(t._h, pa, 0, pb, 100, po, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_divrem(t._h, pa, 300, pb, 0, po, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_divrem(t._h, pa, 300, pb, 100, po, po, 0, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_divrem(t._h, pa, 300, pb, 100, po, po, (1 << 64) // 3, H, None) == FT.ERR_BAD_ARG   # bytes would wrap
    assert L.ecfft_poly_divrem(t._h, pa, 300, pb, 100, po, po, 1, 7, None) == FT.ERR_BAD_ARG         # unknown memory kind
    assert L.ecfft_poly_inv_series(t._h, None, 10, po, 10, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_inv_series(t._h, pa, 10, None, 10, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_inv_series(t._h, pa, 0, po, 10, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_inv_series(t._h, pa, 10, po, 0, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_inv_series(t._h, pa, 10, po, 10, 0, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_inv_series(t._h, pa, 10, po, 10, (1 << 64) // 3, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_inv_series(t._h, pa, 10, po, 10, 1, 7, None) == FT.ERR_BAD_ARG                 # unknown memory kind
    shard = ecfft_amd.FIELDS[field].build_extend_shard(1024, 1, 0)       # EXTEND-only context: holds no full tree
    assert L.ecfft_poly_divrem(shard._h, pa, 8, pb, 4, po, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_inv_series(shard._h, pa, 8, po, 4, 1, H, None) == FT.ERR_BAD_ARG
    # a zero leading coefficient of b (a zero f[0]) in ONE pair of a batch: detected on the device, on every path
    zb = b.copy()
    zb[2 * 100 - 1] = 0                                                  # pair 1 of 3: b[nb - 1] = 0
    for na, nb in [(300, 100), (50, 100), (300, 1)]:
        bb = np.ascontiguousarray(zb.reshape((3, 100) + zb.shape[1:])[:, 100 - nb:]).reshape((3 * nb,) + zb.shape[1:])
        with pytest.raises(ValueError, match="leading coefficient"):
            t.poly_divrem(a[:3 * na], bb, count=3)
    zf = b.copy()
    zf[100] = 0                                                          # pair 1 of 3: f[0] = 0
    with pytest.raises(ValueError, match="constant coefficient"):
        t.poly_inv_series(zf, 500, count=3)
    with pytest.raises(ValueError, match="constant coefficient"):
        t.poly_inv_series(zf, 10, count=3)
    assert np.array_equal(t.poly_inv_series(b, 10, count=3)[:10], t.poly_inv_series(b[:100], 10))   # the context still works


@pytest.mark.parametrize("field", FIELDS)
def test_trim_returns_the_temporaries(field):
    import ecfft_amd
    t = ecfft_amd.FIELDS[field].build_fftree(4096)
    t.trim()
    before = t.device_bytes
    t.poly_divrem(rand_elems_fast(field, 1500, 81), rand_elems_fast(field, 700, 82), count=2)
    assert t.device_bytes > before                          # the pool keeps the call's temporaries ...
    t.trim()
    assert t.device_bytes == before                         # ... until trim


def test_pow_mod(oracle_mod):
    """x^e mod m for a 200-coefficient m by square-and-multiply over poly_mul + poly_divrem (utils::pow_mod, src/utils.rs:195-211,
    as the Schoof example uses it), against the same loop on Python ints"""
    F, p = oracle_mod.field("secp256k1"), P["secp256k1"]
    t = tree("secp256k1", 4096)
    rng = np.random.default_rng(91)
    mi = rand_divisor("secp256k1", 200, rng)
    m = F.from_ints(mi)
    e = 0b1011011011100101101

    def host_mul_mod(x, y):
        prod = [int(c) % p for c in np.convolve(np.array(x, dtype=object), np.array(y, dtype=object))]
        return long_division(prod, mi, p)[1]

    want, base = [1] + [0] * 198, [0, 1] + [0] * 197
    got, gbase = F.from_ints(want), F.from_ints(base)
    for bit in bin(e)[2:]:
        want = host_mul_mod(want, want)
        got = t.poly_divrem(t.poly_mul(got, got), m)[1]
        if bit == "1":
            want = host_mul_mod(want, base)
            got = t.poly_divrem(t.poly_mul(got, gbase), m)[1]
    assert F.to_ints(got) == want
