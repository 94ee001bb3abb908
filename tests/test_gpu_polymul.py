"""GPU tests of ecfft_poly_mul (polynomial multiplication: operands entered at their own size and lifted by EXTENDs, the pointwise
product k_poly_pointwise, one EXIT) against an independent schoolbook product in Python integers mod p — through the oracle's
standard-form converters, so the crate's Montgomery representation of secp256k1 is exercised — and, at the largest sizes, by
Schwartz-Zippel at random points with the oracle's Horner evaluation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}
SHAPES = [(1, 1), (1, 2), (2, 2), (1, 700), (700, 1), (3, 5), (37, 91), (200, 60), (60, 200), (256, 256), (512, 513),
          (1000, 24), (2048, 2048)]

_trees = {}


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def rand_ints(field, n, rng):
    p = P[field]
    return [int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)]


def schoolbook(a, b, p):
    return [int(x) % p for x in np.convolve(np.array(a, dtype=object), np.array(b, dtype=object))]


def rand_elems_fast(field, n, seed):
    """n elements in the in-memory form without a per-element Python loop (secp256k1: any value < 2^255 is a reduced residue)"""
    rng = np.random.default_rng(seed)
    if field == "m31":
        return rng.integers(0, 2**31 - 1, n, dtype=np.uint32)
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)
    return a


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", SHAPES)
def test_matches_schoolbook(oracle_mod, field, na, nb):
    F = oracle_mod.field(field)
    rng = np.random.default_rng(na * 7919 + nb)
    ai, bi = rand_ints(field, na, rng), rand_ints(field, nb, rng)
    c = tree(field, 4096).poly_mul(F.from_ints(ai), F.from_ints(bi))
    assert c.shape[0] == na + nb - 1
    assert F.to_ints(c) == schoolbook(ai, bi, P[field])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [1, 37, 256, 700])
def test_squaring(oracle_mod, field, n):
    F = oracle_mod.field(field)
    ai = rand_ints(field, n, np.random.default_rng(n))
    a = F.from_ints(ai)
    t = tree(field, 4096)
    sq = t.poly_mul(a, a)                                   # the same object: one forward transform
    assert F.to_ints(sq) == schoolbook(ai, ai, P[field])
    assert np.array_equal(sq, t.poly_mul(a, a.copy()))      # two operands with equal values


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", [(37, 91), (200, 60), (1, 700), (256, 256)])
@pytest.mark.parametrize("count", [1, 2, 3, 8])
def test_batch_equals_separate_calls(field, na, nb, count):
    t = tree(field, 4096)
    a = rand_elems_fast(field, count * na, 1 + count)
    b = rand_elems_fast(field, count * nb, 2 + count)
    c = t.poly_mul(a, b, count=count)
    nc = na + nb - 1
    assert c.shape[0] == count * nc
    for i in range(count):
        assert np.array_equal(c[i * nc:(i + 1) * nc], t.poly_mul(a[i * na:(i + 1) * na], b[i * nb:(i + 1) * nb])), i
    if na == nb:
        s = t.poly_mul(a, a, count=count)
        for i in range(count):
            assert np.array_equal(s[i * nc:(i + 1) * nc], t.poly_mul(a[i * na:(i + 1) * na], a[i * na:(i + 1) * na].copy())), i


@pytest.mark.parametrize("field", FIELDS)
def test_device_tensors_match_host(field):
    import torch
    t = tree(field, 4096)
    a = rand_elems_fast(field, 3 * 200, 11)
    b = rand_elems_fast(field, 3 * 60, 12)
    want = t.poly_mul(a, b, count=3)
    v = np.int64 if field != "m31" else np.int32           # torch has no unsigned 64-bit tensors: same bytes, signed view
    ta, tb = torch.from_numpy(a.view(v)).cuda(), torch.from_numpy(b.view(v)).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # the call runs on the tensor's current stream
        tc = t.poly_mul(ta, tb, count=3)
    s.synchronize()
    got = tc.cpu().numpy().view(want.dtype)
    assert np.array_equal(got, want)


def test_batched_large_two_streams(oracle_mod):
    """2 pairs of 2^18 x 2^18 (N = 2^19): the joint ENTER of 4 x 2^18 runs as two half-batches on two streams.  Every pair is
    checked against the reference (Schwartz-Zippel with the oracle's Horner) and against the single call, whose lift, pointwise
    and EXIT code it shares"""
    F = oracle_mod.field("secp256k1")
    t = tree("secp256k1", 1 << 20)
    n = 1 << 18
    a = rand_elems_fast("secp256k1", 2 * n, 21)
    b = rand_elems_fast("secp256k1", 2 * n, 22)
    c = t.poly_mul(a, b, count=2)
    for i in range(2):
        ai, bi, ci = a[i * n:(i + 1) * n], b[i * n:(i + 1) * n], c[i * (2 * n - 1):(i + 1) * (2 * n - 1)]
        _schwartz_zippel(F, "secp256k1", ai, bi, ci, 23 + i)
        assert np.array_equal(ci, t.poly_mul(ai, bi)), i


def _schwartz_zippel(F, field, a, b, c, seed):
    r = F.from_ints(rand_ints(field, 4, np.random.default_rng(seed)))
    ha, hb, hc = F.horner(a, r), F.horner(b, r), F.horner(c, r)
    assert np.array_equal(F.mul(ha, hb), hc)


@pytest.mark.parametrize("field,log_n,log_tree", [("secp256k1", 19, 20), ("m31", 23, 24)])
@pytest.mark.parametrize("device", [False, True])
def test_at_scale_schwartz_zippel(oracle_mod, field, log_n, log_tree, device):
    F = oracle_mod.field(field)
    t = tree(field, 1 << log_tree)
    n = 1 << log_n
    a = rand_elems_fast(field, n, 31 + log_n)
    b = rand_elems_fast(field, n, 32 + log_n)
    if device:
        import torch
        v = np.int64 if field != "m31" else np.int32
        c = t.poly_mul(torch.from_numpy(a.view(v)).cuda(), torch.from_numpy(b.view(v)).cuda())
        torch.cuda.synchronize()
        c = c.cpu().numpy().view(a.dtype)
    else:
        c = t.poly_mul(a, b)
    assert c.shape[0] == 2 * n - 1
    _schwartz_zippel(F, field, a, b, c, log_n)


@pytest.mark.parametrize("field", FIELDS)
def test_limits(field):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    t = tree(field, 4096)
    a = rand_elems_fast(field, 2048, 41)
    b = rand_elems_fast(field, 2050, 42)
    with pytest.raises(ValueError, match="too small"):      # N = 8192 > 4096 leaves
        t.poly_mul(a, b)
    L = t._L
    out = np.zeros_like(a)
    p = a.ctypes.data
    assert L.ecfft_poly_mul(t._h, p, 0, p, 1, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_mul(t._h, p, 1, p, 0, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_mul(t._h, p, 1, p, 1, out.ctypes.data, 0, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_mul(t._h, None, 4, p, 4, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG     # NULL operands / output
    assert L.ecfft_poly_mul(t._h, p, 4, None, 4, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_mul(t._h, p, 4, p, 4, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_mul(t._h, p, 4, p, 4, out.ctypes.data, 1, 7, None) == FT.ERR_BAD_ARG                 # unknown memory kind
    shard = ecfft_amd.FIELDS[field].build_extend_shard(1024, 1, 0)       # EXTEND-only context: holds no full tree
    assert L.ecfft_poly_mul(shard._h, p, 4, p, 4, out.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG


@pytest.mark.parametrize("field", FIELDS)
def test_host_squaring_is_one_operand_inside_the_library(field):
    """a host-memory poly_mul(a, a) reaches the device as ONE staged operand, so the library squares: its lift moves half the
    rows of poly_mul(a, a.copy()).  (Launch counts cannot tell: two operands of equal length share every launch of the lift.)
    The profiler's alg_bytes are computed from the launch arguments, not measured."""
    t = tree(field, 4096)
    a = rand_elems_fast(field, 300, 91)

    def alg_bytes(b):
        t.profile(True)
        c = t.poly_mul(a, b)
        total = sum(r["alg_bytes"] for r in t.profile_read())
        t.profile(False)
        return c, total

    sq, sq_bytes = alg_bytes(a)
    pr, pr_bytes = alg_bytes(a.copy())
    assert np.array_equal(sq, pr)
    assert 0 < sq_bytes < pr_bytes


@pytest.mark.parametrize("field", FIELDS)
def test_trim_returns_the_temporaries(field):
    import ecfft_amd
    t = ecfft_amd.FIELDS[field].build_fftree(4096)
    t.trim()
    before = t.device_bytes
    t.poly_mul(rand_elems_fast(field, 1000, 51), rand_elems_fast(field, 24, 52), count=2)
    assert t.device_bytes > before                          # the pool keeps the call's temporaries ...
    t.trim()
    assert t.device_bytes == before                         # ... until trim


def test_matches_enter_pointwise_exit_by_hand(oracle_mod):
    """the composition a user of the crate writes by hand: ENTER both zero-padded operands, multiply (with the R^-1 of the
    Montgomery form), EXIT — here on the oracle's tree, independent of the device's lifts"""
    F = oracle_mod.field("secp256k1")
    ot = F.build_fftree(4096)                               # the point set of the device tree (ENTER / EXIT of 256 use its T_256)
    rng = np.random.default_rng(61)
    ai, bi = rand_ints("secp256k1", 100, rng), rand_ints("secp256k1", 120, rng)
    pa = F.from_ints(ai + [0] * 156)
    pb = F.from_ints(bi + [0] * 136)
    want = ot.exit(F.mul(ot.enter(pa), ot.enter(pb)))[:219]
    assert np.array_equal(tree("secp256k1", 4096).poly_mul(F.from_ints(ai), F.from_ints(bi)), want)
