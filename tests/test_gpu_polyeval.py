"""GPU tests of ecfft_poly_eval_points (multipoint evaluation at arbitrary points: the subproduct tree of the points, a remainder tree
on poly_mul's lifts with k_tree_pointwise, Horner at leaves of 64 points in k_eval_leaves) against the oracle's C Horner, element for
element, and — at the headline sizes — against ENTER, whose output is the evaluation at the tree's own leaves in order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}
B = 64                                   # leaf size of the remainder tree (device_tree.h kEvalLeaf)
# (nf, m): no tree (nf <= B) with one and several leaf blocks, the first tree size, several groups, m < G, powers of two +- 1
SHAPES = [(1, 1), (1, 5), (7, 1), (64, 64), (64, 1000), (65, 64), (65, 65), (100, 37), (128, 128), (129, 1000), (1000, 100),
          (1024, 1024), (1025, 3000), (3000, 2049)]

_trees = {}


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def rand_ints(field, n, rng):
    p = P[field]
    return [int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)]


def rand_elems_fast(field, n, seed):
    """n elements in the in-memory form without a per-element Python loop (secp256k1: any value < 2^255 is a reduced residue)"""
    rng = np.random.default_rng(seed)
    if field == "m31":
        return rng.integers(0, 2**31 - 1, n, dtype=np.uint32)
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)
    return a


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nf,m", SHAPES)
def test_matches_horner(oracle_mod, field, nf, m):
    F = oracle_mod.field(field)
    rng = np.random.default_rng(nf * 7919 + m)
    f, x = F.from_ints(rand_ints(field, nf, rng)), F.from_ints(rand_ints(field, m, rng))
    got = tree(field, 4096).poly_eval_points(f, x)
    assert got.shape[0] == m
    assert np.array_equal(got, F.horner(f, x))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nf", [50, 300, 2000])
def test_special_points(oracle_mod, field, nf):
    """repeated points, all points equal, 0, p - 1 and the tree's own leaves mixed in"""
    F, p, t = oracle_mod.field(field), P[field], tree(field, 4096)
    rng = np.random.default_rng(nf)
    f = F.from_ints(rand_ints(field, nf, rng))
    leaves = F.to_ints(t.leaves(4096))
    xi = rand_ints(field, 300, rng)
    xi += xi[:40] + [0] * 5 + [p - 1] * 5 + [1] + leaves[::37] + leaves[:70]
    xi = [xi[i] for i in rng.permutation(len(xi))]
    x = F.from_ints(xi)
    assert np.array_equal(t.poly_eval_points(f, x), F.horner(f, x))
    for v in (0, p - 1, xi[3]):
        same = F.from_ints([v] * 200)
        assert np.array_equal(t.poly_eval_points(f, same), F.horner(f, same)), v


@pytest.mark.parametrize("field,log_n", [("secp256k1", 12), ("secp256k1", 20), ("m31", 22)])
def test_at_the_leaves_equals_enter(field, log_n):
    """points = the leaves of T_n, nf = n: the whole output equals ENTER's (the evaluation at the leaves in order)"""
    n = 1 << log_n
    t = tree(field, n)
    f = rand_elems_fast(field, n, 100 + log_n)
    got = t.poly_eval_points(f, t.leaves(n))
    assert np.array_equal(got, t.enter(f))


def test_groups_at_scale(oracle_mod):
    """nf = 2^20 - 3 (G = 2^20), m = 2^20 + 5 random points: two groups, the second holding 5 points and 2^20 - 5 padding points"""
    F = oracle_mod.field("secp256k1")
    t = tree("secp256k1", 1 << 20)
    nf, m = (1 << 20) - 3, (1 << 20) + 5
    f, x = rand_elems_fast("secp256k1", nf, 201), rand_elems_fast("secp256k1", m, 202)
    got = t.poly_eval_points(f, x)
    assert got.shape[0] == m
    idx = np.concatenate([np.random.default_rng(203).choice(m, 56, replace=False), np.arange(m - 8, m)])
    assert np.array_equal(got[idx], F.horner(f, x[idx]))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nf,m", [(40, 300), (200, 1000), (1500, 700)])
@pytest.mark.parametrize("count", [3, 5])
def test_batch_equals_separate_calls(field, nf, m, count):
    t = tree(field, 4096)
    f, x = rand_elems_fast(field, count * nf, nf + count), rand_elems_fast(field, m, m + count)
    got = t.poly_eval_points(f, x, count=count)
    assert got.shape[0] == count * m
    for i in range(count):
        assert np.array_equal(got[i * m:(i + 1) * m], t.poly_eval_points(f[i * nf:(i + 1) * nf], x)), i


@pytest.mark.parametrize("field", FIELDS)
def test_device_tensors_match_host(field):
    """CUDA tensors on a side stream, read after that stream's synchronise only: the call is asynchronous on the current stream"""
    import torch
    t = tree(field, 4096)
    f, x = rand_elems_fast(field, 3 * 1500, 11), rand_elems_fast(field, 2500, 12)
    want = t.poly_eval_points(f, x, count=3)
    v = np.int64 if field != "m31" else np.int32           # torch has no unsigned 64-bit tensors: same bytes, signed view
    tf, tx = torch.from_numpy(f.view(v)).cuda(), torch.from_numpy(x.view(v)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = t.poly_eval_points(tf, tx, count=3)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy().view(want.dtype), want)


@pytest.mark.parametrize("field", FIELDS)
def test_tree_rule(oracle_mod, field):
    """next_pow2(nf) leaves when nf > 64; nf <= 64 needs no transform and works on a tree smaller than 64"""
    F = oracle_mod.field(field)
    rng = np.random.default_rng(31)
    t = tree(field, 4096)
    x = F.from_ints(rand_ints(field, 100, rng))
    f = F.from_ints(rand_ints(field, 4096, rng))
    assert np.array_equal(t.poly_eval_points(f, x), F.horner(f, x))
    with pytest.raises(ValueError, match="too small"):
        t.poly_eval_points(F.from_ints(rand_ints(field, 4097, rng)), x)
    small = tree(field, 8)
    for nf in (1, 8, 9, 64):
        g = f[:nf]
        assert np.array_equal(small.poly_eval_points(g, x), F.horner(g, x)), nf
    with pytest.raises(ValueError, match="too small"):
        small.poly_eval_points(f[:65], x)


@pytest.mark.parametrize("field", FIELDS)
def test_bad_args(field):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    t = tree(field, 4096)
    L = t._L
    f, x = rand_elems_fast(field, 300, 71), rand_elems_fast(field, 100, 72)
    out = np.zeros_like(rand_elems_fast(field, 300, 73))
    pf, px, po, H = f.ctypes.data, x.ctypes.data, out.ctypes.data, FT.MEM_HOST
    assert L.ecfft_poly_eval_points(t._h, None, 300, px, 100, po, 1, H, None) == FT.ERR_BAD_ARG       # NULL input
    assert L.ecfft_poly_eval_points(t._h, pf, 300, None, 100, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_eval_points(t._h, pf, 300, px, 100, None, 1, H, None) == FT.ERR_BAD_ARG       # NULL output
    assert L.ecfft_poly_eval_points(t._h, pf, 0, px, 100, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_eval_points(t._h, pf, 300, px, 0, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_eval_points(t._h, pf, 300, px, 100, po, 0, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_eval_points(t._h, pf, 300, px, 100, po, (1 << 64) // 3, H, None) == FT.ERR_BAD_ARG   # bytes would wrap
    assert L.ecfft_poly_eval_points(t._h, pf, 300, px, (1 << 64) // 3, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_eval_points(t._h, pf, 300, px, 100, po, 1, 7, None) == FT.ERR_BAD_ARG          # unknown memory kind
    shard = ecfft_amd.FIELDS[field].build_extend_shard(1024, 1, 0)        # EXTEND-only context: holds no full tree
    assert L.ecfft_poly_eval_points(shard._h, pf, 8, px, 4, po, 1, H, None) == FT.ERR_BAD_ARG
    with pytest.raises(ValueError):
        t.poly_eval_points(f[:0], x)
    assert np.array_equal(t.poly_eval_points(f, x), t.poly_eval_points(f, x))      # the context still works


@pytest.mark.parametrize("field", FIELDS)
def test_trim_returns_the_temporaries(field):
    import ecfft_amd
    t = ecfft_amd.FIELDS[field].build_fftree(4096)
    f, x = rand_elems_fast(field, 2 * 3000, 81), rand_elems_fast(field, 5000, 82)
    t.poly_eval_points(f, x, count=2)                       # the transform scratch grows once to the largest batched EXIT (kept, as
    t.trim()                                                # after ecfft_enter_many); trim returns the pooled temporaries
    before = t.device_bytes
    t.poly_eval_points(f, x, count=2)
    assert t.device_bytes > before                          # the pool keeps the call's temporaries ...
    t.trim()
    assert t.device_bytes == before                         # ... until trim
