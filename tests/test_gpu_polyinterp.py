"""GPU tests of ecfft_poly_interpolate (interpolation from arbitrary points: Lagrange weights from one remainder descent of M', the
numerators of every 64 points in k_interp_leaves, an ascent in evaluation form with k_interp_combine and one EXTEND per level, one
EXIT at the top).  The interpolant of degree < m through m distinct points is unique and outputs are canonical, so every comparison
is equality of bytes: against the known polynomial whose values (the oracle's C Horner) were interpolated, and against EXIT, which
is the interpolation at the tree's own leaves."""
import numpy as np
import pytest

from conftest import horner_mt, spread_indices, std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}
SIZES = [1, 2, 5, 63, 64, 65, 100, 127, 128, 129, 1000, 1024, 1025, 3000, 4096]

_trees = {}


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def rand_ints(field, n, rng):
    p = P[field]
    return [int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)]


def distinct_ints(field, n, rng):
    xi = rand_ints(field, n, rng) if field != "m31" else [int(v) for v in rng.choice(P[field], n, replace=False)]
    assert len(set(xi)) == n
    return xi


def rand_elems(F, field, n, seed):
    """n full-range elements without a per-element Python loop: random standard-form residues (secp256k1: all of [0, 2^256), which
    misses [p, 2^256) with probability 1 - 2^-223, so [2^255, p) is half of the inputs) brought to the in-memory form"""
    rng = np.random.default_rng(seed)
    if field == "m31":
        return rng.integers(0, P[field], n, dtype=np.uint32)
    return std_to_field(F, rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64))


def distinct_points(F, field, n, seed):
    """n pairwise distinct points: secp256k1 random (checked), M31 x_i = (a i + b) mod p with a != 0, shuffled (2^22 random draws
    from 2^31 values do collide)"""
    rng = np.random.default_rng(seed)
    if field == "m31":
        a, b = int(rng.integers(1, P[field])), int(rng.integers(0, P[field]))
        x = ((np.arange(n, dtype=np.uint64) * np.uint64(a) + np.uint64(b)) % np.uint64(P[field])).astype(np.uint32)
        x = x[rng.permutation(n)]
    else:
        x = rand_elems(F, field, n, seed)
    assert np.unique(x, axis=0).shape[0] == n
    return x


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m", SIZES)
def test_recovers_known_polynomial(oracle_mod, field, m):
    F = oracle_mod.field(field)
    rng = np.random.default_rng(m * 104729 + 1)
    f, x = F.from_ints(rand_ints(field, m, rng)), F.from_ints(distinct_ints(field, m, rng))
    got = tree(field, 4096).poly_interpolate(x, F.horner(f, x))
    assert got.shape[0] == m
    assert np.array_equal(got, f)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m", [40, 100, 700, 2500])
def test_special_inputs(oracle_mod, field, m):
    """0, 1, p - 1 and leaves of the tree among the points, shuffled; zero and constant values; coefficient vectors with runs of zeros
    and a zero top coefficient"""
    F, p, t = oracle_mod.field(field), P[field], tree(field, 4096)
    rng = np.random.default_rng(m)
    leaves = F.to_ints(t.leaves(4096))
    special = ([0, 1, p - 1] + leaves[:3] + leaves[5::411])[:m // 2]
    xi = special + [v for v in distinct_ints(field, m, rng) if v not in special][:m - len(special)]
    xi = [xi[i] for i in rng.permutation(m)]
    assert len(set(xi)) == m and 0 in xi and p - 1 in xi
    x = F.from_ints(xi)
    assert not np.any(t.poly_interpolate(x, F.from_ints([0] * m)))
    for v in (1, p - 1, xi[7]):
        assert np.array_equal(t.poly_interpolate(x, F.from_ints([v] * m)), F.from_ints([v] + [0] * (m - 1))), v
    fi = rand_ints(field, m, rng)
    fi[m - 1] = 0
    for lo, hi in ((0, 3), (m // 3, m // 3 + m // 4), (m - 9, m - 1)):
        fi[lo:hi] = [0] * (hi - lo)
    f = F.from_ints(fi)
    assert np.array_equal(t.poly_interpolate(x, F.horner(f, x)), f)
    mono = F.from_ints([0] * (m - 1) + [p - 1])
    assert np.array_equal(t.poly_interpolate(x, F.horner(mono, x)), mono)


@pytest.mark.parametrize("field,log_n", [("secp256k1", 12), ("secp256k1", 20), ("m31", 22)])
def test_on_the_leaves_it_is_exit(oracle_mod, field, log_n):
    """points = the leaves of T_n in order: the interpolant's coefficients are EXIT's (pinned to the oracle elsewhere)"""
    n = 1 << log_n
    t = tree(field, n)
    v = rand_elems(oracle_mod.field(field), field, n, 300 + log_n)
    assert np.array_equal(t.poly_interpolate(t.leaves(n), v), t.exit(v))


@pytest.mark.parametrize("field,log_n,m", [("secp256k1", 20, (1 << 20) - 3), ("secp256k1", 20, (1 << 19) + 5), ("m31", 22, (1 << 22) - 3)])
def test_scale_not_a_power_of_two(oracle_mod, field, log_n, m):
    """a known random f of m coefficients; its values come from poly_eval_points and are themselves checked against the oracle's
    Horner at >= 1024 seeded positions including the first and the last, so the test does not rest on the GPU evaluator alone"""
    F = oracle_mod.field(field)
    t = tree(field, 1 << log_n)
    f, x = rand_elems(F, field, m, 400 + log_n), distinct_points(F, field, m, 500 + log_n + m % 7)
    y = t.poly_eval_points(f, x)
    idx = np.union1d(spread_indices(m, 1024, seed=m), [0, m - 1])
    assert idx.shape[0] >= 1024
    assert np.array_equal(y[idx], horner_mt(F, f, x[idx]))
    got = t.poly_interpolate(x, y)
    assert got.shape[0] == m
    assert np.array_equal(got, f)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m", [40, 300, 1000, 2049])
@pytest.mark.parametrize("count", [3, 5])
def test_batch_equals_separate_calls(oracle_mod, field, m, count):
    F = oracle_mod.field(field)
    t = tree(field, 4096)
    x, y = distinct_points(F, field, m, m + count), rand_elems(F, field, count * m, m + 2 * count)
    got = t.poly_interpolate(x, y, count=count)
    assert got.shape[0] == count * m
    for i in range(count):
        assert np.array_equal(got[i * m:(i + 1) * m], t.poly_interpolate(x, y[i * m:(i + 1) * m])), i


@pytest.mark.parametrize("field", FIELDS)
def test_device_tensors_match_host(oracle_mod, field):
    """CUDA tensors on a side stream equal the host path"""
    import torch
    F = oracle_mod.field(field)
    t = tree(field, 4096)
    x, y = distinct_points(F, field, 2500, 11), rand_elems(F, field, 3 * 2500, 12)
    want = t.poly_interpolate(x, y, count=3)
    v = np.int64 if field != "m31" else np.int32           # torch has no unsigned 64-bit tensors: same bytes, signed view
    tx, ty = torch.from_numpy(x.view(v)).cuda(), torch.from_numpy(y.view(v)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = t.poly_interpolate(tx, ty, count=3)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy().view(want.dtype), want)


@pytest.mark.parametrize("field", FIELDS)
def test_tree_rule(oracle_mod, field):
    """next_pow2(m) leaves when m > 64; m <= 64 needs no transform and works on a tree smaller than 64"""
    F = oracle_mod.field(field)
    rng = np.random.default_rng(31)
    t = tree(field, 4096)
    x = F.from_ints(distinct_ints(field, 4097, rng))
    f = F.from_ints(rand_ints(field, 4096, rng))
    assert np.array_equal(t.poly_interpolate(x[:4096], F.horner(f, x[:4096])), f)
    with pytest.raises(ValueError, match="too small"):
        t.poly_interpolate(x, F.horner(f, x))
    small = tree(field, 8)
    for m in (1, 8, 9, 64):
        assert np.array_equal(small.poly_interpolate(x[:m], F.horner(f[:m], x[:m])), f[:m]), m
    with pytest.raises(ValueError, match="too small"):
        small.poly_interpolate(x[:65], F.horner(f[:65], x[:65]))


@pytest.mark.parametrize("field", FIELDS)
def test_repeated_point_is_rejected(oracle_mod, field):
    """two equal points raise, wherever they sit: in one block of 64, across two blocks, across the two top halves, in the
    no-transform path, and when the repeated point is 0 next to the 0 pads (one zero is a point like any other)"""
    F, t = oracle_mod.field(field), tree(field, 4096)
    rng = np.random.default_rng(41)

    def check(m, i, j, value=None):
        xi = [v for v in distinct_ints(field, m, rng) if v != 0][:m - 1]
        xi = xi + [P[field] - 2] * (m - len(xi))
        assert len(set(xi)) == m or m == 1
        if value is not None:
            xi[i] = value
        y = F.from_ints(rand_ints(field, m, rng))
        f = t.poly_interpolate(F.from_ints(xi), y)                       # distinct: accepted
        assert np.array_equal(F.horner(f, F.from_ints(xi)), y)
        xi[j] = xi[i]
        with pytest.raises(ValueError, match="repeated point"):
            t.poly_interpolate(F.from_ints(xi), y)

    check(100, 3, 97, value=0)          # two zeros with k = 28 pads of 0; one zero accepted
    check(100, 3, 40)                   # inside one block of 64
    check(40, 0, 39)                    # no transform
    check(40, 5, 20, value=0)
    check(1000, 10, 900)                # across the two top halves
    check(1000, 70, 130)                # across two different blocks of 64 in one half
    check(4096, 4095, 0)
    x, y = distinct_points(F, field, 300, 43), rand_elems(F, field, 300, 44)
    assert np.array_equal(F.horner(t.poly_interpolate(x, y), x), y)      # the context still answers correctly


@pytest.mark.parametrize("field", FIELDS)
def test_bad_args(oracle_mod, field):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    F, t = oracle_mod.field(field), tree(field, 4096)
    L = t._L
    x, y = distinct_points(F, field, 100, 72), rand_elems(F, field, 100, 71)
    out = np.zeros_like(y)
    px, py, po, H = x.ctypes.data, y.ctypes.data, out.ctypes.data, FT.MEM_HOST
    assert L.ecfft_poly_interpolate(t._h, None, 100, py, po, 1, H, None) == FT.ERR_BAD_ARG       # NULL input
    assert L.ecfft_poly_interpolate(t._h, px, 100, None, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_interpolate(t._h, px, 100, py, None, 1, H, None) == FT.ERR_BAD_ARG       # NULL output
    assert L.ecfft_poly_interpolate(t._h, px, 0, py, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_interpolate(t._h, px, 100, py, po, 0, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_interpolate(t._h, px, 100, py, po, (1 << 64) // 3, H, None) == FT.ERR_BAD_ARG   # bytes would wrap
    assert L.ecfft_poly_interpolate(t._h, px, (1 << 64) // 3, py, po, 1, H, None) == FT.ERR_BAD_ARG
    assert L.ecfft_poly_interpolate(t._h, px, 100, py, po, 1, 7, None) == FT.ERR_BAD_ARG          # unknown memory kind
    shard = ecfft_amd.FIELDS[field].build_extend_shard(1024, 1, 0)        # EXTEND-only context: holds no full tree
    assert L.ecfft_poly_interpolate(shard._h, px, 4, py, po, 1, H, None) == FT.ERR_BAD_ARG
    with pytest.raises(ValueError):
        t.poly_interpolate(x[:0], y[:0])
    assert L.ecfft_poly_interpolate(t._h, px, 100, py, po, 1, H, None) == FT.OK
    assert np.array_equal(F.horner(out, x), y)                             # the context still works


@pytest.mark.parametrize("field", FIELDS)
def test_trim_returns_the_temporaries(oracle_mod, field):
    import ecfft_amd
    F = oracle_mod.field(field)
    t = ecfft_amd.FIELDS[field].build_fftree(4096)
    x, y = distinct_points(F, field, 3000, 82), rand_elems(F, field, 2 * 3000, 81)
    t.poly_interpolate(x, y, count=2)                       # the transform scratch grows once to the largest batched transform (kept);
    t.trim()                                                # trim returns the pooled temporaries
    before = t.device_bytes
    t.poly_interpolate(x, y, count=2)
    assert t.device_bytes > before                          # the pool keeps the call's temporaries ...
    t.trim()
    assert t.device_bytes == before                         # ... until trim
