"""GPU tests (run with -m gpu on an MI355X) of the three-core EXIT level: the level driver reduces modulo X^(n/2) through Z1, the
vanishing polynomial of S1, so that the result lands on S0 after three EXTEND cores instead of the reference's four (DESIGN.md
section 2.1a; the identity itself is proved on Python integers in tests/test_exit3_identity_host.py).  The output is the same bytes:
against the CPU oracle at every size at which the level driver takes another path, against the four-core form of the same sources
(the hooks build's ECFFT_EXIT_FOUR_CORES switch, read when a context is built) at the sizes the oracle is too slow for, round
trips, and the fallback of a context whose leaf set contains 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P_SECP = 2**256 - 2**32 - 977
P_M31 = 2**31 - 1


@pytest.fixture(scope="module")
def gpu():
    import ecfft_amd
    ecfft_amd.lib()
    return ecfft_amd


_trees = {}


@pytest.fixture(scope="module")
def gpu_tree(gpu):
    def get(field, n):
        if (field, n) not in _trees:
            _trees[(field, n)] = gpu.FIELDS[field].build_fftree(n)
            assert _trees[(field, n)] is not None
        return _trees[(field, n)]
    return get


def rand_elems(F, n, seed):
    rng = np.random.default_rng(seed)
    if F.limbs == 1:
        return rng.integers(0, P_M31, n, dtype=np.uint32)
    return F.from_ints([int.from_bytes(rng.bytes(32), "little") % P_SECP for _ in range(n)])


def rand_top_bits(n, seed):
    """canonical secp256k1 elements as raw 256-bit patterns, every third one with bit 255 set (bit 254 clear: below p)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)
    a[::3, 3] = (a[::3, 3] & np.uint64(0x3FFFFFFFFFFFFFFF)) | np.uint64(0x8000000000000000)
    return a


# 2^1, 2^2: level code only   2^4: low16 only   2^5: first level with cores in the low-level kernel   2^8, 2^10: whole tiles
# 2^11: level 11 = row passes only, the new store operator in the row kernel   2^12: first column pass, col_mid   2^13
@pytest.mark.parametrize("log_n", [1, 2, 4, 5, 8, 10, 11, 12, 13])
def test_exit_matches_oracle_secp256k1(gpu, gpu_tree, oracle_tree, log_n):
    n = 1 << log_n
    F, ot = oracle_tree("secp256k1", 1 << 13)
    t = gpu_tree("secp256k1", 1 << 13)
    r = rand_elems(F, n, 0xE3170 + log_n)
    assert np.array_equal(t.exit(r), ot.exit(r))


@pytest.mark.parametrize("count", [2, 3])
def test_batched_exit_matches_oracle_secp256k1(gpu, gpu_tree, oracle_tree, count):
    n = 1 << 11
    F, ot = oracle_tree("secp256k1", 1 << 13)
    t = gpu_tree("secp256k1", 1 << 13)
    r = rand_elems(F, n * count, 0xE31B0 + count)
    got = t.exit(r, count=count)
    for v in range(count):
        assert np.array_equal(got[v * n:(v + 1) * n], ot.exit(r[v * n:(v + 1) * n]))


# the low-level kernel of 4-byte fields covers 13 levels; the first column pass is at level 15
@pytest.mark.parametrize("log_n", [13, 14, 15])
def test_exit_matches_oracle_m31(gpu, gpu_tree, oracle_tree, log_n):
    n = 1 << log_n
    F, ot = oracle_tree("m31", 1 << 15)
    t = gpu_tree("m31", 1 << 15)
    r = rand_elems(F, n, 0xE3310 + log_n)
    assert np.array_equal(t.exit(r), ot.exit(r))


# 2^12: small-launch kernels   2^16   2^18: first size on k_exit_low<10,512> and 1024-element tiles   2^19: two-halves schedule
@pytest.mark.parametrize("log_n", [12, 16, 18, 19])
def test_three_cores_equal_four_cores(gpu, log_n, monkeypatch, hooks_lib):
    n = 1 << log_n
    P = gpu.FIELDS["secp256k1"]
    t3 = P.build_fftree(n)
    monkeypatch.setenv("ECFFT_EXIT_FOUR_CORES", "1")
    t4 = P.build_fftree(n)
    monkeypatch.delenv("ECFFT_EXIT_FOUR_CORES")
    assert (t3.exit_cores(), t4.exit_cores()) == (3, 4)
    r = rand_top_bits(n, 0xE3400 + log_n)
    got = t3.exit(r)
    assert np.array_equal(got, t4.exit(r))
    assert np.array_equal(t3.enter(got), r)                    # and they are the coefficients of the interpolant


@pytest.mark.parametrize("log_n", [12, 18])
def test_round_trip(gpu, log_n):
    n = 1 << log_n
    t = gpu.FIELDS["secp256k1"].build_fftree(n)
    c = rand_top_bits(n, 0xE3500 + log_n)
    assert np.array_equal(t.exit(t.enter(c)), c)


def test_m31_three_cores_equal_four_cores(gpu, monkeypatch, hooks_lib):
    """the 4-byte vector path of the new store operator (column passes of 8192-element tiles) against the four-core form"""
    n = 1 << 17
    P = gpu.FIELDS["m31"]
    t3 = P.build_fftree(n)
    monkeypatch.setenv("ECFFT_EXIT_FOUR_CORES", "1")
    t4 = P.build_fftree(n)
    monkeypatch.delenv("ECFFT_EXIT_FOUR_CORES")
    assert (t3.exit_cores(), t4.exit_cores()) == (3, 4)
    r = np.random.default_rng(0xE3600).integers(0, P_M31, n, dtype=np.uint32)
    got = t3.exit(r)
    assert np.array_equal(got, t4.exit(r))
    assert np.array_equal(t3.exit(r[: n // 2], count=2), t4.exit(r[: n // 2], count=2))
    assert np.array_equal(t3.enter(got), r)


def _translated_tree(F, n, t):
    """the standard n-leaf tree translated by t: leaves - t, first map composed with x -> x + t (caller leaves, ecfft_fftree_new)"""
    p = P_M31
    f, num, den = F.build_points(n)
    num, den = num.copy().reshape(-1, 3), den.copy().reshape(-1, 3)
    for m in (num, den):                                            # c0 + c1 (x + t) + c2 (x + t)^2
        c0, c1, c2 = (int(v) for v in m[0])
        m[0] = [(c0 + c1 * t + c2 * t * t) % p, (c1 + 2 * c2 * t) % p, c2]
    shifted = np.array([(int(x) - t) % p for x in f[n:]], dtype=np.uint32)
    return F.new_fftree(shifted, num.reshape(-1), den.reshape(-1)), shifted


def _taylor_shift(P, t, p):
    """coefficients of P(x + t)"""
    n = len(P)
    Q = [0] * n
    for a in reversed(P):                                           # Q <- Q * (x + t) + a
        nxt = [0] * n
        for i, q in enumerate(Q):
            nxt[i] = (nxt[i] + q * t) % p
            if i + 1 < n:
                nxt[i + 1] = (nxt[i + 1] + q) % p
        nxt[0] = (nxt[0] + a) % p
        Q = nxt
    return Q


def test_caller_leaves_and_zero_leaf_fallback(gpu, oracle_tree, hooks_lib):
    """Trees on caller leaves (ecfft_fftree_new): the standard M31 tree translated by t.  If P interpolates r on the standard leaves,
    Q(x) = P(x + t) interpolates r on the translated ones, so the oracle's EXIT on the standard tree gives the expected coefficients
    after a Taylor shift.  With no leaf at 0 the context runs three cores and must match.  Translated by one of its own leaves the
    tree has a leaf at 0: the three-core form would divide by X^(m/2) = 0, so the context must select the four-core form.  No
    oracle comparison for that tree: the reference's own table construction divides by X^(m/4) on every leaf
    (src/fftree.rs:328-330, 430-438), so with a leaf at 0 its z0z0_rem_xnn_s is not the table it names, in the reference as here."""
    p, n = P_M31, 16
    F = gpu.FIELDS["m31"]
    Fo, ot = oracle_tree("m31", n)
    r = np.random.default_rng(0xE3700).integers(0, p, n, dtype=np.uint32)
    want = [int(v) for v in ot.exit(r)]
    t_std = F.build_fftree(n)
    assert t_std.exit_cores() == 3 and np.array_equal(t_std.exit(r), ot.exit(r))
    leaves = [int(x) for x in F.build_points(n)[0][n:]]
    t = next(v for v in range(1, 100) if v not in leaves)
    tt, shifted = _translated_tree(F, n, t)
    assert tt.exit_cores() == 3 and 0 not in shifted
    got = tt.exit(r)
    assert [int(v) for v in got] == _taylor_shift(want, t, p)
    assert np.array_equal(tt.enter(got), r)
    for pos in (1, 6):                                              # a leaf of S1, a leaf of S0
        tz, shifted = _translated_tree(F, n, leaves[pos])
        assert shifted[pos] == 0 and tz.exit_cores() == 4
