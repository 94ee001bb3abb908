"""GPU tests (run with -m gpu on an MI355X) of the symmetric butterflies: the library's own secp256k1 tree
writes its stage tables in the coordinate sigma = (x - c1)/(x - c2) of each layer, where the two pre-images of a point are
opposite, and its full-size row and column passes run one multiply per butterfly.  Every store is a canonical residue, so equal
algebra gives equal bytes: every comparison is np.array_equal — with the CPU oracle where it is fast enough (trees of 2^12 and
2^14 leaves), and with a general-basis context of the same sources (hooks build, ECFFT_NO_SYM_BFLY read when a context is built)
everywhere.  tests/test_gpu_parity.py compares the same symmetric context with the oracle at 2^19 and 2^20 (its background oracle
takes minutes to build, so it is not repeated here).

Shapes: the smallest that launch each changed kernel.  2^12 x 128 = 2^19 elements: 1024-element tiles; levels 11 and 12 run
k_stages_lds<10, SYM> plus a one-stage column pass (k_stages_col<SYM>, k_stages_col_mid<SYM> between EXIT's cores,
k_stages_col_enter<SYM>).  2^14 x 32: three column stages.  One transform of 2^19: the two-halves schedule, eight column stages."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P_SECP = 2**256 - 2**32 - 977


@pytest.fixture(scope="module")
def gpu():
    import ecfft_amd
    ecfft_amd.lib()
    return ecfft_amd


@contextlib.contextmanager
def switches(*names):
    """A/B switches of the hooks build, set while a context is built"""
    for k in names:
        os.environ[k] = "1"
    try:
        yield
    finally:
        for k in names:
            del os.environ[k]


def rand_top_bits(n, seed):
    """canonical secp256k1 elements as raw 256-bit patterns, every third one with bit 255 set (bit 254 clear: below p)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)
    a[::3, 3] = (a[::3, 3] & np.uint64(0x3FFFFFFFFFFFFFFF)) | np.uint64(0x8000000000000000)
    return a


def pair(gpu, n):
    """(symmetric context, general-basis context, symmetric basis under the general kernels) of the hooks build"""
    P = gpu.FIELDS["secp256k1"]
    ts = P.build_fftree(n)
    with switches("ECFFT_NO_SYM_BFLY"):
        tg = P.build_fftree(n)
    with switches("ECFFT_SYM_BFLY_GENERAL_KERNELS"):
        tb = P.build_fftree(n)
    assert (ts.sym_bfly(), tg.sym_bfly(), tb.sym_bfly()) == (1, 0, 2)
    return ts, tg, tb


@pytest.mark.parametrize("log_n,count", [(12, 128), (14, 32)])
def test_batched_transforms(gpu, oracle_mod, oracle_tree, hooks_lib, log_n, count):
    """ENTER, EXIT and EXTEND of `count` vectors: all of them against the general-basis context (and the symmetric tables under the
    general kernels), the first, the last and two seeded ones against the oracle"""
    n = 1 << log_n
    _, ot = oracle_tree("secp256k1", n)
    o = oracle_mod
    ts, tg, tb = pair(gpu, n)
    x = rand_top_bits(n * count, 0x5B0000 + log_n)
    picks = [0, count - 1] + [int(v) for v in np.random.default_rng(0x5B0100 + log_n).choice(np.arange(1, count - 1), 2, replace=False)]
    ent = ts.enter(x, count=count)
    assert np.array_equal(ent, tg.enter(x, count=count)) and np.array_equal(ent, tb.enter(x, count=count))
    ext = ts.exit(x, count=count)
    assert np.array_equal(ext, tg.exit(x, count=count)) and np.array_equal(ext, tb.exit(x, count=count))
    for v in picks:
        s = slice(v * n, (v + 1) * n)
        assert np.array_equal(ent[s], ot.enter(x[s]))
        assert np.array_equal(ext[s], ot.exit(x[s]))
    e = n // 2
    h = x[: e * count]
    for moiety, om in ((gpu.Moiety.S1, o.S1), (gpu.Moiety.S0, o.S0)):
        got = ts.extend(h, moiety, count=count)
        assert np.array_equal(got, tg.extend(h, moiety, count=count)) and np.array_equal(got, tb.extend(h, moiety, count=count))
        for v in picks:
            s = slice(v * e, (v + 1) * e)
            assert np.array_equal(got[s], ot.extend(h[s], om))


def test_single_transform_two_halves(gpu, hooks_lib):
    """one transform of 2^19: the two-halves schedule, eight column stages per pass, k_stages_col_enter"""
    n = 1 << 19
    ts, tg, _ = pair(gpu, n)
    x = rand_top_bits(n, 0x5B0219)
    ent = ts.enter(x)
    assert np.array_equal(ent, tg.enter(x))
    ext = ts.exit(x)
    assert np.array_equal(ext, tg.exit(x))
    assert np.array_equal(ts.exit(ent), x)
    h = x[: n // 2]
    for moiety in (gpu.Moiety.S1, gpu.Moiety.S0):
        assert np.array_equal(ts.extend(h, moiety), tg.extend(h, moiety))


def test_contexts_that_keep_the_general_form(gpu, hooks_lib):
    """shard contexts, M31 and trees on a caller's curve report the general form; so does every context of the shipped library's
    A/B switch; the library's own secp256k1 tree reports the symmetric one"""
    import curve_ref as R
    import poly_ref
    P, M = gpu.FIELDS["secp256k1"], gpu.FIELDS["m31"]
    assert P.build_fftree(1 << 8).sym_bfly() == 1
    assert M.build_fftree(1 << 10).sym_bfly() == 0
    assert P.build_extend_shard(1 << 10, 2, 0).sym_bfly() == 0
    assert P.build_enter_shard(1 << 10, 2, 1).sym_bfly() == 0
    cr = R.CRATE
    cf = lambda ints: P.from_standard(poly_ref.from_ints("secp256k1", ints))
    t = P.build_fftree_on_curve(1 << 8, cf([cr["a"]]), cf([cr["bb"]]), cf(list(cr["gen"])), cr["log_order"], cf(list(cr["offset"])))
    assert t.sym_bfly() == 0
    x = rand_top_bits(1 << 8, 0x5B0308)
    assert np.array_equal(t.enter(x), P.build_fftree(1 << 8).enter(x))      # the same tree in the other basis: the same bytes


def to_limbs(vals):
    return np.array([[(v >> (64 * k)) & (2**64 - 1) for k in range(4)] for v in vals], dtype=np.uint64)


def from_limbs(a):
    return [sum(int(a[i, k]) << (64 * k) for k in range(4)) for i in range(a.shape[0])]


def test_half_directed_operands(gpu, hooks_lib):
    """F::half on 0, 1, p - 1, odd and even values next to the word boundaries, 2^255 and p; and M31's"""
    p = P_SECP
    vals = [0, 1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 2**255, 2**255 + 1, 2**255 - 1, 2**32, 2**32 - 1, 2**64 + 1, 2**128 - 1, 2**192,
            2**256 - 2**33, 0xFFFFFFFE, 0x100000001]
    rng = np.random.default_rng(0x5B0400)
    vals += [int.from_bytes(rng.bytes(32), "little") % p for _ in range(45)]
    a = to_limbs(vals)
    got = from_limbs(gpu.FIELDS["secp256k1"].selftest(6, a, a))
    inv2 = (p + 1) // 2
    assert got == [v * inv2 % p for v in vals]
    q = 2**31 - 1
    m = np.array([0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, 12345, 12346], dtype=np.uint32)
    gm = gpu.FIELDS["m31"].selftest(6, m, m)
    assert [int(v) for v in gm] == [int(v) * ((q + 1) // 2) % q for v in m]
