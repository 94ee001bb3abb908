"""GPU tests (run with -m gpu on an MI355X) of the symmetric butterflies inside the 1024-element low-level kernels (DESIGN.md
section 2.2a): in a symmetric context the one-pair-per-thread VALU sweeps of k_enter_low<10,512>'s EXTEND cores (pair distance
2^(log_e-1) .. 16, around the matrix-core phase) run sym_bfly on the row kernel's pipelined engine, and the cores of the three-core
k_exit_low<10,512,3> run the same sweeps on half of the workgroup, one pair per thread, instead of the one-element-per-thread
register engine — one multiply and one constant per pair in both.  Every store is a canonical residue, so equal algebra
gives equal bytes: every comparison is np.array_equal — among four contexts of the hooks build (symmetric; general basis,
ECFFT_NO_SYM_BFLY; symmetric row and column passes over the general low-level kernels, ECFFT_LOW_GENERAL_KERNELS; symmetric tables
under general kernels throughout, ECFFT_SYM_BFLY_GENERAL_KERNELS) and with the CPU oracle on a few vectors.

Shapes: 2^10 x 256 = 2^18 elements is the smallest launch that takes the 1024-element low-level kernels (256 tiles): the whole
transform is one k_enter_low<10,512,SYM> or one k_exit_low<10,512,3,SYM>.  2^11 x 128: one driver level above them.  2^10 x 255: 255
tiles, the small-tile rule — the 256-element kernels, which did not change.  One transform of 2^19: the two-halves schedule, each
half 256 tiles.  The transforms run on the sub-trees of a tree of 2^13 leaves, which the session's oracle tree mirrors."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P_SECP = 2**256 - 2**32 - 977
LOG_TREE = 13


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


def edge_batch(n, count):
    """`count` vectors of edge values, in turn: all zero, all p - 1, 0 alternating with p - 1, p - 1 alternating with 0 — F::half on
    even and odd differences (0, p - 1, 1), the borrow paths of the subtractions"""
    pm1 = np.array([(P_SECP - 1 >> (64 * k)) & (2**64 - 1) for k in range(4)], dtype=np.uint64)
    x = np.zeros((count, n, 4), dtype=np.uint64)
    x[1::4] = pm1
    x[2::4, 1::2] = pm1
    x[3::4, 0::2] = pm1
    return x.reshape(count * n, 4)


def contexts(gpu, n):
    """(symmetric, general basis, general low-level kernels, general kernels throughout) of the hooks build, reports asserted"""
    P = gpu.FIELDS["secp256k1"]
    ts = P.build_fftree(n)
    with switches("ECFFT_NO_SYM_BFLY"):
        tg = P.build_fftree(n)
    with switches("ECFFT_LOW_GENERAL_KERNELS"):
        tl = P.build_fftree(n)
    with switches("ECFFT_SYM_BFLY_GENERAL_KERNELS"):
        tb = P.build_fftree(n)
    assert (ts.sym_bfly(), tg.sym_bfly(), tl.sym_bfly(), tb.sym_bfly()) == (1, 0, 1, 2)
    assert (ts.low_sym(), tg.low_sym(), tl.low_sym(), tb.low_sym()) == (3, 0, 0, 0)      # bit 0: ENTER, bit 1: EXIT
    return ts, tg, tl, tb


# 2^10 x 256: the low-level kernels alone   2^11 x 128: one driver level above   2^10 x 255: the small-tile rule (256-element kernels)
@pytest.mark.parametrize("log_n,count", [(10, 256), (11, 128), (10, 255)])
def test_batched_transforms(gpu, oracle_tree, hooks_lib, log_n, count):
    """ENTER and EXIT of `count` vectors, seeded values and one batch of edge values: all of them across the four contexts, the first,
    the last and two seeded vectors (edge batch: one of each pattern) against the oracle"""
    n = 1 << log_n
    _, ot = oracle_tree("secp256k1", 1 << LOG_TREE)
    ts, tg, tl, tb = contexts(gpu, 1 << LOG_TREE)
    picks = [0, count - 1] + [int(v) for v in np.random.default_rng(0x105100 + log_n + count).choice(np.arange(1, count - 1), 2, replace=False)]
    for x, chosen in ((rand_top_bits(n * count, 0x105000 + log_n + count), picks), (edge_batch(n, count), [0, 1, 2, 3])):
        ent = ts.enter(x, count=count)
        ext = ts.exit(x, count=count)
        for other in (tg, tl, tb):
            assert np.array_equal(ent, other.enter(x, count=count))
            assert np.array_equal(ext, other.exit(x, count=count))
        for v in chosen:
            s = slice(v * n, (v + 1) * n)
            assert np.array_equal(ent[s], ot.enter(x[s]))
            assert np.array_equal(ext[s], ot.exit(x[s]))


def test_single_transform_two_halves(gpu, hooks_lib):
    """one transform of 2^19: the two-halves schedule, a half is 2^18 elements = 256 tiles of the 1024-element low-level kernels.
    Against the general-basis context (tests/test_gpu_parity.py compares this size with the oracle)."""
    n = 1 << 19
    P = gpu.FIELDS["secp256k1"]
    ts = P.build_fftree(n)
    with switches("ECFFT_NO_SYM_BFLY"):
        tg = P.build_fftree(n)
    assert (ts.sym_bfly(), ts.low_sym(), tg.sym_bfly(), tg.low_sym()) == (1, 3, 0, 0)
    x = rand_top_bits(n, 0x105219)
    ent = ts.enter(x)
    assert np.array_equal(ent, tg.enter(x))
    assert np.array_equal(ts.exit(x), tg.exit(x))
    assert np.array_equal(ts.exit(ent), x)


def test_contexts_that_keep_the_general_low_kernels(gpu, hooks_lib):
    """a four-core context (ECFFT_EXIT_FOUR_CORES), shard contexts and M31 report no symmetric low-level kernel and compute what they
    did: the four-core context the bytes of the general-basis context at 2^10 x 256, the EXTEND shard (world = 1: the whole tables,
    one vector of 2^18 = 2^10 x 256 elements) the EXTEND of the general-basis full context"""
    import torch
    from ecfft_amd import distributed as D
    P, M = gpu.FIELDS["secp256k1"], gpu.FIELDS["m31"]
    n, count = 1 << 10, 256
    with switches("ECFFT_EXIT_FOUR_CORES"):
        t4 = P.build_fftree(1 << LOG_TREE)
    with switches("ECFFT_NO_SYM_BFLY"):
        tg = P.build_fftree(1 << LOG_TREE)
    assert (t4.exit_cores(), t4.exit_low_cores(), t4.low_sym()) == (4, 4, 0) and tg.low_sym() == 0
    with switches("ECFFT_EXIT_LOW_FOUR_CORES"):      # the four-core kernel under a three-core driver: ENTER symmetric, EXIT on the register engine
        tl4 = P.build_fftree(1 << LOG_TREE)
    assert (tl4.exit_cores(), tl4.exit_low_cores(), tl4.low_sym()) == (3, 4, 1)
    x = rand_top_bits(n * count, 0x105300)
    assert np.array_equal(t4.enter(x, count=count), tg.enter(x, count=count))
    assert np.array_equal(t4.exit(x, count=count), tg.exit(x, count=count))
    assert np.array_equal(tl4.enter(x, count=count), tg.enter(x, count=count))
    assert np.array_equal(tl4.exit(x, count=count), tg.exit(x, count=count))
    assert M.build_fftree(1 << 13).low_sym() == 0
    assert P.build_enter_shard(1 << 11, 2, 1).low_sym() == 0
    e = n * count
    shard = P.build_extend_shard(e, 1, 0)
    assert (shard.sym_bfly(), shard.low_sym()) == (0, 0)
    with switches("ECFFT_NO_SYM_BFLY"):
        full = P.build_fftree(2 * e)
    comm = D.Comm.rccl(device=0, world=1, rank=0)
    h = torch.from_numpy(x.view(np.int64)).cuda()
    for moiety in (gpu.Moiety.S1, gpu.Moiety.S0):
        assert torch.equal(shard.extend_sharded(comm, h, e, moiety), full.extend(h, moiety))
