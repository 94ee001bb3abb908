"""GPU tests (run with -m gpu on an MI355X) of the row kernel of ENTER level 11 (DESIGN.md section 2.2a "Which kernels"): the EXTEND
of the one ENTER level whose core is a single row pass with a 2048-element [u0 | v0] block per workgroup (e = 1024) runs, in full
secp256k1 contexts with matrix-core tables, on k_enter_l11 — the block's two 1024-element halves through the engine of the
1024-element row tiles (pipelined sweeps, matrix-core phase, one-multiply butterflies in a symmetric context), then the level's
combine — instead of the run-time-tile kernel k_stages_lds<F, 0>.  Every store is a canonical residue, so equal algebra gives equal
bytes: every comparison is np.array_equal, with a context of the hooks build that keeps the run-time-tile kernel
(ECFFT_ENTER_L11_GENERIC) and with the CPU oracle.

Shapes: the smallest that reach the kernel.  A launch of fewer than 512 tiles of 1024 elements on one stream (256 inside a
two-stream schedule) takes the 256-element kernels, so level 11 needs 2^19 elements: 2^11 x 256 (level 11 alone above k_enter_low,
one vector = one workgroup of the kernel), 2^12 x 128 (level 11 feeding a level with column passes), 2^11 x 512 (two half-batches
on two streams), one transform of 2^19 (the two-halves schedule, 256 tiles per half).  Against the oracle: the first, the last and
six seeded vectors of a batch and one vector of every edge pattern — every workgroup runs the same code, and all of them are
compared with the run-time-tile context.  The batched transforms run on the sub-trees of a tree of 2^13 leaves, which the session's
oracle tree mirrors."""
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


def pair(gpu, n):
    """(tuned, run-time-tile kernel) contexts of the hooks build on the library's own tree of n leaves, reports asserted"""
    P = gpu.FIELDS["secp256k1"]
    tt = P.build_fftree(n)
    with switches("ECFFT_ENTER_L11_GENERIC"):
        tg = P.build_fftree(n)
    assert (tt.enter_l11(), tg.enter_l11()) == (1, 0)
    assert (tt.sym_bfly(), tg.sym_bfly()) == (1, 1)
    return tt, tg


# 2^11 x 256: level 11 alone above k_enter_low   2^12 x 128: level 11 feeding a level with column passes (one stream, 512 tiles each)
@pytest.mark.parametrize("log_n,count", [(11, 256), (12, 128)])
def test_batched_enter(gpu, oracle_tree, hooks_lib, log_n, count):
    """ENTER of `count` vectors, seeded values and one batch of edge values: byte for byte the context that keeps the run-time-tile
    kernel, and the oracle on the first, the last and six seeded vectors (edge batch: one vector of each pattern)"""
    n = 1 << log_n
    _, ot = oracle_tree("secp256k1", 1 << LOG_TREE)
    tt, tg = pair(gpu, 1 << LOG_TREE)
    picks = [0, count - 1] + [int(v) for v in np.random.default_rng(0x111100 + log_n).choice(np.arange(1, count - 1), 6, replace=False)]
    for x, chosen in ((rand_top_bits(n * count, 0x111000 + log_n), picks), (edge_batch(n, count), [0, 1, 2, 3])):
        ent = tt.enter(x, count=count)
        assert np.array_equal(ent, tg.enter(x, count=count))
        for v in chosen:
            s = slice(v * n, (v + 1) * n)
            assert np.array_equal(ent[s], ot.enter(x[s]))


def test_two_stream_batch(gpu, hooks_lib):
    """2^11 x 512 = 2^20 elements: the batch runs as two halves of 256 vectors on two streams, 512 tiles each"""
    n, count = 1 << 11, 512
    tt, tg = pair(gpu, 1 << LOG_TREE)
    x = rand_top_bits(n * count, 0x111200)
    assert np.array_equal(tt.enter(x, count=count), tg.enter(x, count=count))


def test_single_transform_two_halves(gpu, hooks_lib):
    """one transform of 2^19: the two-halves schedule, each half 2^18 elements = 256 tiles on its own stream"""
    n = 1 << 19
    tt, tg = pair(gpu, n)
    x = rand_top_bits(n, 0x111319)
    ent = tt.enter(x)
    assert np.array_equal(ent, tg.enter(x))
    assert np.array_equal(tt.exit(ent), x)


def test_paths_that_do_not_change(gpu, oracle_tree, hooks_lib):
    """what the dispatch rule says, and the oracle's results: a general-basis context (ECFFT_NO_SYM_BFLY: matrix-core tables, so the
    kernel with two-multiply sweeps: 1), a context without matrix-core tables (ECFFT_NO_MFMA: 0), a shard context (0), M31 at its own
    single-row-pass level (e = 8192, level 14: 0), and a launch under the small-tile rule (2^11 x 255 = 510 tiles: the 256-element
    kernels, whatever the context reports)"""
    P, M = gpu.FIELDS["secp256k1"], gpu.FIELDS["m31"]
    _, ot = oracle_tree("secp256k1", 1 << LOG_TREE)
    n, count = 1 << 11, 256
    tt, _ = pair(gpu, 1 << LOG_TREE)
    with switches("ECFFT_NO_SYM_BFLY"):
        tb = P.build_fftree(1 << LOG_TREE)
    with switches("ECFFT_NO_MFMA"):
        tv = P.build_fftree(1 << LOG_TREE)
    assert (tb.sym_bfly(), tb.enter_l11(), tv.enter_l11()) == (0, 1, 0)
    assert P.build_enter_shard(1 << 11, 2, 1).enter_l11() == 0
    assert P.build_fftree(1 << 10).enter_l11() == 0          # no level 11 in this tree
    x = rand_top_bits(n * count, 0x111400)
    ent = tt.enter(x, count=count)
    assert np.array_equal(ent, tb.enter(x, count=count))
    assert np.array_equal(ent, tv.enter(x, count=count))
    for v in (0, 100, count - 1):
        assert np.array_equal(ent[v * n:(v + 1) * n], ot.enter(x[v * n:(v + 1) * n]))
    # the small-tile rule
    small = tt.enter(x[:n * 255], count=255)
    assert np.array_equal(small, ent[:n * 255])
    # M31: tiles of 8192 elements, level 14 is the single-row-pass level; 2^14 x 32 = 2^19 elements
    nm, cm = 1 << 14, 32
    _, om = oracle_tree("m31", nm)
    tm = M.build_fftree(nm)
    assert tm.enter_l11() == 0
    xm = np.random.default_rng(0x111500).integers(0, 2**31 - 1, nm * cm, dtype=np.uint32)
    em = tm.enter(xm, count=cm)
    for v in (0, cm - 1):
        assert np.array_equal(em[v * nm:(v + 1) * nm], om.enter(xm[v * nm:(v + 1) * nm]))
