"""GPU tests (run with -m gpu on an MI355X) of the three-core level inside the fused low-level EXIT kernel (k_exit_low, DESIGN.md
section 2.1a): in a three-core context the kernel's level loop reduces through Z1 as the level driver does — three EXTEND cores and
seven multiplies per pair where the reference's form has four and eight.  The outputs are canonical residues, so equal algebra
gives equal bytes: every comparison is np.array_equal.  Against the CPU oracle at the sizes it is fast enough for; against the
four-core form of the same sources (hooks build: ECFFT_EXIT_FOUR_CORES for the whole context, ECFFT_EXIT_LOW_FOUR_CORES for the
kernel alone, both read when a context is built) elsewhere.

Kernels: secp256k1 launches of fewer than 256 tiles of 1024 run k_exit_low<8,128> (256-element tiles), from 256 tiles up
k_exit_low<10,512>; M31 runs k_exit_low<13,512> (8192-element tiles), its quad body when both pointers are 16-byte aligned."""
import contextlib
import os

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
    """trees of the shipped library, cached for the module (never used inside hooks_lib)"""
    def get(field, n):
        if (field, n) not in _trees:
            _trees[(field, n)] = gpu.FIELDS[field].build_fftree(n)
            assert _trees[(field, n)] is not None
        return _trees[(field, n)]
    return get


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


def rand_m31(n, seed):
    return np.random.default_rng(seed).integers(0, P_M31, n, dtype=np.uint32)


# ---- against the oracle, secp256k1 (shipped library) ---------------------------------------------------------------------------
# 2^5, 2^6: the first levels with EXTEND cores (below one 256-element tile)   2^8: one whole tile of <8,128>, levels 8..5 in its
# loop   2^10: four tiles   2^11: driver level 11 above the kernel
@pytest.mark.parametrize("log_n", [5, 6, 8, 10, 11])
def test_exit_matches_oracle_secp256k1(gpu_tree, oracle_tree, log_n):
    n = 1 << log_n
    _, ot = oracle_tree("secp256k1", 1 << 13)
    t = gpu_tree("secp256k1", 1 << 13)
    r = rand_top_bits(n, 0xE7100 + log_n)
    assert np.array_equal(t.exit(r), ot.exit(r))


def test_batched_exit_matches_oracle_secp256k1(gpu_tree, oracle_tree):
    n, count = 1 << 8, 3
    _, ot = oracle_tree("secp256k1", 1 << 13)
    t = gpu_tree("secp256k1", 1 << 13)
    r = rand_top_bits(n * count, 0xE7180)
    got = t.exit(r, count=count)
    for v in range(count):
        assert np.array_equal(got[v * n:(v + 1) * n], ot.exit(r[v * n:(v + 1) * n]))


# ---- the 1024-element kernel at its smallest launch (256 tiles) ----------------------------------------------------------------
def test_big_tile_kernel_batched(gpu, oracle_tree, hooks_lib):
    """256 vectors of 2^10 = 256 tiles of 1024: k_exit_low<10,512> alone.  All 256 against the four-core context, the first, the
    last and two seeded ones against the oracle."""
    n, count = 1 << 10, 256
    P = gpu.FIELDS["secp256k1"]
    _, ot = oracle_tree("secp256k1", 1 << 13)
    t3 = P.build_fftree(1 << 13)
    with switches("ECFFT_EXIT_FOUR_CORES"):
        t4 = P.build_fftree(1 << 13)
    assert (t3.exit_cores(), t3.exit_low_cores(), t4.exit_cores(), t4.exit_low_cores()) == (3, 3, 4, 4)
    r = rand_top_bits(n * count, 0xE7200)
    got = t3.exit(r, count=count)
    assert np.array_equal(got, t4.exit(r, count=count))
    picks = [0, count - 1] + [int(v) for v in np.random.default_rng(0xE7201).choice(np.arange(1, count - 1), 2, replace=False)]
    for v in picks:
        assert np.array_equal(got[v * n:(v + 1) * n], ot.exit(r[v * n:(v + 1) * n]))


def test_big_tile_kernel_single_and_low_switch(gpu, hooks_lib):
    """one transform of 2^18 (the oracle is too slow): three against four cores and the round trip; and the kernel's own switch —
    a four-core k_exit_low under a three-core driver gives the same bytes at 2^12 (<8,128>) and 2^18 (<10,512>)"""
    n = 1 << 18
    P = gpu.FIELDS["secp256k1"]
    t3 = P.build_fftree(n)
    with switches("ECFFT_EXIT_FOUR_CORES"):
        t4 = P.build_fftree(n)
    with switches("ECFFT_EXIT_LOW_FOUR_CORES"):
        tl = P.build_fftree(n)
    assert (t3.exit_cores(), t3.exit_low_cores()) == (3, 3)
    assert (t4.exit_cores(), t4.exit_low_cores()) == (4, 4)
    assert (tl.exit_cores(), tl.exit_low_cores()) == (3, 4)
    r = rand_top_bits(n, 0xE7300)
    got = t3.exit(r)
    assert np.array_equal(got, t4.exit(r))
    assert np.array_equal(t3.enter(got), r)
    assert np.array_equal(got, tl.exit(r))
    r12 = r[: 1 << 12]
    assert np.array_equal(t3.exit(r12), tl.exit(r12))


# ---- levels 4..1 in the loop ---------------------------------------------------------------------------------------------------
def test_lowest_levels_in_the_loop(gpu, hooks_lib):
    """without the 16-point map (ECFFT_NO_LOW16) the level loop runs down to level 1: the only way the three-core body of the 32-byte
    field runs at e = 1, 2, 4, 8 — in <8,128> at 2^8 and in <10,512> at 2^18"""
    n = 1 << 18
    P = gpu.FIELDS["secp256k1"]
    with switches("ECFFT_NO_LOW16"):
        t3 = P.build_fftree(n)
    with switches("ECFFT_NO_LOW16", "ECFFT_EXIT_FOUR_CORES"):
        t4 = P.build_fftree(n)
    assert (t3.exit_low_cores(), t4.exit_low_cores()) == (3, 4) and (t3.low_map(1), t4.low_map(1)) == (0, 0)
    r = rand_top_bits(n, 0xE7400)
    for m in (1 << 8, n):
        assert np.array_equal(t3.exit(r[:m]), t4.exit(r[:m]))


# ---- fallback: a leaf at 0 -----------------------------------------------------------------------------------------------------
def _translated_tree(F, n, t):
    """the standard n-leaf M31 tree translated by t: leaves - t, first map composed with x -> x + t (caller leaves)"""
    p = P_M31
    f, num, den = F.build_points(n)
    num, den = num.copy().reshape(-1, 3), den.copy().reshape(-1, 3)
    for m in (num, den):                                            # c0 + c1 (x + t) + c2 (x + t)^2
        c0, c1, c2 = (int(v) for v in m[0])
        m[0] = [(c0 + c1 * t + c2 * t * t) % p, (c1 + 2 * c2 * t) % p, c2]
    shifted = ((f[n:].astype(np.int64) - t) % p).astype(np.uint32)
    return F.new_fftree(shifted, num.reshape(-1), den.reshape(-1)), shifted


def test_zero_leaf_keeps_four_cores(gpu, hooks_lib):
    """a tree with a leaf at 0 keeps the four-core form in the kernel as in the driver (k_exit_low<M31,13> at n = 2^13): the same
    bytes as the context built under the four-core switch on the same leaves"""
    n = 1 << 13
    F = gpu.FIELDS["m31"]
    t0 = int(F.build_points(n)[0][n + 6])
    tz, shifted = _translated_tree(F, n, t0)
    assert shifted[6] == 0 and (tz.exit_cores(), tz.exit_low_cores()) == (4, 4)
    with switches("ECFFT_EXIT_FOUR_CORES"):
        t4, _ = _translated_tree(F, n, t0)
    assert (t4.exit_cores(), t4.exit_low_cores()) == (4, 4)
    r = rand_m31(n, 0xE7500)
    assert np.array_equal(tz.exit(r), t4.exit(r))


# ---- M31 -----------------------------------------------------------------------------------------------------------------------
# 2^13: one 8192-element tile   2^14: two tiles under driver level 14
@pytest.mark.parametrize("log_n", [13, 14])
def test_exit_matches_oracle_m31(gpu_tree, oracle_tree, log_n):
    n = 1 << log_n
    _, ot = oracle_tree("m31", 1 << 15)
    t = gpu_tree("m31", 1 << 15)
    r = rand_m31(n, 0xE7600 + log_n)
    assert np.array_equal(t.exit(r), ot.exit(r))


def test_m31_unaligned_input_runs_generic_body(gpu, gpu_tree, oracle_tree):
    """an input tensor that starts one element into its allocation is only 4-byte aligned: the kernel's scalar (non-quad) body runs"""
    import torch
    n = 1 << 13
    _, ot = oracle_tree("m31", 1 << 15)
    t = gpu_tree("m31", 1 << 15)
    r = rand_m31(n, 0xE7700)
    buf = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    buf[1:] = torch.from_numpy(r.view(np.int32)).cuda()
    x = buf[1:]
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    got = t.exit(x).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, ot.exit(r))


def test_m31_three_cores_equal_four_cores(gpu, hooks_lib):
    n = 1 << 17
    P = gpu.FIELDS["m31"]
    t3 = P.build_fftree(n)
    with switches("ECFFT_EXIT_FOUR_CORES"):
        t4 = P.build_fftree(n)
    with switches("ECFFT_EXIT_LOW_FOUR_CORES"):
        tl = P.build_fftree(n)
    assert (t3.exit_low_cores(), t4.exit_low_cores(), tl.exit_low_cores()) == (3, 4, 4)
    r = rand_m31(n, 0xE7800)
    got = t3.exit(r)
    assert np.array_equal(got, t4.exit(r))
    assert np.array_equal(got, tl.exit(r))
    assert np.array_equal(t3.enter(got), r)
