/* TEST AND MEASUREMENT HOOKS of libecfft_hip — NOT part of the shipped library.
 *
 * The reference exposes no such surface (/root/reference/src/fftree.rs:23-38, 123, 164, 227: tables and three methods), and the
 * product build of ecfft_amd/csrc/ecfft_capi.hip exports none of the symbols below.  They exist only in a build with
 * -DECFFT_TEST_HOOKS (tests/hooks/libecfft_hip_hooks.so, made by tests/hooks/build_hooks.py and __graft_entry__.build()), which
 * the tests and the measurement tools load explicitly.  The same build also reads the A/B switches of the tuning experiments from
 * the environment (ECFFT_NO_MFMA, ECFFT_NO_LOW16, ECFFT_LOW32, ECFFT_NO_ROW256, ECFFT_NO_COL256, ECFFT_NO_SMALL_TILES,
 * ECFFT_SMALL_TILES_MAX, ECFFT_SMALL_LOW_MAX, ECFFT_SMALL_MIN_LOGC, ECFFT_NO_FULL_CYCLIC, ECFFT_SPLIT_GATHER_MAX_LOG,
 * ECFFT_SPLIT_Q2_SPLIT, ECFFT_EXIT_FOUR_CORES, ECFFT_EXIT_LOW_FOUR_CORES, ECFFT_NO_SYM_BFLY, ECFFT_SYM_BFLY_GENERAL_KERNELS,
 * ECFFT_LOW_GENERAL_KERNELS, ECFFT_ENTER_L11_GENERIC); the shipped library reads no environment variable at all. */
#ifndef ECFFT_HIP_HOOKS_H
#define ECFFT_HIP_HOOKS_H
#include "ecfft_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* test hook: entries of z0_s1 / z1_s0 of the subtree with m leaves (built as the reference does, src/fftree.rs:386-397) that
 * differ from the pointwise isogeny-chain formula the sharded builds use; 0 = identical, -1 = error */
long ecfft_selfcheck_pointwise_z(ecfft_ctx* ctx, size_t m);

/* MEASUREMENT ONLY: one rank of a `world`-rank job timed on its own.  Every exchange with a remote peer costs delay_us + (bytes on
 * the exchange's most loaded LINK: the messages to one peer add up) / link_gbps GB/s as a spinning kernel on the caller's stream, and the rank's own send buffers are copied
 * into its receive buffers: the stream's timeline is that of a rank whose peers answer after exactly the modelled time; the
 * RESULTS of a sharded call on such a communicator are meaningless (tools/split_project.py: per-rank compute, exchanges, bytes and
 * exposed communication time of the split transforms without multi-GPU hardware).  link_gbps = 0: latency only. */
int ecfft_comm_init_projection(int world, int rank, int device, double delay_us, double link_gbps, ecfft_comm** out);

/* test hooks of the agreement protocol (ecfft_hip.h "Failure on ONE rank"): the local preparation of the context's next sharded
 * call of a NEW shape reports failure */
int ecfft_test_fail_next_collective(ecfft_ctx* ctx);
/* test hook, process wide: the local part of the next collective ecfft_build_exit_shard reports failure on rank `rank` (-1: off) */
int ecfft_test_fail_build_rank(int rank);

/* Test hook: the DEVICE field arithmetic on raw residues (plain integers < p, no Montgomery interpretation), host buffers.
 * op 0: out = a*b + c mod p   1: a*b   2: a - b   3: a + b   6: a / 2 (b ignored)   4 / 5: a*b + c / a*b with a taken as a TABLE constant, i.e. the
 * multiply of the butterfly kernels, result in the kernels' internal (lazy) range, not canonicalised.  Lets the tests drive the hand-written gfx950 multiply with
 * directed operands (results next to p and 2^256, carry-out of the second fold) that random data never reaches. */
int ecfft_selftest_field(int field, int op, const void* a, const void* b, const void* c, void* out, size_t n, int device);

/* Test hook (secp256k1): the matrix-core form of the innermost 16-point map (ecfft_amd/csrc/mfma_blk16.h) with an EXPLICIT map —
 * matrix256 = 16 x 16 plain residues < p, row-major [output][input]; x / out = n raw residues (n a multiple of 1024), every aligned
 * block of 16 is mapped to out_o = sum_i matrix[o][i] * x_i mod p.  Lets the tests reach the carry-out and canonicalisation
 * branches of the normalisation (identity / -1 / 0 constants, inputs next to 0, p and 2^32 + 977) that a tree's constants never hit. */
int ecfft_selftest_blk16(const void* matrix256, const void* x, void* out, size_t n, int device);
/* ... the SMALL-LAUNCH forms of the same map (v_mfma_i32_16x16x64_i8; 256-element tiles of the latency regime).
 * mode 1: 256-element arrays, 4 waves, LDS-resident (k_enter_low<8,256>'s low16)   2: 256-element arrays, 2 waves, two results per
 * lane (k_exit_low<8,128>'s low16)   3: 128-element arrays = 8 blocks, 2 waves, element in registers (k_exit_low<8,128>'s half-tiles)
 * 4: 256-element arrays, 4 waves, element in registers (k_stages_row256, k_enter_low<8,256>'s EXTEND cores).  n: a multiple of 256. */
int ecfft_selftest_blk16_small(const void* matrix256, const void* x, void* out, size_t n, int mode, int device);
/* ... the 32-point form (round 4: the five lowest ENTER / EXIT levels of the 1024-element low-level kernels as one map): matrix1024 =
 * 32 x 32 plain residues, row-major [output][input]; every aligned block of 32 of x is mapped; n a multiple of 1024. */
int ecfft_selftest_blk32(const void* matrix1024, const void* x, void* out, size_t n, int device);
/* measurement / test hook: which composite map the context's 1024-element low-level kernels run for the lowest levels of ENTER
 * (dir 0) / EXIT (dir 1): 32 = levels 1..5, 16 = levels 1..4, 0 = level code (secp256k1 only; A/B: ECFFT_LOW32, ECFFT_NO_LOW16) */
int ecfft_ctx_low_map(const ecfft_ctx* ctx, int dir);
/* test / measurement hook: EXTEND cores per EXIT level of the context's level driver: 3 = the reduction over Z1 (full contexts whose
 * leaves are all non-zero), 4 = the reference's form (a zero leaf, shard contexts, A/B: ECFFT_EXIT_FOUR_CORES, -DECFFT_EXIT_CORES=4) */
int ecfft_ctx_exit_cores(const ecfft_ctx* ctx);
/* ... and per level of the loop of the fused low-level EXIT kernel (k_exit_low): the context's form, or 4 in a three-core context
 * that keeps the four-core kernel (A/B: ECFFT_EXIT_LOW_FOUR_CORES, -DECFFT_EXIT_LOW_CORES=4) */
int ecfft_ctx_exit_low_cores(const ecfft_ctx* ctx);
/* test / measurement hook: the butterfly form of the context.  0 = general basis, two multiplies per butterfly
 * (shard contexts, M31, trees on a caller's curve, A/B: ECFFT_NO_SYM_BFLY, -DECFFT_SYM_BFLY=0)   1 = symmetric basis, one multiply per
 * butterfly in the full-size row and column passes (the library's own secp256k1 tree)   2 = symmetric basis under the general
 * kernels (A/B: ECFFT_SYM_BFLY_GENERAL_KERNELS)   -1 = no context */
int ecfft_ctx_sym_bfly(const ecfft_ctx* ctx);
/* ... and which of the 1024-element low-level kernels run symmetric butterflies in the VALU sweeps of their EXTEND cores: bit 0 =
 * k_enter_low, bit 1 = k_exit_low (three-core form only: not under ECFFT_EXIT_LOW_FOUR_CORES).  0 in every context that reports
 * sym_bfly != 1, in a four-core context (ECFFT_EXIT_FOUR_CORES) and under ECFFT_LOW_GENERAL_KERNELS (A/B: the general low-level
 * kernels under symmetric row and column passes); builds with -DECFFT_ENTER_LOW_SYM=0 / -DECFFT_EXIT_LOW_SYM=0 never set bit 0 / 1
 * -1 = no context */
int ecfft_ctx_low_sym(const ecfft_ctx* ctx);
/* test / measurement hook: which row kernel runs the EXTEND of ENTER level 11 (e = 1024, the one ENTER level whose EXTEND is a single
 * row pass with a 2048-element [u0 | v0] block per workgroup) in full-size launches.  1 = the compile-time engine of the 1024-element
 * row tiles on the block's two halves (pipelined sweeps, matrix-core phase; one-multiply butterflies in a symmetric context): full
 * secp256k1 contexts with matrix-core tables   0 = the run-time-tile row kernel (M31, shard contexts, ECFFT_NO_MFMA, A/B:
 * ECFFT_ENTER_L11_GENERIC, -DECFFT_ENTER_L11_TUNED=0, trees below 2^11 leaves)   -1 = no context.  Launches under the small-tile rule
 * take the 256-element kernels whatever this reads. */
int ecfft_ctx_enter_l11(const ecfft_ctx* ctx);
/* measurement hook (tools/findcurve_time.py): the number of queue entries every stage of the curve search has read since the last
 * reset, summed over batches: [0] bb square, [1] discriminant, [2] point of order 4, [3 + r] halving round r; and the host seconds
 * spent around each stage's launch and the read of its queue length, which waits for it.  Copies up to `cap` entries into each
 * array that is not NULL, clears the counters when `reset` is set, returns how many entries there are.  Not thread safe. */
int ecfft_curve_search_stats(uint64_t* lens, double* seconds, size_t cap, int reset);

/* test / measurement hook, process wide: how the large regime of ecfft_poly_distinct_degree takes a Frobenius iterate h_(i+1) from
 * h_i.  0: the shipped rule (the count of modular products)   1: always the kept composition h_i(h_1)   2: always the fresh power
 * h_i^p on the kept modulus.  The outputs are the same bytes either way (tests/test_gpu_polyddf.py, tools/polyddf_time.py). */
int ecfft_test_ddf_iterate(int mode);

/* test / measurement hook, process wide: how ecfft_curve_trace_mod takes pi^2 from pi.  0: the shipped rule (the count of modular
 * products at the degree of the modulus)   1: always the powers (pi_a^p, pi_b^(p+1))   2: always the composition (pi_a(pi_a),
 * pi_b(pi_a) pi_b).  The residues are the same either way (tests/test_gpu_schoof.py). */
int ecfft_test_schoof_pi2(int mode);

#ifdef __cplusplus
}
#endif
#endif
