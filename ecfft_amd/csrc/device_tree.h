// Device-resident FFTree chain T_1 < T_2 < ... < T_N and the iterative, level-by-level drivers of
// EXTEND / ENTER / EXIT (the reference's recursive extend_impl / enter_impl / exit_impl / redc_impl,
// /root/reference/src/fftree.rs:72-120, 143-161, 200-224, 232-259, re-expressed as batched sweeps,
// SURVEY.md Appendix A) plus the on-GPU table precompute (from_tree, src/fftree.rs:318-463).
//
// HBM layout ("Moiety precompute layout"): per tree T_m (m = 2e leaves), per moiety
// parity s in {0,1}, structure-of-arrays tables holding only the half that parity uses:
//   p0[s], p1[s], np0[s], dinv[s]   e-1 entries, stage k at offset e - 2*h_k   (h_k = e >> (k+1))
//                                   (p0 / p1 = the two pre-images of a layer point — or, in a symmetric context, DESIGN.md 2.2a, their
//                                   images under the layer's sigma = (x - c1)/(x - c2), where p1 = -p0; np0 = -p0, dinv = 1/(p1 - p0))
//   c0t[s] = np0[s]*dinv[s]         likewise    (pair-split decompose of the latency regime: two independent products)
//   w[s], winv[s]                   e entries   (normalisation weights of the parity's leaves)
//   xe, w1x                         e entries   ENTER combine
//   A1, B1, NB2, C1, D1, xie        e entries   EXIT pointwise steps with every inverse pre-fused (four-core form, reduction over Z0)
//   zA1, zB1, zNB2, zC1, zD1, zNB3  e entries   the same for the three-core form (reduction over Z1); a tree holds the set it runs
// All tables are PLAIN residues; user data stays in the crate's Montgomery form (field_secp256k1.h).  The tables above are
// stored as F::telem — for secp256k1 the pair (t, t*2^128 mod p) that the 12-word multiply wants, for M31 the doubled constant
// 2t (field_m31.h) — and are written by to_tables() from plain temporaries; the reference's own tables (xnn, z*) stay plain
// F::elem arrays.  Below the level drivers: the sharded (multi-GPU) drivers extend_split / api_enter_split / api_exit_split.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include <set>
#include <map>
#include <mutex>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <algorithm>
#include "kernels.h"
#include "host_curve.h"
#include "transport.h"

namespace ecfft {

// A/B switches of the tuning experiments (ECFFT_NO_MFMA, ECFFT_NO_LOW16, ECFFT_LOW32, ECFFT_NO_ROW256, ...): a test / tuning build
// (-DECFFT_TEST_HOOKS, tests/hooks/) reads them from the environment, the SHIPPED library has none of them — it reads no environment
// variable at all, so two ranks of one job cannot end up on different exchange patterns because their environments differ.
#ifdef ECFFT_TEST_HOOKS
inline const char* ab_env(const char* name) { return getenv(name); }
#else
inline const char* ab_env(const char*) { return nullptr; }
#endif

#define ECFFT_HIP_TRY(x)                                                                   \
    do { hipError_t e_ = (x); if (e_ != hipSuccess) {                                      \
             fprintf(stderr, "ecfft: HIP error '%s' at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
             return false; } } while (0)

// Allocation failures inside the chain (table arena, temporaries) unwind to the C-ABI entry point, which maps them to
// ECFFT_ERR_HIP — a shared library must never abort() its host process.
struct DeviceAllocError : std::bad_alloc {
    const char* what() const noexcept override { return "ecfft: device allocation failed"; }
};

static inline unsigned ilog2(size_t n) { unsigned l = 0; while (n > 1) { n >>= 1; ++l; } return l; }
static inline size_t next_pow2(size_t n) { size_t m = 1; while (m < n) m <<= 1; return m; }
static inline unsigned nblocks(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

template <class Fn>
static inline void foreach_n(hipStream_t s, size_t n, Fn fn) {
    if (n) hipLaunchKernelGGL(k_foreach<Fn>, dim3(nblocks(n)), dim3(kBlock), 0, s, fn, n);
}


// ---------------------------------------------------------------------------------------------
// Optional per-launch timing with HIP events on the launch stream (bench.py's "roofline" object).
// Every hot-path launch goes through ECFFT_LAUNCH with a kernel class and the ALGORITHMIC bytes of
// that launch in the stage-streaming model of SURVEY.md section 8(d): each butterfly stage it covers
// reads and writes its operand once and reads its stage tables once; each pointwise step reads its
// operands and tables and writes its result once.
// ---------------------------------------------------------------------------------------------
enum KernelClass { KC_DECOMPOSE = 0, KC_RECOMBINE, KC_POINTWISE, KC_ROW, KC_COL, KC_FUSED_ENTER, KC_FUSED_EXIT, KC_COUNT };
static const char* const kKernelClassName[KC_COUNT] = {"k_decompose_stage", "k_recombine_stage", "pointwise",
                                                       "k_stages_lds", "k_stages_col", "k_enter_low", "k_exit_low"};

class Profiler {
public:
    bool on = false;
    ~Profiler() { for (hipEvent_t e : pool_) (void)hipEventDestroy(e); }
    void reset() { used_ = 0; recs_.clear(); for (int i = 0; i < KC_COUNT; ++i) { ms_[i] = 0; bytes_[i] = 0; n_[i] = 0; } }
    hipEvent_t next() {
        if (used_ == pool_.size()) { hipEvent_t e; (void)hipEventCreate(&e); pool_.push_back(e); }
        return pool_[used_++];
    }
    void begin(hipStream_t s, int cls, double bytes) {
        hipEvent_t a = next(); (void)hipEventRecord(a, s);
        recs_.push_back({cls, bytes, a, nullptr});
    }
    void end(hipStream_t s) { hipEvent_t b = next(); (void)hipEventRecord(b, s); recs_.back().stop = b; }
    void collect() {   // caller has synchronised the stream(s)
        for (const Rec& r : recs_) {
            float ms = 0; if (hipEventElapsedTime(&ms, r.start, r.stop) != hipSuccess) continue;
            ms_[r.cls] += ms; bytes_[r.cls] += r.bytes; n_[r.cls] += 1;
        }
        recs_.clear(); used_ = 0;
    }
    double ms(int c) const { return ms_[c]; }
    double bytes(int c) const { return bytes_[c]; }
    uint64_t launches(int c) const { return n_[c]; }
private:
    struct Rec { int cls; double bytes; hipEvent_t start, stop; };
    std::vector<hipEvent_t> pool_; size_t used_ = 0;
    std::vector<Rec> recs_;
    double ms_[KC_COUNT] = {}, bytes_[KC_COUNT] = {}; uint64_t n_[KC_COUNT] = {};
};

#define ECFFT_LAUNCH(cls, alg_bytes, kern, grid, block, lds, stream, ...)               \
    do { if (prof_.on) prof_.begin(stream, cls, (double)(alg_bytes));                  \
         hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);               \
         if (prof_.on) prof_.end(stream); } while (0)

#ifndef ECFFT_BATCH_SPLIT
#define ECFFT_BATCH_SPLIT 1
#endif
#ifndef ECFFT_SYM_BFLY
#define ECFFT_SYM_BFLY 1        // 0: general basis and two-multiply butterflies in every context
#endif
#ifndef ECFFT_BATCH_WAYS
#define ECFFT_BATCH_WAYS 2      // a batch runs as up to this many concurrent parts (whole polynomials each, one stream per part); A/B: profiles/r06/batch_ways_ab.txt
#endif
template <class F>
class DeviceChain {
public:
    using E = typename F::elem;
    using TE = typename F::telem;  // table constant in the form the kernels multiply by (secp256k1: the pair (t, t*2^128))
    using Tree = LevelTables<F>;   // per-tree table set (kernels.h); an array of them is mirrored on the device

    ~DeviceChain() { release(); }

    size_t size() const { return N_; }
    unsigned log_size() const { return L_; }
    const Tree& tree(unsigned log_m) const { return trees_[log_m]; }
    // the table set the EXTEND machinery uses for the tree with 2^log_m leaves: trees_ / sets_, unless a temporary share of that
    // tree is installed (the sharded EXIT build needs two different shares of one tree)
    const Tree& tree_at(unsigned log_m) const { return (ovr_tree_ && ovr_tree_->log_m == log_m) ? *ovr_tree_ : trees_[log_m]; }
    const HostTree<F>& host() const { return host_; }
    int exit_cores() const { return exit3_ ? 3 : 4; }        // EXTEND cores per EXIT level of exit_levels: the form of the context
    // EXTEND cores per level of k_exit_low's loop: the context's form, unless the build (-DECFFT_EXIT_LOW_CORES=4) or the A/B switch
    // keeps the four-core kernel under a three-core driver
    int exit_low_cores() const { return exit3_ && kExitLowForm == 3 && !exit_low4_ ? 3 : 4; }
    // butterfly form of the context: 0 = general basis and butterflies, 1 = symmetric basis with the one-multiply butterflies in the
    // full-size row and column passes, 2 = symmetric basis under the general kernels (A/B)
    int sym_bfly() const { return !sym_ ? 0 : (sym_general_kernels_ ? 2 : 1); }
    // which 1024-element low-level kernels run symmetric butterflies in their VALU sweeps: bit 0 = k_enter_low, bit 1 = k_exit_low
    // (bit 1 in three-core contexts only: the four-core kernel keeps the register engine)
    int low_sym() const { return (kLowSymEnter && low_sym_enter() ? 1 : 0) | (kLowSymExit && low_sym_exit() ? 2 : 0); }
    // 1: the EXTEND of ENTER level 11 (e = 1024) runs on the compile-time row engine in full-size launches, 0: on the run-time-tile row kernel
    int enter_l11() const { return trees_.size() > kLogTileMax + 1 && enter_l11_tuned(trees_[kLogTileMax + 1], 0) ? 1 : 0; }
    int low_map(int dir) const {
        if (trees_.size() > 5 && trees_[5].low32_A[dir]) return 32;
        if (trees_.size() > 4 && trees_[4].low16_A[dir]) return 16;
        return 0;
    }
    const E* f_device() const { return f_; }
    std::mutex& lock() { return mu_; }
    // test hook, process wide: the rank whose local part of the next collective ecfft_build_exit_shard reports failure (-1: none).
    // Set through the ABI only (ecfft_test_fail_build_rank) — no environment variable can reach it.
#ifdef ECFFT_TEST_HOOKS
    static std::atomic<int>& test_fail_build_rank() { static std::atomic<int> r{-1}; return r; }
#endif
    Profiler& profiler() const { return prof_; }

    // ------------------------------------------------------------------------------------------
    // construction
    // ------------------------------------------------------------------------------------------
    bool build(HostTree<F>&& ht, int device) {
        host_ = std::move(ht);
        N_ = host_.n; L_ = ilog2(N_); device_ = device;
        ECFFT_HIP_TRY(hipSetDevice(device_));
        hipStream_t s = nullptr;
        // arena per tree of m leaves: 6m elements of reference tables (xnn, z*) + 11m table constants of the hot path
        // (F::telem each); + f (2N) + den coefficients
        size_t total = 2 * N_ + 64 + 2 * (L_ ? L_ : 1) + 64;      // ... + the critical points of the maps
        for (unsigned l = 0; l <= L_; ++l) total += (6 + 11 * kTeElems) * ((size_t)1 << l) + 1024 + blk16_elems(l);
        // three-core EXIT: the Z1 set has one table more than the Z0 set it replaces (e constants per tree); the trees of the
        // low-level kernels hold both sets (6 e constants more, at most 2^kLogLow leaves)
        if (!exit4_) for (unsigned l = 1; l <= L_; ++l) total += (l <= kLogLow ? 6 : 1) * kTeElems * ((size_t)1 << l) / 2 + 64;   // + take()'s rounding of six tables
        total += low16_elems();
        ECFFT_HIP_TRY(hipMalloc(&arena_, total * sizeof(E)));
        arena_cap_ = total; arena_used_ = 0;
        f_ = take(2 * N_);
        if (!points_on_device(f_, s)) { fprintf(stderr, "ecfft: point set construction failed\n"); return false; }
        if (!exit4_) {
            // the three-core EXIT level divides by X^(m/2) on BOTH moieties: every leaf must be non-zero (the leaves of a subtree
            // are a subset of these, so one check covers every level); otherwise the context keeps the four-core form
            unsigned long long* zc = nullptr; unsigned long long hz = 0;
            ECFFT_HIP_TRY(hipMalloc(&zc, sizeof(unsigned long long)));
            (void)hipMemsetAsync(zc, 0, sizeof(unsigned long long), s);
            const E* leaves = f_ + N_;
            foreach_n(s, N_, [=] __device__(size_t j) { if (F::is_zero(leaves[j])) atomicAdd(zc, 1ull); });
            const bool got = hipMemcpyAsync(&hz, zc, sizeof(hz), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
            (void)hipFree(zc);
            if (!got) { (void)hipGetLastError(); return false; }
            exit3_ = hz == 0;
        }
        // denominators of the maps: v_k(x) = den0 + den1 x (degree 1 for both curve families)
        std::vector<E> den(2 * (L_ ? L_ : 1));
        for (unsigned k = 0; k < L_; ++k) { den[2 * k] = host_.maps[k].den[0]; den[2 * k + 1] = host_.maps[k].den[1]; }
        den_ = take(2 * (L_ ? L_ : 1));
        ECFFT_HIP_TRY(hipMemcpyAsync(den_, den.data(), den.size() * sizeof(E), hipMemcpyHostToDevice, s));
        // symmetric basis: the library's own tree of a 32-byte field whose maps all have rational critical points
        std::vector<E> crit(2 * (L_ ? L_ : 1), F::zero());
        sym_ = false;
        if constexpr (sizeof(E) == 32 && ECFFT_SYM_BFLY != 0) {
            if (host_.sym_candidate && !sym_off_ && L_ >= 1) {
                sym_ = true;
                for (unsigned k = 0; k < L_ && sym_; ++k) sym_ = critical_points<F>(host_.maps[k], &crit[2 * k], &crit[2 * k + 1]);
            }
        }
        crit_ = take(2 * (L_ ? L_ : 1));
        ECFFT_HIP_TRY(hipMemcpyAsync(crit_, crit.data(), crit.size() * sizeof(E), hipMemcpyHostToDevice, s));
        // transform scratch: 5 N (grown on demand for batched calls); side stream for the two-halves schedule
        if (!ensure_scratch(N_)) return false;
        create_side_streams();
        trees_.assign(L_ + 1, Tree{});
        {   // ~32 m temporaries are alive while T_m is built; one slab instead of ~80 hipMalloc/hipFree pairs per tree
            size_t want = 40 * N_ + 16384, cap_bytes = (size_t)16 << 30;
            if (want * sizeof(E) > cap_bytes) want = cap_bytes / sizeof(E);
            if (hipMalloc(&slab_, want * sizeof(E)) == hipSuccess) slab_cap_ = want; else { (void)hipGetLastError(); slab_ = nullptr; slab_cap_ = 0; }
            slab_used_ = 0;
        }
        for (unsigned l = 0; l <= L_; ++l) {
            if (!build_tree(l, s)) return false;
        }
        if (!build_low16(L_, s)) return false;
        ECFFT_HIP_TRY(hipStreamSynchronize(s));
        if (slab_) { (void)hipFree(slab_); slab_ = nullptr; slab_cap_ = slab_used_ = 0; }
        temps_free();
        ECFFT_HIP_TRY(hipMalloc(&d_trees_, (L_ + 1) * sizeof(Tree)));
        ECFFT_HIP_TRY(hipMemcpy(d_trees_, trees_.data(), (L_ + 1) * sizeof(Tree), hipMemcpyHostToDevice));
        return true;
    }

    // ------------------------------------------------------------------------------------------
    // SHARDED EXTEND context ("matrix tables shard the same way").  For ONE EXTEND of e evaluations split over
    // P = 2^log_p GPUs a rank never touches most of T_2e: the cyclic stages k < log_p read only the stage-table entries
    // i = i'*P + rank, the block-local stages k >= log_p only the last e/P entries of each stage table (pair distances <= e/2P),
    // the 1/W and W scalings only the rank's e/P positions, and no other tree of the chain and none of the z tables is needed at
    // all.  Everything a rank does need is pointwise in the point set (layers of f, isogeny denominators) plus batched
    // inversions, so it is built directly — no full tree ever exists on any GPU: ~24 e/P table constants instead of the 28*(2e)
    // elements of T_2e plus the 56e of the chain below it, and a build that is O(e/P) kernels' work instead of the chain's.
    // Layout: trees_[log2(2e)] holds BIASED pointers (base - first_needed_index) for the block-local stage tables and for
    // w / winv, so the single-GPU kernels index them unchanged; the cyclic entries live in compact arrays cyc_* laid out like the
    // stage tables of a length-e/P vector (stage k at offset e/P - 2*h_k/P).
    // ------------------------------------------------------------------------------------------
    // HBM held by this context between calls: table arena + transform scratch (pooled temporaries of the algorithm wrappers
    // and the host-call staging buffer come and go)
    size_t device_bytes() const { return (arena_cap_ + scratch_cap_) * sizeof(E) + pool_bytes() + full_cyc_bytes_; }
    // ecfft_ctx_trim: give every idle pooled temporary back to the device (between calls; takes the context lock)
    // `also`: runs under the same lock (the ABI layer frees its host-call staging buffer there: run_op / run_alg use it under lock())
    template <class Fn>
    void trim(Fn&& also) { std::lock_guard<std::mutex> g(mu_); temps_trim(0); (void)hipDeviceSynchronize(); full_cyclic_free(); also(); }
    enum { kShardNone = 0, kShardExtend = 1, kShardEnter = 2, kShardExit = 3 };
    int shard_kind() const { return shard_kind_; }
    bool shard_mode() const { return shard_kind_ != kShardNone; }
    unsigned shard_log_p() const { return shard_log_p_; }
    unsigned shard_rank() const { return shard_rank_; }
    // side streams of the two-halves schedule (enter_rec / exit_rec)
    void create_side_streams() {
        const int want = ((1 << kSplitDepth) - 1) > (ECFFT_BATCH_WAYS - 1) ? ((1 << kSplitDepth) - 1) : (ECFFT_BATCH_WAYS - 1);   // halves of one transform / parts of a batch
        for (nside_ = 0; nside_ < want && nside_ < kMaxSides; ++nside_) {
            if (hipStreamCreateWithFlags(&sides_[nside_], hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ev_fork_[nside_], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_join_[nside_], hipEventDisableTiming) != hipSuccess) break;
        }
    }
    // One rank's share of the EXTEND tables of the tree with 2^log_m leaves (a tree of the chain of T_N: its layer k is every
    // (N/m)-th point of the top tree's layer k) for a split over 2^log_p ranks; f = the device copy of the point set.
    struct ShardSet {
        bool valid = false; unsigned log_p = 0, rank = 0;
        TE* cyc[2][4] = {};      // per parity: np0, dinv, p0, p1 of the cyclic stages, compact
        TE* cycw[2][2] = {};     // per parity: w, winv of the rank's cyclic positions
    };
    // only_target = 0 / 1: keep only what EXTENDs towards that moiety read (decompose-side tables of the source parity,
    // recombine-side tables of the target parity): half the constants; -1: both directions
    static size_t shard_set_elems(size_t c, int only_target = -1) {
        return (only_target < 0 ? 2 : 1) * ((13 * c + 128) * kTeElems + (sizeof(E) == 32 ? Blk16::kArenaElems + 8 : 0)) + 64;   // + the matrix-core tables of the rank's row passes
    }
    bool build_shard_set(unsigned log_m, unsigned log_p, unsigned rank, const E* f, hipStream_t s, int only_target = -1,
                         Tree* tout = nullptr, ShardSet* sout = nullptr) {
        const size_t m = (size_t)1 << log_m, e = m / 2, P = (size_t)1 << log_p, c = e >> log_p, stride = N_ / m;
        if (log_m < 2 || c < P || c < 2 || rank >= P) return false;
        const unsigned le = log_m - 1;
        Tree& T = tout ? *tout : trees_[log_m]; ShardSet& S = sout ? *sout : sets_[log_m];
        T.m = m; T.e = e; T.log_m = log_m;
        S.valid = true; S.log_p = log_p; S.rank = rank;
        const size_t N = N_;
        const size_t loc0 = e - 2 * (e >> (log_p + 1));          // first entry of the block-local stages: e - 2*h_{log_p} = e - c
        const size_t nloc = c;                                   // entries [loc0, e) (the last one is padding, as in the full tables)
        E* plain[2][4];                                          // local p0, p1, np0, dinv (plain) for the inner constants
        for (int sg = 0; sg < 2; ++sg) {
            const bool dec = only_target < 0 || sg == 1 - only_target;       // this parity is an EXTEND source
            const bool rec = only_target < 0 || sg == only_target;           // ... an EXTEND target
            // ---- block-local stages k >= log_p: the last c entries of every stage table
            E *p0 = temp(nloc), *p1 = temp(nloc), *np0 = temp(nloc), *dinv = temp(nloc), *c0 = temp(nloc);
            (void)hipMemsetAsync(p0 + (nloc - 1), 0, sizeof(E), s); (void)hipMemsetAsync(p1 + (nloc - 1), 0, sizeof(E), s);
            (void)hipMemsetAsync(np0 + (nloc - 1), 0, sizeof(E), s); (void)hipMemsetAsync(dinv + (nloc - 1), 0, sizeof(E), s);
            foreach_n(s, nloc - 1, [=] __device__(size_t gl) {
                const size_t g = loc0 + gl, rem = e - g;         // same entry as build_tree's concatenated stage tables
                unsigned k = 0; size_t h = e >> 1;
                while (rem <= h) { h >>= 1; ++k; }
                const size_t i = g - (e - 2 * h), lay = N >> k;
                E a = f[lay + (2 * i + sg) * stride], b = f[lay + (2 * i + sg + 2 * h) * stride];
                p0[gl] = a; p1[gl] = b; np0[gl] = F::neg(a); dinv[gl] = F::sub(b, a);
            });
            batch_inv(dinv, dinv, nloc - 1, s);
            (void)hipMemsetAsync(c0 + (nloc - 1), 0, sizeof(E), s);
            foreach_n(s, nloc - 1, [=] __device__(size_t gl) { c0[gl] = F::mul(np0[gl], dinv[gl]); });
            plain[sg][0] = p0; plain[sg][1] = p1; plain[sg][2] = np0; plain[sg][3] = dinv;
            if (rec) { T.p0[sg] = to_tables(p0, nloc, s) - loc0; T.p1[sg] = to_tables(p1, nloc, s) - loc0; }
            if (dec) { T.np0[sg] = to_tables(np0, nloc, s) - loc0; T.dinv[sg] = to_tables(dinv, nloc, s) - loc0; T.c0t[sg] = to_tables(c0, nloc, s) - loc0; }
            // ---- cyclic stages k < log_p: entries i = i'*P + rank, compact, laid out like a length-c vector's stage tables
            const size_t ncyc = c;
            E *q0 = temp(ncyc), *q1 = temp(ncyc), *nq0 = temp(ncyc), *qd = temp(ncyc);
            (void)hipMemsetAsync(q0, 0, ncyc * sizeof(E), s); (void)hipMemsetAsync(q1, 0, ncyc * sizeof(E), s);
            (void)hipMemsetAsync(nq0, 0, ncyc * sizeof(E), s); (void)hipMemsetAsync(qd, 0, ncyc * sizeof(E), s);
            for (unsigned k = 0; k < log_p; ++k) {
                const size_t h = e >> (k + 1), hl = h >> log_p, offl = c - 2 * hl, lay = N >> k;
                foreach_n(s, hl, [=] __device__(size_t il) {
                    const size_t i = il * P + rank;
                    E a = f[lay + (2 * i + sg) * stride], b = f[lay + (2 * i + sg + 2 * h) * stride];
                    q0[offl + il] = a; q1[offl + il] = b; nq0[offl + il] = F::neg(a); qd[offl + il] = F::sub(b, a);
                });
            }
            batch_inv(qd, qd, ncyc, s);                          // zero padding stays zero
            if (dec) { S.cyc[sg][0] = to_tables(nq0, ncyc, s); S.cyc[sg][1] = to_tables(qd, ncyc, s); }
            if (rec) { S.cyc[sg][2] = to_tables(q0, ncyc, s); S.cyc[sg][3] = to_tables(q1, ncyc, s); }
            // ---- normalisation weights (DESIGN.md "Normalised butterflies") of the rank's c BLOCK positions g0 + il and of its
            // c CYCLIC positions il*P + rank (cyclic-in / cyclic-out calls)
            const E* dn = den_; const size_t g0 = (size_t)rank * c;
            for (int cyc = 0; cyc < 2; ++cyc) {
                E *w = temp(c), *wi = temp(c);
                foreach_n(s, c, [=] __device__(size_t il) {
                    const size_t j = 2 * (cyc ? il * P + rank : g0 + il) + sg;
                    E U = F::one(), C = F::one();
                    for (unsigned b = 0; b + 1 < le; ++b) {
                        const size_t lsz = m >> b;
                        E sb = f[(N >> b) + (j & (lsz - 1)) * stride];
                        E V = F::mul_add(dn[2 * b + 1], sb, dn[2 * b]);
                        C = F::mul(C, V);
                        U = F::mul(F::sqr(U), C);
                    }
                    w[il] = U;
                });
                batch_inv(w, wi, c, s);
                if (cyc) { if (rec) S.cycw[sg][0] = to_tables(w, c, s); if (dec) S.cycw[sg][1] = to_tables(wi, c, s); }
                else { if (rec) T.w[sg] = to_tables(w, c, s) - g0; if (dec) T.winv[sg] = to_tables(wi, c, s) - g0; }
            }
        }
        for (int sg = 0; sg < 2; ++sg) {                         // merged innermost stage pair (build_tree): entries at index e-2
            if (only_target >= 0 && sg != 1 - only_target) continue;   // indexed by the SOURCE parity
            E* in = temp(2);
            const size_t o = (e - 2) - loc0;
            const E *sp0 = plain[sg][0] + o, *sdi = plain[sg][3] + o, *tp0 = plain[1 - sg][0] + o, *tp1 = plain[1 - sg][1] + o;
            foreach_n(s, 1, [=] __device__(size_t) {
                in[0] = F::mul(F::sub(tp0[0], sp0[0]), sdi[0]);
                in[1] = F::mul(F::sub(tp1[0], sp0[0]), sdi[0]);
            });
            T.inner[sg] = to_tables(in, 2, s);
        }
        // matrix-core form of the innermost stages for the rank's block-local row passes (their table entries e-16 .. e-2 lie in the
        // stored range [e - c, e) whenever c >= 16); an EXTEND from parity sg reads the decompose tables of sg and the recombine
        // tables of 1 - sg
        T.blk16_A[0] = T.blk16_A[1] = nullptr; T.blk16_K[0] = T.blk16_K[1] = nullptr;
        if constexpr (sizeof(E) == 32) {
            if (c >= 16 && !mfma_off_) {
                for (int sg = 0; sg < 2; ++sg) {
                    if (only_target >= 0 && sg != 1 - only_target) continue;
                    uint8_t* A = reinterpret_cast<uint8_t*>(take(Blk16::kArenaElems));
                    unsigned long long* K = reinterpret_cast<unsigned long long*>(A + Blk16::kABytes);
                    const Blk16BuildArgs ba{T.np0[sg], T.dinv[sg], T.p0[1 - sg], T.p1[1 - sg], T.inner[sg], A, K};
                    hipLaunchKernelGGL(k_blk16_build, dim3(1), dim3(256), 0, s, ba, ba, e);
                    T.blk16_A[sg] = A; T.blk16_K[sg] = K;
                }
            }
        }
        return hipGetLastError() == hipSuccess;
    }
    // z0_s1[i] = Z_0(s1_i) (and z1_s0[i] = Z_1(s0_i)) of the tree with 2^log_m leaves WITHOUT any EXTEND: S0 is the leaf set of
    // the subtree, and the vanishing polynomial of a leaf set factors through the isogeny chain — with A_k the image of the set in
    // layer k (|A_k| = 2^(K-k), K = log m - 1) and psi_k = u_k / v_k, Z_{A_k}(x) = Z_{A_{k+1}}(psi_k(x)) * v_k(x)^|A_{k+1}| /
    // lc(u_k)^|A_{k+1}|, down to the single point A_K.  The images psi_{k-1}(..psi_0(x)) of a LEAF x are the stored layers of the
    // point set, so Z(x) = (x_K - root) * prod_k (v_k(x_k) / lc(u_k))^(2^(K-1-k)): K squarings and 2K multiplies per point.
    // (The same holds for S1: its images are the odd-indexed points of every layer.)  which = 0: out[j] = z0_s1[i0 + j*istride];
    // which = 1: out[j] = z1_s0[i0 + j*istride].  lcinv = 1 / lc(u_k), k < log N.  Used by the sharded EXIT build; build_tree keeps the
    // reference's EXTEND-based construction (src/fftree.rs:386-397) and ecfft_selfcheck_pointwise_z compares the two.
    void pointwise_z(unsigned log_m, int which, size_t i0, size_t cnt, E* out, const E* f, const E* lcinv, hipStream_t s, size_t istride = 1) const {
        const size_t m = (size_t)1 << log_m, stride = N_ / m, N = N_;
        const unsigned K = log_m - 1; const E* dn = den_;
        foreach_n(s, cnt, [=] __device__(size_t j) {
            const size_t leaf = (2 * (i0 + j * istride) + (which == 0 ? 1 : 0)) * stride;  // index in the top tree's layer 0
            E U = F::one();
            for (unsigned k = 0; k < K; ++k) {
                const size_t lsz = N >> k;
                const E xk = f[lsz + (leaf & (lsz - 1))];
                const E ck = F::mul(F::mul_add(dn[2 * k + 1], xk, dn[2 * k]), lcinv[k]);
                U = k == 0 ? ck : F::mul(F::sqr(U), ck);
            }
            const size_t lsz = N >> K;
            const E xK = f[lsz + (leaf & (lsz - 1))], root = f[lsz + (which == 0 ? 0 : (stride & (lsz - 1)))];
            out[j] = F::mul(U, F::sub(xK, root));
        });
    }
    // 1 / lc(u_k) for every map of the chain, on the device (temporary)
    E* upload_lcinv(hipStream_t s) {
        std::vector<E> h(L_ ? L_ : 1, F::one());
        for (unsigned k = 0; k < L_; ++k) h[k] = F::inv(host_.maps[k].num[2]);
        E* d = temp(h.size());
        (void)hipMemcpyAsync(d, h.data(), h.size() * sizeof(E), hipMemcpyHostToDevice, s);
        (void)hipStreamSynchronize(s);
        return d;
    }
    // test hook: number of entries of z0_s1 / z1_s0 of T_m (full context) that differ from the pointwise formula
    long selfcheck_pointwise_z(size_t m) {
        if (shard_mode() || m < 2 || m > N_) return -1;
        const unsigned lm = ilog2(m); const size_t e = m / 2; hipStream_t s = nullptr;
        E* lc = upload_lcinv(s); E* a = temp(e); E* b = temp(e);
        unsigned long long* bad = reinterpret_cast<unsigned long long*>(temp(8));
        (void)hipMemsetAsync(bad, 0, sizeof(unsigned long long), s);
        pointwise_z(lm, 0, 0, e, a, f_, lc, s); pointwise_z(lm, 1, 0, e, b, f_, lc, s);
        const E *z0 = trees_[lm].z0_s1, *z1 = trees_[lm].z1_s0;
        foreach_n(s, e, [=] __device__(size_t i) {
            if (!F::eq(F::canon(a[i]), F::canon(z0[i])) || !F::eq(F::canon(b[i]), F::canon(z1[i]))) atomicAdd(bad, 1ull);
        });
        unsigned long long h = 0;
        bool ok = hipMemcpyAsync(&h, bad, sizeof(h), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        temps_done();
        return ok ? (long)h : -1;
    }
    // The point set f (2N elements: layer k at [N >> k, 2*(N >> k))) into fdev: uploaded when the host tree carries it (trees made
    // from user leaves, ecfft_fftree_new), otherwise COMPUTED HERE from the generator data — the FftreeField::build_fftree front
    // end (src/lib.rs:66-81, src/ec.rs:545-551) and FFTree::new's layers (src/fftree.rs:42-70) as GPU passes: leaf i = x(off + i*gen)
    // through log N rounds of batched affine additions P_{r+j} = P_r + P_j (one batched inversion per round), then layer k+1 =
    // psi_k(layer k) pointwise with a batched inversion of the denominators.  Same field elements as host_curve.h produces (the
    // host path stays for ecfft_build_points and as the cross-check in the tests); 2^23 points: milliseconds instead of seconds.
    bool points_on_device(E* fdev, hipStream_t s) {
        const size_t n = N_;
        if (!host_.f.empty() && !host_.leaves_only) { ECFFT_HIP_TRY(hipMemcpyAsync(fdev, host_.f.data(), 2 * n * sizeof(E), hipMemcpyHostToDevice, s)); return true; }
        if (!host_.have_gen && !host_.leaves_only) return false;
        const E a2 = host_.curve.a2, a4 = host_.curve.a4, offx = host_.off.x, offy = host_.off.y;
        E* den = temp(n);
        unsigned long long* bad = reinterpret_cast<unsigned long long*>(temp(8));
        (void)hipMemsetAsync(bad, 0, sizeof(unsigned long long), s);
        (void)hipMemsetAsync(fdev, 0, n * sizeof(E), s);          // f[0] is unused; the layers below the leaves are written next
        E* leaves = fdev + n;
        if (host_.leaves_only) {
            ECFFT_HIP_TRY(hipMemcpyAsync(leaves, host_.f.data() + n, n * sizeof(E), hipMemcpyHostToDevice, s));
        } else {
        E *px = temp(n), *py = temp(n);
        if (n > 1) {
            ECFFT_HIP_TRY(hipMemcpyAsync(px + 1, &host_.gen.x, sizeof(E), hipMemcpyHostToDevice, s));
            ECFFT_HIP_TRY(hipMemcpyAsync(py + 1, &host_.gen.y, sizeof(E), hipMemcpyHostToDevice, s));
        }
        for (size_t r = 1; 2 * r <= n && r < n; r <<= 1) {        // compute_leaves (host_curve.h): i*gen for every 0 < i < n
            const size_t cnt = r - 1;
            if (cnt) {
                foreach_n(s, cnt, [=] __device__(size_t t) { den[t] = F::sub(px[t + 1], px[r]); });
                batch_inv(den, den, cnt, s);
                foreach_n(s, cnt, [=] __device__(size_t t) {
                    const size_t j = t + 1;
                    const E xr = px[r], yr = py[r];
                    const E lambda = F::mul(F::sub(py[j], yr), den[t]);
                    const E x3 = F::sub(F::sub(F::sub(F::sqr(lambda), a2), xr), px[j]);
                    px[r + j] = x3;
                    py[r + j] = F::sub(F::mul(lambda, F::sub(xr, x3)), yr);
                });
            }
            if (2 * r < n) foreach_n(s, 1, [=] __device__(size_t) {   // P_{2r} = 2 * P_r (pt_add with p == q)
                const E x = px[r], y = py[r], xx = F::sqr(x);
                const E num = F::add(F::add(F::add(xx, xx), xx), F::add(F::mul(F::add(a2, a2), x), a4));
                const E lambda = F::mul(num, F::inv(F::add(y, y)));
                const E x3 = F::sub(F::sub(F::sub(F::sqr(lambda), a2), x), x);
                px[2 * r] = x3; py[2 * r] = F::sub(F::mul(lambda, F::sub(x, x3)), y);
            });
        }
        foreach_n(s, 1, [=] __device__(size_t) { leaves[0] = offx; });
        if (n > 1) {
            foreach_n(s, n - 1, [=] __device__(size_t t) { den[t] = F::sub(px[t + 1], offx); });
            batch_inv(den, den, n - 1, s);
            foreach_n(s, n - 1, [=] __device__(size_t t) {
                const size_t i = t + 1;
                const E lambda = F::mul(F::sub(py[i], offy), den[t]);
                leaves[i] = F::sub(F::sub(F::sub(F::sqr(lambda), a2), offx), px[i]);
            });
        }
        }
        unsigned k = 0;
        for (size_t sz = n; sz > 1; ++k, sz >>= 1) {              // fill_layers (host_curve.h / src/fftree.rs:42-70)
            const size_t half = sz / 2;
            const E* prev = fdev + sz; E* layer = fdev + half;
            const RatMap<F> m = host_.maps[k];
            foreach_n(s, half, [=] __device__(size_t j) {
                const E x = prev[j];
                const E d = F::mul_add(F::mul_add(m.den[2], x, m.den[1]), x, m.den[0]);
                if (F::is_zero(d)) atomicAdd(bad, 1ull);
                den[j] = d;
            });
            batch_inv(den, den, half, s);
            foreach_n(s, half, [=] __device__(size_t j) {
                const E x = prev[j];
                layer[j] = F::mul(F::mul_add(F::mul_add(m.num[2], x, m.num[1]), x, m.num[0]), den[j]);
            });
        }
        unsigned long long h = 0;
        ECFFT_HIP_TRY(hipMemcpyAsync(&h, bad, sizeof(h), hipMemcpyDeviceToHost, s));
        ECFFT_HIP_TRY(hipStreamSynchronize(s));
        temps_done();
        bad_points_ = h != 0;                                      // a leaf is a pole of its isogeny map: not a valid point set
        return h == 0 && hipGetLastError() == hipSuccess;
    }
    bool bad_points() const { return bad_points_; }
    bool upload_points(E*& fdev, hipStream_t s) {               // the caller hipFree()s fdev
        ECFFT_HIP_TRY(hipMalloc(&fdev, 2 * N_ * sizeof(E)));
        if (!points_on_device(fdev, s)) { (void)hipFree(fdev); fdev = nullptr; return false; }
        std::vector<E> den(2 * (L_ ? L_ : 1));
        for (unsigned k = 0; k < L_; ++k) { den[2 * k] = host_.maps[k].den[0]; den[2 * k + 1] = host_.maps[k].den[1]; }
        den_ = take(2 * (L_ ? L_ : 1));
        if (hipMemcpyAsync(den_, den.data(), den.size() * sizeof(E), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {             // `den` is a stack vector; fdev must not leak on this path either
            (void)hipGetLastError(); (void)hipFree(fdev); fdev = nullptr; return false;
        }
        return true;
    }
    bool build_extend_shard(HostTree<F>&& ht, int device, unsigned log_p, unsigned rank) {
        host_ = std::move(ht);
        N_ = host_.n; L_ = ilog2(N_); device_ = device;
        const size_t c = (N_ / 2) >> log_p;
        if (L_ < 2 || c < ((size_t)1 << log_p) || c < 2 || rank >= ((size_t)1 << log_p)) return false;
        ECFFT_HIP_TRY(hipSetDevice(device_));
        hipStream_t s = nullptr;
        // arena: den + per parity {5 local tables + 4 cyclic tables + w + winv of the block and of the cyclic positions} of c
        // constants each + inner.  The point set f (all layers, 2N elements) is needed only while the tables are computed: a
        // temporary, freed before returning.
        size_t total = 64 + 2 * L_ + shard_set_elems(c) + 4096;
        ECFFT_HIP_TRY(hipMalloc(&arena_, total * sizeof(E)));
        arena_cap_ = total; arena_used_ = 0;
        E* fdev = nullptr;
        if (!upload_points(fdev, s)) return false;
        trees_.assign(L_ + 1, Tree{}); sets_.assign(L_ + 1, ShardSet{});
        const bool built = build_shard_set(L_, log_p, rank, fdev, s);
        const bool drained = hipStreamSynchronize(s) == hipSuccess;
        (void)hipFree(fdev);
        temps_free();
        if (!built || !drained) { fprintf(stderr, "ecfft: shard table build failed\n"); return false; }
        host_.f.clear(); host_.f.shrink_to_fit();                // the host copy of the point set is not needed either
        shard_kind_ = kShardExtend; shard_log_p_ = log_p; shard_rank_ = rank;
        return true;
    }

    // SHARDED ENTER context for ONE ENTER of n coefficients split over P = 2^log_p GPUs (api_enter_split): the full chain
    // T_1 .. T_c, c = n/P, for the rank-local low levels (every rank runs the same ENTER of its chunk on T_c), and for each of
    // the log P top levels m = c*Q only the rank's share of T_m: the EXTEND tables of the split over its half-group (a ShardSet
    // with 2^log_p' = Q/2, rank' = rank mod Q/2; Q = 2 is a local EXTEND = the "split" over one rank) and the c entries of
    // xnn_s = leaf^(m/2) its combine step reads (the positions i'*Q + a it owns in the level's cyclic order).  All pointwise in the point set: no tree above T_c is materialised anywhere.
    // ~56 c elements for the chain + 13 c constants per top level (ENTER only extends towards S1) instead of 56 n.
    bool build_enter_shard(HostTree<F>&& ht, int device, unsigned log_p, unsigned rank) {
        host_ = std::move(ht);
        N_ = host_.n; L_ = ilog2(N_); device_ = device;
        const size_t P = (size_t)1 << log_p, c = N_ >> log_p;
        if (log_p == 0 || L_ < 2 || c < 2 * P || rank >= P) return false;
        const unsigned lc = ilog2(c);
        ECFFT_HIP_TRY(hipSetDevice(device_));
        hipStream_t s = nullptr;
        size_t total = 64 + 2 * L_ + 4096;
        for (unsigned l = 0; l <= lc; ++l) total += (6 + 11 * kTeElems) * ((size_t)1 << l) + 1024 + blk16_elems(l);
        total += log_p * (shard_set_elems(c, 1) + c + 64);
        total += low16_elems();
        ECFFT_HIP_TRY(hipMalloc(&arena_, total * sizeof(E)));
        arena_cap_ = total; arena_used_ = 0;
        E* fdev = nullptr;
        if (!upload_points(fdev, s)) return false;
        struct Free { E* p; ~Free() { (void)hipFree(p); } } free_f{fdev};
        f_ = fdev;                                               // build_tree reads f_; reset below
        if (!ensure_scratch(c)) return false;
        create_side_streams();                                   // the rank-local ENTER / EXIT of the chunk runs the two-halves schedule too
        trees_.assign(L_ + 1, Tree{}); sets_.assign(L_ + 1, ShardSet{});
        for (unsigned l = 0; l <= lc; ++l) { if (!build_tree(l, s)) { f_ = nullptr; return false; } }
        if (!build_low16(lc, s)) { f_ = nullptr; return false; }
        for (size_t Q = 2; Q <= P; Q *= 2) {
            const size_t half = Q / 2, m = c * Q;
            const unsigned lm = ilog2(m);
            const size_t a = rank % Q, stride = N_ / m;
            if (!build_shard_set(lm, ilog2(half), (unsigned)(a % half), fdev, s, 1)) { f_ = nullptr; return false; }   // ENTER extends towards S1 only
            E* x = take(c); const E* f = fdev; const size_t N = N_; const uint64_t ex = m / 2;
            foreach_n(s, c, [=] __device__(size_t j) { x[j] = F::pow_u64(f[N + (j * Q + a) * stride], ex); });   // the rank's positions in the level's cyclic order
            trees_[lm].xnn = x;
            if (hipStreamSynchronize(s) != hipSuccess) { f_ = nullptr; return false; }
            temps_free();
        }
        f_ = nullptr;
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) { fprintf(stderr, "ecfft: kernel launch failed: %s\n", hipGetErrorString(err)); return false; }
        ECFFT_HIP_TRY(hipStreamSynchronize(s));
        temps_free();
        host_.f.clear(); host_.f.shrink_to_fit();
        ECFFT_HIP_TRY(hipMalloc(&d_trees_, (L_ + 1) * sizeof(Tree)));
        ECFFT_HIP_TRY(hipMemcpy(d_trees_, trees_.data(), (L_ + 1) * sizeof(Tree), hipMemcpyHostToDevice));
        shard_kind_ = kShardEnter; shard_log_p_ = log_p; shard_rank_ = rank;
        return true;
    }

    // SHARDED EXIT context for ONE EXIT of n evaluations split over the P ranks of `tr` (api_exit_split) — a COLLECTIVE build: the
    // full chain T_1 .. T_c (c = n/P) for the rank-local low levels, and for each top level m = c*Q the rank's share of T_m: the
    // EXTEND tables of the split over its group of Q ranks (both directions, hc = c/2 entries per rank), its c entries of xnn_s
    // and 1/xnn_s, its hc entries of 1/z0_s1 (pointwise_z), and its c entries of z0z0_rem_xnn_s.  The last is (Z_0^2 mod X^(m/2))
    // on the leaves — a truncation in the monomial basis, not pointwise — and is built the way the reference builds it
    // (src/fftree.rs:418-452) but distributed, level by level, with the very operators the split EXIT consists of:
    //   zz0 = modular_reduce_{T_(m/2)}(z0z0' * z1z1') over the half-group (on the blocks of T_(m/2)'s tables from the level below),
    //   zz1 = EXTEND_{T_m}(zz0 -> S1) inside the half-group (a temporary one-direction share of T_m), one exchange re-blocks
    //   interleave(zz0, zz1) over the whole group, then two modular reductions on T_m over the group give the rank's blocks of
    //   z0z0_rem_xnn_s and z1z1_rem_xnn_s (the latter only feeds the next level).  No tree above T_c exists on any GPU.
    struct TempArena {           // to_tables() / take() allocate from a scratch region while this lives
        DeviceChain* ch; E* a; size_t cap, used; E* mine = nullptr;
        TempArena(DeviceChain* c, size_t elems) : ch(c), a(c->arena_), cap(c->arena_cap_), used(c->arena_used_) {
            if (hipMalloc(&mine, elems * sizeof(E)) != hipSuccess) { (void)hipGetLastError(); throw DeviceAllocError(); }
            ch->arena_ = mine; ch->arena_cap_ = elems; ch->arena_used_ = 0;
        }
        ~TempArena() { ch->arena_ = a; ch->arena_cap_ = cap; ch->arena_used_ = used; (void)hipFree(mine); }
    };
    // min_memory: never keep the full tree T_2c — the pair level then runs as four split EXTENDs (9 exchanges instead of 1) and the
    // context holds no tree above T_c at all.  Otherwise T_2c is kept when it fits this rank's free memory, and the ranks AGREE on
    // the form (one rank short of memory => every rank takes the split form): ADVICE r04.
    bool build_exit_shard(HostTree<F>&& ht, int device, Transport& tr, bool min_memory = false) {
        host_ = std::move(ht);
        N_ = host_.n; L_ = ilog2(N_); device_ = device;
        const size_t P = (size_t)tr.world;
        if (P < 2 || (P & (P - 1))) return false;
        const unsigned log_p = ilog2(P), rank = (unsigned)tr.rank;
        const size_t c = N_ >> log_p, hc = c / 2;
        if (L_ < 2 || c < 2 * P || hc < P || rank >= P) return false;
        const unsigned lc = ilog2(c);
        ECFFT_HIP_TRY(hipSetDevice(device_));
        hipStream_t s = nullptr;
        E* fdev = nullptr; E* lc_inv = nullptr;
        struct Free { E*& p; DeviceChain* ch; ~Free() { if (p) (void)hipFree(p); ch->f_ = nullptr; ch->ovr_tree_ = nullptr; ch->ovr_set_ = nullptr; } } free_f{fdev, this};
        // Form of the pair level (groups of two ranks), agreed before anything is allocated.  Redundant (round 4): the chain goes up
        // to T_2c and both ranks of a pair run the level on the whole 2c block from ONE exchange (api_exit_split) — for P = 2 the
        // context is then as large as a full one.  Split: no tree above T_c, the level is four split EXTENDs on the ranks' shares (9
        // exchanges) — the form for transforms whose tables exceed a GPU, chosen with min_memory or when T_2c does not fit the free
        // memory of ANY rank (Transport::vote is an AND over the ranks).
        auto arena_elems = [&](bool red) {
            size_t total = 64 + 3 * L_ + 4096;
            for (unsigned l = 0; l <= lc + (red ? 1u : 0u); ++l) total += (6 + 11 * kTeElems) * ((size_t)1 << l) + 1024 + blk16_elems(l);
            if (P > 2 || !red) total += log_p * (shard_set_elems(hc) + 5 * c + 256);   // P = 2, redundant: the pair level is the only top level — no share at all
            return total + low16_elems();
        };
        bool want_red = !min_memory;
        if (want_red) {
            size_t fr = 0, tt = 0;
            // arena + point set (2N) + transform scratch and pooled temporaries of the block level (~16 c) + headroom
            const size_t need = (arena_elems(true) + 2 * N_ + 16 * c) * sizeof(E) + ((size_t)256 << 20);
            if (hipMemGetInfo(&fr, &tt) != hipSuccess) { (void)hipGetLastError(); want_red = false; } else want_red = need <= fr;
        }
        if (const char* tr_rank = ab_env("ECFFT_TEST_PAIR_SPLIT_RANK")) if (atoi(tr_rank) == (int)rank) want_red = false;   // test builds: this rank "does not fit"
        const bool red = tr.vote(want_red, s);
        // everything up to the first exchange is LOCAL work that can fail on one rank only (allocations, the chain up to n/P):
        // the ranks agree on its outcome before any of them enters the collective part
        auto local_part = [&]() -> bool {
            try {
                const size_t total = arena_elems(red);
                ECFFT_HIP_TRY(hipMalloc(&arena_, total * sizeof(E)));
                arena_cap_ = total; arena_used_ = 0;
                if (!upload_points(fdev, s)) return false;
                f_ = fdev;                                               // build_tree reads f_
                if (!ensure_scratch(2 * c)) return false;
                create_side_streams();                                   // the rank-local ENTER / EXIT of the chunk runs the two-halves schedule too
                trees_.assign(L_ + 1, Tree{}); sets_.assign(L_ + 1, ShardSet{});
                for (unsigned l = 0; l <= lc + (red ? 1u : 0u); ++l) if (!build_tree(l, s)) return false;
                if (red) { pair_full_ = trees_[lc + 1]; have_pair_full_ = true; }   // the level-Q=2 iteration below re-points trees_[lc + 1] at the rank's shares (the distributed
                                                                         // build of the level above still splits T_2c over the pairs); the full tables stay in the arena
                if (!build_low16(lc, s)) return false;
                lc_inv = take(L_);
                std::vector<E> h(L_, F::one());
                for (unsigned k = 0; k < L_; ++k) h[k] = F::inv(host_.maps[k].num[2]);
                ECFFT_HIP_TRY(hipMemcpy(lc_inv, h.data(), L_ * sizeof(E), hipMemcpyHostToDevice));
                return !fail_next_collective_;
            } catch (const DeviceAllocError&) { return false; }
        };
        bool local_ok = local_part();
        fail_next_collective_ = false;
#ifdef ECFFT_TEST_HOOKS
        if (test_fail_build_rank().load() == (int)rank) local_ok = false;   // test hook (ecfft_test_fail_build_rank): this rank's local part "fails"
#endif
        if (!tr.vote(local_ok, s)) { fprintf(stderr, "ecfft: sharded EXIT build: the local part failed on %s rank\n", local_ok ? "another" : "this"); return false; }
        shard_kind_ = kShardExit; shard_log_p_ = log_p; shard_rank_ = rank;      // extend_split must read the shares from here on
        const E* f = fdev; const size_t N = N_;
        bool ok = true;
        E *pz0[2] = {nullptr, nullptr}, *pz1[2] = {nullptr, nullptr};     // the level below: z0z0 / z1z1 _rem_xnn_s on the rank's S0 / S1 positions
        for (size_t Q = 2; ok && Q <= P; Q *= 2) {
            if (P == 2 && red) break;                                      // redundant pair level: the shares of T_2c only feed the distributed build of the level above
            const size_t half = Q / 2, m = c * Q, stride = N_ / m;
            const unsigned lm = ilog2(m), lq = ilog2(Q), lh = ilog2(half);
            const int base = (int)((rank / Q) * Q), a = (int)rank - base, g = a / (int)half, ap = a % (int)half, subbase = base + g * (int)half;
            // Every length-m/2 vector of the level is CYCLIC over the group: entry j of the rank = position j*Q + a (api_exit_split).
            // ---- permanent: the rank's share of T_m for the level's split EXTENDs + its pointwise entries, compact
            bool lvl_ok = false;
            try { lvl_ok = build_shard_set(lm, lq, (unsigned)a, fdev, s, -1); } catch (const DeviceAllocError&) { lvl_ok = false; }
            if (!tr.vote(lvl_ok, s)) return false;                         // the level's exchanges follow: all ranks or none
            Tree& T = trees_[lm];
            E *xe = temp(hc), *xei = take(hc), *xo = take(hc), *zib = take(hc), *c0 = take(hc), *c1 = take(hc), *q0 = take(hc), *q1 = take(hc);
            { const uint64_t ex = m / 2; const size_t qq = Q, aa = (size_t)a;
              foreach_n(s, hc, [=] __device__(size_t j) { const size_t i = j * qq + aa; xe[j] = F::pow_u64(f[N + (2 * i) * stride], ex); xo[j] = F::pow_u64(f[N + (2 * i + 1) * stride], ex); }); }
            batch_inv(xe, xei, hc, s);
            E* zb = temp(hc);                                                      // z0_s1 on the rank's S1 positions (plain), also used below
            pointwise_z(lm, 0, (size_t)a, hc, zb, fdev, lc_inv, s, Q);
            batch_inv(zb, zib, hc, s);
            // in an EXIT-shard context these fields of a top tree are the rank's COMPACT views: 1/xnn_s on its S0 positions, xnn_s on
            // its S1 positions, 1/z0_s1, z0z0_rem_xnn_s on its S0 positions (z0z0) and on its S1 positions (z1z1 field)
            T.xnn_inv = xei; T.xnn = xo; T.z0_inv_s1 = zib; T.z0z0 = c0; T.z1z1 = c1;
            // ---- zz0 = modular_reduce_{T_(m/2)}(z0z0' * z1z1', c = z0z0') (:421-425), then as a length-m/2 vector cyclic over the HALF-group
            E *Z = temp(c), *ZZ1 = temp(c);
            E *e0 = temp(hc), *e1 = temp(hc), *h0 = temp(hc), *h1 = temp(hc), *t0 = temp(hc), *x0 = temp(hc), *x1 = temp(hc), *A = temp(c), *B = temp(c);
            if (half == 1) {
                const Tree& S = trees_[lc];
                E* sq = temp(c);
                ew_mul(sq, S.z0z0, S.z1z1, c, s);
                { const E *xi = S.xnn_inv, *x = S.xnn; foreach_n(s, hc, [=] __device__(size_t i) { e0[i] = xi[2 * i]; e1[i] = x[2 * i + 1]; }); }
                b_modular_reduce(lc, sq, e0, e1, S.z0z0, Z, s);                      // natural order = cyclic over one rank
            } else {
                const Tree& S = trees_[lm - 1];                                   // compact views of T_(m/2), built one level down (rank ap of the half-group)
                { const E *a0 = pz0[0], *a1 = pz0[1], *b0 = pz1[0], *b1 = pz1[1]; foreach_n(s, hc, [=] __device__(size_t j) { e0[j] = F::mul(a0[j], b0[j]); e1[j] = F::mul(a1[j], b1[j]); }); }
                ok = modred_split(tr, subbase, lh, m / 2, e0, e1, h0, h1, S.xnn_inv, S.xnn, 1, S.z0_inv_s1, 1, S.z0z0, S.z1z1, 1, t0, x0, x1, A, B, s, true);
                if (!ok) break;
                // (h0, h1)[j] = zz0 at index i = j*Q + 2*ap + {0, 1} of the length-m/2 vector; as a vector cyclic over the half-group,
                // index i sits on sub-rank i mod half at slot i / half = 2j + t, t = (2*ap + b) / half
                const int hq = (int)half;
                P2P snd[2] = {{subbase + (2 * ap) % hq, h0, hc * sizeof(E)}, {subbase + (2 * ap + 1) % hq, h1, hc * sizeof(E)}};
                const int par = ap & 1, s1 = (ap - par) / 2, s2 = s1 + hq / 2;       // the two senders whose (2*a' + par) mod half == ap
                P2P rcv[2] = {{subbase + s1, e0, hc * sizeof(E)}, {subbase + s2, e1, hc * sizeof(E)}};
                ok = tr.exchange(snd, 2, rcv, 2, s);
                if (!ok) break;
                const size_t ta = (size_t)((2 * s1 + par) / hq), tb = (size_t)((2 * s2 + par) / hq);
                foreach_n(s, hc, [=] __device__(size_t j) { Z[2 * j + ta] = e0[j]; Z[2 * j + tb] = e1[j]; });
            }
            // ---- zz1 = EXTEND_{T_m}(zz0 -> S1) inside the half-group, c entries per rank, cyclic  (:426)
            {
                TempArena ta(this, shard_set_elems(c, 1) + 4096);
                Tree tt{}; ShardSet ts{};
                if (!build_shard_set(lm, lh, (unsigned)ap, fdev, s, 1, &tt, &ts)) return false;
                ovr_tree_ = &tt; ovr_set_ = &ts;
                ok = half == 1 ? extend(Z, ZZ1, c, 1, 1, s) : extend_split(tr, subbase, lh, Z, ZZ1, m / 2, 1, s, A, B, true, true);
                ok = (hipStreamSynchronize(s) == hipSuccess) && ok;
                ovr_tree_ = nullptr; ovr_set_ = nullptr;
            }
            if (!ok) break;
            // ---- zz = interleave(zz0, zz1) (:427-429) on the rank's positions 2*(j*Q + a) + {0, 1}: index i = j*Q + a of zz0 / zz1 sits
            // on this very rank (i mod half = ap) at slot i / half = 2j + g — no exchange
            E *zc0 = temp(hc), *zc1 = temp(hc);
            { const size_t gg = (size_t)g; foreach_n(s, hc, [=] __device__(size_t j) { zc0[j] = Z[2 * j + gg]; zc1[j] = ZZ1[2 * j + gg]; }); }
            // ---- z0z0_rem_xnn_s on the rank's positions  (:430-446)
            E *xqe = temp(hc), *xqo = temp(hc), *xqei = temp(hc), *xqoi = temp(hc);
            { const uint64_t ex = m / 4; const size_t qq = Q, aa = (size_t)a;
              foreach_n(s, hc, [=] __device__(size_t j) { const size_t i = j * qq + aa; xqe[j] = F::pow_u64(f[N + (2 * i) * stride], ex); xqo[j] = F::pow_u64(f[N + (2 * i + 1) * stride], ex); }); }
            batch_inv(xqe, xqei, hc, s); batch_inv(xqo, xqoi, hc, s);
            foreach_n(s, hc, [=] __device__(size_t j) {                          // even leaf: z0 = 0; odd leaf: z0 = z0_s1
                e0[j] = F::mul(F::sub(F::sqr(xe[j]), zc0[j]), xqei[j]);
                e1[j] = F::mul(F::sub(F::sqr(F::sub(zb[j], xo[j])), zc1[j]), xqoi[j]);
            });
            ok = modred_split(tr, base, lq, m, e0, e1, h0, h1, xqei, xqo, 1, zib, 1, zc0, zc1, 1, t0, x0, x1, A, B, s, true);
            if (!ok) break;
            foreach_n(s, hc, [=] __device__(size_t j) { c0[j] = F::mul_add(xqe[j], h0[j], zc0[j]); c1[j] = F::mul_add(xqo[j], h1[j], zc1[j]); });
            // ---- z1z1_rem_xnn_s on the rank's positions (:449-452): only the next level's zz0 reads it
            E* z1s = temp(hc);
            pointwise_z(lm, 1, (size_t)a, hc, z1s, fdev, lc_inv, s, Q);
            foreach_n(s, hc, [=] __device__(size_t j) { e0[j] = F::sqr(F::sub(z1s[j], xe[j])); e1[j] = F::sqr(xo[j]); });
            ok = modred_split(tr, base, lq, m, e0, e1, q0, q1, xei, xo, 1, zib, 1, c0, c1, 1, t0, x0, x1, A, B, s, true);
            if (!ok) break;
            pz0[0] = c0; pz0[1] = c1; pz1[0] = q0; pz1[1] = q1;
            if (hipStreamSynchronize(s) != hipSuccess) { ok = false; break; }
            temps_free();
        }
        ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        temps_free();
        ok = tr.vote(ok, s);                                                // every rank reports the same outcome
        if (!ok) { fprintf(stderr, "ecfft: sharded EXIT table build failed\n"); return false; }
        host_.f.clear(); host_.f.shrink_to_fit();
        ECFFT_HIP_TRY(hipMalloc(&d_trees_, (L_ + 1) * sizeof(Tree)));
        ECFFT_HIP_TRY(hipMemcpy(d_trees_, trees_.data(), (L_ + 1) * sizeof(Tree), hipMemcpyHostToDevice));
        return true;
    }

    // ------------------------------------------------------------------------------------------
    // EXTEND core: all 2*log(e) normalised stages on `total` elements = count vectors of length
    // e = m/2 laid end to end, as a chain of fused passes:
    //     [column passes: top decompose stages, <= 4 per pass] -> row pass (every stage with
    //     2h <= tile, decompose then recombine) -> [column passes: top recombine stages].
    // `io` describes where the first pass loads from (with an optional fused pointwise op) and what
    // the last pass does with its result; intermediate passes run in place on `buf`.
    // srcpar = parity of the moiety the data lives on.
    // ------------------------------------------------------------------------------------------
#ifndef ECFFT_LOG_TILE_BYTES
#define ECFFT_LOG_TILE_BYTES 15
#endif
#ifndef ECFFT_CT_ALL
#define ECFFT_CT_ALL 0      // 1: compile-time tile sizes for every field (default: 4-byte fields only)
#endif
#ifndef ECFFT_ENTER_L11_TUNED
#define ECFFT_ENTER_L11_TUNED 1      // 0: the EXTEND of an ENTER level with e = 1024 keeps the run-time-tile row kernel (A/B)
#endif
#ifndef ECFFT_ENTER_L11_THREADS
#define ECFFT_ENTER_L11_THREADS 1024 // threads per workgroup of k_enter_l11: 512 (the block's halves in turn) or 1024 (side by side)
#endif
    static constexpr unsigned kLogTileMax = (sizeof(E) == 32) ? ECFFT_LOG_TILE_BYTES - 5 : ECFFT_LOG_TILE_BYTES - 2;   // 32 KiB LDS tiles by default (A/B on MI355X: 512 threads x 32 KiB beat 64 KiB tiles by ~5%)
#ifndef ECFFT_COL_STAGES
#define ECFFT_COL_STAGES 9      // round 5: 9 (was 8) together with ECFFT_COL_MIN_LOGC 1 — the nine column stages of an EXTEND of 2^19 (every core of
#endif                          // level 20) run as ONE pass on tiles of 2^9 rows x 2 elements instead of two passes of 5 + 4 stages: 2^20 -1.4 %, 2^21 -0.8 %
#ifndef ECFFT_LOG_COL_TILE_BYTES
#define ECFFT_LOG_COL_TILE_BYTES 15
#endif
#ifndef ECFFT_COL_MIN_LOGC
#define ECFFT_COL_MIN_LOGC 1     // log2 of the shortest column-tile row of a full-size launch (2: rows of >= 4 elements = 128 B, rounds 1-4; 1: 64-byte rows
                                 // are accepted where they save a whole pass, i.e. for exactly nine column stages)
#endif
#ifndef ECFFT_COL_STAGES_4B
#define ECFFT_COL_STAGES_4B 9
#endif
    // max stages per column pass (A/B on MI355X: 8 stages x 4-element rows beat 5 x 32 on secp256k1; 9 x 16-element rows are 1 %
    // better than 8 on M31 at 2^24 and equal below, profiles/r02/knob_sweep.txt)
    static constexpr unsigned kColStages = sizeof(E) == 4 ? ECFFT_COL_STAGES_4B : ECFFT_COL_STAGES;
    static constexpr bool kSymKernels = sizeof(E) == 32 && ECFFT_SYM_BFLY != 0;   // the SYM instantiations exist for 32-byte fields only
    // ... and in the VALU sweeps of the 1024-element low-level ENTER kernel (-DECFFT_ENTER_LOW_SYM=0 keeps the general sweeps there)
    static constexpr bool kLowSymEnter = kSymKernels && ECFFT_ENTER_LOW_SYM != 0;
    // the EXTEND of an ENTER level with e = 1024 on the compile-time engine (k_enter_l11: one [u0 | v0] block per workgroup)
    static constexpr bool kEnterL11 = sizeof(E) == 32 && ECFFT_ENTER_L11_TUNED != 0 && kBlockRow == 512 && kLogTileMax == 10;
    // ... and of the three-core low-level EXIT kernel (-DECFFT_EXIT_LOW_SYM=0 keeps its register engine; kLowSymExit is defined next to kExitLowForm)
    static constexpr unsigned kLogColTileMax = (sizeof(E) == 32) ? ECFFT_LOG_COL_TILE_BYTES - 5 : ECFFT_LOG_COL_TILE_BYTES - 2;
    // Fusion of consecutive cores (EXIT): `next_ld` != nullptr says that another core of the same tree and size, opposite
    // direction, follows on `buf` with that load operator; if this core ends in a column pass, that pass and the next
    // core's first column pass run as ONE launch (k_stages_col_mid) and the function returns true; the next core is then
    // called with skip_first_col = true.
    struct NextLoad { int ld_mode; const TE* ld_tbl; double extra_first; };
    // ENTER fusion: `ef` != nullptr says that this core is the EXTEND of an ENTER level (total = whole [u0 | v0] blocks, target
    // S1) and that its LAST pass must also do the level's combine (src/fftree.rs:155-159) and write the level's output to
    // ef->dst — k_stages_col_enter when the core ends in a column pass, the row kernel's ST_ENTER store operator otherwise.
    struct EnterFuse { const E* src; E* dst; double extra; };
    bool extend_core(unsigned log_m, IoDesc<F> io, E* buf, size_t total, int srcpar, hipStream_t s,
                     double extra_first = 0.0, double extra_last = 0.0, unsigned k_begin = 0,
                     const NextLoad* next_ld = nullptr, bool skip_first_col = false, const EnterFuse* ef = nullptr) const {
        // k_begin > 0: only stages k >= k_begin (block-distributed shard of a split EXTEND)
        const Tree& T = tree_at(log_m);
        size_t e = T.e; unsigned le = ilog2(e);
        int tgt = 1 - srcpar;
        const bool symk = kSymKernels && sym_kernels();                       // symmetric context: one-multiply butterflies in the full-size passes
        unsigned tz = (unsigned)__builtin_ctzll((unsigned long long)total);   // tiles must divide count*e
        unsigned log_tile = tz < kLogTileMax ? tz : kLogTileMax;
        const bool small = small_launch(total) && !ef_small_off_;           // latency regime: 4x smaller tiles, 4x as many workgroups
        if (small && log_tile > kLogLowSmall) log_tile = kLogLowSmall;
        unsigned k_first = le > log_tile ? le - log_tile : 0;                 // first stage with 2h <= tile
        if (k_first < k_begin) k_first = k_begin;
        // ST_ENTER wants whole [U | V] blocks in the tile (64 KiB at e = tile).  At e = 1024 that is ENTER level 11: served by the compile-time
        // engine on the block's two 1024-element halves (k_enter_l11, see enter_l11_tuned) where the tree has matrix-core tables,
        // by the run-time-tile kernel k_stages_lds<F, 0> otherwise (M31, shard contexts, small tiles, no matrix cores) and at every smaller e
        if (ef && k_first == 0 && le + 1 > log_tile) log_tile = le + 1;
        // pass list: (kind, ka, kb)
        struct Pass { int kind; unsigned ka, kb; };                           // kind 0 col-decompose, 1 row, 2 col-recombine
        Pass passes[2 * 8 + 1]; int np = 0;
        if (k_first > k_begin) {                                              // balanced groups of <= kColStages stages
            unsigned log_ct0 = tz < kLogColTileMax ? tz : kLogColTileMax;
            if (small && log_ct0 > kLogLowSmall) log_ct0 = kLogLowSmall;
            const unsigned minc = (small && log_ct0 == kLogLowSmall) ? small_min_logc_ : (unsigned)ECFFT_COL_MIN_LOGC;
            unsigned rmax = kColStages < log_ct0 - minc ? kColStages : log_ct0 - minc;    // keep rows >= 4 elements (128 B)
            if (rmax < 1) rmax = 1;
            unsigned ncol = k_first - k_begin, ngrp = (ncol + rmax - 1) / rmax;
            unsigned k = k_begin;
            for (unsigned g = 0; g < ngrp; ++g) { unsigned sz = ncol / ngrp + (g < ncol % ngrp ? 1 : 0); passes[np++] = {0, k, k + sz - 1}; k += sz; }
        }
        int nd = np;
        passes[np++] = {1, k_first, le};
        for (int g = nd - 1; g >= 0; --g) passes[np++] = {2, passes[g].ka, passes[g].kb};
        // results of launches of at most 2^kNtStoreMaxLog elements leave with non-temporal stores (kernels.h data_st; 32-byte fields)
        const uint32_t nt_st = (sizeof(E) == 32 && kNtStoreMaxLog && total <= ((size_t)1 << kNtStoreMaxLog)) ? 1u : 0u;
        const E* plain_src = buf;
        const bool fuse_tail = next_ld && nd >= 1 && (io.st_mode == ST_PLAIN || io.st_mode == ST_SCALE || io.st_mode == ST_AXPBY) && io.dst == buf;
        const int pi0 = (skip_first_col && nd >= 1) ? 1 : 0;
        for (int pi = pi0; pi < np; ++pi) {
            IoDesc<F> d;
            bool first = pi == 0, last = pi == np - 1;
            if (last && fuse_tail) {
                // this core's last recombine group + the next core's first decompose group (same stages, same tiles)
                const Pass& P = passes[pi];
                d = io; d.src = buf; d.dst = buf; d.ld_mode = next_ld->ld_mode; d.ld_tbl = next_ld->ld_tbl; d.nt_st = nt_st;
                unsigned log_ct = tz < kLogColTileMax ? tz : kLogColTileMax;
                if (small && log_ct > kLogLowSmall) log_ct = kLogLowSmall;
                unsigned R = P.kb - P.ka + 1, log_c = log_ct - R;
                double hsum = 0; for (unsigned k = P.ka; k <= P.kb; ++k) hsum += (double)(e >> (k + 1));
                double bytes = 2.0 * sizeof(E) * (2.0 * R * total + 4.0 * hsum * tblw_) + extra_last + next_ld->extra_first;
                const unsigned lv = pair_spans(total, le, P.ka, log_ct, d);
                if (col256_ok(log_ct, le) && T.c0t[tgt])      // latency regime: one element per thread in registers (reg_col_stages)
                    ECFFT_LAUNCH(KC_COL, bytes, k_stages_col_mid256<F>, dim3((unsigned)(total >> log_ct)), dim3(256), 0, s, d, T.p0[tgt], T.p1[tgt], T.c0t[tgt], T.dinv[tgt], le, P.ka, P.kb, log_c);
                else if (symk)
                ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col_mid<F, kSymKernels>), dim3((unsigned)(total >> (log_ct + lv))), dim3(kBlockLds), (sizeof(E) * ((size_t)col_row_stride<E>(1u << log_c) << R)) << lv, s,
                             d, T.p0[tgt], T.p1[tgt], T.np0[tgt], T.dinv[tgt], le, P.ka, P.kb, log_c, T.c0t[tgt], (uint32_t)lv);
                else
                ECFFT_LAUNCH(KC_COL, bytes, k_stages_col_mid<F>, dim3((unsigned)(total >> (log_ct + lv))), dim3(kBlockLds), (sizeof(E) * ((size_t)col_row_stride<E>(1u << log_c) << R)) << lv, s,
                             d, T.p0[tgt], T.p1[tgt], T.np0[tgt], T.dinv[tgt], le, P.ka, P.kb, log_c, T.c0t[tgt], (uint32_t)lv);
                return true;
            }
            if (last && ef && passes[pi].kind == 2) {
                // last recombine group (stages kb..0) + the ENTER level's combine, two vectors per workgroup
                const Pass& P = passes[pi];
                unsigned log_ct = le < kLogColTileMax ? le : kLogColTileMax;
                if (small && log_ct > kLogLowSmall) log_ct = kLogLowSmall;
                unsigned R = P.kb + 1, log_c = log_ct - R;
                double hsum = 0; for (unsigned k = P.ka; k <= P.kb; ++k) hsum += (double)(e >> (k + 1));
                double bytes = sizeof(E) * (2.0 * R * total + 4.0 * hsum * tblw_) + ef->extra;
                if (col256_ok(log_ct, le))
                    ECFFT_LAUNCH(KC_COL, bytes, k_stages_col_enter256<F>, dim3((unsigned)(total >> (log_ct + 1))), dim3(512), 0, s,
                                 (const E*)buf, ef->src, ef->dst, T.p0[tgt], T.p1[tgt], T.xe, T.w[1], T.w1x, le, P.kb, log_c);
                else if (symk)
                ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col_enter<F, kSymKernels>), dim3((unsigned)(total >> (log_ct + 1))), dim3(kBlockLds),
                             2 * sizeof(E) * ((size_t)col_row_stride<E>(1u << log_c) << R), s,
                             (const E*)buf, ef->src, ef->dst, T.p0[tgt], T.p1[tgt], T.xe, T.w[1], T.w1x, le, P.kb, log_c);
                else
                ECFFT_LAUNCH(KC_COL, bytes, k_stages_col_enter<F>, dim3((unsigned)(total >> (log_ct + 1))), dim3(kBlockLds),
                             2 * sizeof(E) * ((size_t)col_row_stride<E>(1u << log_c) << R), s,
                             (const E*)buf, ef->src, ef->dst, T.p0[tgt], T.p1[tgt], T.xe, T.w[1], T.w1x, le, P.kb, log_c);
                return false;
            }
            // load side
            if (first) { d = io; d.st_tr_logp = 0; } else { d = IoDesc<F>{}; d.src = plain_src; d.src_stride = 1; d.src_off = 0; d.ld_mode = LD_PLAIN; d.ld_tbl = nullptr; }
            // store side
            if (last) { d.dst = io.dst; d.st_mode = io.st_mode; d.st_a = io.st_a; d.st_b = io.st_b; d.aux = io.aux; d.aux_stride = io.aux_stride; d.aux_off = io.aux_off; d.aux_out = io.aux_out; d.st_c = io.st_c; d.aux2 = io.aux2;
                        d.st_tr_logp = io.st_tr_logp; d.tr_chunk = io.tr_chunk; }
            else { d.dst = buf; d.st_mode = ST_PLAIN; d.st_a = d.st_b = nullptr; d.aux = nullptr; d.aux_stride = d.aux_off = 0; d.aux_out = nullptr; }
            d.nt_st = nt_st;
            double extra = (first ? extra_first : 0.0) + (last ? extra_last : 0.0);
            const Pass& P = passes[pi];
            if (last && ef) {   // row pass is the last one: pair store operator
                d.dst = ef->dst; d.st_mode = ST_ENTER; d.st_a = T.xe; d.st_b = T.w1x; d.st_c = T.w[1]; d.aux = ef->src; d.aux_stride = 1; d.aux_off = 0; d.aux_out = nullptr;
                extra += ef->extra;
            }
            if (P.kind == 1) {
                unsigned nst = le - k_first;
                double hsum = (double)((e >> k_first) - 1);                   // sum of h over the fused stages
                double bytes = sizeof(E) * (2.0 * nst * 2.0 * total + 8.0 * hsum * tblw_) + extra;
                // compile-time tiles of 4-byte fields run the register-resident stage engine, which works on chunks of 16 elements
                // per thread: only valid when the default tile IS such a chunk (non-default ECFFT_LOG_TILE_BYTES / ECFFT_BLOCK_ROW
                // builds fall back to the run-time-tile kernel)
                constexpr bool ct_row = sizeof(E) == 4 ? ((size_t)1 << kLogTileMax) == (size_t)kBlockRow * 16 : (ECFFT_CT_ALL != 0);
                // matrix-core form of the stages with pair distance <= 8 (mfma_blk16.h): whole 1024-element sub-tiles, >= 4 in-tile stages
                const bool use_blk16 = sizeof(E) == 32 && kBlockRow == 512 && kLogTileMax == 10 && !mfma_off_ && T.blk16_A[srcpar] && log_tile == kLogTileMax && le - k_first >= 4;
                const uint8_t* bA = use_blk16 ? T.blk16_A[srcpar] : nullptr;
                const unsigned long long* bK = use_blk16 ? T.blk16_K[srcpar] : nullptr;
                if (sizeof(E) == 32 && log_tile == kLogLowSmall && !row256_off_ && d.st_mode != ST_ENTER && T.c0t[srcpar]) {
                    // latency regime: one element per thread in registers; round 4: the stages with pair distance <= 8 on the matrix
                    // cores here too (v_mfma_i32_16x16x64_i8: the 16 blocks of a 256-element tile are one MFMA's columns)
                    const bool mf = !mfma_off_ && T.blk16_A[srcpar] && le >= 4 && le - k_first >= 4;
                    ECFFT_LAUNCH(KC_ROW, bytes, (k_stages_row256<F>), dim3((unsigned)(total >> kLogLowSmall)), dim3(256), 0, s, d, T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.inner[srcpar],
                                 le, k_first, T.c0t[srcpar], mf ? T.blk16_A[srcpar] : (const uint8_t*)nullptr, mf ? T.blk16_K[srcpar] : (const unsigned long long*)nullptr);
                } else
                if (ef && k_first == 0 && le == kLogTileMax && log_tile == le + 1 && !small && enter_l11_tuned(T, srcpar)) {
                    // ENTER level 11 (e = 1024): one [u0 | v0] block per workgroup, its halves through the 1024-element engine
                    if constexpr (kEnterL11) {
                    if (symk)
                    ECFFT_LAUNCH(KC_ROW, bytes, (k_enter_l11<F, kSymKernels, ECFFT_ENTER_L11_THREADS>), dim3((unsigned)(total >> log_tile)), dim3(ECFFT_ENTER_L11_THREADS), ((size_t)sizeof(E)) << log_tile, s,
                                 d, T.np0[srcpar], T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.blk16_A[srcpar], T.blk16_K[srcpar]);
                    else
                    ECFFT_LAUNCH(KC_ROW, bytes, (k_enter_l11<F, false, ECFFT_ENTER_L11_THREADS>), dim3((unsigned)(total >> log_tile)), dim3(ECFFT_ENTER_L11_THREADS), ((size_t)sizeof(E)) << log_tile, s,
                                 d, T.np0[srcpar], T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.blk16_A[srcpar], T.blk16_K[srcpar]);
                    }
                } else
                if (log_tile == kLogTileMax + 1 && ct_row) {
                    // (only instantiated for the fields that launch it: the 32-byte instantiation was dead code in the code object)
                    if constexpr (ct_row)
                    ECFFT_LAUNCH(KC_ROW, bytes, (k_stages_lds<F, (int)kLogTileMax + 1>), dim3((unsigned)(total >> log_tile)), dim3(kBlockRow),
                                 ((size_t)sizeof(E)) << log_tile, s, d, T.np0[srcpar], T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.inner[srcpar], le, k_first, log_tile, T.c0t[srcpar], bA, bK);
                } else if (log_tile == kLogTileMax && (ct_row || bA) && symk)   // ... with the one-multiply butterflies of a symmetric context
                    ECFFT_LAUNCH(KC_ROW, bytes, (k_stages_lds<F, (int)kLogTileMax, kSymKernels>), dim3((unsigned)(total >> log_tile)), dim3(kBlockRow),
                                 ((size_t)sizeof(E)) << log_tile, s, d, T.np0[srcpar], T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.inner[srcpar], le, k_first, log_tile, T.c0t[srcpar], bA, bK);
                else if (log_tile == kLogTileMax && (ct_row || bA))   // compile-time tile (always for the matrix-core row passes): +16% on M31 (8 pairs/thread unroll), -3% on secp256k1
                    ECFFT_LAUNCH(KC_ROW, bytes, (k_stages_lds<F, (int)kLogTileMax>), dim3((unsigned)(total >> log_tile)), dim3(kBlockRow),
                                 ((size_t)sizeof(E)) << log_tile, s, d, T.np0[srcpar], T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.inner[srcpar], le, k_first, log_tile, T.c0t[srcpar], bA, bK);
                else
                    ECFFT_LAUNCH(KC_ROW, bytes, (k_stages_lds<F, 0>), dim3((unsigned)(total >> log_tile)), dim3(kBlockRow),
                                 ((size_t)sizeof(E)) << log_tile, s, d, T.np0[srcpar], T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.inner[srcpar], le, k_first, log_tile, T.c0t[srcpar], bA, bK);
            } else {
                unsigned log_ct = tz < kLogColTileMax ? tz : kLogColTileMax;           // column tiles may be larger than row tiles
                if (small && log_ct > kLogLowSmall) log_ct = kLogLowSmall;
                unsigned R = P.kb - P.ka + 1, log_c = log_ct - R;
                double hsum = 0; for (unsigned k = P.ka; k <= P.kb; ++k) hsum += (double)(e >> (k + 1));
                double bytes = sizeof(E) * (2.0 * R * total + 4.0 * hsum * tblw_) + extra;
                const bool ct = (log_ct == kLogColTileMax && (sizeof(E) == 4 || ECFFT_CT_ALL));
                const unsigned lv = ct ? pair_spans(total, le, P.ka, log_ct, d) : 0;
                dim3 grid((unsigned)(total >> (log_ct + lv))); size_t lds = (sizeof(E) * ((size_t)col_row_stride<E>(1u << log_c) << R)) << lv;
                // compile-time column tiles exist for 4-byte fields only (or with ECFFT_CT_ALL): the 32-byte instantiation is not even
                // compiled — it was dead code with 24 B of scratch in the library's code object
                constexpr bool kCtCol = sizeof(E) == 4 || ECFFT_CT_ALL;
                if (col256_ok(log_ct, le) && lv == 0 && (P.kind != 0 || T.c0t[srcpar])) {
                    if (P.kind == 0) ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col256<F, true>), dim3((unsigned)(total >> log_ct)), dim3(256), 0, s, d, T.c0t[srcpar], T.dinv[srcpar], le, P.ka, P.kb, log_c);
                    else ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col256<F, false>), dim3((unsigned)(total >> log_ct)), dim3(256), 0, s, d, T.p0[tgt], T.p1[tgt], le, P.ka, P.kb, log_c);
                } else
                if (symk && !ct) {
                    if (P.kind == 0) ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, true, 0, kSymKernels>), grid, dim3(kBlockLds), lds, s, d, T.np0[srcpar], T.dinv[srcpar], le, P.ka, P.kb, log_c, T.c0t[srcpar], (uint32_t)lv);
                    else ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, false, 0, kSymKernels>), grid, dim3(kBlockLds), lds, s, d, T.p0[tgt], T.p1[tgt], le, P.ka, P.kb, log_c, (const TE*)nullptr, (uint32_t)lv);
                } else
                if (P.kind == 0) {
                    if constexpr (kCtCol) { if (ct) { ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, true, (int)kLogColTileMax>), grid, dim3(kBlockLds), lds, s, d, T.np0[srcpar], T.dinv[srcpar], le, P.ka, P.kb, log_c, T.c0t[srcpar], (uint32_t)lv); continue; } }
                    ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, true, 0>), grid, dim3(kBlockLds), lds, s, d, T.np0[srcpar], T.dinv[srcpar], le, P.ka, P.kb, log_c, T.c0t[srcpar], (uint32_t)lv);
                } else {
                    if constexpr (kCtCol) { if (ct) { ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, false, (int)kLogColTileMax>), grid, dim3(kBlockLds), lds, s, d, T.p0[tgt], T.p1[tgt], le, P.ka, P.kb, log_c, (const TE*)nullptr, (uint32_t)lv); continue; } }
                    ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, false, 0>), grid, dim3(kBlockLds), lds, s, d, T.p0[tgt], T.p1[tgt], le, P.ka, P.kb, log_c, (const TE*)nullptr, (uint32_t)lv);
                }
            }
        }
        return false;
    }
    // 4-byte fields, full-size column tiles: two consecutive spans (2h_ka-blocks; they read the same table entries) per workgroup
    // when the number of spans is even and the halved grid still fills the chip twice over
    static unsigned pair_spans(size_t total, unsigned le, unsigned ka, unsigned log_ct, const IoDesc<F>& d) {
        if (sizeof(E) != 4 || ECFFT_COL_PAD != 0 || log_ct != kLogColTileMax) return 0;
        if (((size_t)1 << log_ct) != (size_t)kBlockLds * 16) return 0;    // the kernels' vector path (kFast) exists for 16 elements per thread only
        // the paired form exists only on the kernels' 16-byte vector path: every buffer the pass touches must be 16-byte aligned
        // (user buffers may be only element-aligned) and the operator must be one the vector path implements
        auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
        if (!al(d.src) || !al(d.dst) || !al(d.aux) || !al(d.aux_out) || !al(d.aux2) || d.ld_tr_logp || d.st_tr_logp || le < 2) return 0;
        if (!((d.src_stride == 1 && d.src_off == 0) || (d.src_stride == 2 && d.src_off < 2))) return 0;
        const size_t nspans = total >> (le - ka);
        return (nspans >= 2 && (nspans & 1) == 0 && (total >> (log_ct + 1)) >= 512) ? 1u : 0u;
    }
    // latency regime, 32-byte fields: 256-element column tiles run on the register-resident engine (k_stages_col256 & co.)
    bool col256_ok(unsigned log_ct, unsigned le) const { return sizeof(E) == 32 && log_ct == kLogLowSmall && le < 31 && !col256_off_; }
    static IoDesc<F> io_plain(const E* src, E* dst) {
        IoDesc<F> d{}; d.src = src; d.src_stride = 1; d.src_off = 0; d.ld_mode = LD_PLAIN; d.ld_tbl = nullptr;
        d.dst = dst; d.st_mode = ST_PLAIN; d.st_a = d.st_b = nullptr; d.aux = nullptr; d.aux_stride = d.aux_off = 0; d.aux_out = nullptr;
        return d;
    }

    // FFTree::extend (src/fftree.rs:123-126) on `count` vectors of length e: uses T_{2e}; `target`
    // names the TARGET moiety.  in/out device pointers (may alias).
    bool extend(const E* in, E* out, size_t e, size_t count, int target, hipStream_t s) const {
        unsigned log_m = ilog2(e) + 1;
        const Tree& T = tree_at(log_m);
        size_t total = e * count; int src = 1 - target;
        IoDesc<F> io = io_plain(in, out);
        io.ld_mode = LD_SCALE; io.ld_tbl = T.winv[src];
        io.st_mode = ST_SCALE; io.st_a = T.w[target];
        extend_core(log_m, io, out, total, src, s);
        return hipGetLastError() == hipSuccess;
    }

    // ecfft_extend with count > 1 (the low-degree extension of many columns): like a batched ENTER / EXIT, a batch whose parts have at
    // least 2^kSplitMinLog elements runs as concurrent parts of whole vectors, one stream each (round 6, batch_ways / run_ways)
    bool extend_api(const E* in, E* out, size_t e, size_t count, int target, hipStream_t s) {
        const size_t total = e * count;
        // only for LONG vectors (e >= 2^kSplitMinLog): their launches are one or two rounds of tiles, which is what a second stream fills
        // (-2.5 .. -4.4 % at e = 2^19 .. 2^22); many short vectors are deep launches already (2^16 x 32: +1.3 %, profiles/r06/extend_split_ab.txt)
        const int ways = (e >> kSplitMinLog) == 0 ? 1 : batch_ways(total, count);
        if (ways <= 1) return extend(in, out, e, count, target, s);
        const size_t part = total / (size_t)ways, cnt = count / (size_t)ways;
        bool ok = true;
        run_ways(ways, s, [&](int i, hipStream_t si) { ok = extend(in + part * i, out + part * i, e, cnt, target, si) && ok; });
        return ok;
    }

    // ------------------------------------------------------------------------------------------
    // Building blocks of ONE EXTEND split over P = 2^log_p GPUs.  The vector of
    // length e lives on T_{2e}; `target` is the target moiety.
    //   cyclic shard: local element j' <-> global position j'*P + rank, local length e/P; stage k < log
    //     e - log_p pairs (j', j' + h_k/P) and reads table entry (j' mod h_k/P)*P + rank.
    //   block shard: local element j' <-> global position rank*e/P + j'; stages k >= log_p are local and
    //     use exactly the single-GPU kernels (table index = local pair index mod h).
    // ------------------------------------------------------------------------------------------
    // cyclic shard, decompose side: multiply by 1/W_src, then stages 0 .. log_p-1
    // cyclic shard, recombine side: stages log_p-1 .. 0, then multiply by W_tgt
    void extend_top_cyclic(E* buf, size_t e, int target, unsigned log_p, unsigned rank, bool recombine, hipStream_t s) const {
        unsigned log_m = ilog2(e) + 1;
        const Tree& T = trees_[log_m];
        int src = 1 - target;
        size_t P = (size_t)1 << log_p, el = e >> log_p, npairs = el / 2;
        if (!recombine) {
            ECFFT_LAUNCH(KC_POINTWISE, 0.0, k_scale_by_table<F>, dim3(nblocks(el)), dim3(kBlock), 0, s, buf, (const E*)buf, T.winv[src], el - 1, el, (uint32_t)P, rank);
            for (unsigned k = 0; k < log_p; ++k) {
                size_t h = e >> (k + 1), off = e - 2 * h;
                ECFFT_LAUNCH(KC_DECOMPOSE, sizeof(E) * (2.0 * el + 4.0 * (h >> log_p)), k_decompose_stage<F>, dim3(nblocks(npairs)), dim3(kBlock), 0, s,
                             buf, T.np0[src] + off, T.dinv[src] + off, ilog2(h >> log_p), npairs, (uint32_t)P, rank);
            }
        } else {
            for (unsigned k = log_p; k-- > 0;) {
                size_t h = e >> (k + 1), off = e - 2 * h;
                ECFFT_LAUNCH(KC_RECOMBINE, sizeof(E) * (2.0 * el + 4.0 * (h >> log_p)), k_recombine_stage<F>, dim3(nblocks(npairs)), dim3(kBlock), 0, s,
                             buf, T.p0[target] + off, T.p1[target] + off, ilog2(h >> log_p), npairs, (uint32_t)P, rank);
            }
            ECFFT_LAUNCH(KC_POINTWISE, 0.0, k_scale_by_table<F>, dim3(nblocks(el)), dim3(kBlock), 0, s, buf, (const E*)buf, T.w[target], el - 1, el, (uint32_t)P, rank);
        }
    }
    // block shard: decompose stages k >= log_p then recombine stages back down to log_p, fused passes, in place
    void extend_local_block(E* buf, size_t e, int target, unsigned log_p, hipStream_t s) const {
        unsigned log_m = ilog2(e) + 1;
        extend_core(log_m, io_plain(buf, buf), buf, e >> log_p, 1 - target, s, 0.0, 0.0, log_p);
    }

    // ------------------------------------------------------------------------------------------
    // ONE transform split over the ranks of a Transport (one process per GPU).
    // Everything below the exchange calls is the single-GPU kernels; the block <-> cyclic re-distributions cost no pass of
    // their own: the pack / unpack index maps ride on the 1/W and W scalings that an EXTEND needs anyway and on the
    // load / store operators (IoDesc::ld_tr_logp / st_tr_logp) of the block-local fused passes.
    // ------------------------------------------------------------------------------------------
    // equal pieces of `piece` elements to / from every rank of the group [gbase, gbase + P)
    bool exchange_group(Transport& tr, int gbase, size_t P, E* from, E* to, size_t piece, hipStream_t s) const {
        P2P snd[64], rcv[64];
        if (P > 64) return false;
        for (size_t q = 0; q < P; ++q) { snd[q] = {gbase + (int)q, from + q * piece, piece * sizeof(E)}; rcv[q] = {gbase + (int)q, to + q * piece, piece * sizeof(E)}; }
        // every rank of the communicator is in such a group of P at this point of the call sequence (aligned groups): rank q sends one
        // piece to each member of its own group — the pattern the link striping needs (small groups leave most links of the mesh idle)
        const size_t pb = piece * sizeof(E); const int Pg = (int)P;
        return xchg(tr, [pb, Pg](int q, std::vector<Transport::MsgDesc>& m) { const int gb = (q / Pg) * Pg; for (int j = 0; j < Pg; ++j) m.push_back({gb + j, pb}); },
                    snd, (int)P, rcv, (int)P, s, P < (size_t)tr.world);
    }
    // one grouped exchange of a split transform, striped over the links of the mesh when that pays (Transport::exchange_striped);
    // `pat(q)` = what rank q sends at this point of the call sequence.  Only inside api_enter_split / api_exit_split, which provide
    // the relays' staging buffer; everywhere else (and with ECFFT_NO_STRIPE in a test build) the plain exchange.
    bool xchg(Transport& tr, const Transport::PatternFn& pat, const P2P* snd, int ns, const P2P* rcv, int nr, hipStream_t s, bool worth = true) const {
        if (!worth || !stripe_stage_ || stripe_off_) return tr.exchange(snd, ns, rcv, nr, s);
        if (stripe_gain_ != ~(size_t)0) tr.stripe_min_gain = stripe_gain_;
        return tr.exchange_striped(pat, snd, ns, rcv, nr, stripe_stage_, stripe_bytes_, s);
    }
    // FULL contexts: the same compact cyclic tables, gathered once per (tree, P, rank, table) from the full stage tables on first
    // use (entry i'*P + rank of stage k -> offset c - 2*(h_k/P) + i', the layout build_shard_set writes) and kept until the context
    // is destroyed or trimmed — so the split EXTEND of a full context also runs its log P cyclic stages as one fused pass instead
    // of log P one-stage launches with stride-P table reads.  nullptr (allocation failed): the caller runs the one-stage kernels.
    // which: 0 np0, 1 dinv, 2 p0, 3 p1 (stage tables), 4 w, 5 winv (the c cyclic positions i'*P + rank).
    const TE* full_cyclic_table(const Tree& T, unsigned log_p, unsigned r, int sg, int which, hipStream_t s) const {
        const uint64_t key = ((uint64_t)T.log_m << 40) | ((uint64_t)log_p << 32) | ((uint64_t)r << 8) | ((uint64_t)sg << 4) | (uint64_t)which;
        auto it = full_cyc_.find(key);
        if (it != full_cyc_.end()) return it->second;
        const size_t e = T.e, P = (size_t)1 << log_p, c = e >> log_p;
        TE* dst = nullptr;
        if (hipMalloc(&dst, c * sizeof(TE)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        const TE* src = which == 0 ? T.np0[sg] : which == 1 ? T.dinv[sg] : which == 2 ? T.p0[sg] : which == 3 ? T.p1[sg] : which == 4 ? T.w[sg] : T.winv[sg];
        if (which >= 4) {
            foreach_n(s, c, [=] __device__(size_t il) { dst[il] = src[il * P + r]; });
        } else {
            (void)hipMemsetAsync(dst, 0, c * sizeof(TE), s);
            for (unsigned k = 0; k < log_p; ++k) {
                const size_t h = e >> (k + 1), hl = h >> log_p, offl = c - 2 * hl, off = e - 2 * h;
                foreach_n(s, hl, [=] __device__(size_t il) { dst[offl + il] = src[off + il * P + r]; });
            }
        }
        full_cyc_[key] = dst; full_cyc_bytes_ += c * sizeof(TE);
        return dst;
    }
    void full_cyclic_free() { for (auto& kv : full_cyc_) (void)hipFree(kv.second); full_cyc_.clear(); full_cyc_bytes_ = 0; }

    // Shard contexts keep the cyclic stages' table entries compact and laid out like the stage tables of a length-c vector, so the
    // log_p cyclic stages are the TOP log_p stages of a "length-c EXTEND" on those tables: ONE fused column pass (k_stages_col)
    // instead of log_p one-stage launches, with the 1/W or W scaling of a cyclic-in / cyclic-out call riding on its load / store.
    // Returns false when the stage count does not fit one column tile (the caller then runs the one-stage kernels).
    bool cyclic_stages_fused(const TE* ta, const TE* tb, const E* src, E* dst, size_t c, unsigned log_p, bool dec, const TE* ld_scale,
                             const TE* st_scale, hipStream_t s) const {
        const unsigned lc = ilog2(c);
        unsigned log_ct = lc < kLogColTileMax ? lc : kLogColTileMax;
        if (small_launch(c) && !ef_small_off_ && log_ct > kLogLowSmall) log_ct = kLogLowSmall;
        const unsigned R = log_p;
        if (R == 0 || R > kColStages || R + 2 > log_ct) return false;
        const unsigned log_cc = log_ct - R;
        IoDesc<F> d = io_plain(src, dst);
        if (ld_scale) { d.ld_mode = LD_SCALE; d.ld_tbl = ld_scale; }
        if (st_scale) { d.st_mode = ST_SCALE; d.st_a = st_scale; }
        const bool ct = (log_ct == kLogColTileMax && (sizeof(E) == 4 || ECFFT_CT_ALL));
        dim3 grid((unsigned)(c >> log_ct)); const size_t lds = sizeof(E) * ((size_t)col_row_stride<E>(1u << log_cc) << R);
        double hsum = 0; for (unsigned k = 0; k < log_p; ++k) hsum += (double)(c >> (k + 1));
        const double bytes = sizeof(E) * (2.0 * R * c + 4.0 * hsum);
        constexpr bool kCtCol = sizeof(E) == 4 || ECFFT_CT_ALL;              // compile-time column tiles: 4-byte fields only (see extend_core)
        if (dec) {
            if constexpr (kCtCol) { if (ct) { ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, true, (int)kLogColTileMax>), grid, dim3(kBlockLds), lds, s, d, ta, tb, lc, 0u, log_p - 1, log_cc, (const TE*)nullptr, 0u); return true; } }
            ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, true, 0>), grid, dim3(kBlockLds), lds, s, d, ta, tb, lc, 0u, log_p - 1, log_cc, (const TE*)nullptr, 0u);
        } else {
            if constexpr (kCtCol) { if (ct) { ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, false, (int)kLogColTileMax>), grid, dim3(kBlockLds), lds, s, d, ta, tb, lc, 0u, log_p - 1, log_cc, (const TE*)nullptr, 0u); return true; } }
            ECFFT_LAUNCH(KC_COL, bytes, (k_stages_col<F, false, 0>), grid, dim3(kBlockLds), lds, s, d, ta, tb, lc, 0u, log_p - 1, log_cc, (const TE*)nullptr, 0u);
        }
        return true;
    }
    // FFTree::extend (src/fftree.rs:123-126) of ONE vector of e evaluations held block-distributed by the P = 2^log_p ranks
    // [gbase, gbase + P) of `tr`: rank gbase + r holds positions [r*c, (r+1)*c), c = e/P.  in / out: this rank's shard (may
    // alias).  A, B: scratch of c elements each.  Stage k pairs (i, i + e >> (k+1)): stages k >= log_p are local in the block
    // distribution, stages k < log_p in the cyclic one (position j on rank j mod P).
    // cyc_in / cyc_out: the shard is CYCLIC instead (local j' <-> global position j'*P + r), which drops the first / last of the
    // four exchanges — for callers that chain split EXTENDs or produce / consume the cyclic order anyway.
    bool extend_split(Transport& tr, int gbase, unsigned log_p, const E* in, E* out, size_t e, int target, hipStream_t s, E* A, E* B,
                      bool cyc_in = false, bool cyc_out = false) const {
        const unsigned log_m = ilog2(e) + 1;
        const Tree& T = tree_at(log_m);
        const size_t P = (size_t)1 << log_p, c = e >> log_p, cp = c >> log_p, g0 = (size_t)(tr.rank - gbase) * c;
        const unsigned r = (unsigned)(tr.rank - gbase);
        const int src = 1 - target;
        if (c < P || c < 2) return false;
        const bool sh = shard_mode();                                          // tables of this context hold only this rank's share
        const ShardSet* sp = (ovr_tree_ && ovr_tree_->log_m == log_m) ? ovr_set_ : (log_m < sets_.size() && sets_[log_m].valid ? &sets_[log_m] : nullptr);
        if (sh && (!sp || sp->log_p != log_p || sp->rank != r)) return false;
        static const ShardSet kNoSet{};
        const ShardSet& SS = sh ? *sp : kNoSet;
        const auto& cyc_ = SS.cyc; const auto& cycw_ = SS.cycw;               // [parity][np0, dinv, p0, p1] and [parity][w, winv], compact
        bool dec_done = false;
        // full context: compact copies of the cyclic entries, gathered on first use (full_cyclic_table)
        const TE *fd0 = nullptr, *fd1 = nullptr, *fr0 = nullptr, *fr1 = nullptr, *fwi = nullptr, *fw = nullptr;
        if (!sh && log_p >= 1 && !full_cyc_off_) {
            fd0 = full_cyclic_table(T, log_p, r, src, 0, s); fd1 = full_cyclic_table(T, log_p, r, src, 1, s);
            fr0 = full_cyclic_table(T, log_p, r, target, 2, s); fr1 = full_cyclic_table(T, log_p, r, target, 3, s);
            if (cyc_in) fwi = full_cyclic_table(T, log_p, r, src, 5, s);
            if (cyc_out) fw = full_cyclic_table(T, log_p, r, target, 4, s);
        }
        const bool fdec = fd0 && fd1 && (!cyc_in || fwi), frec = fr0 && fr1 && (!cyc_out || fw);
        if (cyc_in && fdec && cyclic_stages_fused(fd0, fd1, in, B, c, log_p, true, fwi, nullptr, s)) {
            dec_done = true;
        } else if (cyc_in && sh && cyclic_stages_fused(cyc_[src][0], cyc_[src][1], in, B, c, log_p, true, cycw_[src][1], nullptr, s)) {
            dec_done = true;                                                   // 1/W + every cyclic decompose stage in one pass
        } else if (cyc_in) {   // already cyclic: 1/W_src of positions j'*P + r
            if (sh) ECFFT_LAUNCH(KC_POINTWISE, 0.0, k_scale_by_table<F>, dim3(nblocks(c)), dim3(kBlock), 0, s, B, in, (const TE*)cycw_[src][1], c - 1, c, 1u, 0u);
            else ECFFT_LAUNCH(KC_POINTWISE, 0.0, k_scale_by_table<F>, dim3(nblocks(c)), dim3(kBlock), 0, s, B, in, T.winv[src], c - 1, c, (uint32_t)P, r);
        } else {
            {   // 1/W_src scaling + pack for block -> cyclic: element i goes to rank i mod P, slot i / P
                const TE* wi = T.winv[src]; const unsigned lp = log_p;
                foreach_n(s, c, [=] __device__(size_t i) { A[(i & (P - 1)) * cp + (i >> lp)] = F::canon(F::tmul(wi[g0 + i], in[i])); });
            }
            if (!exchange_group(tr, gbase, P, A, B, cp, s)) return false;      // B = cyclic shard, ascending local index
        }
        const size_t npairs = c / 2;
        if (!dec_done && sh && cyclic_stages_fused(cyc_[src][0], cyc_[src][1], B, B, c, log_p, true, nullptr, nullptr, s)) dec_done = true;
        if (!dec_done && fdec && cyclic_stages_fused(fd0, fd1, B, B, c, log_p, true, nullptr, nullptr, s)) dec_done = true;
        for (unsigned k = 0; k < log_p && !dec_done; ++k) {                    // cyclic shard: top decompose stages, table stride P / offset r
            size_t h = e >> (k + 1), off = e - 2 * h;
            if (sh) {
                const size_t offl = c - 2 * (h >> log_p);
                ECFFT_LAUNCH(KC_DECOMPOSE, sizeof(E) * (2.0 * c + 4.0 * (h >> log_p)), k_decompose_stage<F>, dim3(nblocks(npairs)), dim3(kBlock), 0, s,
                             B, (const TE*)(cyc_[src][0] + offl), (const TE*)(cyc_[src][1] + offl), ilog2(h >> log_p), npairs, 1u, 0u);
                continue;
            }
            ECFFT_LAUNCH(KC_DECOMPOSE, sizeof(E) * (2.0 * c + 4.0 * (h >> log_p)), k_decompose_stage<F>, dim3(nblocks(npairs)), dim3(kBlock), 0, s,
                         B, T.np0[src] + off, T.dinv[src] + off, ilog2(h >> log_p), npairs, (uint32_t)P, r);
        }
        if (!exchange_group(tr, gbase, P, B, A, cp, s)) return false;          // A = the P chunks of the block shard, source major
        {   // block shard: every stage k >= log_p, fused passes; unpack on the first load, pack on the last store
            IoDesc<F> io = io_plain(A, B);
            io.ld_tr_logp = log_p; io.st_tr_logp = log_p; io.tr_chunk = cp;
            extend_core(log_m, io, out, c, src, s, 0.0, 0.0, log_p);
        }
        if (!exchange_group(tr, gbase, P, B, A, cp, s)) return false;          // A = cyclic shard
        bool rec_done = false;
        if (sh && cyclic_stages_fused(cyc_[target][2], cyc_[target][3], A, cyc_out ? out : A, c, log_p, false, nullptr, cyc_out ? cycw_[target][0] : nullptr, s)) {
            if (cyc_out) return hipGetLastError() == hipSuccess;               // every cyclic recombine stage + W in one pass
            rec_done = true;
        }
        if (!rec_done && frec && cyclic_stages_fused(fr0, fr1, A, cyc_out ? out : A, c, log_p, false, nullptr, cyc_out ? fw : nullptr, s)) {
            if (cyc_out) return hipGetLastError() == hipSuccess;
            rec_done = true;
        }
        for (unsigned k = log_p; !rec_done && k-- > 0;) {
            size_t h = e >> (k + 1), off = e - 2 * h;
            if (sh) {
                const size_t offl = c - 2 * (h >> log_p);
                ECFFT_LAUNCH(KC_RECOMBINE, sizeof(E) * (2.0 * c + 4.0 * (h >> log_p)), k_recombine_stage<F>, dim3(nblocks(npairs)), dim3(kBlock), 0, s,
                             A, (const TE*)(cyc_[target][2] + offl), (const TE*)(cyc_[target][3] + offl), ilog2(h >> log_p), npairs, 1u, 0u);
                continue;
            }
            ECFFT_LAUNCH(KC_RECOMBINE, sizeof(E) * (2.0 * c + 4.0 * (h >> log_p)), k_recombine_stage<F>, dim3(nblocks(npairs)), dim3(kBlock), 0, s,
                         A, T.p0[target] + off, T.p1[target] + off, ilog2(h >> log_p), npairs, (uint32_t)P, r);
        }
        if (cyc_out) {  // stay cyclic: W_target of positions j'*P + r
            if (sh) ECFFT_LAUNCH(KC_POINTWISE, 0.0, k_scale_by_table<F>, dim3(nblocks(c)), dim3(kBlock), 0, s, out, (const E*)A, (const TE*)cycw_[target][0], c - 1, c, 1u, 0u);
            else ECFFT_LAUNCH(KC_POINTWISE, 0.0, k_scale_by_table<F>, dim3(nblocks(c)), dim3(kBlock), 0, s, out, (const E*)A, T.w[target], c - 1, c, (uint32_t)P, r);
            return hipGetLastError() == hipSuccess;
        }
        if (!exchange_group(tr, gbase, P, A, B, cp, s)) return false;          // B = chunks of the block shard
        {   // unpack + W_target scaling
            const TE* w = T.w[target]; const unsigned lp = log_p;
            foreach_n(s, c, [=] __device__(size_t i) { out[i] = F::canon(F::tmul(w[g0 + i], B[(i & (P - 1)) * cp + (i >> lp)])); });
        }
        return hipGetLastError() == hipSuccess;
    }
    // Local preparation of a collective call (its temporaries) + agreement across the ranks (Transport::vote) the FIRST time a
    // call shape is seen on this context: a rank whose allocation failed must not leave its peers blocked in ncclRecv.  After
    // an agreed first call the shape's temporaries are pinned in the pool, so later calls of that shape allocate nothing, cannot
    // fail locally and stay asynchronous (no vote).  Every rank makes the same calls with the same sizes (the ABI's contract), so
    // "first time" is the same moment on all of them.
    template <class Alloc>
    bool collective_prepare(Transport& tr, int op, size_t len, int variant, hipStream_t s, Alloc alloc) {
        bool local_ok = true;
        try { alloc(); } catch (const DeviceAllocError&) { local_ok = false; }
        const uint64_t key = ((uint64_t)op << 60) | ((uint64_t)variant << 56) | ((uint64_t)(unsigned)tr.world << 48) | (uint64_t)len;
        // An agreed shape cannot fail locally: its temporaries are pinned in the pool.  It therefore never votes again — a vote is a
        // symmetric all-rank exchange, and a rank voting alone would pair its 4-byte messages with its peers' data messages
        // (ADVICE r04).  Should the impossible happen, the rank reports the error and its peers are released by the caller's
        // ecfft_comm_abort; the failure-injection hook only applies to shapes that still vote (it stays armed until one comes).
        if (agreed_shapes_.count(key) && tr.voted()) {
            if (!local_ok) { fprintf(stderr, "ecfft: a pinned temporary of an agreed sharded call shape could not be taken\n"); temps_done(); }
            return local_ok;
        }
#ifdef ECFFT_TEST_HOOKS
        if (fail_next_collective_) { local_ok = false; fail_next_collective_ = false; }        // test hook
#endif
        if (!tr.vote(local_ok, s)) { temps_done(); return false; }
        agreed_shapes_.insert(key);
        for (auto& b : pool_) if (b.busy) b.pinned = true;
        return true;
    }
#ifdef ECFFT_TEST_HOOKS
    void test_fail_next_collective() { std::lock_guard<std::mutex> g(mu_); fail_next_collective_ = true; }
#endif
    bool api_extend_split(Transport& tr, const E* in, E* out, size_t e, int target, hipStream_t s, bool cyc_in = false, bool cyc_out = false) {
        const size_t P = (size_t)tr.world, c = e / P;
        if (P & (P - 1)) return false;
        E *A = nullptr, *B = nullptr;
        if (!collective_prepare(tr, 1, e, (cyc_in ? 1 : 0) | (cyc_out ? 2 : 0), s, [&] { A = temp(c); B = temp(c); })) return false;
        bool ok = extend_split(tr, 0, ilog2(P), in, out, e, target, s, A, B, cyc_in, cyc_out);
        temps_done();
        return ok;
    }
    // FFTree::enter of n coefficients block-distributed over all ranks of `tr` (rank r holds [r*c, (r+1)*c), c = n/P).
    // Levels m <= c are the rank-local ENTER of the chunk; level m = c*Q (Q = 2, 4, .. P) works inside groups of Q consecutive
    // ranks, and every vector of a level stays CYCLIC across it: u0 (on the lower half-group) and v0 (upper) arrive cyclic over
    // their half-group, the split EXTEND runs cyclic-in / cyclic-out (2 exchanges; none for Q = 2), and ONE exchange hands every
    // rank the operands of the outputs it owns in the NEXT level's cyclic order — position i = i'*Q + a of the level's result is
    // out[i] = X + xnn_s[i] * Y (src/fftree.rs:155-159) with (X, Y) = (u0, v0)[i/2] for even i and (u1, v1)[i/2] for odd i, and
    // all positions of a rank have the parity of a, so rank a needs the whole `cur` (a even) or `ext` (a odd) of sub-rank a/2 of
    // both half-groups.  3 exchanges per level (block form: 5), one more at the end to return to the block order.
    bool api_enter_split(Transport& tr, const E* in, E* out, size_t n, hipStream_t s) {
        const size_t P = (size_t)tr.world, c = n / P, cp = c / P;
        if ((P & (P - 1)) || c < 2 * P) return false;
        const bool sh = shard_mode();
        E *cur = nullptr, *ext = nullptr, *U = nullptr, *V = nullptr, *A = nullptr, *B = nullptr;
        E* stg = nullptr;
        const bool stripe = P >= 4 && !stripe_off_;
        if (!collective_prepare(tr, 2, n, stripe ? 1 : 0, s, [&] { cur = temp(c); ext = temp(c); U = temp(c); V = temp(c); A = temp(c); B = temp(c); if (stripe) stg = temp(2 * c); })) return false;
        StripeScope stripe_scope(this, stg, 2 * c * sizeof(E));                 // relays' staging of the striped exchanges (2c elements bound every pattern below)
        bool ok = enter(in, cur, c, 1, s);
        for (size_t Q = 2; ok && Q <= P; Q *= 2) {
            const size_t half = Q / 2, m = c * Q, e = m / 2;
            const int base = (int)((tr.rank / Q) * Q), a = tr.rank - base, g = a / (int)half, ap = a % (int)half;
            if (half == 1) ok = extend(cur, ext, e, 1, 1, s);
            else ok = extend_split(tr, base + g * (int)half, ilog2(half), cur, ext, e, 1, s, A, B, true, true);
            if (!ok) break;
            P2P snd[2] = {{base + 2 * ap, cur, c * sizeof(E)}, {base + 2 * ap + 1, ext, c * sizeof(E)}};
            P2P rcv[2] = {{base + a / 2, U, c * sizeof(E)}, {base + (int)half + a / 2, V, c * sizeof(E)}};
            { const size_t cb = c * sizeof(E); const int Qi = (int)Q, hi = (int)half;
              ok = xchg(tr, [cb, Qi, hi](int q, std::vector<Transport::MsgDesc>& m) { const int b = (q / Qi) * Qi, p = (q - b) % hi; m.push_back({b + 2 * p, cb}); m.push_back({b + 2 * p + 1, cb}); },
                        snd, 2, rcv, 2, s); }
            // a shard context holds exactly the c entries xnn_s[i'*Q + a] of T_m, compact; a full one the whole table
            const E* xnn = trees_[ilog2(m)].xnn + (sh ? 0 : a); const size_t xs = sh ? 1 : Q;
            foreach_n(s, c, [=] __device__(size_t i) { cur[i] = F::mul_add(xnn[i * xs], V[i], U[i]); });      // :157-158
        }
        if (ok) {   // cyclic over all ranks -> block: local i' = r'*cp + k is global (r'*cp + k)*P + r = block r', offset k*P + r
            ok = exchange_group(tr, 0, P, cur, B, cp, s);
            const size_t lp = ilog2(P);
            foreach_n(s, c, [=] __device__(size_t i) { out[i] = B[(i & (P - 1)) * cp + (i >> lp)]; });
        }
        ok = ok && hipGetLastError() == hipSuccess;
        temps_done();
        return ok;
    }
    // modular_reduce_impl (src/fftree.rs:277-281) = REDC, multiply by c, REDC (redc_impl :232-259 with moiety S0) of a length-m
    // vector spread over the Q = 2^lq ranks [base, base + Q): every length-m/2 vector has hc = m/2Q entries per rank, in BLOCK
    // order (entry j of the rank = position a*hc + j) or, with cyc, in CYCLIC order (position j*Q + a; the split EXTENDs then run
    // cyclic-in / cyclic-out: 2 exchanges each instead of 4).  (e0, e1) = the rank's de-interleaved input, (h0, h1) = its share
    // of the result; a0i[j*sa], a1[j*sa], zi[j*sz] = the rank's entries of 1/a on S0, a on S1 and 1/Z_0 on S1, cc0[j*sc], cc1[j*sc]
    // = its entries of c on S0 / S1.  t0, x0, x1, A, B: scratch of hc elements each.
    bool modred_split(Transport& tr, int base, unsigned lq, size_t m, const E* e0, const E* e1, E* h0, E* h1, const E* a0i, const E* a1, size_t sa,
                      const E* zi, size_t sz, const E* cc0, const E* cc1, size_t sc, E* t0, E* x0, E* x1, E* A, E* B, hipStream_t s, bool cyc = false) {
        const size_t e = m / 2, hc = e >> lq;
        auto redc = [&](const E* y0, const E* y1) -> bool {
            foreach_n(s, hc, [=] __device__(size_t j) { t0[j] = F::mul(a0i[j * sa], y0[j]); });                                         // :238
            if (!extend_split(tr, base, lq, t0, t0, e, 1, s, A, B, cyc, cyc)) return false;                                            // g1 (:239-245)
            foreach_n(s, hc, [=] __device__(size_t j) { h1[j] = F::mul(zi[j * sz], F::sub(y1[j], F::mul(a1[j * sa], t0[j]))); });      // :253-255
            return extend_split(tr, base, lq, h1, h0, e, 0, s, A, B, cyc, cyc);                                                        // :256
        };
        if (!redc(e0, e1)) return false;
        foreach_n(s, hc, [=] __device__(size_t j) { x0[j] = F::mul(cc0[j * sc], h0[j]); x1[j] = F::mul(cc1[j * sc], h1[j]); });
        return redc(x0, x1);
    }
    // FFTree::exit of n evaluations block-distributed over all ranks.  Level m = c*Q runs inside groups of Q ranks with every
    // length-m/2 vector spread over the whole group, c/2 entries per rank; REDC and the pointwise steps are
    // src/fftree.rs:206-219, 232-259, 277-281 restricted to the rank's positions.
    //   Every vector of a level stays CYCLIC (position j*Q + a on rank a): one all-to-all turns the user's block into (e0, e1)
    //   cyclic over all ranks, each level is 4 cyclic split EXTENDs (8 exchanges) and ONE exchange that re-distributes (u0 | v0)
    //   for the two half-groups of the next level — rank a's whole u0 share is exactly the even (a even) or odd (a odd) half of
    //   what sub-rank a/2 of the lower half-group needs next, its v0 share the same for the upper half-group: 9 exchanges per
    //   level (block form: 17).
    bool api_exit_split(Transport& tr, const E* in, E* out, size_t n, hipStream_t s) {
        const size_t P = (size_t)tr.world, c = n / P, hc = c / 2;
        if ((P & (P - 1)) || c < 2 * P || hc < P) return false;
        E *cur = nullptr, *e0 = nullptr, *e1 = nullptr, *t0 = nullptr, *h0 = nullptr, *h1 = nullptr, *A = nullptr, *B = nullptr, *x0 = nullptr, *x1 = nullptr, *Rb = nullptr;
        E *blk = nullptr, *Y = nullptr;
        const bool sh = shard_mode();
        // round 4, FULL contexts and transforms of at most 2^gather_max_log_: EVERY top level redundantly.  The projection
        // (tools/split_project.py) shows the split top levels latency bound at these sizes — a split level of an n = 2^20 EXIT costs a
        // rank ~0.45 ms in ~30 small launches plus nine exchanges, the same level on the WHOLE block ~0.2 ms at full-chip efficiency.
        // So: ONE all-gather of the input, then every rank walks its own path down the tree — level Q on the Q c block that contains
        // its chunk (single-GPU fused passes on the full tables), keep the half that contains the chunk, level Q / 2 on that, ...
        // — less than twice the top level's arithmetic in total, no exchange after the first.  Needs the whole chain on every GPU
        // (a full context; EXIT-shard contexts keep the split levels — their point is a transform whose tables exceed one GPU, and at
        // those sizes a split level is throughput bound and wins).
        if (!sh && ilog2(n) <= gather_max_log_ && trees_.size() > ilog2(n)) {
            E *ga = nullptr, *gb = nullptr;
            if (!collective_prepare(tr, 3, n, 2, s, [&] { ga = temp(n); gb = temp(n); if (!ensure_scratch(n)) throw DeviceAllocError(); })) return false;
            P2P snd[64], rcv[64];
            if (P > 64) { temps_done(); return false; }
            for (size_t q = 0; q < P; ++q) { snd[q] = {(int)q, const_cast<E*>(in), c * sizeof(E)}; rcv[q] = {(int)q, ga + q * c, c * sizeof(E)}; }
            bool ok = tr.exchange(snd, (int)P, rcv, (int)P, s);
            E *src = ga, *dst = gb; size_t off = 0;                         // the current block starts at src + off
            for (size_t Q = P; ok && Q >= 2; Q /= 2) {
                const size_t m = c * Q;
                const size_t blk0 = ((size_t)tr.rank / Q) * Q * c;           // global position of the block of Q c that contains this rank's chunk
                if (Q == P) off = blk0;                                      // (0: the whole vector)
                exit_levels(src + off, dst, m, 1, s, scratch_, ilog2(m), ilog2(m));       // dst[0, m) = [u0 | v0] of the block
                off = (((size_t)tr.rank / (Q / 2)) & 1) * (m / 2);            // the half that contains the chunk
                E* t = src; src = dst; dst = t;
            }
            if (ok) ok = exit(src + off, out, c, 1, s);
            ok = ok && hipGetLastError() == hipSuccess;
            temps_done();
            return ok;
        }
        // round 4: the level of the PAIRS (Q = 2, blocks of 2c) runs redundantly on both ranks of a pair: ONE exchange hands each rank
        // its partner's (e0, e1) share, the level itself is the single-GPU EXIT level of the 2c block on the full tree T_2c (fused
        // passes, no pack / unpack, no cyclic passes), and each rank keeps its own half of [u0 | v0] — which IS its chunk for the
        // local levels: 1 exchange instead of 9 (8 of the split EXTENDs + the re-blocking one) for twice the level's arithmetic.
        // EXIT-shard contexts carry T_2c for it (build_exit_shard); ECFFT_SPLIT_Q2_SPLIT=1 keeps the split form on a FULL context (A/B).
        const bool q2_local = sh ? have_pair_full_ : !q2_split_;      // shard contexts: the form the ranks agreed on at build time
        E* stg = nullptr;
        const bool stripe = P >= 4 && !stripe_off_;
        if (!collective_prepare(tr, 3, n, (q2_local ? 1 : 0) | (stripe ? 4 : 0), s, [&] { if (stripe) stg = temp(c); cur = temp(c); e0 = temp(hc); e1 = temp(hc); t0 = temp(hc); h0 = temp(hc); h1 = temp(hc); A = temp(hc); B = temp(hc);
                                                      x0 = temp(hc); x1 = temp(hc); Rb = temp(c);
                                                      if (q2_local) { blk = temp(2 * c); Y = temp(2 * c); if (!ensure_scratch(2 * c)) throw DeviceAllocError(); } })) return false;
        StripeScope stripe_scope(this, stg, c * sizeof(E));
        bool ok = true;
        {   // block -> (e0, e1) cyclic over all ranks: pair t = t'*P + r' of the chunk goes to rank r', slot t'
            const size_t cpp = hc / P; const unsigned lp = ilog2(P);
            E* S = cur;                                                      // [target r'][e0 piece | e1 piece]
            foreach_n(s, hc, [=] __device__(size_t t) {
                const size_t rp = t & (P - 1), tp = t >> lp;
                S[rp * 2 * cpp + tp] = in[2 * t]; S[rp * 2 * cpp + cpp + tp] = in[2 * t + 1];
            });
            ok = exchange_group(tr, 0, P, S, Rb, 2 * cpp, s);
            foreach_n(s, hc, [=] __device__(size_t j) { const size_t r = j / cpp, tp = j - r * cpp; e0[j] = Rb[r * 2 * cpp + tp]; e1[j] = Rb[r * 2 * cpp + cpp + tp]; });
        }
        for (size_t Q = P; ok && Q >= 2; Q /= 2) {
            const size_t half = Q / 2, m = c * Q;
            const int base = (int)((tr.rank / Q) * Q), a = tr.rank - base, ap = a % (int)half;
            const Tree& T = trees_[ilog2(m)];
            if (Q == 2 && q2_local) {
                // (e0, e1)[j] = evaluations 2i, 2i + 1 of the 2c block for i = 2j + a; the partner holds i = 2j + (1 - a)
                E *pe0 = h0, *pe1 = h1;
                P2P snd[2] = {{base + 1 - a, e0, hc * sizeof(E)}, {base + 1 - a, e1, hc * sizeof(E)}};
                P2P rcv[2] = {{base + 1 - a, pe0, hc * sizeof(E)}, {base + 1 - a, pe1, hc * sizeof(E)}};
                { const size_t hb = hc * sizeof(E);
                  ok = xchg(tr, [hb](int q, std::vector<Transport::MsgDesc>& m) { m.push_back({q ^ 1, hb}); m.push_back({q ^ 1, hb}); }, snd, 2, rcv, 2, s); }
                if (!ok) break;
                { const size_t aa = (size_t)a, bb = (size_t)(1 - a);
                  foreach_n(s, hc, [=] __device__(size_t j) {
                      blk[2 * (2 * j + aa)] = e0[j]; blk[2 * (2 * j + aa) + 1] = e1[j];
                      blk[2 * (2 * j + bb)] = pe0[j]; blk[2 * (2 * j + bb) + 1] = pe1[j];
                  }); }
                const unsigned lm = ilog2(m);
                if (sh) { if (!have_pair_full_) { ok = false; break; } ovr_tree_ = &pair_full_; ovr_set_ = nullptr; }     // the full T_2c an EXIT-shard context keeps aside
                exit_levels(blk, Y, m, 1, s, scratch_, lm, lm);            // src/fftree.rs:200-224 for the block: Y = [u0 | v0]
                ovr_tree_ = nullptr;
                ok = exit(Y + (size_t)a * c, out, c, 1, s);                   // this rank's half is its chunk of the local levels
                ok = ok && hipGetLastError() == hipSuccess;
                temps_done();
                return ok;
            }
            // the rank's entries of 1/xnn_s on S0, xnn_s on S1, 1/z0_s1 and z0z0_rem_xnn_s on S0 / S1 (positions j*Q + a of each
            // half): strided views of the full tables, or the compact arrays an EXIT-shard context holds in the same fields
            const size_t s2 = sh ? 1 : 2 * Q, s1 = sh ? 1 : Q;
            const E *xi = sh ? T.xnn_inv : T.xnn_inv + 2 * a, *xo = sh ? T.xnn : T.xnn + 2 * a + 1, *zi = sh ? T.z0_inv_s1 : T.z0_inv_s1 + a;
            const E *cc0 = sh ? T.z0z0 : T.z0z0 + 2 * a, *cc1 = sh ? T.z1z1 : T.z0z0 + 2 * a + 1;
            ok = modred_split(tr, base, ilog2(Q), m, e0, e1, h0, h1, xi, xo, s2, zi, s1, cc0, cc1, s2, t0, x0, x1, A, B, s, true);
            if (!ok) break;
            foreach_n(s, hc, [=] __device__(size_t j) { h1[j] = F::mul(xi[j * s2], F::sub(e0[j], h0[j])); });               // :215-219
            P2P snd[2] = {{base + a / 2, h0, hc * sizeof(E)}, {base + (int)half + a / 2, h1, hc * sizeof(E)}};
            P2P rcv[2] = {{base + 2 * ap, e0, hc * sizeof(E)}, {base + 2 * ap + 1, e1, hc * sizeof(E)}};
            { const size_t hb = hc * sizeof(E); const int Qi = (int)Q, hi = (int)half;
              ok = xchg(tr, [hb, Qi, hi](int q, std::vector<Transport::MsgDesc>& m) { const int b = (q / Qi) * Qi, aq = q - b; m.push_back({b + aq / 2, hb}); m.push_back({b + hi + aq / 2, hb}); },
                        snd, 2, rcv, 2, s); }
        }
        if (ok) foreach_n(s, hc, [=] __device__(size_t j) { cur[2 * j] = e0[j]; cur[2 * j + 1] = e1[j]; });
        if (ok) ok = exit(cur, out, c, 1, s);
        ok = ok && hipGetLastError() == hipSuccess;
        temps_done();
        return ok;
    }

    // FFTree::enter (src/fftree.rs:164-167): n coefficients -> n evaluations on the leaves of T_n.
    // in/out: device pointers, n elements, may alias.  Uses ctx scratch (caller holds lock()).
    // `count` independent polynomials of length n laid end to end share every launch (batched form; count = 1 is the
    // reference call): level l treats the buffer as count*n/m blocks.
    bool enter(const E* in, E* out, size_t n, size_t count, hipStream_t s) {
        const size_t nt = n * count;
        if (n == 1) { if (in != out) (void)hipMemcpyAsync(out, in, nt * sizeof(E), hipMemcpyDeviceToDevice, s); return true; }
        if (!ensure_scratch(nt)) return false;
        unsigned ln = ilog2(n);
        if (count == 1 && ln >= kSplitMinLog && nside_ > 0) {
            int next_side = 0;
            in_halves_ = true;
            enter_rec(in, out, n, s, scratch_, kSplitDepth, next_side);
            in_halves_ = false;
        } else if (const int ways = batch_ways(nt, count); ways > 1) {
            // round 6: a batch runs as `ways` parts of whole polynomials on as many streams — nothing to join but the end: one part's
            // load / store phases and launch fill / drain meet the others' multiplies, as in the two-halves schedule of one transform
            const size_t part = nt / (size_t)ways, cnt = count / (size_t)ways;
            run_ways(ways, s, [&](int i, hipStream_t si) { enter_levels(in + part * i, out + part * i, n, cnt, si, scratch_ + 3 * part * i, 1, ln); });
        } else {
            enter_levels(in, out, n, count, s, scratch_, 1, ln);
        }
        return true;
    }
    // fork `ways - 1` side streams off `s`, run part i on stream i (part 0 on `s` itself), join them back into `s`
    template <class Fn>
    void run_ways(int ways, hipStream_t s, Fn fn) {
        for (int i = 1; i < ways; ++i) { (void)hipEventRecord(ev_fork_[i - 1], s); (void)hipStreamWaitEvent(sides_[i - 1], ev_fork_[i - 1], 0); }
        in_halves_ = true;
        const double w = tblw_;
        for (int i = 0; i < ways; ++i) { if (i) tblw_ = 0.0; fn(i, i ? sides_[i - 1] : s); }     // (the tables are credited once in the byte model)
        tblw_ = w;
        in_halves_ = false;
        for (int i = 1; i < ways; ++i) { (void)hipEventRecord(ev_join_[i - 1], sides_[i - 1]); (void)hipStreamWaitEvent(s, ev_join_[i - 1], 0); }
    }
    // batched ENTER / EXIT / EXTEND as concurrent parts: the number of parts (1 = one stream) — a power of two <= ECFFT_BATCH_WAYS that
    // divides the count, every part at least 2^kSplitMinLog elements
    int batch_ways(size_t nt, size_t count) const {
        if (!ECFFT_BATCH_SPLIT || count < 2) return 1;
        for (int w = ECFFT_BATCH_WAYS; w >= 2; w >>= 1)
            if (count % (size_t)w == 0 && w - 1 <= nside_ && ((nt / (size_t)w) >> kSplitMinLog) != 0) return w;
        return 1;
    }
    // Concurrent halves, recursively: levels 1..L-1 never mix the two half-blocks, so they run as two independent ENTERs
    // of n/2 on two streams.  Their launches (each half as wide) interleave on the chip, so one half's load / store phases
    // overlap the other's compute; only the top level runs on the whole array.  Scratch: f(n) = n + 2 f(n/2), f = 3n at a leaf.
    void enter_rec(const E* in, E* out, size_t n, hipStream_t s, E* base, unsigned depth, int& next_side) {
        unsigned ln = ilog2(n);
        if (depth == 0 || ln < kSplitMinLog || next_side >= nside_) { enter_levels(in, out, n, 1, s, base, 1, ln); return; }
        int me = next_side++;
        hipStream_t s2 = sides_[me];
        E* X = base; E* sA = base + n; E* sB = sA + scratch_need(n / 2, depth - 1);
        (void)hipEventRecord(ev_fork_[me], s); (void)hipStreamWaitEvent(s2, ev_fork_[me], 0);
        enter_rec(in, X, n / 2, s, sA, depth - 1, next_side);
        double w = tblw_; tblw_ = 0.0; enter_rec(in + n / 2, X + n / 2, n / 2, s2, sB, depth - 1, next_side); tblw_ = w;
        (void)hipEventRecord(ev_join_[me], s2); (void)hipStreamWaitEvent(s, ev_join_[me], 0);
        enter_levels(X, out, n, 1, s, sA, ln, ln);
    }
    static size_t scratch_need(size_t n, unsigned depth) { return depth == 0 ? 3 * n : n + 2 * scratch_need(n / 2, depth - 1) > 4 * n ? n + 2 * scratch_need(n / 2, depth - 1) : 4 * n; }
    // levels l_begin..l_end of ENTER on count arrays of n elements; `in` = state before level l_begin; base = 3*n*count
    // elements of scratch (ping, pong, EXTEND work)
    void enter_levels(const E* in, E* out, size_t n, size_t count, hipStream_t s, E* base, unsigned l_begin, unsigned l_end) const {
        const size_t nt = n * count;
        E* bufA = base; E* bufB = base + nt; E* work = base + 2 * nt;
        const E* src = in;
        unsigned l0 = l_begin;
        const unsigned ll = log_low_for(nt);
        if (l_begin == 1 && l_end >= ll) {
            // levels 1..ll: one launch, one HBM round trip (k_enter_low)
            E* dst = (l_end == ll && out != in) ? out : bufA;
            double bytes = 0; for (unsigned l = 1; l <= ll; ++l) bytes += enter_level_alg_bytes(nt, l);
            if (ll == kLogLow && kLowSymEnter && low_sym_enter())       // symmetric context: one-multiply butterflies in the cores' VALU sweeps
                ECFFT_LAUNCH(KC_FUSED_ENTER, bytes, (k_enter_low<F, (int)kLogLow, (int)kBlockLds, kLowSymEnter>), dim3((unsigned)(nt >> kLogLow)), dim3(kBlockLds),
                             2 * (sizeof(E) << kLogLow), s, dst, src, (const Tree*)d_trees_);
            else if (ll == kLogLow)
                ECFFT_LAUNCH(KC_FUSED_ENTER, bytes, (k_enter_low<F, (int)kLogLow>), dim3((unsigned)(nt >> kLogLow)), dim3(kBlockLds),
                             2 * (sizeof(E) << kLogLow), s, dst, src, (const Tree*)d_trees_);
            else
                ECFFT_LAUNCH(KC_FUSED_ENTER, bytes, (k_enter_low<F, (int)kLogLowSmall, 2 * (int)kBlockLowSmall>), dim3((unsigned)(nt >> kLogLowSmall)), dim3(2 * kBlockLowSmall),
                             2 * (sizeof(E) << kLogLowSmall), s, dst, src, (const Tree*)d_trees_);
            src = dst; l0 = ll + 1;
        }
        for (unsigned l = l0; l <= l_end; ++l) {
            const Tree& T = trees_[l];
            size_t e = T.e;
            E* dst = (l == l_end && out != in) ? out : (src == bufA ? bufB : bufA);
            // EXTEND of every [u0 | v0] half onto S1 with the combine (:155-159) folded into its last pass
            IoDesc<F> io = io_plain(src, work); io.ld_mode = LD_SCALE; io.ld_tbl = T.winv[0];
            EnterFuse ef{src, dst, sizeof(E) * (3.0 * nt + 2.0 * e * tblw_)};
            extend_core(l, io, work, nt, 0, s, 0.0, 0.0, 0, nullptr, false, &ef);
            src = dst;
        }
        if (src != out) (void)hipMemcpyAsync(out, src, nt * sizeof(E), hipMemcpyDeviceToDevice, s);
    }
    // algorithmic bytes of one ENTER / EXIT level in the stage-streaming model
    // (tblw_ = 0 while the second of two concurrent halves is enqueued: each table is credited once)
    double enter_level_alg_bytes(size_t n, unsigned l) const {
        double e = (double)((size_t)1 << (l - 1));
        return sizeof(E) * (4.0 * (l - 1) * (double)n + 3.0 * (double)n + tblw_ * (8.0 * (e - 1) + 2.0 * e));
    }
    double exit_level_alg_bytes(size_t n, unsigned l) const {
        double e = (double)((size_t)1 << (l - 1));
        return sizeof(E) * (8.0 * (l - 1) * (double)n + 8.5 * (double)n + tblw_ * (32.0 * (e - 1) + 8.5 * e));
    }
#ifndef ECFFT_SPLIT_MIN_LOG
#define ECFFT_SPLIT_MIN_LOG 19
#endif
#ifndef ECFFT_EXIT_CORES
#define ECFFT_EXIT_CORES 3      // EXTEND cores per EXIT level (exit_levels): 3 = reduction over Z1, 4 = the reference's form (A/B)
#endif
#ifndef ECFFT_EXIT_LOW_CORES
#define ECFFT_EXIT_LOW_CORES 3  // EXTEND cores per level of k_exit_low's loop in a three-core context; 4 = the four-core kernel under a three-core driver (A/B)
#endif
    static constexpr int kExitLowForm = (ECFFT_EXIT_CORES == 4 || ECFFT_EXIT_LOW_CORES == 4) ? 4 : 3;   // the second k_exit_low form a build holds
    static constexpr bool kLowSymExit = kSymKernels && ECFFT_EXIT_LOW_SYM != 0 && kExitLowForm == 3;   // k_exit_low<10,512,3,SYM> exists and is used
    static constexpr unsigned kSplitMinLog = ECFFT_SPLIT_MIN_LOG;   // single transforms of at least 2^this run as concurrent halves
#ifndef ECFFT_SPLIT_DEPTH
#define ECFFT_SPLIT_DEPTH 1
#endif
#ifndef ECFFT_NT_STORE_MAX_LOG
#define ECFFT_NT_STORE_MAX_LOG 0
#endif
    // launches of <= 2^this elements store their results non-temporally (IoDesc::nt_st, kernels.h data_st); 0 = never, the shipped value:
    // the non-temporal store itself measures neutral (<= 2^19) to negative (above) — profiles/r06/nt_data_ab.txt
    static constexpr unsigned kNtStoreMaxLog = ECFFT_NT_STORE_MAX_LOG;
    static constexpr unsigned kSplitDepth = ECFFT_SPLIT_DEPTH;      // recursion depth of the halving (2^depth concurrent streams)
    static constexpr int kMaxSides = 7;
    static constexpr unsigned kLogLow = (sizeof(E) == 32) ? 10 : 13;     // tile of the fused low-level kernels (2 x 32 KiB of LDS)
    // SMALL launches (fewer tiles than CUs) are latency bound: tools/ubench/sweep.hip shows that ONE 512-thread workgroup
    // already saturates its CU's integer VALUs (a sweep of 512 pairs = 4 multiplies per SIMD, ~3900 cycles), so the only way
    // to shorten a sweep is to spread a tile's pairs over more CUs.  For 32-byte fields launches with < kSmallTiles tiles of
    // the default size use 4x smaller tiles: 256 elements, 128-thread low-level kernels, one wave per SIMD.
    static constexpr unsigned kLogLowSmall = 8, kBlockLowSmall = 128, kSmallTiles = 256;
    // Round 4: the fused PASSES (row / column kernels) of a launch on ONE stream switch to the small tiles below 2 x kSmallTiles tiles
    // (a 2^18 launch is 256 big tiles = half the workgroup slots: ENTER at 2^18 0.77 -> 0.69 ms); inside the two-halves schedule the
    // other stream fills the chip and the rule stays at kSmallTiles (2^20 with 512: +14 %).  The low-level kernels keep kSmallTiles.
    // ECFFT_SMALL_TILES_MAX / ECFFT_SMALL_LOW_MAX: A/B knobs for both.
    unsigned small_tiles_max() const {
        static const int v = ab_env("ECFFT_SMALL_TILES_MAX") ? atoi(ab_env("ECFFT_SMALL_TILES_MAX")) : -1;
        return v >= 0 ? (unsigned)v : (in_halves_ ? kSmallTiles : 2 * kSmallTiles);
    }
    bool small_launch(size_t total) const { return sizeof(E) == 32 && (total >> kLogLow) < small_tiles_max() && total >= ((size_t)1 << kLogLowSmall); }
    static unsigned small_low_max() { static const unsigned v = ab_env("ECFFT_SMALL_LOW_MAX") ? (unsigned)atoi(ab_env("ECFFT_SMALL_LOW_MAX")) : kSmallTiles; return v; }
    unsigned log_low_for(size_t total) const { return sizeof(E) == 32 && (total >> kLogLow) < small_low_max() && total >= ((size_t)1 << kLogLowSmall) && !ef_small_off_ ? kLogLowSmall : kLogLow; }

    // FFTree::exit (src/fftree.rs:227-230): n evaluations -> n coefficients.
    bool exit(const E* in, E* out, size_t n1, size_t count, hipStream_t s) {
        const size_t n = n1 * count;
        if (n1 == 1) { if (in != out) (void)hipMemcpyAsync(out, in, n * sizeof(E), hipMemcpyDeviceToDevice, s); return true; }
        if (!ensure_scratch(n)) return false;
        unsigned ln = ilog2(n1);
        if (count == 1 && ln >= kSplitMinLog && nside_ > 0) {
            int next_side = 0;
            in_halves_ = true;
            exit_rec(in, out, n, s, scratch_, kSplitDepth, next_side);
            in_halves_ = false;
        } else if (const int ways = batch_ways(n, count); ways > 1) {
            const size_t part = n / (size_t)ways, cnt = count / (size_t)ways;
            run_ways(ways, s, [&](int i, hipStream_t si) { exit_levels(in + part * i, out + part * i, n1, cnt, si, scratch_ + 3 * part * i, ln, 1); });
        } else {
            exit_levels(in, out, n1, count, s, scratch_, ln, 1);
        }
        return true;
    }
    // top level on the whole array, then its two output blocks [u0 | v0] are independent EXITs of n/2: two streams, recursively
    void exit_rec(const E* in, E* out, size_t n, hipStream_t s, E* base, unsigned depth, int& next_side) {
        unsigned ln = ilog2(n);
        if (depth == 0 || ln < kSplitMinLog || next_side >= nside_) { exit_levels(in, out, n, 1, s, base, ln, 1); return; }
        int me = next_side++;
        hipStream_t s2 = sides_[me];
        E* Y = base; E* sA = base + n; E* sB = sA + scratch_need(n / 2, depth - 1);
        exit_levels(in, Y, n, 1, s, sA, ln, ln);
        (void)hipEventRecord(ev_fork_[me], s); (void)hipStreamWaitEvent(s2, ev_fork_[me], 0);
        exit_rec(Y, out, n / 2, s, sA, depth - 1, next_side);
        double w = tblw_; tblw_ = 0.0; exit_rec(Y + n / 2, out + n / 2, n / 2, s2, sB, depth - 1, next_side); tblw_ = w;
        (void)hipEventRecord(ev_join_[me], s2); (void)hipStreamWaitEvent(s, ev_join_[me], 0);
    }
    // levels l_from down to l_to of EXIT on count arrays of n1 evaluations; base = 3*n1*count elements of scratch
    void exit_levels(const E* in, E* out, size_t n1, size_t count, hipStream_t s, E* base, unsigned l_from, unsigned l_to) const {
        const size_t n = n1 * count;      // all sizes below are totals over the batch; the level count comes from n1
        E* bufA = base; E* bufB = base + n; E* G = base + 2 * n; E* H = G + n / 2;
        const E* cur = in;
        size_t nh = n / 2;
        const unsigned ll = log_low_for(n);
        unsigned l_stop = (l_to == 1 && l_from >= ll) ? ll : l_to - 1;      // levels l_stop..1 run fused in k_exit_low
        for (unsigned l = l_from; l > l_stop; --l) {
            const Tree& T = tree_at(l);
            E* dst = (l == l_to && out != in) ? out : (cur == bufA ? bufB : bufA);
            // The reference's pointwise steps of this level (8.5 n + 8.5 e algorithmic element moves)
            // are all folded into the first load / last store of the four EXTEND cores:
            //   core 1  load  t0 = e0 * (xinv_even / W0)                    [t0 = e0/a0        : n + e   ]
            //           store h1~ = e1 * (zinv/W1) - g1~ * (x_odd zinv)      [h1                : 1.5n + 2e], kept in H
            //   core 2  h1~ -> h0~ (S1 -> S0)
            //   core 3  load  t0' = h0~ * (c_even xinv_even)                 [h*c and t0'       : 3n + 3e ]
            //           store h1'~ = H * (c_odd zinv) - g1'~ * (x_odd zinv)  [h1'               : 1.5n + 2e]
            //   core 4  store u0 = W0 q0~ ; v0 = (e0 - u0) * xinv_even       [exit split        : 1.5n + 0.5e]
            double se = sizeof(E), ee = (double)T.e * tblw_;
            if (T.zA1 && !exit4_) {
                // THREE cores: the same Montgomery reduction over Z1, the vanishing polynomial of S1, lands on S0
                //   core 1  load  t1 = e1 * (xinv_odd / W1)                      [t1 = e1/a1]
                //           store h0~ = e0 * (z1inv/W0) - g0~ * (x_even z1inv)    [h0], kept in H
                //   core 2  h0~ -> h1~ (S0 -> S1)
                //   core 3  load  t1' = h1~ * (c'_odd xinv_odd)                   [h*c' and t1']
                //           store u0 = H * (c'_even z1inv W0) - g0'~ * (x_even z1inv W0) ; v0 = (e0 - u0) * xinv_even
                // The level is credited exit_level_alg_bytes all the same (the closed form models the reference's four cores): the
                // fourth core's stage bytes and the split's pointwise bytes go to core 3's last pass.
                IoDesc<F> io1 = io_plain(cur, G);
                io1.src_stride = 2; io1.src_off = 1; io1.ld_mode = LD_SCALE; io1.ld_tbl = T.zA1;
                io1.st_mode = ST_AXPBY; io1.st_a = T.zNB2; io1.st_b = T.zB1; io1.aux = cur; io1.aux_stride = 2; io1.aux_off = 0; io1.aux_out = H;
                NextLoad nl2{LD_PLAIN, nullptr, 0.0}, nl3{LD_SCALE, T.zC1, se * (3.0 * n + 3.0 * ee)};
                bool f1 = extend_core(l, io1, G, nh, 1, s, se * (1.0 * n + ee), se * (1.5 * n + 2.0 * ee), 0, &nl2, false);
                bool f2 = extend_core(l, io_plain(G, G), G, nh, 0, s, 0.0, 0.0, 0, &nl3, f1);
                IoDesc<F> io3 = io_plain(G, dst);
                io3.ld_mode = LD_SCALE; io3.ld_tbl = T.zC1;
                io3.st_mode = ST_EXIT3; io3.st_a = T.zNB3; io3.st_b = T.zD1; io3.aux = H; io3.aux_stride = 1; io3.aux_off = 0;
                io3.st_c = T.xie; io3.aux2 = cur;
                const double core4 = se * (2.0 * (l - 1) * (double)n + tblw_ * 8.0 * ((double)T.e - 1.0));
                extend_core(l, io3, G, nh, 1, s, f2 ? 0.0 : se * (3.0 * n + 3.0 * ee), se * (1.5 * n + 2.0 * ee) + core4 + se * (1.5 * n + 0.5 * ee), 0, nullptr, f2);
                cur = dst;
                continue;
            }
            IoDesc<F> io1 = io_plain(cur, G);
            io1.src_stride = 2; io1.src_off = 0; io1.ld_mode = LD_SCALE; io1.ld_tbl = T.A1;
            io1.st_mode = ST_AXPBY; io1.st_a = T.NB2; io1.st_b = T.B1; io1.aux = cur; io1.aux_stride = 2; io1.aux_off = 1; io1.aux_out = H;
            // consecutive cores meet at a column pass on the same tiles: run those two passes as one launch (k_stages_col_mid)
            NextLoad nl2{LD_PLAIN, nullptr, 0.0}, nl3{LD_SCALE, T.C1, se * (3.0 * n + 3.0 * ee)}, nl4{LD_PLAIN, nullptr, 0.0};
            bool f1 = extend_core(l, io1, G, nh, 0, s, se * (1.0 * n + ee), se * (1.5 * n + 2.0 * ee), 0, &nl2, false);
            bool f2 = extend_core(l, io_plain(G, G), G, nh, 1, s, 0.0, 0.0, 0, &nl3, f1);
            IoDesc<F> io3 = io_plain(G, G);
            io3.ld_mode = LD_SCALE; io3.ld_tbl = T.C1;
            io3.st_mode = ST_AXPBY; io3.st_a = T.NB2; io3.st_b = T.D1; io3.aux = H; io3.aux_stride = 1; io3.aux_off = 0; io3.aux_out = nullptr;
            bool f3 = extend_core(l, io3, G, nh, 0, s, f2 ? 0.0 : se * (3.0 * n + 3.0 * ee), se * (1.5 * n + 2.0 * ee), 0, &nl4, f2);
            IoDesc<F> io4 = io_plain(G, dst);
            io4.st_mode = ST_EXIT_SPLIT; io4.st_a = T.w[0]; io4.st_b = T.xie; io4.aux = cur; io4.aux_stride = 2; io4.aux_off = 0;
            extend_core(l, io4, G, nh, 1, s, 0.0, se * (1.5 * n + 0.5 * ee), 0, nullptr, f3);
            cur = dst;
        }
        if (l_to == 1 && l_from >= ll) {
            E* dst = out != in ? out : (cur == bufA ? bufB : bufA);
            double bytes = 0; for (unsigned l = 1; l <= ll; ++l) bytes += exit_level_alg_bytes(n, l);
            // the kernel's level loop runs the context's form (the credit above models the reference's four cores all the same)
            const bool low3 = exit_low_cores() == 3;
            if (ll == kLogLow) {
                if (low3 && kLowSymExit && low_sym_exit())      // symmetric context: pair-per-thread one-multiply sweeps in the cores
                    ECFFT_LAUNCH(KC_FUSED_EXIT, bytes, (k_exit_low<F, (int)kLogLow, (int)kBlockLds, kExitLowForm, kLowSymExit>), dim3((unsigned)(n >> kLogLow)), dim3(kBlockLds),
                                 2 * (sizeof(E) << kLogLow), s, dst, cur, (const Tree*)d_trees_);
                else if (low3) ECFFT_LAUNCH(KC_FUSED_EXIT, bytes, (k_exit_low<F, (int)kLogLow, (int)kBlockLds, kExitLowForm>), dim3((unsigned)(n >> kLogLow)), dim3(kBlockLds),
                                       2 * (sizeof(E) << kLogLow), s, dst, cur, (const Tree*)d_trees_);
                else ECFFT_LAUNCH(KC_FUSED_EXIT, bytes, (k_exit_low<F, (int)kLogLow, (int)kBlockLds, 4>), dim3((unsigned)(n >> kLogLow)), dim3(kBlockLds),
                                  2 * (sizeof(E) << kLogLow), s, dst, cur, (const Tree*)d_trees_);
            } else {
                if (low3) ECFFT_LAUNCH(KC_FUSED_EXIT, bytes, (k_exit_low<F, (int)kLogLowSmall, (int)kBlockLowSmall, kExitLowForm>), dim3((unsigned)(n >> kLogLowSmall)), dim3(kBlockLowSmall),
                                       2 * (sizeof(E) << kLogLowSmall), s, dst, cur, (const Tree*)d_trees_);
                else ECFFT_LAUNCH(KC_FUSED_EXIT, bytes, (k_exit_low<F, (int)kLogLowSmall, (int)kBlockLowSmall, 4>), dim3((unsigned)(n >> kLogLowSmall)), dim3(kBlockLowSmall),
                                  2 * (sizeof(E) << kLogLowSmall), s, dst, cur, (const Tree*)d_trees_);
            }
            cur = dst;
        }
        if (cur != out) (void)hipMemcpyAsync(out, cur, n * sizeof(E), hipMemcpyDeviceToDevice, s);
    }

    // ecfft_poly_mul (no reference counterpart): out_b = a_b * b_b for `count` pairs laid end to end (a: count x na, b: count x nb,
    // out: count x (na + nb - 1) coefficients) on T_N, N = next_pow2(na + nb - 1) <= size().  Device pointers, asynchronous on `s`;
    // caller holds lock().  An operand of at most N/2 coefficients is entered at its own size m = next_pow2(len) and LIFTED: with the
    // high half zero, enter_impl (src/fftree.rs:143-161) is ENTER_2m(p | 0) = interleave(E, EXTEND_S1(E)), E = ENTER_m(p) — v0 = v1 = 0
    // drop the xnn_s term — so every doubling costs one EXTEND of the current size.  The two operands (and all pairs) share the launches
    // from the size at which they meet, the last lift's interleave is the load of k_poly_pointwise, and one batched EXIT_N returns the
    // coefficients.  An operand longer than N/2 is zero-padded and entered at N.  a == b with na == nb (squaring) enters one operand.
    bool poly_mul(const E* a, size_t na, const E* b, size_t nb, E* out, size_t count, hipStream_t s) {
        const bool ok = poly_mul_body(a, na, na, b, nb, nb, out, count, s);
        temps_done();
        return ok && hipGetLastError() == hipSuccess;
    }
    // The leaves an operation needs, checked by the C ABI before anything runs and used by the drivers below (1: no transform)
    static size_t mul_leaves(size_t na, size_t nb) { return next_pow2(na + nb - 1); }
    // the last Newton step: p = ceil(k / 2), p' = k on next_pow2(2p + k - 2) leaves (k <= kSeriesBase runs none; the rule is the same)
    static size_t inv_series_leaves(size_t k) { return next_pow2(2 * k - 1); }
    // the two products of divrem_body: rev(a) g (2 nq - 1 coefficients) and (b mod x^nr)(q mod x^nr)
    static size_t divrem_leaves(size_t na, size_t nb) {
        const size_t nq = na >= nb ? na - nb + 1 : 0, nr = nb - 1;
        if (nq == 0 || nr == 0) return 1;
        const size_t mq = nq < nr ? nq : nr;
        return next_pow2(2 * nq - 1 > nr + mq - 1 ? 2 * nq - 1 : nr + mq - 1);
    }
    // the modular products of a power on residues of d = nm - 1 coefficients (powmod_step); the reduction of the base is divrem_leaves
    static size_t powmod_leaves(size_t nm) { return nm - 1 <= kPowSmall ? 1 : next_pow2(2 * (nm - 1) - 1); }

    // ecfft_poly_inv_series (no reference counterpart): out_b = 1/f_b mod x^k for `count` series laid end to end (f: count x nf,
    // out: count x k, crate representation).  The first p0 = ceil(k / 2^t) <= kSeriesBase coefficients come from the schoolbook
    // recurrence (k_series_base, one workgroup per pair); each Newton step p -> p' = ceil(k / 2^(t-1)) is then one fused step on
    // T_N, N = next_pow2(2p + p' - 2) (newton_step), the last one on next_pow2(2k - 1) leaves.  Device pointers; synchronous (the
    // flag of a zero f_b[0] is read back: *singular).  Caller holds lock().
    bool inv_series(const E* f, size_t nf, E* out, size_t k, size_t count, bool* singular, hipStream_t s) {
        int* flag = new_flag(s);
        const bool ok = inv_series_body(f, nf, nf, out, k, count, flag, s);
        return finish_flagged(ok, flag, singular, s);
    }

    // ecfft_poly_divrem (utils::div_rem, src/utils.rs:184-193 = ark-poly divide_with_q_and_r): a_b = b_b q_b + r_b, deg r_b < deg b_b
    // (a: count x na, b: count x nb, q: count x nq, nq = na - nb + 1 or 0, r: count x (nb - 1); q or r may be null).  With
    // g = 1/rev(b) mod x^nq, q = rev(rev(a) g mod x^nq) and r = a - (b mod x^nr)(q mod x^nr) mod x^nr: one reciprocal and two
    // products on poly_mul's lifts.  nb == 1 scales by 1/b_0; na < nb copies a into r.  Every path inverts (and checks) the
    // divisor's leading coefficient on the device.  Synchronous; *singular = some b_b[nb-1] == 0.  Caller holds lock().
    bool poly_divrem(const E* a, size_t na, const E* b, size_t nb, E* q, E* r, size_t count, bool* singular, hipStream_t s) {
        int* flag = new_flag(s);
        const bool ok = divrem_body(a, na, b, nb, q, r, count, flag, s);
        return finish_flagged(ok, flag, singular, s);
    }

    // ecfft_poly_mul_mod (the step of utils::pow_mod, src/utils.rs:205, 207: div_rem(&a.naive_mul(&b), modulus)): out_b =
    // a_b b_b mod f_b for `count` triples laid end to end (out: count x (nm - 1), zero-padded above its degree).  One poly_mul and one
    // division on its output, the temporaries held across both.  Synchronous; *singular = some f_b[nm-1] == 0.  Caller holds lock().
    bool poly_mul_mod(const E* a, size_t na, const E* b, size_t nb, const E* f, size_t nm, E* out, size_t count, bool* singular, hipStream_t s) {
        int* flag = new_flag(s);
        const size_t nc = na + nb - 1;
        E* c = temp(count * nc);
        bool ok = poly_mul_body(a, na, na, b, nb, nb, c, count, s);
        ok = divrem_body(c, nc, f, nm, nullptr, out, count, flag, s) && ok;
        return finish_flagged(ok, flag, singular, s);
    }

    // residues of at most this many coefficients are exponentiated by k_powmod_small (one workgroup per pair, no transform)
    static constexpr size_t kPowSmall = 64;
    // ecfft_poly_pow_mod (utils::pow_mod, src/utils.rs:194-211): out_b = a_b^e mod f_b for `count` pairs laid end to end (a: count x
    // na, f: count x nm, out: count x d, d = nm - 1, zero-padded above its degree); e: `nbits` bits in little-endian HOST bytes with
    // bit nbits - 1 set (nbits == 0: out_b = 1), shared by all pairs.  a is reduced below nm coefficients first (divrem_body).
    //   d <= kPowSmall: k_powmod_small, the whole scan in one launch.
    //   otherwise, on T_N, N = next_pow2(2d - 1): g = 1/rev(f) mod x^(d-1) once (inv_series_body), then g, f mod x^d and the base
    //   lifted ONCE to evaluations kept for the call (keep_modulus: 3 count N elements); res = a, then per bit below the top one a
    //   squaring and, on a set bit, a product with the kept base.  A modular product (powmod_step) is three lifts and three batched EXIT_N:
    //     c = x y                                  (2d - 1 coefficients; y is x itself or the kept base)
    //     q = rev(rev(c) mod x^(d-1) g mod x^(d-1))   against the kept g   (2d - 3 coefficients before the cut)
    //     res = (c mod x^d) - (f mod x^d) q mod x^d   against the kept f   (2d - 2 coefficients before the cut)
    //   none of which wraps on N leaves.  No Newton step and no transform of g, f or the base inside the scan; a step's temporaries
    //   go back to the pool after every product.
    // Synchronous; *singular = some f_b[nm-1] == 0.  Caller holds lock() and checks the tree rule.
    bool poly_pow_mod(const E* a, size_t na, const uint8_t* exp, size_t nbits, const E* f, size_t nm, E* out, size_t count, bool* singular,
                      hipStream_t s) {
        int* flag = new_flag(s);
        const bool ok = pow_mod_body(a, na, exp, nbits, f, nm, out, count, flag, s);
        return finish_flagged(ok, flag, singular, s);
    }
    // poly_pow_mod without the read-back of the flag and the release of the temporaries, which stay with the caller (seq_nth_term
    // takes the power of x with it)
    bool pow_mod_body(const E* a, size_t na, const uint8_t* exp, size_t nbits, const E* f, size_t nm, E* out, size_t count, int* flag,
                      hipStream_t s) {
        const size_t d = nm - 1;
        bool ok = true;
        const RowsRef base = reduced_below(a, na, f, nm, count, flag, &ok, s);           // the base below nm coefficients
        const E* ar = base.p;
        const size_t lda = base.ld, la = base.len;
        const E r1 = crate_one();
        const TE rinv = rinv_table();
        if (d <= kPowSmall) {
            const size_t nbytes = (nbits + 7) / 8;
            uint8_t* dexp = temp_as<uint8_t>(nbytes);
            if (nbytes) ok = hipMemcpyAsync(dexp, exp, nbytes, hipMemcpyHostToDevice, s) == hipSuccess && ok;
            for_chunks(count, [&](size_t c0, size_t c) {
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)c * (double)(la + nm + d) + (double)nbytes,
                             (k_powmod_small<F, (int)kPowSmall>), dim3((unsigned)c), dim3((unsigned)kPowSmall), 0, s, out + c0 * d,
                             ar + c0 * lda, lda, (uint32_t)la, f + c0 * nm, (uint32_t)d, (const uint8_t*)dexp, (uint32_t)nbits, rinv, r1, flag);
            });
            return ok;
        }
        E* kept = temp(3 * count * powmod_leaves(nm));
        KeptModulus km;
        ok = keep_modulus(f, d, ar, la, lda, count, kept, flag, &km, s) && ok;
        if (nbits == 0) foreach_n(s, count * d, [=] __device__(size_t i) { out[i] = i % d == 0 ? r1 : F::zero(); });
        else foreach_n(s, count * d, [=] __device__(size_t i) { const size_t b = i / d, j = i - b * d; out[i] = j < la ? ar[b * lda + j] : F::zero(); });
        for (size_t i = nbits > 0 ? nbits - 1 : 0; i-- > 0;) {
            ok = powmod_step(out, nullptr, km, count, rinv, s) && ok;
            if ((exp[i >> 3] >> (i & 7)) & 1) ok = powmod_step(out, km.base, km, count, rinv, s) && ok;
        }
        return ok;
    }

    // residues of at most this many coefficients are composed by k_compose_small (one workgroup per triple, no transform)
    static constexpr size_t kComposeSmall = kPowSmall;
    // the chunking of Brent-Kung: k = ceil(sqrt(nf)) baby steps, k' = ceil(nf / k) chunks of k coefficients
    static size_t compose_chunk(size_t nf) { size_t k = 1; while (k * k < nf) ++k; return k; }
    // ecfft_poly_compose_mod: out_b = f_b(g_b) mod h_b for `count` triples laid end to end (f: count x nf, g: count x ng, h: count x
    // nm, out: count x d, d = nm - 1, zero-padded above its degree).  g is reduced below nm coefficients first (divrem_body).
    //   d <= kComposeSmall: k_compose_small, Horner in one launch.
    //   otherwise Brent-Kung on the kept-modulus products of poly_pow_mod, with k = ceil(sqrt(nf)), k' = ceil(nf / k):
    //     keep_modulus(h, g) once, g the kept base;
    //     baby steps B_t = g^t mod h, t = 0 .. k ((k + 1) x count x d): B_0 = 1, B_1 = g, B_(t+1) = one copy and one powmod_step
    //       against the kept base; B_k is the giant step, so it is only taken when there is a second chunk;
    //     C_i = sum_{t<k} f[i k + t] B_t for i < k' (k_compose_rows: k' x count x d);
    //     giant steps: G = B_k lifted once and kept (count x N), res = C_(k'-1), then res = res G + C_i for i = k' - 2 .. 0.
    //   (k - 1) + (k' - 1) modular products where Horner takes nf - 1; nf <= 2 runs none.  compose_prepare takes the baby steps and
    //   compose_apply the rest: the kept composition of the distinct-degree driver, applied once here.
    // Temporaries beyond a product's own: (k + 1 + k') count d + 4 count N elements (B and C; the three kept operands and G).
    // Synchronous; *singular = some h_b[nm-1] == 0.  Caller holds lock() and checks the tree rule (powmod_leaves(nm), and
    // divrem_leaves(ng, nm) when ng >= nm: independent of nf).
    bool poly_compose_mod(const E* f, size_t nf, const E* g, size_t ng, const E* h, size_t nm, E* out, size_t count, bool* singular,
                          hipStream_t s) {
        int* flag = new_flag(s);
        const size_t d = nm - 1, cd = count * d;
        bool ok = true;
        const RowsRef gred = reduced_below(g, ng, h, nm, count, flag, &ok, s);           // g below nm coefficients
        const E* gr = gred.p;
        const size_t ldg = gred.ld, lg = gred.len;
        if (d <= kComposeSmall) {
            const TE rinv = rinv_table();
            for_chunks(count, [&](size_t c0, size_t c) {
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)c * (double)(nf + lg + nm + d), (k_compose_small<F, (int)kComposeSmall>),
                             dim3((unsigned)c), dim3((unsigned)kComposeSmall), 0, s, out + c0 * d, f + c0 * nf, (uint32_t)nf, gr + c0 * ldg, ldg,
                             (uint32_t)lg, h + c0 * nm, (uint32_t)d, rinv, flag);
            });
            return finish_flagged(ok, flag, singular, s);
        }
        E* kept = temp(3 * count * powmod_leaves(nm));
        KeptModulus km;
        ok = keep_modulus(h, d, gr, lg, ldg, count, kept, flag, &km, s) && ok;
        const size_t k = compose_chunk(nf), kp = (nf + k - 1) / k;
        KeptCompose kc;
        kc.B = temp((k + 1) * cd); kc.C = temp(kp * cd);
        ok = compose_prepare(km, gr, lg, ldg, nf, count, &kc, s) && ok;
        ok = compose_apply(kc, f, out, s) && ok;
        return finish_flagged(ok, flag, singular, s);
    }

private:
    // poly_divrem without the read-back of the flag and the release of the temporaries, which stay with the caller: the one
    // division of this layer.  poly_mul_mod and poly_pow_mod reduce with it (q == nullptr); gcd_pair, gcd_half and roots_one_large
    // divide one pair under gcd_flag_.  q or r may be null; a zero leading coefficient of some b_b raises *flag on every path.
    bool divrem_body(const E* a, size_t na, const E* b, size_t nb, E* q, E* r, size_t count, int* flag, hipStream_t s) {
        const size_t nq = na >= nb ? na - nb + 1 : 0, nr = nb - 1;
        if (nq == 0 || nb == 1) {
            E* binv = temp(count);                                // 1/b_{nb-1} of every pair, crate form
            series_base(b + nb - 1, nb, 1, binv, 1, 1, count, flag, s);
            if (nq == 0 && r) {
                foreach_n(s, count * nr, [=] __device__(size_t i) { const size_t bi = i / nr, j = i - bi * nr; r[i] = j < na ? a[bi * na + j] : F::zero(); });
            } else if (nq && q) {
                const E rinv = rinv_;
                foreach_n(s, count * na, [=] __device__(size_t i) { q[i] = F::canon(F::mul(F::mul(a[i], binv[i / na]), rinv)); });
            }
            return true;
        }
        const size_t nf = nq < nb ? nq : nb, np = 2 * nq - 1;    // rev(b) mod x^nq; rev(a) mod x^nq times g
        E* fr = temp(count * nf); E* ar = temp(count * nq); E* g = temp(count * nq); E* pq = temp(count * np);
        E* qq = q ? q : temp(count * nq);
        foreach_n(s, count * nf, [=] __device__(size_t i) { const size_t bi = i / nf, j = i - bi * nf; fr[i] = b[bi * nb + nb - 1 - j]; });
        foreach_n(s, count * nq, [=] __device__(size_t i) { const size_t bi = i / nq, j = i - bi * nq; ar[i] = a[bi * na + na - 1 - j]; });
        bool ok = inv_series_body(fr, nf, nf, g, nq, count, flag, s);
        ok = poly_mul_body(ar, nq, nq, g, nq, nq, pq, count, s) && ok;
        foreach_n(s, count * nq, [=] __device__(size_t i) { const size_t bi = i / nq, j = i - bi * nq; qq[i] = pq[bi * np + nq - 1 - j]; });
        if (r) {
            const size_t mq = nq < nr ? nq : nr, npr = nr + mq - 1, total = count * nr;
            E* pr = temp(count * npr);
            ok = poly_mul_body(b, nr, nb, qq, mq, nq, pr, count, s) && ok;    // (b mod x^nr)(q mod x^nr): rows read in place
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 3.0 * (double)total, k_divrem_sub<F>, dim3(nblocks(total)), dim3(kBlock), 0, s,
                         r, nr, a, na, (const E*)pr, npr, total);
        }
        return ok;
    }
    // An operand of a modular power or composition below the modulus: a itself, or a mod f in a temporary when na >= nm
    // (divrem_body).  Returns count rows as (pointer, row stride, length).
    struct RowsRef { const E* p; size_t ld, len; };
    RowsRef reduced_below(const E* a, size_t na, const E* f, size_t nm, size_t count, int* flag, bool* ok, hipStream_t s) {
        if (na < nm) return {a, na, na};
        E* r = temp(count * (nm - 1));
        *ok = divrem_body(a, na, f, nm, nullptr, r, count, flag, s) && *ok;
        return {r, nm - 1, nm - 1};
    }
    // rows x d coefficients lifted to T_N and written to dst (rows x N) in the natural leaf order EXIT reads; the work goes back
    // to the pool
    bool lift_and_keep(const E* src, size_t d, size_t N, size_t rows, E* dst, hipStream_t s) {
        const TempMark mark = temps_mark();
        const size_t h = N / 2;
        E* U = temp(rows * h); E* V = temp(rows * h); E* X = temp(rows * h);
        PolyEvals<F> ev;
        const bool ok = lift_one(src, d, d, false, 0, N, rows, U, V, X, &ev, s);
        materialise(ev, N, rows, dst, s);
        temps_release(mark);
        return ok;
    }
    // What the large regime of a modular power keeps for the call: the evaluations on T_N, N = powmod_leaves(d + 1), in the natural
    // leaf order EXIT reads, of g = 1/rev(f) mod x^(d-1), f mod x^d and, where there is one, the base (count x N each)
    struct KeptModulus { const E* g; const E* f; const E* base; size_t d, N; };
    // Once per call, for `count` moduli f (count x (d + 1)) and, unless null, bases of lb coefficients at a row stride of ldb: g by
    // inv_series_body, then g | f mod x^d [| base] stacked and lifted in ONE pass and written into `kept` (3 count N elements, 2 count
    // N without a base), which the caller takes before its own later temporaries; everything taken here goes back to the pool.
    bool keep_modulus(const E* f, size_t d, const E* base, size_t lb, size_t ldb, size_t count, E* kept, int* flag, KeptModulus* km, hipStream_t s) {
        const size_t nm = d + 1, ng = d - 1, cd = count * d, rows = base ? 3 : 2, N = powmod_leaves(nm);
        const TempMark mark = temps_mark();
        E* fr = temp(count * ng); E* g = temp(count * ng); E* S = temp(rows * cd);
        foreach_n(s, count * ng, [=] __device__(size_t i) { const size_t b = i / ng, j = i - b * ng; fr[i] = f[b * nm + d - j]; });
        bool ok = inv_series_body(fr, ng, ng, g, ng, count, flag, s);
        foreach_n(s, rows * cd, [=] __device__(size_t i) {
            const size_t w = i / cd, k = i - w * cd, b = k / d, j = k - b * d;
            S[i] = w == 0 ? (j < ng ? g[b * ng + j] : F::zero()) : w == 1 ? f[b * nm + j] : (j < lb ? base[b * ldb + j] : F::zero());
        });
        ok = lift_and_keep(S, d, N, rows * count, kept, s) && ok;
        temps_release(mark);
        *km = KeptModulus{kept, kept + count * N, base ? kept + 2 * count * N : nullptr, d, N};
        return ok;
    }
    // One modular product in place: res (count x d) = res y mod f, y = res itself (kept_y == nullptr) or the kept base
    bool powmod_step(E* res, const E* kept_y, const KeptModulus& km, size_t count, TE rinv, hipStream_t s) {
        const size_t d = km.d, N = km.N, h = N / 2, total = count * N;
        const unsigned lN = ilog2(N);
        const TempMark mark = temps_mark();
        E* U = temp(count * h); E* V = temp(count * h); E* X = temp(count * h); E* C = temp(total); E* T = temp(total);
        PolyEvals<F> ev;
        bool ok = lift_one(res, d, d, false, 0, N, count, U, V, X, &ev, s);
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (kept_y ? 3.0 : 2.0) * (double)total, k_powmod_pointwise<F>, dim3(nblocks(total)), dim3(kBlock), 0, s,
                     C, ev, kept_y, rinv, lN, total);
        ok = exit(C, C, N, count, s) && ok;                      // c = res y: 2d - 1 coefficients
        ok = lift_one(C, d - 1, N, true, 2 * d - 2, N, count, U, V, X, &ev, s) && ok;
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 3.0 * (double)total, k_powmod_pointwise<F>, dim3(nblocks(total)), dim3(kBlock), 0, s,
                     T, ev, km.g, rinv, lN, total);
        ok = exit(T, T, N, count, s) && ok;                      // rev(c) g: its first d - 1 coefficients are rev(q)
        ok = lift_one(T, d - 1, N, true, d - 2, N, count, U, V, X, &ev, s) && ok;
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 3.0 * (double)total, k_powmod_pointwise<F>, dim3(nblocks(total)), dim3(kBlock), 0, s,
                     T, ev, km.f, rinv, lN, total);
        ok = exit(T, T, N, count, s) && ok;                      // (f mod x^d) q
        const size_t nres = count * d;
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 3.0 * (double)nres, k_powmod_sub<F>, dim3(nblocks(nres)), dim3(kBlock), 0, s,
                     res, d, (const E*)C, (const E*)T, N, nres);
        temps_release(mark);
        return ok;
    }
    // A kept composition: what the large regime of poly_compose_mod computes from the inner polynomial g and the modulus alone, so
    // that several outer polynomials of nf coefficients share it (the Frobenius iterates of ddf_one_large all compose with x^p).
    //   prepare: on a kept modulus whose base is g, the baby steps B_t = g^t mod h, t = 0 .. k (B: (k + 1) x count x d, taken by the
    //     caller like C: k' x count x d).
    //   apply: C_i = sum_t f[i k + t] B_t (k_compose_rows), res = C_(k'-1), then res = res G + C_i against G = B_k lifted and kept
    //     (count x N, made by the first apply that has a second chunk; G == nullptr: taken here): k' - 1 modular products.
    // prepare then one apply are the launches of poly_compose_mod in their order.
    struct KeptCompose { KeptModulus km; E* B = nullptr; E* C = nullptr; E* G = nullptr; size_t nf = 0, k = 0, kp = 0, count = 0; bool lifted = false; };
    bool compose_prepare(const KeptModulus& km, const E* gr, size_t lg, size_t ldg, size_t nf, size_t count, KeptCompose* kc, hipStream_t s) {
        const size_t d = km.d, cd = count * d, k = compose_chunk(nf), kp = (nf + k - 1) / k;
        const E r1 = crate_one();
        const TE rinv = rinv_table();
        E* B = kc->B;
        kc->km = km; kc->nf = nf; kc->k = k; kc->kp = kp; kc->count = count; kc->lifted = false;
        bool ok = true;
        foreach_n(s, 2 * cd, [=] __device__(size_t i) {
            const size_t w = i / cd, q = i - w * cd, b = q / d, j = q - b * d;
            B[i] = w == 0 ? (j == 0 ? r1 : F::zero()) : (j < lg ? F::canon(gr[b * ldg + j]) : F::zero());
        });
        const size_t nb = kp > 1 ? k : k - 1;                    // the highest baby step anything reads
        for (size_t t = 1; t < nb; ++t) {
            ok = hipMemcpyAsync(B + (t + 1) * cd, B + t * cd, cd * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess && ok;
            ok = powmod_step(B + (t + 1) * cd, km.base, km, count, rinv, s) && ok;
        }
        return ok;
    }
    bool compose_apply(KeptCompose& kc, const E* f, E* out, hipStream_t s) {
        const KeptModulus& km = kc.km;
        const size_t d = km.d, count = kc.count, cd = count * d, nf = kc.nf, k = kc.k, kp = kc.kp;
        const TE rinv = rinv_table();
        const E* B = kc.B; E* C = kc.C;
        bool ok = true;
        constexpr size_t TR = ComposeTile<F>::TR;
        for_chunks(count, [&](size_t c0, size_t c) {
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)c * ((double)nf + (double)(k + kp) * (double)d), k_compose_rows<F>,
                         dim3(nblocks(d), (unsigned)((kp + TR - 1) / TR), (unsigned)c), dim3(kBlock), 0, s, C + c0 * d, B + c0 * d,
                         f + c0 * nf, nf, k, kp, d, count, rinv);
        });
        ok = hipMemcpyAsync(out, C + (kp - 1) * cd, cd * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess && ok;
        if (kp > 1) {
            if (!kc.G) kc.G = temp(count * km.N);
            if (!kc.lifted) { ok = lift_and_keep(B + k * cd, d, km.N, count, kc.G, s) && ok; kc.lifted = true; }
            const E* G = kc.G;
            for (size_t i = kp - 1; i-- > 0;) {
                ok = powmod_step(out, G, km, count, rinv, s) && ok;
                const E* Ci = C + i * cd;
                foreach_n(s, cd, [=] __device__(size_t q) { out[q] = F::canon(F::add(out[q], Ci[q])); });
            }
        }
        return ok;
    }
    // One lift: cnt vectors of mm evaluations on T_mm (cur) -> 2mm evaluations on T_2mm (dst): interleave(cur, EXTEND_S1(cur)); ext: work
    bool lift_step(const E* cur, E* dst, E* ext, size_t mm, size_t cnt, hipStream_t s) {
        if (!extend_api(cur, ext, mm, cnt, 1, s)) return false;
        foreach_n(s, 2 * mm * cnt, [=] __device__(size_t i) { dst[i] = (i & 1) ? ext[i >> 1] : cur[i >> 1]; });
        return true;
    }
    // lift_operands for ONE operand of at most N/2 coefficients with the reversal folded into its pad load: count rows of len
    // coefficients at a row stride of ld (rev: read downwards from index top) entered at m = next_pow2(len) and lifted to N; *ev
    // reads the evaluations on the leaves of T_N (the last lift's interleave).  U, V, X: count x N/2 elements of work each.
    bool lift_one(const E* src, size_t len, size_t ld, bool rev, size_t top, size_t N, size_t count, E* U, E* V, E* X, PolyEvals<F>* ev,
                  hipStream_t s) {
        const size_t h = N / 2, m = next_pow2(len), padded = count * m;
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * ((double)count * (double)len + (double)padded), k_powmod_pad<F>, dim3(nblocks(padded)), dim3(kBlock),
                     0, s, U, src, len, ld, rev ? 1u : 0u, top, ilog2(m), padded);
        bool ok = enter(U, U, m, count, s);
        E* c = U;
        for (size_t mm = m; mm < h; mm *= 2) { E* dst = c == U ? V : U; ok = lift_step(c, dst, X, mm, count, s) && ok; c = dst; }
        ok = extend_api(c, X, h, count, 1, s) && ok;              // the last lift's EXTEND; its interleave is the pointwise load
        *ev = PolyEvals<F>{c, X, h, 1u};
        return ok;
    }
    // count rows of evaluations on the leaves of T_N as a last lift leaves them (even / odd halves) -> dst (count x N), natural leaf order
    void materialise(const PolyEvals<F>& ev, size_t N, size_t count, E* dst, hipStream_t s) {
        const PolyEvals<F> e = ev;
        const unsigned lN = ilog2(N);
        foreach_n(s, count * N, [=] __device__(size_t i) {
            const size_t r = i >> lN, k = (i & (N - 1)) >> 1;
            dst[i] = ((i & 1) ? e.odd : e.even)[r * e.batch + k * e.stride];
        });
    }

public:
    // ---- ecfft_poly_gcd / ecfft_poly_xgcd (utils::gcd / utils::xgcd, src/utils.rs:132-182) ----
    // pairs of at most this many coefficients run their whole remainder sequence in k_gcd_small (one workgroup per pair, no transform)
    static constexpr size_t kGcdSmall = 256;
    // A half-GCD node, or what is left of a pair, of at most this many coefficients is one launch of k_gcd_small with as many
    // threads: the kernel's time is linear in the size where a recursion node costs milliseconds whatever its size,
    // so the leaf is as large as the hardware takes: 1024 threads per workgroup for M31 (24 KiB of LDS rows), 512 for secp256k1
    // (96 KiB of the CU's 160 KiB; 1024 would need 192)
    static constexpr size_t kGcdLeaf = sizeof(E) == 4 ? 1024 : 512;
    static_assert(kGcdLeaf >= kGcdSmall, "the leaf kernel takes whatever the small regime takes");
    // The leaves the large regime may need, checked before anything runs.  Degrees are only known on the device, so this is the
    // worst case over every degree pattern of rows of nmax coefficients: the division step of gcd_pair with a short second operand
    // (true lengths la <= nmax and lb >= 2) has a quotient of nq = la - lb + 1 < nmax coefficients, and its reciprocal's last Newton
    // step and the product rev(a) g both take next_pow2(2 nq - 1) leaves, the rule of ecfft_poly_divrem.  Everything else is
    // smaller: the top half-GCD's matrix (at most n - ceil(n/2) + 1 coefficients per entry, n = nmax - 1) times the operands is
    // nmax + (nmax - 1) / 2 coefficients, matrix and cofactor products stay below nmax + 1 (cofactor degrees add up to at most
    // deg a), and a division inside gcd_half has deg d >= m.
    static size_t gcd_leaves(size_t nmax) {
        return nmax <= kGcdSmall ? 1 : next_pow2(2 * nmax - 1);
    }
    // gcd (and, with so / to, the cofactors of the classical extended Euclidean algorithm: a s + b t = g) of `count` pairs laid end
    // to end (a: count x na, b: count x nb, g: count x max(na, nb), so: count x max(nb - 1, 1), to: count x max(na - 1, 1), all
    // zero-padded; so / to may be null).  Rows need not be trimmed.  degrees (host, may be null): deg g per pair, -1 for a = b = 0.
    //   max(na, nb) <= kGcdSmall: one launch of k_gcd_small for all pairs.
    //   otherwise the pairs run one after another (their degree sequences differ): gcd_pair.
    // Synchronous (degrees are read back per half-GCD node).  Caller holds lock() and checks the tree rule (gcd_leaves).
    bool poly_gcd(const E* a, size_t na, const E* b, size_t nb, E* so, E* to, E* g, long long* degrees, size_t count, bool want_cof, hipStream_t s) {
        const size_t ng = na > nb ? na : nb, ns = nb > 1 ? nb - 1 : 1, nt = na > 1 ? na - 1 : 1;
        const E r1 = crate_one();
        bool ok = true;
        std::vector<long long> hdeg(count, -1);
        if (ng <= kGcdSmall) {
            long long* ddeg = temp_as<long long>(count);
            for_chunks(count, [&](size_t c0, size_t c) {
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)c * (double)(na + nb + ng + ns + nt), (k_gcd_small<F, (int)kGcdSmall>), dim3((unsigned)c),
                             dim3((unsigned)kGcdSmall), 0, s, a + c0 * na, na, (uint32_t)na, b + c0 * nb, nb, (uint32_t)nb, (int32_t)0, 0u, want_cof ? 1u : 0u,
                             g + c0 * ng, (uint32_t)ng, so ? so + c0 * ns : nullptr, (uint32_t)ns, to ? to + c0 * nt : nullptr, (uint32_t)nt, ddeg + c0,
                             (E*)nullptr, (size_t)0, 0u, (int32_t*)nullptr, r1);
            });
            ok = hipMemcpyAsync(hdeg.data(), ddeg, count * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess;
        } else {
            gcd_flag_ = new_flag(s);
            for (size_t p = 0; p < count && ok; ++p) {
                const TempMark mark = temps_mark();
                ok = gcd_pair(a + p * na, na, b + p * nb, nb, so ? so + p * ns : nullptr, ns, to ? to + p * nt : nullptr, nt, g + p * ng, ng, &hdeg[p], want_cof, s);
                temps_release(mark);
            }
        }
        ok = finish_api(s) && ok;
        if (degrees) for (size_t p = 0; p < count; ++p) degrees[p] = hdeg[p];
        return ok;
    }
    // ---- ecfft_poly_xgcd_partial: the first row of the classical remainder sequence below a degree ----
    // Per pair the row (r_j, s_j, t_j), r_j = s_j a + t_j b, with the smallest j >= 1 such that deg r_j < stop (deg 0 = -1), scaled
    // so that t_j is monic (s_j where t_j = 0).  a: count x na, b: count x nb, r: count x max(na, nb), so: count x max(nb, 1) (may
    // be null), to: count x max(na, 1), all zero-padded.  degrees (host, may be null): deg r, deg s, deg t per pair.
    //   max(na, nb) <= kGcdSmall: one launch of k_xgcd_partial_small for all pairs.
    //   otherwise the pairs run one after another: gcd_partial_pair.
    // Synchronous.  Caller holds lock() and checks the tree rule (gcd_leaves).
    bool poly_xgcd_partial(const E* a, size_t na, const E* b, size_t nb, size_t stop, E* r, E* so, E* to, long long* degrees, size_t count,
                           hipStream_t s) {
        const size_t ng = na > nb ? na : nb, ns = nb, nt = na;
        if (stop > ng) stop = ng;                              // deg b < ng: every stop from ng up selects row 1
        const E r1 = crate_one();
        bool ok = true;
        std::vector<long long> hdeg(3 * count, -1);
        if (ng <= kGcdSmall) {
            long long* ddeg = temp_as<long long>(3 * count);
            for_chunks(count, [&](size_t c0, size_t c) {
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)c * (double)(na + nb + ng + ns + nt), (k_xgcd_partial_small<F, (int)kGcdSmall>),
                             dim3((unsigned)c), dim3((unsigned)kGcdSmall), 0, s, a + c0 * na, na, (uint32_t)na, b + c0 * nb, nb, (uint32_t)nb,
                             (int32_t)stop, r + c0 * ng, (uint32_t)ng, so ? so + c0 * ns : nullptr, (uint32_t)ns, to + c0 * nt, (uint32_t)nt,
                             ddeg + 3 * c0, r1);
            });
            ok = hipMemcpyAsync(hdeg.data(), ddeg, 3 * count * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess;
        } else {
            gcd_flag_ = new_flag(s);
            for (size_t p = 0; p < count && ok; ++p) {
                const TempMark mark = temps_mark();
                ok = gcd_partial_pair(a + p * na, na, b + p * nb, nb, stop, r + p * ng, ng, so ? so + p * ns : nullptr, ns, to + p * nt, nt, &hdeg[3 * p], s);
                temps_release(mark);
            }
        }
        ok = finish_api(s) && ok;
        if (degrees) for (size_t p = 0; p < 3 * count; ++p) degrees[p] = hdeg[p];
        return ok;
    }
    // ---- ecfft_seq_min_poly / ecfft_seq_nth_term: linear recurrences ----
    // rows of at most this many terms find their minimal polynomial in one workgroup (k_seq_minpoly_small), on any tree: x^n has
    // n + 1 <= kGcdSmall coefficients
    static constexpr size_t kSeqSmall = kGcdSmall - 1;
    static size_t seq_leaves(size_t n) { return n <= kSeqSmall ? 1 : gcd_leaves(n + 1); }
    // min_poly (count x (n / 2 + 1)) and orders (host) of `count` rows of n terms (seq: count x n): per row the order L and the
    // monic minimal polynomial C (leading 1 at index L, zero above) where 2 L <= n, else -1 and a zero row.  (r, ., t) = the partial
    // row of (x^n, the row) with stop = n / 2, d = max(1 + deg r, deg t); determined iff t(0) != 0 and 2 d <= n, and then L = d,
    // C = x^d t(1/x) / t(0).
    //   n <= kSeqSmall: one launch of k_seq_minpoly_small for all rows; x^n is built in LDS.
    //   otherwise x^n is written once and the rows run one after another through gcd_partial_pair (no s cofactor), each finished
    //     by k_seq_minpoly_finish on the device.
    // The verdicts are read back once.  Synchronous.  Caller holds lock() and checks the tree rule (seq_leaves).
    bool seq_min_poly(const E* seq, size_t n, E* min_poly, long long* orders, size_t count, hipStream_t s) {
        const size_t nh = n / 2 + 1;
        const E r1 = crate_one();
        bool ok = true;
        std::vector<long long> hord(count, -1);
        long long* dord = temp_as<long long>(count);
        if (n <= kSeqSmall) {
            for_chunks(count, [&](size_t c0, size_t c) {
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)c * (double)(n + nh), (k_seq_minpoly_small<F, (int)kGcdSmall>), dim3((unsigned)c),
                             dim3((unsigned)kGcdSmall), 0, s, seq + c0 * n, (uint32_t)n, min_poly + c0 * nh, dord + c0, r1);
            });
        } else {
            E* xn = temp(n + 1); E* r = temp(n + 1); E* t = temp(n + 1);
            foreach_n(s, n + 1, [=] __device__(size_t j) { E v = F::zero(); if (j == n) v = r1; xn[j] = v; });
            gcd_flag_ = new_flag(s);
            for (size_t p = 0; p < count && ok; ++p) {
                const TempMark mark = temps_mark();
                long long deg[3] = {-1, -1, -1};
                ok = gcd_partial_pair(xn, n + 1, seq + p * n, n, n / 2, r, n + 1, nullptr, n, t, n + 1, deg, s);
                if (ok) {
                    ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)(2 * (n + 1) + nh), k_seq_minpoly_finish<F>, dim3(1u), dim3(kBlock), 0, s,
                                 (const E*)r, (const E*)t, (uint32_t)n, min_poly + p * nh, dord + p, r1);
                }
                temps_release(mark);
            }
        }
        ok = ok && hipMemcpyAsync(hord.data(), dord, count * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = finish_api(s) && ok;
        for (size_t p = 0; p < count; ++p) orders[p] = hord[p];
        return ok;
    }
    // recurrences of at most this order take their terms in one workgroup (k_seq_terms_small), on any tree
    static constexpr size_t kSeqTermSmall = kPowSmall;
    // out (count x nout) = the terms s_K .. s_(K + nout - 1) of the `count` sequences with characteristic polynomials char_poly
    // (count x nc, any non-zero leading coefficient) and initial terms init (count x L, L = nc - 1): u = x^K mod C, then per term
    // the sum of u_j s_j and the shift u <- x u mod C.  index: K as `nbits` bits in little-endian HOST bytes, bit nbits - 1 set
    // (nbits == 0: K = 0), shared by all rows.
    //   L <= kSeqTermSmall: one launch of k_seq_terms_small for all rows.
    //   otherwise pow_mod_body on the base x for all rows at once (the kept-modulus scan of poly_pow_mod), then one launch of
    //     k_seq_terms; the shifted residue alternates between the power's row and a second one taken only for nout > 1.
    // Synchronous; *singular = some char_poly_b[nc-1] == 0.  Caller holds lock() and checks the tree rule (powmod_leaves(nc)).
    bool seq_nth_term(const E* char_poly, size_t nc, const E* init, const uint8_t* index, size_t nbits, E* out, size_t nout, size_t count,
                      bool* singular, hipStream_t s) {
        int* flag = new_flag(s);
        const size_t L = nc - 1;
        const E r1 = crate_one();
        const TE rinv = rinv_table();
        bool ok = true;
        if (L <= kSeqTermSmall) {
            const size_t nbytes = (nbits + 7) / 8;
            uint8_t* didx = temp_as<uint8_t>(nbytes);
            if (nbytes) ok = hipMemcpyAsync(didx, index, nbytes, hipMemcpyHostToDevice, s) == hipSuccess;
            for_chunks(count, [&](size_t c0, size_t c) {
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)c * (double)(nc + L + nout) + (double)nbytes, (k_seq_terms_small<F, (int)kPowSmall>),
                             dim3((unsigned)c), dim3((unsigned)kPowSmall), 0, s, out + c0 * nout, (uint32_t)nout, char_poly + c0 * nc, (uint32_t)L,
                             init + c0 * L, (const uint8_t*)didx, (uint32_t)nbits, rinv, r1, flag);
            });
            return finish_flagged(ok, flag, singular, s);
        }
        E* x = temp(2 * count); E* u = temp(count * L);
        E* alt = nout > 1 ? temp(count * L) : nullptr;
        foreach_n(s, 2 * count, [=] __device__(size_t i) { E v = F::zero(); if (i & 1) v = r1; x[i] = v; });
        ok = pow_mod_body(x, 2, index, nbits, char_poly, nc, u, count, flag, s);
        for_chunks(count, [&](size_t c0, size_t c) {
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)c * (double)(nc + L + nout + (nout > 1 ? 2 * (nout - 1) * L : L)), k_seq_terms<F>,
                         dim3((unsigned)c), dim3(kBlock), 0, s, out + c0 * nout, (uint32_t)nout, u + c0 * L, alt ? alt + c0 * L : (E*)nullptr,
                         char_poly + c0 * nc, (uint32_t)L, init + c0 * L, rinv);
        });
        return finish_flagged(ok, flag, singular, s);
    }

private:
    // a 2x2 polynomial matrix of the half-GCD: rows 00, 01, 10, 11 at p + i*ld, each zero-padded to len <= ld coefficients
    struct GcdMat {
        E* p = nullptr; size_t ld = 0, len = 1; bool ident = true;
        const E* at(int i) const { return p + (size_t)i * ld; }
    };
    int* gcd_flag_ = nullptr;
    // true lengths (degree + 1; 0: the zero polynomial) of nrows <= 2 rows of n coefficients at a stride of ld.  Synchronous.
    bool gcd_row_lens(const E* p, size_t ld, size_t n, int nrows, size_t* lens, hipStream_t s) {
        int h[2] = {-1, -1};
        if (n) {
            int* d = temp_as<int>(2);
            if (hipMemsetAsync(d, 0xFF, 2 * sizeof(int), s) != hipSuccess) return false;
            // from the top down, and only where the degree seen so far is lower: few lanes reach the atomic.  The look at d[r] is a
            // relaxed atomic load that only prunes work: a stale value costs one more atomicMax, never a wrong degree
            foreach_n(s, (size_t)nrows * n, [=] __device__(size_t i) {
                const size_t r = i / n, j = n - 1 - (i - r * n);
                if ((int)j > __hip_atomic_load(d + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) && !F::is_zero(F::canon(p[r * ld + j])))
                    atomicMax(d + r, (int)j);
            });
            if (hipMemcpyAsync(h, d, 2 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return false;
        }
        for (int r = 0; r < nrows; ++r) lens[r] = (size_t)(h[r] + 1);
        return true;
    }
    void gcd_gather(E* dst, const GcdRows<F>& rows, int nrows, size_t n, hipStream_t s) {
        if (!n) return;
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 2.0 * (double)nrows * (double)n, k_gcd_gather<F>, dim3(nblocks(n), (unsigned)nrows), dim3(kBlock), 0, s, dst, rows, n);
    }
    void gcd_combine(E* out, size_t ldo, int nrows, const E* P, size_t np, const GcdRows<F>* base, bool single, bool subtract, hipStream_t s) {
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 3.0 * (double)nrows * (double)ldo, k_gcd_combine<F>, dim3(nblocks(ldo), (unsigned)nrows), dim3(kBlock), 0, s,
                     out, ldo, P, np, base ? *base : GcdRows<F>{}, base ? 1u : 0u, single ? 1u : 0u, subtract ? 1u : 0u);
    }
    // P (nprod x (nl + nr - 1)) = L_i R_i: the operand rows gathered into two zero-padded blocks, then ONE batched poly_mul_body
    bool gcd_products(const GcdRows<F>& L, size_t nl, const GcdRows<F>& R, size_t nr, int nprod, E* P, hipStream_t s) {
        E* lb = temp((size_t)nprod * nl); E* rb = temp((size_t)nprod * nr);
        gcd_gather(lb, L, nprod, nl, s);
        gcd_gather(rb, R, nprod, nr, s);
        return poly_mul_body(lb, nl, nl, rb, nr, nr, P, (size_t)nprod, s);
    }
    // out = M (copy; out.p holds 4 rows of out.ld >= M.len)
    bool gcd_mat_copy(const GcdMat& M, GcdMat& out, hipStream_t s) {
        out.ident = M.ident; out.len = M.len;
        if (M.ident) return true;
        if (M.len > out.ld) return false;
        GcdRows<F> rows{};
        for (int i = 0; i < 4; ++i) { rows.p[i] = M.at(i); rows.len[i] = M.len; }
        gcd_gather(out.p, rows, 4, out.ld, s);
        return true;
    }
    // the identity written out (rows 1, 0, 0, 1 in crate form)
    void gcd_mat_materialise(GcdMat& M, hipStream_t s) {
        if (!M.ident) return;
        E* p = M.p; const size_t ld = M.ld; const E r1 = crate_one();
        foreach_n(s, 4 * ld, [=] __device__(size_t i) { E v = F::zero(); if (i == 0 || i == 3 * ld) v = r1; p[i] = v; });
        M.ident = false; M.len = 1;
    }
    // (c, d) = M (a, b) as two rows of n coefficients at cd and cd + n (n >= la, lb: the coefficients of the products from n up cancel)
    bool gcd_apply(const GcdMat& M, const E* a, size_t la, const E* b, size_t lb, E* cd, size_t n, hipStream_t s) {
        GcdRows<F> ab{};
        ab.p[0] = a; ab.len[0] = la; ab.p[1] = b; ab.len[1] = lb; ab.p[2] = a; ab.len[2] = la; ab.p[3] = b; ab.len[3] = lb;
        if (M.ident) { gcd_gather(cd, ab, 2, n, s); return true; }
        const size_t nr = la > lb ? la : lb, np = M.len + nr - 1;
        GcdRows<F> L{};
        for (int i = 0; i < 4; ++i) { L.p[i] = M.at(i); L.len[i] = M.len; }
        E* P = temp(4 * np);
        const bool ok = gcd_products(L, M.len, ab, nr, 4, P, s);
        gcd_combine(cd, n, 2, P, np, nullptr, false, false, s);
        return ok;
    }
    // out = S M (out.p holds 4 rows of out.ld coefficients)
    bool gcd_matmul(const GcdMat& S, const GcdMat& M, GcdMat& out, hipStream_t s) {
        if (S.ident) return gcd_mat_copy(M, out, s);
        if (M.ident) return gcd_mat_copy(S, out, s);
        const size_t np = S.len + M.len - 1;
        if (np > out.ld) return false;
        GcdRows<F> L{}, R{};
        static constexpr int li[8] = {0, 1, 0, 1, 2, 3, 2, 3}, ri[8] = {0, 2, 1, 3, 0, 2, 1, 3};
        for (int i = 0; i < 8; ++i) { L.p[i] = S.at(li[i]); L.len[i] = S.len; R.p[i] = M.at(ri[i]); R.len[i] = M.len; }
        E* P = temp(8 * np);
        const bool ok = gcd_products(L, S.len, R, M.len, 8, P, s);
        gcd_combine(out.p, out.ld, 4, P, np, nullptr, false, false, s);
        out.ident = false; out.len = np;
        return ok;
    }
    // out = Q M for one division step, Q = (0 1; 1 -q): rows (M10, M11, M00 - q M10, M01 - q M11)
    bool gcd_qstep(const E* q, size_t nq, const GcdMat& M0, GcdMat& out, hipStream_t s) {
        GcdMat M = M0;
        const TempMark mark = temps_mark();
        if (M.ident) { M.ld = 1; M.p = temp(4); gcd_mat_materialise(M, s); }
        const size_t np = nq + M.len - 1;
        if (np > out.ld) { temps_release(mark); return false; }
        GcdRows<F> L{}, R{}, base{};
        L.p[0] = L.p[1] = q; L.len[0] = L.len[1] = nq;
        R.p[0] = M.at(2); R.p[1] = M.at(3); R.len[0] = R.len[1] = M.len;
        E* P = temp(2 * np);
        const bool ok = gcd_products(L, nq, R, M.len, 2, P, s);
        base.p[0] = M.at(0); base.p[1] = M.at(1); base.len[0] = base.len[1] = M.len;
        gcd_combine(out.p + 2 * out.ld, out.ld, 2, P, np, &base, true, true, s);
        base.p[0] = M.at(2); base.p[1] = M.at(3);
        gcd_gather(out.p, base, 2, out.ld, s);
        out.ident = false; out.len = np;
        temps_release(mark);
        return ok;
    }
    // k_gcd_small on ONE pair of at most kGcdLeaf coefficients, with kGcdSmall threads where those hold it
    template <class... A>
    void gcd_small_one(size_t la, double bytes, hipStream_t s, A... args) {
        if (la <= kGcdSmall) ECFFT_LAUNCH(KC_POINTWISE, bytes, (k_gcd_small<F, (int)kGcdSmall>), dim3(1), dim3((unsigned)kGcdSmall), 0, s, args...);
        else ECFFT_LAUNCH(KC_POINTWISE, bytes, (k_gcd_small<F, (int)kGcdLeaf>), dim3(1), dim3((unsigned)kGcdLeaf), 0, s, args...);
    }
    // The leaf of the recursion: out = the matrix of the remainder sequence of (a, b), la <= kGcdLeaf coefficients, down to the first
    // row of degree below `bound`, by one launch of k_gcd_small in its leaf mode (out.p: 4 rows of out.ld >= la).  The row lengths
    // and the number of swaps (0: the identity) are read back.
    bool gcd_leaf_matrix(const E* a, size_t la, const E* b, size_t lb, size_t bound, GcdMat& out, hipStream_t s) {
        int32_t* info = temp_as<int32_t>(8);
        gcd_small_one(la, sizeof(E) * (double)(la + lb + 4 * la), s,
                      a, la, (uint32_t)la, b, lb, (uint32_t)lb, (int32_t)bound, 1u, 1u, (E*)nullptr, 0u, (E*)nullptr, 0u, (E*)nullptr, 0u,
                      (long long*)nullptr, out.p, out.ld, (uint32_t)la, info, crate_one());
        int32_t h[8];
        if (hipMemcpyAsync(h, info, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return false;
        out.ident = h[4] == 0;
        out.len = (size_t)(h[2] > h[3] ? h[2] : h[3]);
        return out.len <= la;
    }
    // The half-GCD of (a, b), deg a > deg b (la > lb true lengths), in the form of Thull and Yap, which is correct for abnormal
    // remainder sequences: with n = deg a and m = ceil(n / 2), out = the matrix M_j of the Euclidean algorithm (rows scaled) with
    // deg r_j >= m > deg r_{j+1}, where (r_j, r_{j+1}) = M_j (a, b).  out.p holds 4 rows of out.ld >= la coefficients.
    //   deg b < m: the identity.  la <= kGcdLeaf (512 / 1024): one launch of k_gcd_small.  Otherwise R = hgcd(a div x^m, b div x^m), (c, d) =
    //   R (a, b); if deg d >= m one division step (c, d) -> (d, e) and S = hgcd(d div x^k, e div x^k), k = 2m - deg d: out = S Q R.
    // The degrees of (c, d) and of e are read back (two waits per inner node); the node's temporaries go back to the pool.
    bool gcd_half(const E* a, size_t la, const E* b, size_t lb, GcdMat& out, hipStream_t s) {
        const size_t n = la - 1, m = (n + 1) / 2;
        out.ident = true; out.len = 1;
        if (lb < m + 1) return true;
        if (la <= kGcdLeaf) return gcd_leaf_matrix(a, la, b, lb, m, out, s);
        const TempMark mark = temps_mark();
        GcdMat R; R.ld = la - m; R.p = temp(4 * R.ld);
        bool ok = gcd_half(a + m, la - m, b + m, lb - m, R, s);
        E* cd = temp(2 * la);
        size_t l2[2] = {0, 0};
        ok = ok && gcd_apply(R, a, la, b, lb, cd, la, s) && gcd_row_lens(cd, la, la, 2, l2, s);
        const E* c = cd; const E* d = cd + la;
        const size_t lc = l2[0], ld = l2[1];
        if (!ok || ld < m + 1 || lc <= ld) {                   // lc <= ld cannot happen (deg c > deg d in a remainder sequence)
            ok = ok && ld < m + 1 && gcd_mat_copy(R, out, s);
            temps_release(mark);
            return ok;
        }
        const size_t nq = lc - ld + 1;
        E* q = temp(nq); E* e = temp(ld);
        size_t le = 0;
        ok = divrem_body(c, lc, d, ld, q, e, 1, gcd_flag_, s) && gcd_row_lens(e, ld, ld - 1, 1, &le, s);
        GcdMat M1; M1.ld = la; M1.p = temp(4 * la);
        ok = ok && gcd_qstep(q, nq, R, M1, s);
        const size_t k = 2 * m - (ld - 1);
        if (ok && le > k) {
            GcdMat S; S.ld = ld - k; S.p = temp(4 * S.ld);
            ok = gcd_half(d + k, ld - k, e + k, le - k, S, s) && gcd_matmul(S, M1, out, s);
        } else {
            ok = ok && gcd_mat_copy(M1, out, s);
        }
        temps_release(mark);
        return ok;
    }
    // The state of the outer loop of gcd_pair and gcd_partial_pair: two consecutive rows (a, b) = M (a0, b0) of la and lb true
    // coefficients on two alternating work buffers of 2 W, and M (cof only) on two alternating matrices of 4 W.
    struct GcdRun {
        const E* a; const E* b; size_t la, lb, W; bool cof;
        E* work[2]; GcdMat acc[2]; int wi = 0, mi = 0;
        GcdMat& mat() { return acc[mi]; }
    };
    GcdRun gcd_run_start(const E* a, size_t la, const E* b, size_t lb, size_t W, bool cof) {
        GcdRun g{a, b, la, lb, W, cof};
        g.work[0] = temp(2 * W); g.work[1] = temp(2 * W);
        if (cof) for (auto& M : g.acc) { M.ld = W; M.p = temp(4 * W); }
        return g;
    }
    // (a, b) <- R (a, b), M <- R M; the new lengths are read back
    bool gcd_run_apply(GcdRun& g, const GcdMat& R, hipStream_t s) {
        E* cd = g.work[g.wi]; g.wi ^= 1;
        size_t l2[2] = {0, 0};
        bool ok = gcd_apply(R, g.a, g.la, g.b, g.lb, cd, g.W, s) && gcd_row_lens(cd, g.W, g.W, 2, l2, s);
        if (ok && g.cof) { ok = gcd_matmul(R, g.acc[g.mi], g.acc[g.mi ^ 1], s); g.mi ^= 1; }
        g.a = cd; g.b = cd + g.W; g.la = l2[0]; g.lb = l2[1];
        return ok;
    }
    // one division step (a, b) <- (b, a mod b), M <- Q M (la >= lb >= 1); the remainder's length is read back
    bool gcd_run_divide(GcdRun& g, hipStream_t s) {
        const size_t nq = g.la - g.lb + 1, W = g.W, lb = g.lb;
        E* q = temp(nq);
        E* cd = g.work[g.wi]; g.wi ^= 1;
        size_t le = 0;
        GcdRows<F> rows{}; rows.p[0] = g.b; rows.len[0] = lb;
        gcd_gather(cd, rows, 1, W, s);
        if (lb > 1) (void)hipMemsetAsync(cd + W + lb - 1, 0, (W - (lb - 1)) * sizeof(E), s);
        else (void)hipMemsetAsync(cd + W, 0, W * sizeof(E), s);
        bool ok = divrem_body(g.a, g.la, g.b, lb, q, cd + W, 1, gcd_flag_, s) && gcd_row_lens(cd + W, W, lb - 1, 1, &le, s);
        if (ok && g.cof) { ok = gcd_qstep(q, nq, g.acc[g.mi], g.acc[g.mi ^ 1], s); g.mi ^= 1; }
        g.a = cd; g.b = cd + W; g.la = lb; g.lb = le;
        return ok;
    }
    // One pair above kGcdSmall: true lengths first, the longer operand first (the cofactor outputs swap with it, as the Euclidean
    // algorithm's first step does), then { half-GCD; apply; one division step } on two alternating work buffers, the accumulated
    // matrix alternating likewise (want_cof only), until the pair fits k_gcd_small, which finishes and normalises it; its cofactors
    // (s', t') of the current pair become (s, t) = (s', t') M.  A second operand that reaches zero first (b | a) ends the loop
    // with g = a / lc(a) and the first row of M.
    bool gcd_pair(const E* a0, size_t na, const E* b0, size_t nb, E* so, size_t ns, E* to, size_t nt, E* g, size_t ng, long long* deg,
                  bool want_cof, hipStream_t s) {
        size_t la = 0, lb = 0;
        if (!gcd_row_lens(a0, na, na, 1, &la, s) || !gcd_row_lens(b0, nb, nb, 1, &lb, s)) return false;
        const E* a = a0; const E* b = b0;
        if (la < lb) { std::swap(a, b); std::swap(la, lb); std::swap(so, to); std::swap(ns, nt); }
        if (!want_cof) so = to = nullptr;
        GcdRun run = gcd_run_start(a, la, b, lb, ng + 1, want_cof);
        bool ok = true;
        const E r1 = crate_one();
        while (ok && run.lb > 0 && run.la > kGcdLeaf) {
            const TempMark lvl = temps_mark();
            if (run.la > run.lb) {
                GcdMat R; R.ld = run.la; R.p = temp(4 * run.la);
                ok = gcd_half(run.a, run.la, run.b, run.lb, R, s);
                if (ok && !R.ident) ok = gcd_run_apply(run, R, s);
            }
            if (ok && run.lb > 0 && run.la > kGcdLeaf) {
                if (run.la < run.lb) { temps_release(lvl); return false; }   // cannot happen: the rows of a remainder sequence
                ok = gcd_run_divide(run, s);
            }
            temps_release(lvl);
        }
        if (!ok) return false;
        a = run.a; b = run.b; la = run.la; lb = run.lb;
        GcdMat& M = run.mat();
        if (lb == 0) {
            // g = a / lc(a); (s, t) = the first row of M over lc(a)
            *deg = (long long)la - 1;
            E* c = temp(1);
            const E* ap = a; const size_t lla = la;
            foreach_n(s, 1, [=] __device__(size_t) { E v = F::zero(); if (lla) v = F::canon(F::mul(F::inv(F::canon(ap[lla - 1])), r1)); c[0] = v; });
            foreach_n(s, ng, [=] __device__(size_t j) { E v = F::zero(); if (j < lla) v = F::canon(F::mul(ap[j], c[0])); g[j] = v; });
            if (want_cof) {
                if (M.ident) gcd_mat_materialise(M, s);
                const E* m0 = M.at(0); const E* m1 = M.at(1); const size_t ml = M.len;
                if (so) foreach_n(s, ns, [=] __device__(size_t j) { E v = F::zero(); if (j < ml) v = F::canon(F::mul(m0[j], c[0])); so[j] = v; });
                if (to) foreach_n(s, nt, [=] __device__(size_t j) { E v = F::zero(); if (j < ml) v = F::canon(F::mul(m1[j], c[0])); to[j] = v; });
            }
            return hipGetLastError() == hipSuccess;
        }
        // the pair fits the kernel: finish there
        const size_t fs = lb > 1 ? lb - 1 : 1, ft = la > 1 ? la - 1 : 1;
        const bool direct = !want_cof || M.ident;              // no matrix to apply: the kernel writes the outputs themselves
        E* gs = temp(la); E* ss = temp(fs); E* ts = temp(ft);
        long long* ddeg = temp_as<long long>(1);
        gcd_small_one(la, sizeof(E) * 4.0 * (double)(la + lb), s,
                     a, la, (uint32_t)la, b, lb, (uint32_t)lb, (int32_t)0, 0u, want_cof ? 1u : 0u, gs, (uint32_t)la, want_cof ? ss : (E*)nullptr, (uint32_t)fs,
                     want_cof ? ts : (E*)nullptr, (uint32_t)ft, ddeg, (E*)nullptr, (size_t)0, 0u, (int32_t*)nullptr, r1);
        GcdRows<F> rows{};
        rows.p[0] = gs; rows.len[0] = la;
        gcd_gather(g, rows, 1, ng, s);
        if (want_cof && direct) {
            rows.p[0] = ss; rows.len[0] = fs; if (so) gcd_gather(so, rows, 1, ns, s);
            rows.p[0] = ts; rows.len[0] = ft; if (to) gcd_gather(to, rows, 1, nt, s);
        } else if (want_cof) {
            // (s, t) = (s' M00 + t' M10, s' M01 + t' M11)
            const size_t nl = fs > ft ? fs : ft, np = nl + M.len - 1;
            GcdRows<F> L{}, R{};
            static constexpr int ri[4] = {0, 2, 1, 3};
            for (int i = 0; i < 4; ++i) { L.p[i] = (i & 1) ? ts : ss; L.len[i] = (i & 1) ? ft : fs; R.p[i] = M.at(ri[i]); R.len[i] = M.len; }
            E* P = temp(4 * np);
            ok = gcd_products(L, nl, R, M.len, 4, P, s);
            if (so) gcd_combine(so, ns, 1, P, np, nullptr, false, false, s);
            if (to) gcd_combine(to, nt, 1, P + 2 * np, np, nullptr, false, false, s);
        }
        ok = ok && hipMemcpyAsync(deg, ddeg, sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        return ok;
    }
    // One pair of ecfft_poly_xgcd_partial above kGcdSmall: gcd_pair stopped at the straddle point.  deg b < stop: row 1 = (b, 0, 1).
    // Otherwise the longer operand first (deg a < deg b: the sequence's own swap, the cofactor outputs swap with it), and with
    // (x, y) = M (a, b) two consecutive rows, deg x >= stop, while deg y >= stop and x is above kGcdLeaf:
    //   deg x = deg y: one division step (y has deg >= stop: the step cannot pass the wanted row).
    //   m = ceil(deg x / 2) >= stop: gcd_half (it ends on rows of deg >= m > deg), then one division step if still deg y >= stop.
    //   m < stop: gcd_half of (x div x^k, y div x^k), k = 2 stop - deg x: its operands have degree 2 (deg x - stop) and its
    //     half-point deg x - stop, which is stop in the rows of (x, y) — the truncation of gcd_half's own second call — so it ends
    //     on deg x' >= stop > deg y': y' is the wanted row.
    // A pair that fits the leaf kernel finishes there with bound = stop, in its matrix form; its matrix joins M like any other.
    // The wanted row is then y with the second row of M, made monic in t (in s where t = 0) by one inversion.  deg: deg r, s, t.
    bool gcd_partial_pair(const E* a0, size_t na, const E* b0, size_t nb, size_t stop, E* r, size_t ng, E* so, size_t ns, E* to, size_t nt,
                          long long* deg, hipStream_t s) {
        size_t la = 0, lb = 0;
        if (!gcd_row_lens(a0, na, na, 1, &la, s) || !gcd_row_lens(b0, nb, nb, 1, &lb, s)) return false;
        const E r1 = crate_one();
        if (lb <= stop) {
            const size_t llb = lb;
            foreach_n(s, ng, [=] __device__(size_t j) { E v = F::zero(); if (j < llb) v = F::canon(b0[j]); r[j] = v; });
            if (so) (void)hipMemsetAsync(so, 0, ns * sizeof(E), s);
            foreach_n(s, nt, [=] __device__(size_t j) { E v = F::zero(); if (j == 0) v = r1; to[j] = v; });
            deg[0] = (long long)lb - 1; deg[1] = -1; deg[2] = 0;
            return hipGetLastError() == hipSuccess;
        }
        const E* a = a0; const E* b = b0;
        bool swapped = false;
        if (la < lb) { std::swap(a, b); std::swap(la, lb); swapped = true; }
        GcdRun run = gcd_run_start(a, la, b, lb, ng + 1, true);
        bool ok = true;
        while (ok && run.lb > stop && run.la > kGcdLeaf) {
            const TempMark lvl = temps_mark();
            if (run.la < run.lb) { temps_release(lvl); return false; }   // cannot happen: the rows of a remainder sequence
            const size_t n = run.la - 1, m = (n + 1) / 2;
            if (run.la == run.lb) {
                ok = gcd_run_divide(run, s);
            } else if (m >= stop) {
                GcdMat R; R.ld = run.la; R.p = temp(4 * run.la);
                ok = gcd_half(run.a, run.la, run.b, run.lb, R, s);
                if (ok && !R.ident) ok = gcd_run_apply(run, R, s);
                if (ok && run.lb > stop && run.la > kGcdLeaf) ok = gcd_run_divide(run, s);
            } else {
                const size_t k = 2 * stop - n;                           // stop <= deg y < n and 2 stop > n: 0 < k <= stop < lb
                GcdMat R; R.ld = run.la - k; R.p = temp(4 * R.ld);
                ok = gcd_half(run.a + k, run.la - k, run.b + k, run.lb - k, R, s);
                ok = ok && !R.ident && gcd_run_apply(run, R, s);         // never the identity: deg y >= stop is its half-point,
                ok = ok && run.lb <= stop;                               // and it ends below it
            }
            temps_release(lvl);
        }
        if (!ok) return false;
        if (run.lb > stop) {
            // the pair fits the kernel: its matrix down to the first row below stop (at least one swap: deg y >= stop)
            GcdMat L; L.ld = run.la; L.p = temp(4 * run.la);
            if (!gcd_leaf_matrix(run.a, run.la, run.b, run.lb, stop, L, s) || L.ident) return false;
            if (!gcd_run_apply(run, L, s) || run.lb > stop) return false;
        }
        b = run.b; lb = run.lb;
        GcdMat& M = run.mat();
        if (M.ident) gcd_mat_materialise(M, s);
        // the row (y; M10, M11), its cofactors in the order of (a0, b0)
        const E* ps = M.at(swapped ? 3 : 2); const E* pt = M.at(swapped ? 2 : 3);
        E* both = temp(2 * M.len);
        GcdRows<F> rows{};
        rows.p[0] = ps; rows.len[0] = M.len; rows.p[1] = pt; rows.len[1] = M.len;
        gcd_gather(both, rows, 2, M.len, s);
        size_t l2[2] = {0, 0};
        if (!gcd_row_lens(both, M.len, M.len, 2, l2, s)) return false;
        const size_t ls = l2[0], lt = l2[1], lr = lb;
        if ((ls == 0 && lt == 0) || ls > ns || lt > nt || lr > ng) return false;   // cannot happen: a row of a unimodular matrix
        const E* lead = lt ? both + M.len + lt - 1 : both + ls - 1;
        const E* sp = both; const E* tp = both + M.len; const E* rp = b;
        E* c = temp(1);
        foreach_n(s, 1, [=] __device__(size_t) { c[0] = F::canon(F::mul(F::inv(F::canon(lead[0])), r1)); });
        foreach_n(s, ng, [=] __device__(size_t j) { E v = F::zero(); if (j < lr) v = F::canon(F::mul(rp[j], c[0])); r[j] = v; });
        if (so) foreach_n(s, ns, [=] __device__(size_t j) { E v = F::zero(); if (j < ls) v = F::canon(F::mul(sp[j], c[0])); so[j] = v; });
        foreach_n(s, nt, [=] __device__(size_t j) { E v = F::zero(); if (j < lt) v = F::canon(F::mul(tp[j], c[0])); to[j] = v; });
        deg[0] = (long long)lr - 1; deg[1] = (long long)ls - 1; deg[2] = (long long)lt - 1;
        return hipGetLastError() == hipSuccess;
    }
    // ---- ecfft_poly_find_roots (utils::find_roots, src/utils.rs:25-44) ----
    // out (count x d, crate form) = (x + c)^exp mod f_b for `count` MONIC moduli of degree d > kRootsSmall laid end to end (f: count x
    // (d + 1), f_b[d] = 1 in crate form).  The large regime of poly_pow_mod with another epilogue: the same kept evaluations of g =
    // 1/rev(f) and f on T_N (keep_modulus without a base), and the same squaring (powmod_step); on a set bit the product with the base is
    // not a second modular product but x r + c r - r_{d-1} f, one pass over the rows.  exp: host bytes, bit nbits - 1 set, nbits >= 1.
    bool roots_pow_body(const E* f, size_t d, uint32_t c, const uint8_t* exp, size_t nbits, E* out, size_t count, int* flag, hipStream_t s) {
        static_assert(kRootsSmall >= kPowSmall, "d > kRootsSmall is the large regime of powmod_leaves");
        E* kept = temp(2 * count * powmod_leaves(d + 1));
        E* next = temp(count * d);
        KeptModulus km;
        const bool ok = keep_modulus(f, d, nullptr, 0, 0, count, kept, flag, &km, s);
        return roots_pow_kept(f, km, c, exp, nbits, out, next, count, s) && ok;
    }
    // the scan of roots_pow_body on a modulus that is already kept (next: count x d elements of work)
    bool roots_pow_kept(const E* f, const KeptModulus& km, uint32_t c, const uint8_t* exp, size_t nbits, E* out, E* next, size_t count,
                        hipStream_t s) {
        const size_t d = km.d, nm = d + 1;
        const E r1 = crate_one();
        const TE rinv = rinv_table();
        bool ok = true;
        const E cE = F::from_u32(c), ri = rinv_;
        const E c_crate = F::canon(F::mul(cE, r1));
        foreach_n(s, count * d, [=] __device__(size_t i) {
            const size_t j = i % d;
            E v = F::zero();
            if (j == 0) v = c_crate;
            if (j == 1) v = r1;
            out[i] = v;
        });
        for (size_t i = nbits - 1; i-- > 0;) {
            ok = powmod_step(out, nullptr, km, count, rinv, s) && ok;
            if ((exp[i >> 3] >> (i & 7)) & 1) {
                foreach_n(s, count * d, [=] __device__(size_t k) {
                    const size_t b = k / d, j = k - b * d;
                    E v = F::zero();
                    if (j) v = out[k - 1];
                    if (c) v = F::canon(F::add(v, F::canon(F::mul(cE, out[k]))));
                    next[k] = F::canon(F::sub(v, F::canon(F::mul(F::mul(out[b * d + d - 1], f[b * nm + j]), ri))));
                });
                ok = hipMemcpyAsync(out, next, count * d * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess && ok;
            }
        }
        return ok;
    }
    // What a factorisation call (find_roots, squarefree, distinct_degree, equal_degree, Schoof) shares between its rows: p and
    // (p - 1) / 2 of the field as little-endian bytes (p is odd: (p - 1) / 2 is p >> 1) with their bit counts, the same 64 bytes on
    // the device (p first), and the flag its kernels raise (the attempt cap; Schoof: a sum the group law excludes).
    struct FactorCall {
        uint8_t e[64]; uint32_t nbits_p = 0, nbits_h = 0; const uint8_t* dexp = nullptr; int* flag = nullptr;
        const uint8_t* ep() const { return e; }
        const uint8_t* eh() const { return e + 32; }
    };
    // the host half of a FactorCall: the bytes and bit counts
    static FactorCall factor_exponents() {
        FactorCall fc;
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int nw = 1;
        if constexpr (sizeof(E) == 4) w[0] = F::P;
        else { nw = 8; for (int i = 0; i < 8; ++i) w[i] = F::p_limb(i); }
        for (int i = 0; i < 64; ++i) fc.e[i] = 0;
        for (int i = 0; i < nw; ++i) {
            const uint32_t hi = i + 1 < nw ? w[i + 1] : 0u, half = (w[i] >> 1) | (hi << 31);
            for (int k = 0; k < 4; ++k) { fc.e[4 * i + k] = (uint8_t)(w[i] >> (8 * k)); fc.e[32 + 4 * i + k] = (uint8_t)(half >> (8 * k)); }
        }
        auto bits = [](const uint8_t* e) { uint32_t n = 256; while (n && !((e[(n - 1) >> 3] >> ((n - 1) & 7)) & 1)) --n; return n; };
        fc.nbits_p = bits(fc.ep()); fc.nbits_h = bits(fc.eh());
        return fc;
    }
    // the whole of it: the bytes uploaded once and, for the calls whose kernels raise one, a fresh flag
    bool factor_call_init(FactorCall* fc, bool with_flag, hipStream_t s) {
        *fc = factor_exponents();
        uint8_t* dexp = temp_as<uint8_t>(64);
        fc->dexp = dexp;
        const bool ok = hipMemcpyAsync(dexp, fc->e, 64, hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        if (with_flag) fc->flag = new_flag(s);
        return ok;
    }
    // fm (d + 1 elements) = f / f[d], the row made monic: lc = R / (stored leading coefficient) is the PLAIN inverse of the leading
    // coefficient (plain x crate stays crate), fm = f lc below a leading R
    void monic_row(const E* f, size_t d, E* fm, hipStream_t s) {
        const E r1 = crate_one();
        E* lc = temp(1);
        foreach_n(s, 1, [=] __device__(size_t) { lc[0] = F::canon(F::mul(F::inv(F::canon(f[d])), r1)); });
        foreach_n(s, d + 1, [=] __device__(size_t j) { E v = r1; if (j < d) v = F::canon(F::mul(f[j], lc[0])); fm[j] = v; });
    }
    // One launch of the leaf kernel of the splitting calls over nblk rows or descriptors: k_roots_small (d == 0; frob: its Frobenius
    // flag) or k_edf_small for factors of degree d.  The latter's workspace of the h_i, d - 1 rows of the longest degree a workgroup
    // can meet (nin - 1, or K for descriptors), is shared by the chunks, which run one after another on the stream.
    void split_small_launch(const FactorCall& fc, const E* in, size_t ldin, size_t nin, size_t d, E* out, size_t ldout, const uint32_t* desc,
                            long long* n_out, bool frob, uint32_t c0, size_t nblk, double coeffs, hipStream_t s) {
        constexpr size_t K = kRootsSmall;
        static_assert(kEdfSmall == kRootsSmall, "one launch shape and one workspace rule for both leaf kernels");
        const E r1 = crate_one();
        const TE rinv = rinv_table();
        const size_t chunk = nblk < ((size_t)1 << 16) ? nblk : (size_t)1 << 16;
        const size_t nmax = desc || nin > K ? K : (nin ? nin - 1 : 0);
        const size_t ldws = d && 2 * d <= nmax ? (d - 1) * nmax : 0;           // a row that splits has 2 d <= its degree
        E* ws = ldws ? temp(chunk * ldws) : nullptr;
        for_chunks(nblk, [&](size_t b0, size_t nb) {
            const double bytes = sizeof(E) * coeffs * (double)nb / (double)nblk + 64.0;
            const E* ib = desc ? in : in + b0 * ldin;
            E* ob = desc ? out : out + b0 * ldout;
            const uint32_t* db = desc ? desc + 3 * b0 : (const uint32_t*)nullptr;
            long long* nb_out = n_out ? n_out + b0 : (long long*)nullptr;
            if (!d)
                ECFFT_LAUNCH(KC_POINTWISE, bytes, (k_roots_small<F, (int)K>), dim3((unsigned)nb), dim3((unsigned)K), 0, s, ib, ldin, (uint32_t)nin, ob,
                             ldout, db, nb_out, frob ? 1u : 0u, c0, fc.dexp, fc.nbits_p, fc.dexp + 32, fc.nbits_h, rinv, r1, fc.flag);
            else
                ECFFT_LAUNCH(KC_POINTWISE, bytes, (k_edf_small<F, (int)K>), dim3((unsigned)nb), dim3((unsigned)K), 0, s, ib, ldin, (uint32_t)nin,
                             (uint32_t)d, ob, ldout, db, nb_out, ws, ldws, c0, fc.dexp, fc.nbits_p, fc.dexp + 32, fc.nbits_h, rinv, r1, fc.flag);
        });
    }
    // The canonical order: src (rows x lds, roots (d == 0) or factors of d coefficients, in any order) -> dst (rows x ldd).
    // k_roots_rank converts as it goes; k_edf_rank reads the standard form of src, converted once per element before it.
    void split_rank_launch(E* dst, size_t ldd, const E* src, size_t lds, size_t d, const long long* n_dev, long long n_fixed, size_t rows,
                           hipStream_t s) {
        if (!ldd) return;
        const TE rinv = rinv_table();
        E* sf = d ? temp(rows * lds) : nullptr;
        if (d) foreach_n(s, rows * lds, [=] __device__(size_t i) {
            E v = F::canon(src[i]);
            if constexpr (sizeof(E) == 32) v = F::canon(F::tmul(rinv, v));
            sf[i] = v;
        });
        for (size_t r0 = 0; r0 < rows; r0 += 32768) {
            const size_t nr = rows - r0 < 32768 ? rows - r0 : 32768;
            const long long* nd = n_dev ? n_dev + r0 : (const long long*)nullptr;
            if (!d)
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 2.0 * (double)nr * (double)ldd, k_roots_rank<F>, dim3(nblocks(ldd), (unsigned)nr), dim3(kBlock), 0, s,
                             dst + r0 * ldd, ldd, src + r0 * lds, lds, nd, n_fixed, rinv);
            else
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 3.0 * (double)nr * (double)ldd, k_edf_rank<F>, dim3(nblocks(ldd), (unsigned)nr), dim3(kBlock), 0, s,
                             dst + r0 * ldd, ldd, src + r0 * lds, (const E*)sf + r0 * lds, lds, (uint32_t)d, nd, n_fixed);
        }
    }
    // A short polynomial in a long row (true length la <= kRootsSmall + 1 of nf): the small regime on its true length, ordered
    // into out; *n as the kernel reports it.  uns: nf - 1 elements of work.
    bool split_short_row(const FactorCall& fc, const E* f, size_t nf, size_t la, size_t d, E* uns, E* out, long long* n, hipStream_t s) {
        long long* dn = temp_as<long long>(1);
        split_small_launch(fc, f, nf, la ? la : 1, d, uns, nf - 1, nullptr, dn, d == 0, 1u, 1, (double)(la + kRootsSmall), s);
        split_rank_launch(out, nf - 1, uns, nf - 1, d, dn, 0, 1, s);
        return hipMemcpyAsync(n, dn, sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    // The splitting rounds of roots_one_large and edf_one_large: g, monic of degree e0 > 0 with its leading 1, is a
    // squarefree product of irreducibles of one degree (1 for the roots); its nfac factors go to out (ldo elements), ordered.
    //   Pending factors (degree > kRootsSmall) are packed with their leading 1 in two alternating buffers, the leaves (degree <=
    //   kRootsSmall) likewise in a third with a descriptor (input offset, length, output offset) each; a piece of degree dout > 0
    //   goes straight to the output (dout = 0: none does; roots end in the leaf kernel), and a gcd whose degree dout does not
    //   divide is outside the precondition.
    //   Rounds with one shift c = 1, 2, ... for all pending factors, after round_start(c): the factors are grouped by N =
    //   powmod_leaves(e + 1), the first pending one's group first, and padded inside a group to its largest degree D as the rows
    //   x^(D-e) h of M (h divides its row, so gcd(h, w - 1) is unchanged; one gather kernel on an uploaded (offset, shift) descriptor
    //   per row); group_pow(c, M, D, hs, W) takes ONE modular power per group, W (cnt x D) = the splitting element to
    //   (p - 1) / 2 modulo the rows of M, hs = the group's factors; then per factor u = gcd_pair(h, w - 1) and
    //   v = h / u (divrem_body), kept as u then v.  A factor that no shift has split in 64 consecutive rounds fails the call: the
    //   attempt cap of the leaf kernels, for the same reason.
    //   Temporaries go back to the pool per factor, per group and per round.  The leaves are finished by ONE launch of the leaf
    //   kernel from the next shift on, then the rank kernel orders the row.  uns: ldo elements of work.
    struct Fac { const E* p; size_t e; uint32_t fails; };     // a pending factor: where it lies, its degree, the shifts that failed
    template <class RoundStart, class GroupPow>
    bool split_rounds(const FactorCall& fc, const E* g, size_t e0, size_t dout, E* uns, E* out, size_t ldo, size_t nfac, RoundStart&& round_start,
                      GroupPow&& group_pow, hipStream_t s) {
        const size_t K = kRootsSmall;
        const E r1 = crate_one();
        E* pend[2] = {temp(2 * e0 + 2), temp(2 * e0 + 2)};
        E* leaf = temp(2 * e0 + 2);
        std::vector<Fac> cur, nxt;
        std::vector<uint32_t> ldesc;
        size_t leaf_used = 0, out_used = 0, nxt_used = 0;
        bool ok = true;
        E* Q = pend[0];
        auto copy = [&](E* dst, const E* src, size_t len) { ok = hipMemcpyAsync(dst, src, len * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess && ok; };
        auto keep = [&](const E* p, size_t e, uint32_t fails) {
            if (e == dout) {
                copy(uns + out_used, p, e);
                out_used += e;
            } else if (e <= K) {
                copy(leaf + leaf_used, p, e + 1);
                ldesc.push_back((uint32_t)leaf_used); ldesc.push_back((uint32_t)(e + 1)); ldesc.push_back((uint32_t)out_used);
                leaf_used += e + 1; out_used += e;
            } else {
                copy(Q + nxt_used, p, e + 1);
                nxt.push_back({Q + nxt_used, e, fails});
                nxt_used += e + 1;
            }
        };
        keep(g, e0, 0);
        cur.swap(nxt);
        int pi = 0;                                           // the buffer the pending factors are copied to
        uint32_t c = 1;
        for (; ok && !cur.empty(); ++c) {
            const TempMark round = temps_mark();
            nxt.clear();
            nxt_used = 0;
            const E* P = pend[pi]; Q = pend[pi ^= 1];
            ok = round_start(c);
            std::vector<char> done(cur.size(), 0);
            for (size_t i0 = 0; i0 < cur.size() && ok; ++i0) {
                if (done[i0]) continue;
                const size_t N = powmod_leaves(cur[i0].e + 1);
                std::vector<Fac> hs;
                size_t D = 0;
                for (size_t i = i0; i < cur.size(); ++i)
                    if (!done[i] && powmod_leaves(cur[i].e + 1) == N) { hs.push_back(cur[i]); done[i] = 1; if (cur[i].e > D) D = cur[i].e; }
                const size_t cnt = hs.size(), nm = D + 1;
                const TempMark gm = temps_mark();
                // rows x^(D - e) h: row i reads P + off_i shifted up by D - e_i
                std::vector<uint32_t> hd(2 * cnt);
                for (size_t i = 0; i < cnt; ++i) { hd[2 * i] = (uint32_t)(hs[i].p - P); hd[2 * i + 1] = (uint32_t)(D - hs[i].e); }
                uint32_t* dd = temp_as<uint32_t>(2 * cnt);
                ok = hipMemcpyAsync(dd, hd.data(), 2 * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && ok;
                E* M = temp(cnt * nm); E* W = temp(cnt * D);
                foreach_n(s, cnt * nm, [=] __device__(size_t k) {
                    const size_t b = k / nm, j = k - b * nm, sh = dd[2 * b + 1];
                    E v = F::zero();
                    if (j >= sh) v = P[dd[2 * b] + (j - sh)];
                    M[k] = v;
                });
                ok = ok && group_pow(c, (const E*)M, D, hs, W);
                foreach_n(s, cnt, [=] __device__(size_t b) { W[b * D] = F::canon(F::sub(F::canon(W[b * D]), r1)); });
                E* u = temp(D + 1); E* v = temp(D + 1); E* rem = temp(D + 1);
                for (size_t i = 0; i < cnt && ok; ++i) {
                    const E* hp = hs[i].p;
                    const size_t e = hs[i].e;
                    long long du = -1;
                    const TempMark fm = temps_mark();
                    ok = gcd_pair(hp, e + 1, W + i * D, D, nullptr, 1, nullptr, 1, u, D + 1, &du, false, s);
                    if (ok && du > 0 && (size_t)du < e) {
                        if (dout && (size_t)du % dout != 0) ok = false;     // outside the precondition
                        ok = ok && divrem_body(hp, e + 1, u, (size_t)du + 1, v, rem, 1, gcd_flag_, s);
                        keep(u, (size_t)du, 0);
                        keep(v, e - (size_t)du, 0);                   // copied on the stream before the next factor reuses u and v
                    } else if (ok) {
                        if (hs[i].fails + 1 >= 64) ok = false;
                        keep(hp, e, hs[i].fails + 1);
                    }
                    temps_release(fm);
                }
                temps_release(gm);
            }
            cur.swap(nxt);
            temps_release(round);
        }
        if (!ok) return false;
        // ---- the leaves: one launch, then the order ----
        const size_t nleaf = ldesc.size() / 3;
        if (nleaf) {
            uint32_t* ddesc = temp_as<uint32_t>(ldesc.size());
            ok = hipMemcpyAsync(ddesc, ldesc.data(), ldesc.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
            split_small_launch(fc, leaf, 0, 0, dout, uns, 0, ddesc, nullptr, false, c, nleaf, (double)(leaf_used + out_used), s);
        }
        split_rank_launch(out, ldo, uns, ldo, dout, nullptr, (long long)nfac, 1, s);
        return ok && hipGetLastError() == hipSuccess;
    }
    // The roots of ONE polynomial of nf > kRootsSmall + 1 coefficients (untrimmed, crate form) into roots (nf - 1, sorted, zero-padded).
    //   g = gcd(f, x^p - x mod f) on roots_pow_body (base x) and gcd_pair, the product of the distinct linear factors; then
    //   split_rounds with no round start, no direct output and, as a group's power, (x + c)^((p-1)/2) by ONE roots_pow_body.
    bool roots_one_large(const FactorCall& fc, const E* f, size_t nf, E* roots, long long* n, hipStream_t s) {
        const E r1 = crate_one();
        *n = 0;
        size_t la = 0;
        if (!gcd_row_lens(f, nf, nf, 1, &la, s)) return false;
        E* uns = temp(nf - 1);                                // the roots before they are ordered
        if (la <= kRootsSmall + 1) return split_short_row(fc, f, nf, la, 0, uns, roots, n, s);
        const size_t d = la - 1;
        // ---- the linear part: fm = f / lc(f), w = x^p mod fm, g = gcd(fm, w - x) ----
        E* fm = temp(la); E* w = temp(d); E* g = temp(la);
        monic_row(f, d, fm, s);
        bool ok = roots_pow_body(fm, d, 0u, fc.ep(), fc.nbits_p, w, 1, gcd_flag_, s);
        foreach_n(s, 1, [=] __device__(size_t) { w[1] = F::canon(F::sub(F::canon(w[1]), r1)); });
        long long dg = -1;
        ok = ok && gcd_pair(fm, la, w, d, nullptr, 1, nullptr, 1, g, la, &dg, false, s);
        if (!ok) return false;
        if (dg <= 0) { split_rank_launch(roots, nf - 1, uns, nf - 1, 0, nullptr, 0, 1, s); return true; }
        ok = split_rounds(fc, g, (size_t)dg, 0, uns, roots, nf - 1, (size_t)dg, [](uint32_t) { return true; },
                          [&](uint32_t c, const E* M, size_t D, const std::vector<Fac>& hs, E* W) {
                              return roots_pow_body(M, D, c, fc.eh(), fc.nbits_h, W, hs.size(), gcd_flag_, s);
                          }, s);
        if (ok) *n = dg;
        return ok;
    }
public:
    // a polynomial of at most kRootsSmall + 1 coefficients (degree <= kRootsSmall) is finished by k_roots_small, one workgroup each
    static constexpr size_t kRootsSmall = 64;
    // The leaves ecfft_poly_find_roots needs for rows of nf coefficients, checked before anything runs: poly_gcd's rule for rows of
    // nf, which covers every later step
    static size_t roots_leaves(size_t nf) {
        return nf <= kRootsSmall + 1 ? 1 : next_pow2(2 * nf - 1);
    }
    // ecfft_poly_find_roots: roots (count x (nf - 1), crate form) = the distinct roots of f_b in ascending order of their standard
    // form, zero-padded; n_roots (host): their number, -1 for the zero polynomial.  nf <= kRootsSmall + 1: ONE launch of k_roots_small
    // (with its Frobenius flag) for all rows and one of k_roots_rank.  Otherwise the polynomials run one after another
    // (roots_one_large).  *capped = a factor exhausted the attempt cap.  Synchronous.  Caller holds lock() and checks the tree rule.
    bool poly_find_roots(const E* f, size_t nf, E* roots, long long* n_roots, size_t count, bool* capped, hipStream_t s) {
        FactorCall rc;
        bool ok = factor_call_init(&rc, true, s);
        const size_t nr = nf - 1;
        if (nf <= kRootsSmall + 1) {
            long long* dn = temp_as<long long>(count);
            E* uns = temp(count * nr);
            split_small_launch(rc, f, nf, nf, 0, uns, nr, nullptr, dn, true, 1u, count, (double)count * (double)(nf + nr), s);
            split_rank_launch(roots, nr, uns, nr, 0, dn, 0, count, s);
            ok = hipMemcpyAsync(n_roots, dn, count * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && ok;
        } else {
            gcd_flag_ = new_flag(s);
            for (size_t p = 0; p < count && ok; ++p) {
                const TempMark mark = temps_mark();
                ok = roots_one_large(rc, f + p * nf, nf, roots + p * nr, &n_roots[p], s);
                temps_release(mark);
            }
        }
        return finish_flagged(ok, rc.flag, capped, s);
    }

    // ---- ecfft_poly_squarefree / ecfft_poly_distinct_degree (utils::square_free_factors / distinct_degree_factors, src/utils.rs:46-78) ----
    // a polynomial of at most kDdfSmall + 1 coefficients is finished by k_ddf_small, one workgroup each
    static constexpr size_t kDdfSmall = kRootsSmall;
    // The leaves both calls need for rows of nf coefficients, checked before anything runs: the rule of ecfft_poly_find_roots (the
    // gcds with f' and with h_i - x are pairs of at most nf coefficients; the kept modulus s has at most nf)
    static size_t ddf_leaves(size_t nf) { return roots_leaves(nf); }
    // How the large regime takes the Frobenius iterate h_(i+1) from h_i on a kept modulus of degree ds: true = the kept composition
    // h_i(h_1) (k' - 1 modular products and one k_compose_rows), false = the fresh power h_i^p (bits + popcount(p) - 2 products).
    // The rule is the count of modular products; profiles/polyddf/polyddf_time.json is the measurement behind it.
    static bool ddf_iterate_composes(size_t ds) {
#ifdef ECFFT_TEST_HOOKS
        if (ddf_iterate_force() == 1) return true;
        if (ddf_iterate_force() == 2) return false;
#endif
        const size_t k = compose_chunk(ds), kp = (ds + k - 1) / k;
        return kp - 1 <= (size_t)schoof_pow_cost();
    }
#ifdef ECFFT_TEST_HOOKS
    // ecfft_test_ddf_iterate (include/ecfft_hip_hooks.h): 0 = the rule, 1 = always the kept composition, 2 = always the fresh power
    static int& ddf_iterate_force() { static int v = 0; return v; }
#endif
private:
    // one launch of k_ddf_small over nblk rows: nin coefficients read and nw entries written per row
    void ddf_small_launch(const FactorCall& dc, const E* in, size_t ldin, size_t nin, E* out, size_t ldout, size_t nw, long long* deg, size_t lddeg,
                          bool squarefree, size_t nblk, hipStream_t s) {
        const E r1 = crate_one();
        const TE rinv = rinv_table();
        for_chunks(nblk, [&](size_t b0, size_t nb) {
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)nb * (double)(nin + nw) + 32.0, (k_ddf_small<F, (int)kDdfSmall>), dim3((unsigned)nb),
                         dim3((unsigned)kDdfSmall), 0, s, in + b0 * ldin, ldin, (uint32_t)nin, out + b0 * ldout, ldout, (uint32_t)nw, deg + b0 * lddeg, lddeg,
                         squarefree ? 1u : 0u, dc.dexp, dc.nbits_p, rinv, r1);
        });
    }
    // The monic squarefree part of ONE polynomial of true length la > kDdfSmall + 1 (f: untrimmed, crate form) into sq (la elements):
    // fm = f / lc(f), g = gcd_pair(fm, fm'), s = fm / g (divrem_body) where deg g > 0.  *ls = deg s + 1.  p exceeds every degree a
    // tree holds (the C ABI asserts it), so f' = 0 only for constants and there is no p-th-power case.
    bool squarefree_one_large(const E* f, size_t la, E* sq, size_t* ls, hipStream_t s) {
        const size_t d = la - 1;
        E* fm = temp(la); E* fd = temp(d); E* g = temp(la);
        monic_row(f, d, fm, s);
        foreach_n(s, d, [=] __device__(size_t j) { fd[j] = F::canon(F::mul(F::from_u32((uint32_t)(j + 1)), fm[j + 1])); });   // the plain integer j + 1 times a crate coefficient
        long long dg = -1;
        bool ok = gcd_pair(fm, la, fd, d, nullptr, 1, nullptr, 1, g, la, &dg, false, s);
        if (!ok || dg < 0) return false;
        *ls = la - (size_t)dg;
        if (dg == 0) return hipMemcpyAsync(sq, fm, la * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
        ok = divrem_body(fm, la, g, (size_t)dg + 1, sq, nullptr, 1, gcd_flag_, s);
        return ok;
    }
    // The Frobenius iterates of one row on its kept modulus (degree ds, N leaves; `kept` holds 4 N elements, the modulus in the first
    // two), as ddf_one_large and edf_one_large take them: h_(i+1) from h_i by ddf_iterate_composes, either
    //   the kept composition h_i(h_1): h_1 lifted as the kept base (kept + 2 N) and the baby steps taken before the first iterate
    //     that needs them (compose_prepare), then compose_apply per iterate, G at kept + 3 N;
    //   or the fresh power h_i^p: h_i lifted once to kept + 3 N (lift_and_keep), then poly_pow_mod's scan on the kept modulus.
    // frob_init takes the baby steps' and chunk sums' rows ((k + 1 + k') ds elements) where the composition is chosen.
    struct FrobIterate { KeptModulus km; KeptCompose kc; const E* h1 = nullptr; E* kept = nullptr; bool composes = false, prepared = false; };
    void frob_init(FrobIterate* fr, const KeptModulus& km, E* kept, const E* h1) {
        const size_t ds = km.d, k = compose_chunk(ds), kp = (ds + k - 1) / k;
        fr->km = km; fr->kept = kept; fr->h1 = h1;
        fr->composes = ddf_iterate_composes(ds);
        fr->prepared = false;
        if (fr->composes) { fr->kc.B = temp((k + 1) * ds); fr->kc.C = temp(kp * ds); fr->kc.G = kept + 3 * km.N; }
    }
    // hn (ds elements) = h^p mod the kept modulus for h = x^(p^i): the next iterate.  ep: p as host bytes, bit nbits_p - 1 set.
    bool frob_next(FrobIterate& fr, const E* h, E* hn, const uint8_t* ep, uint32_t nbits_p, hipStream_t s) {
        const size_t ds = fr.km.d, N = fr.km.N;
        const TE rinv = rinv_table();
        E* lifted = fr.kept + 3 * N;                          // G of the kept composition, or the lifted h_i of a fresh power
        bool ok = true;
        const TempMark mark = temps_mark();
        if (fr.composes) {
            if (!fr.prepared) {
                ok = lift_and_keep(fr.h1, ds, N, 1, fr.kept + 2 * N, s) && ok;
                fr.km.base = fr.kept + 2 * N;
                ok = compose_prepare(fr.km, fr.h1, ds, ds, ds, 1, &fr.kc, s) && ok;
                fr.prepared = true;
            }
            ok = compose_apply(fr.kc, h, hn, s) && ok;
        } else {
            ok = lift_and_keep(h, ds, N, 1, lifted, s) && ok;
            ok = hipMemcpyAsync(hn, h, ds * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess && ok;
            for (size_t bit = nbits_p - 1; bit-- > 0;) {
                ok = powmod_step(hn, nullptr, fr.km, 1, rinv, s) && ok;
                if ((ep[bit >> 3] >> (bit & 7)) & 1) ok = powmod_step(hn, lifted, fr.km, 1, rinv, s) && ok;
            }
        }
        temps_release(mark);
        return ok;
    }
    // The distinct-degree factors of ONE polynomial of nf > kDdfSmall + 1 coefficients: fac (device, nd = nf - 1 elements) and hdeg
    // (host, nd entries), both zero on entry.  ddeg: nd device entries of work.
    //   true length la <= kDdfSmall + 1, or deg s <= kDdfSmall after the squarefree part: k_ddf_small on that length.
    //   otherwise the modulus s is kept ONCE for the row (keep_modulus: g = 1/rev(s) and s on T_N, N = powmod_leaves(deg s + 1));
    //   h_1 = x^p mod s (roots_pow_kept); for i = 1, 2, ... while deg f* >= 2i: g = gcd_pair(f*, h_i - x), appended and divided out
    //   (divrem_body) where its degree is positive; then, unless the loop is about to end, h_(i+1) by ddf_iterate_composes:
    //     the kept composition h_i(h_1): h_1 lifted as the kept base and the baby steps taken before the first iterate that needs
    //       them (compose_prepare), then compose_apply per iterate;
    //     or the fresh power h_i^p: h_i lifted once (lift_and_keep), then poly_pow_mod's scan on the kept modulus.
    //   What is left of f* is irreducible of its own degree.  The modulus stays s for the whole row.
    // Temporaries beyond a step's own: 4 N elements (the kept g, s, h_1 and G or the lifted h_i), (k + 1 + k') deg s for the baby
    // steps and chunk sums, and eight rows of at most nf.  Synchronous (gcd_pair reads degrees back).
    bool ddf_one_large(const FactorCall& dc, const E* f, size_t nf, E* fac, long long* ddeg, long long* hdeg, hipStream_t s) {
        const size_t K = kDdfSmall, nd = nf - 1;
        const E r1 = crate_one();
        size_t la = 0;
        if (!gcd_row_lens(f, nf, nf, 1, &la, s)) return false;
        auto small = [&](const E* p, size_t ld, size_t len) {     // the small regime on `len` coefficients: len - 1 entries (at least one)
            const size_t nw = len > 1 ? len - 1 : 1;
            ddf_small_launch(dc, p, ld, len ? len : 1, fac, nd, nw, ddeg, nd, false, 1, s);
            return hipMemcpyAsync(hdeg, ddeg, nw * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        };
        if (la <= K + 1) return small(f, nf, la);
        E* sq = temp(la);
        size_t ls = 0;
        if (!squarefree_one_large(f, la, sq, &ls, s)) return false;
        if (ls <= K + 1) return small(sq, la, ls);
        const size_t ds = ls - 1, N = powmod_leaves(ls);
        E* kept = temp(4 * N); E* next = temp(ds);
        E* h1 = temp(ds); E* hb[2] = {temp(ds), temp(ds)}; E* w = temp(ds);
        E* fs[2] = {temp(ls), temp(ls)}; E* g = temp(ls);
        KeptModulus km;
        bool ok = keep_modulus(sq, ds, nullptr, 0, 0, 1, kept, gcd_flag_, &km, s);
        ok = roots_pow_kept(sq, km, 0u, dc.ep(), dc.nbits_p, h1, next, 1, s) && ok;
        ok = hipMemcpyAsync(hb[0], h1, ds * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess && ok;
        FrobIterate fr;
        frob_init(&fr, km, kept, h1);
        const E* fcur = sq;
        size_t e = ds, pos = 0;
        int hi = 0, fi = 0;
        for (size_t i = 1; ok && e >= 2 * i; ++i) {
            const E* h = hb[hi];
            {
                const TempMark mark = temps_mark();
                foreach_n(s, ds, [=] __device__(size_t j) { E v = F::canon(h[j]); if (j == 1) v = F::canon(F::sub(v, r1)); w[j] = v; });
                long long dg = -1;
                ok = gcd_pair(fcur, e + 1, w, ds, nullptr, 1, nullptr, 1, g, ls, &dg, false, s);
                if (ok && dg > 0) {
                    const size_t du = (size_t)dg;
                    hdeg[i - 1] = dg;
                    ok = hipMemcpyAsync(fac + pos, g, du * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
                    if (ok && du < e) {
                        ok = divrem_body(fcur, e + 1, g, du + 1, fs[fi], nullptr, 1, gcd_flag_, s);
                        fcur = fs[fi]; fi ^= 1;
                    }
                    pos += du; e -= du;
                }
                temps_release(mark);
            }
            if (!ok || e < 2 * (i + 1)) break;
            ok = frob_next(fr, h, hb[hi ^ 1], dc.ep(), dc.nbits_p, s) && ok;
            hi ^= 1;
        }
        if (ok && e > 0) {
            hdeg[e - 1] = (long long)e;
            ok = hipMemcpyAsync(fac + pos, fcur, e * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
        }
        return ok && hipGetLastError() == hipSuccess;
    }
public:
    // ecfft_poly_squarefree: out (count x nf, crate form) = the monic s_b = f_b / gcd(f_b, f_b'), zero-padded; degrees (host) = deg
    // s_b, 0 for a non-zero constant (s = 1), -1 for the zero polynomial (a zero row).  nf <= kDdfSmall + 1: ONE launch of
    // k_ddf_small in its squarefree mode for all rows.  Otherwise the rows run one after another: a short polynomial in a long row
    // goes to the same kernel on its true length, the others to squarefree_one_large.  Synchronous.  Caller holds lock() and checks
    // the tree rule (ddf_leaves).
    bool poly_squarefree(const E* f, size_t nf, E* out, long long* degrees, size_t count, hipStream_t s) {
        FactorCall dc;
        bool ok = factor_call_init(&dc, false, s);
        long long* ddeg = temp_as<long long>(count);
        if (nf <= kDdfSmall + 1) {
            ddf_small_launch(dc, f, nf, nf, out, nf, nf, ddeg, 1, true, count, s);
            ok = hipMemcpyAsync(degrees, ddeg, count * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && ok;
            return finish_api(s) && ok;
        }
        gcd_flag_ = new_flag(s);
        ok = hipMemsetAsync(out, 0, count * nf * sizeof(E), s) == hipSuccess && ok;
        for (size_t p = 0; p < count && ok; ++p) {
            const TempMark mark = temps_mark();
            const E* fp = f + p * nf;
            size_t la = 0;
            ok = gcd_row_lens(fp, nf, nf, 1, &la, s);
            if (ok && la <= kDdfSmall + 1) {
                ddf_small_launch(dc, fp, nf, la ? la : 1, out + p * nf, nf, la ? la : 1, ddeg + p, 1, true, 1, s);
                ok = hipMemcpyAsync(&degrees[p], ddeg + p, sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
            } else if (ok) {
                size_t ls = 0;
                ok = squarefree_one_large(fp, la, out + p * nf, &ls, s);
                degrees[p] = (long long)ls - 1;
            }
            temps_release(mark);
        }
        return finish_api(s) && ok;
    }
    // ecfft_poly_distinct_degree: with nd = max(nf - 1, 1), degrees (host, count x nd): degrees[b][d-1] = deg g_d, the product of the
    // monic irreducible factors of degree d of f_b (zero polynomial: -1, 0, 0, ...); factors (count x nd, crate form): the g_d of
    // positive degree in ascending d, each as its low deg g_d coefficients, then zeros.  nf <= kDdfSmall + 1: ONE launch of
    // k_ddf_small for all rows.  Otherwise the rows run one after another (their degree sequences differ): ddf_one_large.
    // Synchronous.  Caller holds lock() and checks the tree rule (ddf_leaves).
    bool poly_distinct_degree(const E* f, size_t nf, E* factors, long long* degrees, size_t count, hipStream_t s) {
        FactorCall dc;
        bool ok = factor_call_init(&dc, false, s);
        const size_t nd = nf > 1 ? nf - 1 : 1;
        long long* ddeg = temp_as<long long>(count * nd);
        if (nf <= kDdfSmall + 1) {
            ddf_small_launch(dc, f, nf, nf, factors, nd, nd, ddeg, nd, false, count, s);
            ok = hipMemcpyAsync(degrees, ddeg, count * nd * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && ok;
            return finish_api(s) && ok;
        }
        gcd_flag_ = new_flag(s);
        ok = hipMemsetAsync(factors, 0, count * nd * sizeof(E), s) == hipSuccess && ok;
        for (size_t i = 0; i < count * nd; ++i) degrees[i] = 0;
        for (size_t p = 0; p < count && ok; ++p) {
            const TempMark mark = temps_mark();
            ok = ddf_one_large(dc, f + p * nf, nf, factors + p * nd, ddeg + p * nd, degrees + p * nd, s);
            temps_release(mark);
        }
        return finish_api(s) && ok;
    }

    // ---- ecfft_poly_equal_degree (utils::equal_degree_factorization, src/utils.rs:82-113) ----
    // a polynomial of at most kEdfSmall + 1 coefficients is finished by k_edf_small, one workgroup each
    static constexpr size_t kEdfSmall = kRootsSmall;
    // The leaves the call needs for rows of ng coefficients, checked before anything runs: the rule of ecfft_poly_find_roots (the
    // kept modulus g has at most ng coefficients; every pending factor, gcd and division is smaller)
    static size_t edf_leaves(size_t ng) { return roots_leaves(ng); }
private:
    // The irreducible factors of degree d of ONE polynomial of ng > kEdfSmall + 1 coefficients (untrimmed, crate form; a squarefree
    // product of irreducibles of degree d) into fac (ng - 1 elements, ordered, zero on entry).
    //   true degree <= kEdfSmall: k_edf_small on the true length.  Otherwise gm = g / lc(g) is kept ONCE for the row (keep_modulus
    //   without a base), h_1 = x^p mod gm (roots_pow_kept, base x) and h_2 .. h_(d-1) by frob_next, kept as coefficient rows.
    //   Then split_rounds with pieces of degree d going straight to the output;
    //     at the start of round c: N_c = (x + c) prod_i (h_i + c) mod gm, each h_i + c lifted for its one powmod_step;
    //     a group's power: per factor u != gm the base N_c mod u (divrem_body, remainder only), then poly_pow_mod's large body with
    //     the bases as rows (keep_modulus with the bases, then the powmod_step scan on (p - 1) / 2).
    // Temporaries beyond a step's own: 4 N for the kept modulus and the lifted operand, (d - 1) n for the h_i, the composition's
    // baby steps, and the pending and leaf buffers of 2 n.  Synchronous (gcd_pair reads degrees back).
    bool edf_one_large(const FactorCall& fc, const E* g, size_t ng, size_t d, E* fac, long long* n, hipStream_t s) {
        const size_t nd = ng - 1;
        const E r1 = crate_one();
        const TE rinv = rinv_table();
        *n = 0;
        size_t la = 0;
        if (!gcd_row_lens(g, ng, ng, 1, &la, s)) return false;
        E* uns = temp(nd);                                    // the factors before they are ordered
        if (la <= kEdfSmall + 1) return split_short_row(fc, g, ng, la, d, uns, fac, n, s);
        const size_t dg = la - 1;
        if (dg % d != 0) { *n = -2; return true; }
        E* gm = temp(la);
        monic_row(g, dg, gm, s);
        const size_t r = dg / d;
        *n = (long long)r;
        if (r == 1) return hipMemcpyAsync(fac, gm, d * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
        // ---- the kept modulus and the Frobenius iterates, once for the row ----
        const size_t N = powmod_leaves(la);
        E* kept = temp(4 * N); E* next = temp(dg);
        E* H = temp(d > 1 ? (d - 1) * dg : 1);                // h_1 .. h_(d-1), dg coefficients each
        E* Nc = temp(dg); E* y = temp(dg);
        KeptModulus km;
        bool ok = keep_modulus(gm, dg, nullptr, 0, 0, 1, kept, gcd_flag_, &km, s);
        if (d > 1) {
            ok = roots_pow_kept(gm, km, 0u, fc.ep(), fc.nbits_p, H, next, 1, s) && ok;
            if (d > 2) {
                FrobIterate fr;
                frob_init(&fr, km, kept, H);
                for (size_t i = 2; i < d && ok; ++i) ok = frob_next(fr, H + (i - 2) * dg, H + (i - 1) * dg, fc.ep(), fc.nbits_p, s);
            }
        }
        if (!ok) return false;
        E* lifted = kept + 3 * N;                             // free once the iterates are taken: the lifted h_i + c of a norm's product
        auto norm = [&](uint32_t c) {                         // N_c modulo gm
            bool ok = true;
            const E c_crate = F::canon(F::mul(F::from_u32(c), r1));
            foreach_n(s, dg, [=] __device__(size_t j) { E v = F::zero(); if (j == 0) v = c_crate; if (j == 1) v = r1; Nc[j] = v; });
            for (size_t i = 1; i < d && ok; ++i) {
                const E* hi = H + (i - 1) * dg;
                foreach_n(s, dg, [=] __device__(size_t j) { E v = F::canon(hi[j]); if (j == 0) v = F::canon(F::add(v, c_crate)); y[j] = v; });
                ok = lift_and_keep(y, dg, N, 1, lifted, s) && ok;
                ok = powmod_step(Nc, lifted, km, 1, rinv, s) && ok;
            }
            return ok;
        };
        auto power = [&](uint32_t, const E* M, size_t D, const std::vector<Fac>& hs, E* W) {   // W = (N_c mod u)^((p-1)/2) modulo the rows of M
            const size_t cnt = hs.size();
            bool ok = true;
            E* B = temp(cnt * D);                             // the bases, zero-padded to D coefficients
            ok = hipMemsetAsync(B, 0, cnt * D * sizeof(E), s) == hipSuccess && ok;
            for (size_t i = 0; i < cnt && ok; ++i) {
                if (hs[i].e == dg) ok = hipMemcpyAsync(B + i * D, Nc, dg * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
                else ok = divrem_body(Nc, dg, hs[i].p, hs[i].e + 1, nullptr, B + i * D, 1, gcd_flag_, s);
            }
            E* kept2 = temp(3 * cnt * powmod_leaves(D + 1));
            KeptModulus kg;
            ok = ok && keep_modulus(M, D, B, D, D, cnt, kept2, gcd_flag_, &kg, s);
            ok = hipMemcpyAsync(W, B, cnt * D * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess && ok;
            for (size_t bit = fc.nbits_h - 1; ok && bit-- > 0;) {
                ok = powmod_step(W, nullptr, kg, cnt, rinv, s);
                if (ok && ((fc.eh()[bit >> 3] >> (bit & 7)) & 1)) ok = powmod_step(W, kg.base, kg, cnt, rinv, s);
            }
            return ok;
        };
        return split_rounds(fc, gm, dg, d, uns, fac, nd, r, norm, power, s);
    }
public:
    // ecfft_poly_equal_degree: with nd = max(ng - 1, 1), factors (count x nd, crate form) = the n_factors[b] monic irreducible
    // factors of degree d of g_b, each as its low d coefficients, in ascending lexicographic order of their standard form, then
    // zeros; n_factors (host): their number, -1 for the zero polynomial, 0 for a non-zero constant, -2 where d does not divide the
    // degree.  ng <= kEdfSmall + 1: ONE launch of k_edf_small for all rows and one of k_edf_rank.  Otherwise the polynomials run one
    // after another (edf_one_large).  *capped = a factor exhausted the attempt cap.  Synchronous.  Caller holds lock() and checks
    // the tree rule (edf_leaves).
    bool poly_equal_degree(const E* g, size_t ng, size_t d, E* factors, long long* n_factors, size_t count, bool* capped, hipStream_t s) {
        FactorCall ec;
        bool ok = factor_call_init(&ec, true, s);
        const size_t nd = ng > 1 ? ng - 1 : 1;
        if (ng <= kEdfSmall + 1) {
            long long* dn = temp_as<long long>(count);
            E* uns = temp(count * nd);
            split_small_launch(ec, g, ng, ng, d, uns, nd, nullptr, dn, false, 1u, count, (double)count * (double)(ng + nd), s);
            split_rank_launch(factors, nd, uns, nd, d, dn, 0, count, s);
            ok = hipMemcpyAsync(n_factors, dn, count * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && ok;
        } else {
            gcd_flag_ = new_flag(s);
            ok = hipMemsetAsync(factors, 0, count * nd * sizeof(E), s) == hipSuccess && ok;
            for (size_t p = 0; p < count && ok; ++p) {
                const TempMark mark = temps_mark();
                ok = edf_one_large(ec, g + p * ng, ng, d, factors + p * nd, &n_factors[p], s);
                temps_release(mark);
            }
        }
        return finish_flagged(ok, ec.flag, capped, s);
    }

    // ---- ecfft_poly_squarefree_decompose / ecfft_poly_factor: f = lc prod_i a_i^i = lc prod_j q_j^e_j ----
    // a polynomial of at most kFactorSmall + 1 coefficients is taken apart by the workgroup kernels, one workgroup per row or part
    static constexpr size_t kFactorSmall = kRootsSmall;
    // The leaves both calls need for rows of nf coefficients are ddf_leaves(nf), the rule of ecfft_poly_find_roots: Yun's gcds and
    // divisions are pairs of at most nf coefficients, and every part goes to ddf_one_large and edf_one_large on fewer.
private:
    static_assert(kFactorSmall == kDdfSmall && kFactorSmall == kEdfSmall, "the parts of a small row go to k_ddf_small and k_edf_small as they are");
    // A squarefree part a_e of row `row`: its low `deg` coefficients on the device (the leading 1 implied), and a group of r = len / d
    // irreducible factors of degree d at multiplicity e, ranked, laid end to end at src.
    struct FacPart { size_t row; long long e; size_t deg; const E* src; };
    struct FacGroup { size_t row; long long e, d; size_t len; const E* src; };
    struct FacSeg { const E* src; E* dst; size_t len; };
    // one launch of k_yun_small over nblk rows: nin coefficients read, nw entries of parts and degrees written per row
    void yun_small_launch(const E* in, size_t ldin, size_t nin, E* out, size_t ldout, size_t nw, long long* deg, size_t lddeg, E* lead, size_t nblk,
                          hipStream_t s) {
        const E r1 = crate_one();
        for_chunks(nblk, [&](size_t b0, size_t nb) {
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (double)nb * (double)(nin + nw) + 32.0, (k_yun_small<F, (int)kFactorSmall>), dim3((unsigned)nb),
                         dim3((unsigned)kFactorSmall), 0, s, in + b0 * ldin, ldin, (uint32_t)nin, out + b0 * ldout, ldout, (uint32_t)nw, deg + b0 * lddeg, lddeg,
                         lead ? lead + b0 : (E*)nullptr, r1);
        });
    }
    // The segments (uploaded once) laid into rows of ld entries of dst, row i = segment i: its len coefficients, then with `monic`
    // the leading 1, then zeros.  With ld == 0 each segment goes to its own dst instead and nothing else is written (w: the longest).
    bool factor_segments(const std::vector<FacSeg>& segs, E* dst, size_t ld, size_t w, hipStream_t s) {
        const size_t n = segs.size();
        if (!n) return true;
        const E r1 = crate_one();
        FacSeg* dsegs = temp_as<FacSeg>(n);
        const bool ok = hipMemcpyAsync(dsegs, segs.data(), n * sizeof(FacSeg), hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        if (ld) foreach_n(s, n * ld, [=] __device__(size_t k) {
            const size_t i = k / ld, j = k - i * ld, len = dsegs[i].len;
            E v = F::zero();
            if (j < len) v = F::canon(dsegs[i].src[j]);
            if (j == len) v = r1;
            dst[k] = v;
        });
        else foreach_n(s, n * w, [=] __device__(size_t k) {
            const size_t i = k / w, j = k - i * w;
            if (j < dsegs[i].len) dsegs[i].dst[j] = F::canon(dsegs[i].src[j]);
        });
        return ok;
    }
    // Yun's loop on ONE polynomial of true length la > kFactorSmall + 1 (f: untrimmed, crate form), k_yun_small's steps on gcd_pair and
    // the division body: b (monic, degree db) and a row d of db coefficients; u = gcd_pair(b, d) (d = 0: u = b); where deg u > 0,
    // b <- b / u and c = d / u (divrem_body), else c = d; d <- c - b' (the plain integer j + 1 times a crate coefficient).  Step 0
    // starts from b = f / lc(f), d = f' and yields nothing; step i >= 1 hands a_i = u of positive degree to emit(i, u with its leading
    // 1, deg u), and a step with deg u = db is the last.  A squarefree f costs steps 0 and 1.  Synchronous (gcd_pair reads degrees back).
    template <class Emit>
    bool yun_one_large(const E* f, size_t la, Emit&& emit, hipStream_t s) {
        const size_t n = la - 1;
        E* bb[2] = {temp(la), temp(la)}; E* dd[2] = {temp(la), temp(la)}; E* u = temp(la);
        monic_row(f, n, bb[0], s);
        { const E* b0 = bb[0]; E* d0 = dd[0]; foreach_n(s, n, [=] __device__(size_t j) { d0[j] = F::canon(F::mul(F::from_u32((uint32_t)(j + 1)), b0[j + 1])); }); }
        size_t db = n;
        int bi = 0, di = 0;
        bool ok = true;
        for (size_t i = 0; ok && db > 0 && i <= n; ++i) {
            const TempMark mark = temps_mark();
            const E* b = bb[bi];
            const E* c = dd[di];
            long long dg = -1;
            ok = gcd_pair(b, db + 1, c, db, nullptr, 1, nullptr, 1, u, la, &dg, false, s) && dg >= 0 && (size_t)dg <= db;
            bool last = false;
            if (ok && dg > 0) {
                const size_t du = (size_t)dg;
                if (i > 0) ok = emit(i, (const E*)u, du);
                last = i > 0 && du == db;
                if (ok && !last) {
                    ok = du < db && divrem_body(b, db + 1, u, du + 1, bb[bi ^ 1], nullptr, 1, gcd_flag_, s)
                                 && divrem_body(c, db, u, du + 1, dd[di ^ 1], nullptr, 1, gcd_flag_, s);
                    bi ^= 1; di ^= 1; db -= du;
                    c = dd[di];
                }
            }
            if (ok && !last) {
                const E* bn = bb[bi]; E* dn = dd[di ^ 1];
                foreach_n(s, db, [=] __device__(size_t j) {
                    dn[j] = F::canon(F::sub(F::canon(c[j]), F::canon(F::mul(F::from_u32((uint32_t)(j + 1)), bn[j + 1]))));
                });
                di ^= 1;
            }
            temps_release(mark);
            if (last) break;
        }
        return ok && hipGetLastError() == hipSuccess;
    }
    // A part above kFactorSmall (u: deg + 1 coefficients with the leading 1) of row `row` at multiplicity e: ddf_one_large, then per
    // non-empty d edf_one_large on g_d with its leading 1 appended (a g_d of one factor is copied).  The ranked factors go to dst
    // (deg elements, zero on entry) in ascending d, one group each.
    bool factor_large_part(const FactorCall& fc, const E* u, size_t deg, size_t row, long long e, E* dst, std::vector<FacGroup>& groups,
                           hipStream_t s) {
        const E r1 = crate_one();
        const TempMark mark = temps_mark();
        E* fac = temp(deg);
        long long* ddeg = temp_as<long long>(deg);
        std::vector<long long> hdeg(deg, 0);
        bool ok = hipMemsetAsync(fac, 0, deg * sizeof(E), s) == hipSuccess;
        ok = ok && ddf_one_large(fc, u, deg + 1, fac, ddeg, hdeg.data(), s);
        size_t pos = 0;
        for (size_t d = 1; d <= deg && ok; ++d) {
            if (hdeg[d - 1] <= 0) continue;
            const size_t m = (size_t)hdeg[d - 1];
            if (m % d != 0 || pos + m > deg) { ok = false; break; }
            if (m == d) {
                ok = hipMemcpyAsync(dst + pos, fac + pos, m * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
            } else {
                const TempMark dm = temps_mark();
                E* gd = temp(m + 1);
                const E* src = fac + pos;
                foreach_n(s, m + 1, [=] __device__(size_t j) { gd[j] = j < m ? src[j] : r1; });
                long long nq = 0;
                ok = edf_one_large(fc, gd, m + 1, d, dst + pos, &nq, s) && nq == (long long)(m / d);
                temps_release(dm);
            }
            groups.push_back({row, e, (long long)d, m, dst + pos});
            pos += m;
        }
        temps_release(mark);
        return ok;
    }
    // The parts of the decomposition rows that k_yun_small wrote (rows x ld on the device, degrees read back to hdeg), appended to
    // parts; rowid[r] (null: r0 + r) names the call's row.
    static void factor_parts_of(const E* yparts, const long long* hdeg, size_t ld, size_t rows, const size_t* rowid, size_t r0, std::vector<FacPart>& parts) {
        for (size_t r = 0; r < rows; ++r) {
            size_t pos = 0;
            for (size_t i = 1; i <= ld; ++i) {
                const long long dg = hdeg[r * ld + i - 1];
                if (dg <= 0) continue;
                parts.push_back({rowid ? rowid[r] : r0 + r, (long long)i, (size_t)dg, yparts + r * ld + pos});
                pos += (size_t)dg;
            }
        }
    }
    // The shared launches of the small regime over every part of degree <= kFactorSmall of the call, whichever row it came from:
    //   ONE gather lays the parts with their leading 1 into rows of w + 1 (w: the highest degree among them), ONE k_ddf_small takes
    //   them all and its degrees are read back ONCE; a g_d of degree d is a factor as it is; the others are gathered with their
    //   leading 1, ordered by d, and split by ONE k_edf_small per distinct d present on descriptors (input offset, length, output
    //   offset), then ranked (split_rank_launch).  Each (row, e, d) becomes one group.  The launches do not depend on the number of rows.
    bool factor_small_parts(const FactorCall& fc, const std::vector<FacPart>& parts, std::vector<FacGroup>& groups, hipStream_t s) {
        const size_t P = parts.size();
        if (!P) return true;
        size_t w = 1;
        for (const FacPart& p : parts) if (p.deg > w) w = p.deg;
        std::vector<FacSeg> segs(P);
        for (size_t i = 0; i < P; ++i) segs[i] = {parts[i].src, nullptr, parts[i].deg};
        E* G = temp(P * (w + 1)); E* DD = temp(P * w);
        long long* ddeg = temp_as<long long>(P * w);
        std::vector<long long> hd(P * w);
        bool ok = factor_segments(segs, G, w + 1, w, s);
        ddf_small_launch(fc, G, w + 1, w + 1, DD, w, w, ddeg, w, false, P, s);
        ok = hipMemcpyAsync(hd.data(), ddeg, P * w * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && ok;
        if (!ok) return false;
        struct Split { size_t part, d, len; const E* src; };
        std::vector<Split> sp;
        size_t w2 = 0;
        for (size_t i = 0; i < P; ++i) {
            size_t pos = 0;
            for (size_t d = 1; d <= w; ++d) {
                const long long m = hd[i * w + d - 1];
                if (m <= 0) continue;
                if ((size_t)m % d != 0 || pos + (size_t)m > parts[i].deg) return false;
                if ((size_t)m == d) groups.push_back({parts[i].row, parts[i].e, (long long)d, d, DD + i * w + pos});
                else { sp.push_back({i, d, (size_t)m, DD + i * w + pos}); if ((size_t)m > w2) w2 = (size_t)m; }
                pos += (size_t)m;
            }
        }
        const size_t Q = sp.size();
        if (!Q) return true;
        std::stable_sort(sp.begin(), sp.end(), [](const Split& a, const Split& b) { return a.d < b.d; });
        if (Q * (w2 + 1) > 0xFFFFFFFFull) return false;               // the descriptors are 32-bit offsets; the callers bound the rows of a pass
        segs.resize(Q);
        std::vector<uint32_t> desc(3 * Q);
        for (size_t q = 0; q < Q; ++q) {
            segs[q] = {sp[q].src, nullptr, sp[q].len};
            desc[3 * q] = (uint32_t)(q * (w2 + 1)); desc[3 * q + 1] = (uint32_t)(sp[q].len + 1); desc[3 * q + 2] = (uint32_t)(q * w2);
        }
        E* H = temp(Q * (w2 + 1)); E* U = temp(Q * w2); E* V = temp(Q * w2);
        long long* dn = temp_as<long long>(Q);
        uint32_t* ddesc = temp_as<uint32_t>(3 * Q);
        ok = factor_segments(segs, H, w2 + 1, w2, s);
        ok = hipMemcpyAsync(ddesc, desc.data(), 3 * Q * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && ok;
        ok = hipMemsetAsync(U, 0, Q * w2 * sizeof(E), s) == hipSuccess && ok;
        for (size_t q0 = 0; q0 < Q && ok;) {
            size_t q1 = q0, coeffs = 0;
            while (q1 < Q && sp[q1].d == sp[q0].d) coeffs += 2 * sp[q1++].len + 1;
            const size_t d = sp[q0].d;
            const TempMark dm = temps_mark();
            split_small_launch(fc, H, 0, 0, d, U, 0, ddesc + 3 * q0, dn + q0, false, 1u, q1 - q0, (double)coeffs, s);
            split_rank_launch(V + q0 * w2, w2, U + q0 * w2, w2, d, dn + q0, 0, q1 - q0, s);
            temps_release(dm);
            q0 = q1;
        }
        for (size_t q = 0; q < Q; ++q) groups.push_back({parts[sp[q].part].row, parts[sp[q].part].e, (long long)sp[q].d, sp[q].len, V + q * w2});
        return ok && hipGetLastError() == hipSuccess;
    }
    // The end of ecfft_poly_factor: the groups in ascending (row, e, d) are the canonical order, since each is ranked inside; the host
    // arrays are filled from them and ONE scatter writes the factors (count x nd, zero on entry).
    bool factor_finish(std::vector<FacGroup>& groups, size_t nd, E* factors, long long* fdeg, long long* fmult, long long* n_factors, hipStream_t s) {
        std::sort(groups.begin(), groups.end(), [](const FacGroup& a, const FacGroup& b) {
            return a.row != b.row ? a.row < b.row : a.e != b.e ? a.e < b.e : a.d < b.d;
        });
        std::vector<FacSeg> segs;
        size_t w = 0, row = ~(size_t)0, off = 0, j = 0;
        for (const FacGroup& g : groups) {
            if (g.row != row) { row = g.row; off = 0; j = 0; }
            const size_t r = g.len / (size_t)g.d;
            if (off + g.len > nd || j + r > nd) return false;
            segs.push_back({g.src, factors + row * nd + off, g.len});
            for (size_t k = 0; k < r; ++k) { fdeg[row * nd + j + k] = g.d; fmult[row * nd + j + k] = g.e; }
            n_factors[row] += (long long)r;
            off += g.len; j += r;
            if (g.len > w) w = g.len;
        }
        return factor_segments(segs, nullptr, 0, w, s);
    }
public:
    // ecfft_poly_squarefree_decompose: with nd = max(nf - 1, 1), degrees (host, count x nd): degrees[b][i-1] = deg a_i of f_b = lead_b
    // prod a_i^i (zero polynomial: -1, 0, 0, ...); parts (count x nd, crate form): the a_i of positive degree in ascending i, each as
    // its low deg a_i coefficients, then zeros; lead (device, may be null): the leading coefficients, 0 for the zero polynomial.
    // nf <= kFactorSmall + 1: ONE launch of k_yun_small for all rows and one read-back.  Otherwise the rows run one after another: a
    // short polynomial in a long row goes to the same kernel on its true length, the others to yun_one_large.  Synchronous.  Caller
    // holds lock() and checks the tree rule (ddf_leaves).
    bool poly_squarefree_decompose(const E* f, size_t nf, E* parts, long long* degrees, E* lead, size_t count, hipStream_t s) {
        const size_t K = kFactorSmall, nd = nf > 1 ? nf - 1 : 1;
        long long* ddeg = temp_as<long long>(count * nd);
        if (nf <= K + 1) {
            yun_small_launch(f, nf, nf, parts, nd, nd, ddeg, nd, lead, count, s);
            const bool ok = hipMemcpyAsync(degrees, ddeg, count * nd * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess;
            return finish_api(s) && ok;
        }
        gcd_flag_ = new_flag(s);
        bool ok = hipMemsetAsync(parts, 0, count * nd * sizeof(E), s) == hipSuccess;
        for (size_t i = 0; i < count * nd; ++i) degrees[i] = 0;
        for (size_t p = 0; p < count && ok; ++p) {
            const TempMark mark = temps_mark();
            const E* fp = f + p * nf;
            E* op = parts + p * nd;
            long long* hp = degrees + p * nd;
            size_t la = 0;
            ok = gcd_row_lens(fp, nf, nf, 1, &la, s);
            if (ok && la <= K + 1) {
                const size_t nw = la > 1 ? la - 1 : 1;
                yun_small_launch(fp, nf, la ? la : 1, op, nd, nw, ddeg + p * nd, nd, lead ? lead + p : (E*)nullptr, 1, s);
                ok = hipMemcpyAsync(hp, ddeg + p * nd, nw * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
            } else if (ok) {
                if (lead) { E* lp = lead + p; foreach_n(s, 1, [=] __device__(size_t) { lp[0] = F::canon(fp[la - 1]); }); }
                size_t pos = 0;
                ok = yun_one_large(fp, la, [&](size_t i, const E* u, size_t du) {
                    if (pos + du > nd || i > nd) return false;
                    hp[i - 1] = (long long)du;
                    const bool c = hipMemcpyAsync(op + pos, u, du * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
                    pos += du;
                    return c;
                }, s);
            }
            temps_release(mark);
        }
        return finish_api(s) && ok;
    }
    // ecfft_poly_factor: f_b = lead_b prod_j q_j^e_j over the distinct monic irreducible q_j.  With nd = max(nf - 1, 1): n_factors (host)
    // their number (-1: the zero polynomial), fdeg / fmult (host, count x nd) deg q_j and e_j, factors (count x nd, crate form) the
    // q_j laid end to end, each as its low deg q_j coefficients, in ascending (e_j, deg q_j, the order of ecfft_poly_equal_degree),
    // then zeros; lead as above.
    //   nf <= kFactorSmall + 1: k_yun_small over all rows (passes of at most 2^16 rows), one read-back, then factor_small_parts and
    //   factor_finish: the launches and read-backs do not depend on count.
    //   Otherwise the rows run one after another: a row of true length <= kFactorSmall + 1 is set aside for one k_yun_small at the end;
    //   the others run yun_one_large, whose parts of degree <= kFactorSmall are queued (copied into the row's store) and whose longer
    //   parts go to factor_large_part.  The queued parts of ALL rows then share the launches of factor_small_parts.
    // *capped = a factor exhausted the attempt cap.  Synchronous.  Caller holds lock() and checks the tree rule (ddf_leaves).
    bool poly_factor(const E* f, size_t nf, E* factors, long long* fdeg, long long* fmult, long long* n_factors, E* lead, size_t count,
                     bool* capped, hipStream_t s) {
        const size_t K = kFactorSmall, nd = nf > 1 ? nf - 1 : 1;
        FactorCall fc;
        bool ok = factor_call_init(&fc, true, s);
        ok = hipMemsetAsync(factors, 0, count * nd * sizeof(E), s) == hipSuccess && ok;
        for (size_t i = 0; i < count * nd; ++i) fdeg[i] = fmult[i] = 0;
        for (size_t b = 0; b < count; ++b) n_factors[b] = 0;
        std::vector<FacGroup> groups;
        std::vector<FacPart> parts;
        if (nf <= K + 1) {
            const size_t pass = (size_t)1 << 16;
            for (size_t r0 = 0; r0 < count && ok; r0 += pass) {
                const size_t rows = count - r0 < pass ? count - r0 : pass;
                const TempMark mark = temps_mark();
                E* yp = temp(rows * nd);
                long long* ddeg = temp_as<long long>(rows * nd);
                std::vector<long long> hdeg(rows * nd);
                yun_small_launch(f + r0 * nf, nf, nf, yp, nd, nd, ddeg, nd, lead ? lead + r0 : (E*)nullptr, rows, s);
                ok = hipMemcpyAsync(hdeg.data(), ddeg, rows * nd * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
                parts.clear(); groups.clear();
                if (ok) {
                    for (size_t r = 0; r < rows; ++r) if (hdeg[r * nd] < 0) n_factors[r0 + r] = -1;
                    factor_parts_of(yp, hdeg.data(), nd, rows, nullptr, r0, parts);
                }
                ok = ok && factor_small_parts(fc, parts, groups, s) && factor_finish(groups, nd, factors, fdeg, fmult, n_factors, s);
                temps_release(mark);
            }
            return finish_flagged(ok, fc.flag, capped, s);
        }
        gcd_flag_ = new_flag(s);
        E* store = temp(count * nd);                         // per row: the queued parts from the front, the factors of the long parts from the back
        ok = hipMemsetAsync(store, 0, count * nd * sizeof(E), s) == hipSuccess && ok;
        std::vector<size_t> shortrows;
        for (size_t p = 0; p < count && ok; ++p) {
            const TempMark mark = temps_mark();
            const E* fp = f + p * nf;
            size_t la = 0;
            ok = gcd_row_lens(fp, nf, nf, 1, &la, s);
            if (ok && lead) { E* lp = lead + p; foreach_n(s, 1, [=] __device__(size_t) { lp[0] = la ? F::canon(fp[la - 1]) : F::zero(); }); }
            if (ok && la == 0) n_factors[p] = -1;
            else if (ok && la <= K + 1) shortrows.push_back(p);
            else if (ok) {
                E* sp = store + p * nd;
                size_t front = 0, back = nd;
                ok = yun_one_large(fp, la, [&](size_t i, const E* u, size_t du) {
                    if (front + du > back) return false;
                    if (du <= K) {
                        parts.push_back({p, (long long)i, du, sp + front});
                        front += du;
                        return hipMemcpyAsync(sp + front - du, u, du * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
                    }
                    back -= du;
                    return factor_large_part(fc, u, du, p, (long long)i, sp + back, groups, s);
                }, s);
            }
            temps_release(mark);
        }
        if (ok && !shortrows.empty()) {
            const size_t ns = shortrows.size();
            E* sr = temp(ns * (K + 1)); E* yp = temp(ns * K);
            long long* ddeg = temp_as<long long>(ns * K);
            std::vector<long long> hdeg(ns * K);
            std::vector<FacSeg> segs(ns);
            for (size_t r = 0; r < ns; ++r) segs[r] = {f + shortrows[r] * nf, sr + r * (K + 1), K + 1};
            ok = factor_segments(segs, nullptr, 0, K + 1, s);
            yun_small_launch(sr, K + 1, K + 1, yp, K, K, ddeg, K, nullptr, ns, s);
            ok = hipMemcpyAsync(hdeg.data(), ddeg, ns * K * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && ok;
            if (ok) factor_parts_of(yp, hdeg.data(), K, ns, shortrows.data(), 0, parts);
        }
        ok = ok && factor_small_parts(fc, parts, groups, s) && factor_finish(groups, nd, factors, fdeg, fmult, n_factors, s);
        return finish_flagged(ok, fc.flag, capped, s);
    }

    // ---- ecfft_division_polynomial (division_polynomial, examples/schoofs.rs:368-431) ----
    static constexpr size_t kDivpolyMaxN = 199;
    // L(n): the coefficients of psi_n with the factor 2y of an even index removed
    static size_t divpoly_len(size_t n) { return n < 2 ? 1 : ((n & 1) ? (n * n - 1) / 2 + 1 : (n * n - 4) / 2 + 1); }
    // The leaves the call needs: psi_0 .. psi_4 are closed forms (1: no transform); above, every product of the recurrence is a
    // factor of one term of some psi_k, k <= n, so none has more than L(n) coefficients, and the last ones have exactly L(n)
    static size_t divpoly_leaves(size_t n) { return n <= 4 ? 1 : next_pow2(divpoly_len(n)); }
    // out (count x L(n), crate form, not monic) = psi_n of the curves (A[b], B[b]): a host driver on poly_mul_body, batched over
    // count, memoised over the O(log n) indices the recurrence reaches (m - 2 .. m + 2 of m = k / 2, downwards), each computed
    // once in ascending order.  A factor psi_1 = psi_2 = 1 costs no product.  Temporaries: after every index the products it
    // took go back to the pool, and so does every psi_j that no index still to come reads, so at most the five psi of two
    // neighbouring levels and one index's products are held at a time.  Asynchronous on s.  Caller holds lock() and checks n
    // and the tree rule (divpoly_leaves).
    bool division_polynomial(const E* A, const E* B, size_t n, E* out, size_t count, hipStream_t s) {
        const bool ok = division_polynomial_body(A, B, n, out, count, s);
        temps_done();
        return ok && hipGetLastError() == hipSuccess;
    }
    // the same without handing every temporary back: what it took itself is released, what the caller holds stays
    bool division_polynomial_body(const E* A, const E* B, size_t n, E* out, size_t count, hipStream_t s) {
        struct Poly { const E* p; size_t len; bool one; };
        auto deps = [](size_t k) {
            const size_t m = k / 2;
            std::vector<size_t> d{m - 1, m, m + 1, m + 2};
            if (k % 2 == 0) d.push_back(m - 2);
            return d;
        };
        std::set<size_t> seen;
        {
            std::vector<size_t> todo{n};
            while (!todo.empty()) {
                const size_t k = todo.back();
                todo.pop_back();
                if (!seen.insert(k).second || k <= 4) continue;
                for (size_t j : deps(k)) todo.push_back(j);
            }
        }
        std::vector<E*> memo(n + 4, nullptr);
        bool ok = true;
        const TempMark entry = temps_mark();
        // the closed forms, and 16 f^2 = 16 (x^3 + A x + B)^2, one thread per curve
        E* base = temp(count * 22);
        E *q0 = base, *q1 = base + count, *q3 = base + 2 * count, *q4 = base + 7 * count, *F2 = base + 14 * count;
        {
            const E r1 = crate_one(), rinv = rinv_;
            foreach_n(s, count, [=] __device__(size_t b) {
                auto cm = [&](const E& x, const E& y) { return F::canon(F::mul(F::canon(F::mul(x, y)), rinv)); };
                auto sc = [&](uint32_t k, const E& v) { return F::canon(F::mul(F::from_u32(k), v)); };
                const E a = F::canon(A[b]), bb = F::canon(B[b]);
                const E aa = cm(a, a), ab = cm(a, bb), b2 = cm(bb, bb), a3 = cm(aa, a);
                q0[b] = F::zero();
                q1[b] = r1;
                E* p3 = q3 + 5 * b;
                p3[0] = F::canon(F::neg(aa)); p3[1] = sc(12, bb); p3[2] = sc(6, a); p3[3] = F::zero(); p3[4] = sc(3, r1);
                E* p4 = q4 + 7 * b;
                p4[0] = F::canon(F::neg(F::canon(F::add(sc(2, a3), sc(16, b2)))));
                p4[1] = F::canon(F::neg(sc(8, ab))); p4[2] = F::canon(F::neg(sc(10, aa))); p4[3] = sc(40, bb); p4[4] = sc(10, a);
                p4[5] = F::zero(); p4[6] = sc(2, r1);
                E* f2 = F2 + 7 * b;
                f2[0] = sc(16, b2); f2[1] = sc(32, ab); f2[2] = sc(16, aa); f2[3] = sc(32, bb); f2[4] = sc(32, a); f2[5] = F::zero();
                f2[6] = sc(16, r1);
            });
        }
        memo[0] = q0; memo[1] = q1; memo[2] = q1; memo[3] = q3; memo[4] = q4;
        auto P = [&](size_t j) { return Poly{memo[j], divpoly_len(j), j == 1 || j == 2}; };
        auto prod = [&](const Poly& x, const Poly& y) {
            if (x.one) return y;
            if (y.one) return x;
            const size_t len = x.len + y.len - 1;
            E* o = temp(count * len);
            ok = poly_mul_body(x.p, x.len, x.len, y.p, y.len, y.len, o, count, s) && ok;
            return Poly{o, len, false};
        };
        auto diff = [&](const Poly& x, const Poly& y) {
            const size_t len = x.len > y.len ? x.len : y.len, lx = x.len, ly = y.len;
            E* o = temp(count * len);
            const E *xp = x.p, *yp = y.p;
            foreach_n(s, count * len, [=] __device__(size_t i) {
                const size_t b = i / len, j = i - b * len;
                E u = F::zero(), v = F::zero();
                if (j < lx) u = F::canon(xp[b * lx + j]);
                if (j < ly) v = F::canon(yp[b * ly + j]);
                o[i] = F::canon(F::sub(u, v));
            });
            return Poly{o, len, false};
        };
        const Poly f2{F2, 7, false};
        for (size_t k : seen) {
            if (k <= 4 || !ok) continue;
            const size_t m = k / 2;
            Poly r;
            if (k % 2 == 0) {
                const Poly t0 = prod(prod(P(m - 1), P(m - 1)), P(m + 2)), t1 = prod(prod(P(m + 1), P(m + 1)), P(m - 2));
                r = prod(diff(t0, t1), P(m));
            } else {
                Poly t0 = prod(P(m + 2), prod(prod(P(m), P(m)), P(m))), t1 = prod(P(m - 1), prod(prod(P(m + 1), P(m + 1)), P(m + 1)));
                if (m % 2 == 0) t0 = prod(f2, t0); else t1 = prod(f2, t1);
                r = diff(t0, t1);
            }
            memo[k] = const_cast<E*>(r.p);
            ok = ok && r.len == divpoly_len(k);
            // keep what was busy on entry, the closed forms, and every psi_j that k itself (the result) or a later index reads
            TempMark keep = entry;
            keep.push_back(base);
            keep.push_back(memo[k]);
            for (size_t k2 : seen)
                if (k2 > k && k2 > 4)
                    for (size_t j : deps(k2)) if (memo[j]) keep.push_back(memo[j]);
            temps_release(keep);
        }
        ok = ok && hipMemcpyAsync(out, memo[n], count * divpoly_len(n) * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
        temps_release(entry);
        return ok;
    }

    // ---- ecfft_curve_trace_mod (frobenius_trace_mod_l, examples/schoofs.rs:76-138) ----
    // a modulus of at most kSchoofSmall + 1 coefficients is finished by k_schoof_small, one workgroup per curve
    static constexpr size_t kSchoofSmall = kRootsSmall;
    static constexpr uint32_t kSchoofMaxL = 199;
    // 2 and the odd primes up to kSchoofMaxL
    static bool schoof_valid_l(uint32_t l) {
        if (l == 2) return true;
        if (l < 3 || l > kSchoofMaxL || l % 2 == 0) return false;
        for (uint32_t q = 3; q * q <= l; q += 2) if (l % q == 0) return false;
        return true;
    }
    // The leaves the call needs, checked before anything runs: none where psi_l fits the small regime (l <= 11); otherwise gcd's
    // rule on rows of L(l) coefficients, next_pow2(2 L(l) - 1), which covers the kept-modulus products (2 d - 1 coefficients,
    // d = L(l) - 1), the composition and the driver of psi_l (L(l) coefficients)
    static size_t schoof_leaves(uint32_t l) {
        const size_t L = divpoly_len(l);
        return l == 2 || L <= kSchoofSmall + 1 ? 1 : next_pow2(2 * L - 1);
    }
    // the modular products of one general-base power with p: bits + popcount(p) - 2
    static uint32_t schoof_pow_cost() {
        const FactorCall fc = factor_exponents();
        uint32_t pop = 0;
        for (int i = 0; i < 32; ++i) pop += (uint32_t)__builtin_popcount(fc.e[i]);
        return fc.nbits_p + pop - 2;
    }
    // How pi^2 = (x^(p^2), y^(p^2)) is taken from pi = (a, b y) on a modulus of degree d: true = the composition (a(a), b(a) b),
    // false = the powers (a^p, b^p b), 2 c products with c = schoof_pow_cost().  The rule is the count of modular products, as
    // ddf_iterate_composes has it: Horner's loop in the small regime takes 2 (d - 1) (k_schoof_small applies the same rule to
    // the degree it meets); the kept composition of the large regime shares its k - 1 baby steps between a and b and takes
    // k' - 1 products per coordinate.
    static bool schoof_pi2_composes(size_t d) {
#ifdef ECFFT_TEST_HOOKS
        if (schoof_pi2_force() == 1) return false;
        if (schoof_pi2_force() == 2) return true;
#endif
        const size_t c = schoof_pow_cost();
        if (d <= kSchoofSmall) return d - 1 < c;
        const size_t k = compose_chunk(d), kp = (d + k - 1) / k;
        return (k - 1) + 2 * (kp - 1) < 2 * c;
    }
#ifdef ECFFT_TEST_HOOKS
    // ecfft_test_schoof_pi2 (include/ecfft_hip_hooks.h): 0 = the rule, 1 = always the powers, 2 = always the composition
    static int& schoof_pi2_force() { static int v = 0; return v; }
#endif
    // p as 32 little-endian bytes
    static void modulus_bytes(uint8_t* ep) { const FactorCall fc = factor_exponents(); for (int i = 0; i < 32; ++i) ep[i] = fc.e[i]; }
    // p mod l for a small l
    static uint32_t schoof_p_mod(uint32_t l) {
        const FactorCall fc = factor_exponents();
        uint64_t r = 0;
        for (int i = 31; i >= 0; --i) r = (r * 256 + fc.e[i]) % l;
        return (uint32_t)r;
    }
private:
    // what a call shares between its curves: the exponents p and (p - 1) / 2 as host and device bytes, p mod l, the flag
    struct SchoofCall { const uint8_t* dexp = nullptr; uint8_t e[64]; uint32_t nbits_p = 0, nbits_h = 0, kq = 0, cost = 0, pi2 = 0; int* flag = nullptr; };
    // one launch of k_schoof_small: psi_l built in the kernel (mod == nullptr) or the given monic moduli of nmod coefficients
    void schoof_small_launch(const SchoofCall& sc, const E* A, const E* B, const E* mod, size_t nmod, uint32_t l, long long* dn, size_t count,
                             hipStream_t s) {
        const E r1 = crate_one();
        const TE rinv = rinv_table();
        for_chunks(count, [&](size_t b0, size_t nb) {
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (2.0 + (double)nmod) * (double)nb + 64.0, (k_schoof_small<F, (int)kSchoofSmall>),
                         dim3((unsigned)nb), dim3((unsigned)kSchoofSmall), 0, s, A + b0, B + b0, mod ? mod + b0 * nmod : (const E*)nullptr,
                         (uint32_t)nmod, l, sc.kq, dn + b0, sc.pi2, sc.cost, sc.dexp, sc.nbits_p, sc.dexp + 32, sc.nbits_h, rinv, r1, sc.flag);
        });
    }
    // t mod l of ONE curve whose psi_l has more than kSchoofSmall + 1 coefficients.  psi_l comes from division_polynomial_body and
    // is made monic; then attempts on a modulus h of degree d, the steps of k_schoof_small on device rows of d coefficients:
    //   d <= kSchoofSmall (after a split): the modulus is handed to k_schoof_small, which finishes the curve;
    //   otherwise h is kept ONCE for the attempt (keep_modulus); a product is a lift of its right operand and one powmod_step
    //   (the product of compose_apply); pi_a = x^p by roots_pow_kept's scan, pi_b and the powers of pi^2 by the powmod_step scan
    //   of poly_pow_mod; the composition shares ONE compose_prepare (the baby steps of pi_a) between pi_a(pi_a) and pi_b(pi_a);
    //   an inverse is the s cofactor of the gcd of (denominator, h) — k_gcd_small up to kGcdSmall coefficients, gcd_pair above —
    //   whose degree is read back; a proper gcd becomes the modulus, which is kept again by the next attempt.
    // Row equality is decided on the device and read back.  Temporaries: the rows and the kept modulus of the attempt; a product's
    // or a sum's own go back to the pool when it ends, so nothing grows with l.  *t = the residue.  Returns false on a HIP error;
    // a sum the group law excludes raises *sc.flag.
    bool schoof_one_large(const SchoofCall& sc, const E* A, const E* B, uint32_t l, long long* t, hipStream_t s) {
        const size_t d0 = divpoly_len(l) - 1, ld = d0 + 1;
        const E r1 = crate_one(), rinvE = rinv_;
        const TE rinv = rinv_table();
        bool ok = true;
        int* dint = temp_as<int>(2);
        auto read_int = [&]() { int h = 0; ok = hipMemcpyAsync(&h, dint, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && ok; return h; };
        foreach_n(s, 1, [=] __device__(size_t) {
            auto cm = [&](const E& x, const E& y) { return F::canon(F::mul(F::canon(F::mul(x, y)), rinvE)); };
            const E a = F::canon(A[0]), b = F::canon(B[0]);
            const E disc = F::canon(F::add(F::canon(F::mul(F::from_u32(4), cm(cm(a, a), a))), F::canon(F::mul(F::from_u32(27), cm(b, b)))));
            dint[0] = F::is_zero(disc) ? 1 : 0;
        });
        if (read_int()) { *t = -1; return ok; }
        E* h = temp(ld);
        {
            E* psi = temp(ld);
            ok = division_polynomial_body(A, B, l, psi, 1, s) && ok;
            E* cinv = temp(1);                                    // 1 / lc(psi_l) as a plain number: the one inversion of the curve
            foreach_n(s, 1, [=] __device__(size_t) { cinv[0] = F::canon(F::mul(F::inv(F::canon(psi[d0])), r1)); });
            foreach_n(s, d0, [=] __device__(size_t j) { h[j] = F::canon(F::mul(psi[j], cinv[0])); });
            foreach_n(s, 1, [=] __device__(size_t) { h[d0] = r1; });
        }
        enum { X, ONE, FX, PA, PB, EA, EB, QA, QB, NUM, DEN, RR, A3, B3, INV, TMP, NROWS };
        E* W = temp((size_t)NROWS * ld);
        E* G = temp(ld);
        long long* dn = temp_as<long long>(1);
        auto row = [&](int i) { return W + (size_t)i * ld; };
        size_t d = d0;
        *t = 0;
        for (;;) {
            if (d <= kSchoofSmall) {
                schoof_small_launch(sc, A, B, h, d + 1, l, dn, 1, s);
                ok = hipMemcpyAsync(t, dn, sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && ok;
                return ok;
            }
            const TempMark am = temps_mark();
            const size_t N = powmod_leaves(d + 1);
            E* kept = temp(2 * N);
            KeptModulus km;
            ok = keep_modulus(h, d, nullptr, 0, 0, 1, kept, sc.flag, &km, s) && ok;
            const size_t dd = d;
            auto copy = [&](E* dst, const E* src) { if (dst != src) ok = hipMemcpyAsync(dst, src, dd * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess && ok; };
            // out = a b mod h; out may be a or b
            auto mulmod = [&](E* out, const E* a, const E* b) {
                const TempMark m = temps_mark();
                if (a == b) { copy(out, a); ok = powmod_step(out, nullptr, km, 1, rinv, s) && ok; }
                else {
                    E* K = temp(N);
                    ok = lift_and_keep(b, dd, N, 1, K, s) && ok;
                    copy(out, a);
                    ok = powmod_step(out, K, km, 1, rinv, s) && ok;
                }
                temps_release(m);
            };
            // out = base^e mod h for nbits >= 1 bits of e (host bytes, top bit set); out is not base
            auto powgen = [&](E* out, const E* base, const uint8_t* e, uint32_t nbits) {
                const TempMark m = temps_mark();
                E* K = temp(N);
                ok = lift_and_keep(base, dd, N, 1, K, s) && ok;
                copy(out, base);
                for (uint32_t i = nbits - 1; i-- > 0;) {
                    ok = powmod_step(out, nullptr, km, 1, rinv, s) && ok;
                    if ((e[i >> 3] >> (i & 7)) & 1) ok = powmod_step(out, K, km, 1, rinv, s) && ok;
                }
                temps_release(m);
            };
            // out = a + sign b on the d coefficients
            auto lin = [&](E* out, const E* a, const E* b, bool minus) {
                foreach_n(s, dd, [=] __device__(size_t j) { out[j] = F::canon(minus ? F::sub(F::canon(a[j]), F::canon(b[j])) : F::add(F::canon(a[j]), F::canon(b[j]))); });
            };
            // a == b (plus == false) or a == -b, decided on the device
            auto same = [&](const E* a, const E* b, bool plus) {
                ok = hipMemsetAsync(dint, 0, sizeof(int), s) == hipSuccess && ok;
                foreach_n(s, dd, [=] __device__(size_t j) {
                    const E v = F::canon(plus ? F::add(F::canon(a[j]), F::canon(b[j])) : F::sub(F::canon(a[j]), F::canon(b[j])));
                    if (!F::is_zero(v)) dint[0] = 1;
                });
                return read_int() == 0;
            };
            // the gcd of (den, h): its degree; INV = the cofactor of den, G = the monic gcd
            auto gcd_h = [&](const E* den) {
                long long deg = -1;
                const size_t na = dd, nb = dd + 1, nt = na > 1 ? na - 1 : 1;
                const TempMark m = temps_mark();
                if (nb <= kGcdSmall) {
                    long long* ddeg = temp_as<long long>(1);
                    ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 4.0 * (double)nb, (k_gcd_small<F, (int)kGcdSmall>), dim3(1u), dim3((unsigned)kGcdSmall), 0, s,
                                 den, na, (uint32_t)na, (const E*)h, nb, (uint32_t)nb, (int32_t)0, 0u, 1u, G, (uint32_t)nb, row(INV), (uint32_t)na,
                                 (E*)nullptr, (uint32_t)nt, ddeg, (E*)nullptr, (size_t)0, 0u, (int32_t*)nullptr, r1);
                    ok = hipMemcpyAsync(&deg, ddeg, sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && ok;
                } else {
                    ok = gcd_pair(den, na, h, nb, row(INV), na, nullptr, nt, G, nb, &deg, true, s) && ok;
                }
                temps_release(m);
                return deg;
            };
            auto split_to = [&](long long dg) {
                ok = hipMemcpyAsync(h, G, ((size_t)dg + 1) * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess && ok;
                d = (size_t)dg;
            };
            // SchoofWg::add on device rows: (A3, B3) = (a1, b1) + (a2, b2); 0 done, 1 infinity, 2 the modulus was split, 3 a defect
            auto add = [&](const E* a1, const E* b1, const E* a2, const E* b2) {
                if (same(a1, a2, false)) {
                    if (same(b1, b2, true)) return 1;
                    if (same(b1, b2, false)) {
                        mulmod(row(NUM), a1, a1);
                        { E* num = row(NUM); const E* pA = A; foreach_n(s, dd, [=] __device__(size_t j) {
                              E v = F::canon(F::mul(F::from_u32(3), num[j]));
                              if (j == 0) v = F::canon(F::add(v, F::canon(pA[0])));
                              num[j] = v; }); }
                        mulmod(row(DEN), row(FX), b1);
                        lin(row(DEN), row(DEN), row(DEN), false);
                    } else {
                        for (int sgn = 0; sgn < 2; ++sgn) {
                            lin(row(DEN), b1, b2, sgn == 0);
                            const long long dg = gcd_h(row(DEN));
                            if (dg > 0 && dg < (long long)dd) { split_to(dg); return 2; }
                        }
                        return 3;
                    }
                } else {
                    lin(row(NUM), b1, b2, true);
                    lin(row(DEN), a1, a2, true);
                }
                const long long dg = gcd_h(row(DEN));
                if (!ok || dg < 0 || dg >= (long long)dd) return 3;
                if (dg > 0) { split_to(dg); return 2; }
                mulmod(row(RR), row(NUM), row(INV));
                mulmod(row(A3), row(RR), row(RR));
                mulmod(row(A3), row(A3), row(FX));
                lin(row(A3), row(A3), a1, true);
                lin(row(A3), row(A3), a2, true);
                lin(row(B3), a1, row(A3), true);
                mulmod(row(B3), row(RR), row(B3));
                lin(row(B3), row(B3), b1, true);
                return 0;
            };
            // x, 1, f
            {
                E *x = row(X), *one = row(ONE), *fx = row(FX);
                const E *pA = A, *pB = B;
                foreach_n(s, dd, [=] __device__(size_t j) {
                    x[j] = j == 1 ? r1 : F::zero();
                    one[j] = j == 0 ? r1 : F::zero();
                    fx[j] = j == 0 ? F::canon(pB[0]) : j == 1 ? F::canon(pA[0]) : j == 3 ? r1 : F::zero();
                });
            }
            ok = roots_pow_kept(h, km, 0u, sc.e, sc.nbits_p, row(PA), row(TMP), 1, s) && ok;
            powgen(row(PB), row(FX), sc.e + 32, sc.nbits_h);
            if (schoof_pi2_composes(d)) {
                E* K = temp(N);
                ok = lift_and_keep(row(PA), d, N, 1, K, s) && ok;
                const KeptModulus kb{km.g, km.f, K, d, N};
                const size_t k = compose_chunk(d), kp = (d + k - 1) / k;
                KeptCompose kc;
                kc.B = temp((k + 1) * d); kc.C = temp(kp * d);
                ok = compose_prepare(kb, row(PA), d, d, d, 1, &kc, s) && ok;
                ok = compose_apply(kc, row(PA), row(EA), s) && ok;
                ok = compose_apply(kc, row(PB), row(TMP), s) && ok;
            } else {
                powgen(row(EA), row(PA), sc.e, sc.nbits_p);
                powgen(row(TMP), row(PB), sc.e, sc.nbits_p);
            }
            mulmod(row(EB), row(TMP), row(PB));
            int st = 0;
            long long res = 0;
            copy(row(QA), row(X)); copy(row(QB), row(ONE));
            for (uint32_t i = 1; i < sc.kq && st == 0 && ok; ++i) {
                st = add(row(QA), row(QB), row(X), row(ONE));
                if (st == 0) { copy(row(QA), row(A3)); copy(row(QB), row(B3)); }
            }
            if (st == 1) st = 3;                                  // [i](x, y) is never the point at infinity below l
            if (st == 0 && ok) {
                st = add(row(EA), row(EB), row(QA), row(QB));
                if (st == 1) st = 4;                              // pi^2 + [p] = O: the residue is 0
            }
            if (st == 0 && ok) {
                copy(row(EA), row(A3)); copy(row(EB), row(B3));
                copy(row(QA), row(PA)); copy(row(QB), row(PB));
                for (uint32_t j = 1; j < l && ok; ++j) {
                    if (same(row(QA), row(EA), false) && same(row(QB), row(EB), false)) { res = (long long)j; break; }
                    if (j + 1 == l) break;
                    st = add(row(QA), row(QB), row(PA), row(PB));
                    if (st != 0) break;
                    copy(row(QA), row(A3)); copy(row(QB), row(B3));
                }
                if (st == 1) st = 4;
            }
            temps_release(am);
            if (!ok) return false;
            if (st == 2) continue;
            if (st == 3) { const int one = 1; ok = hipMemcpyAsync(sc.flag, &one, sizeof(int), hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess; }
            *t = res;
            return ok;
        }
    }
public:
    // ecfft_curve_trace_mod: t_out[b] (host) = t mod l for the curve (A[b], B[b]) with #E = p + 1 - t, -1 for a singular curve.
    // psi_l of at most kSchoofSmall + 1 coefficients (l <= 11) and l = 2: ONE launch of k_schoof_small for all curves, no
    // transform.  Otherwise the curves run one after another (schoof_one_large).  *defect = a sum the group law excludes.
    // Synchronous.  Caller holds lock() and checks l (schoof_valid_l) and the tree rule (schoof_leaves).  done == false leaves
    // the temporaries to a caller that goes on (curve_cardinality).
    bool curve_trace_mod(const E* A, const E* B, uint32_t l, long long* t_out, size_t count, bool* defect, hipStream_t s, bool done = true) {
        const TempMark entry = temps_mark();
        SchoofCall sc;
        const FactorCall fc = factor_exponents();
        for (int i = 0; i < 64; ++i) sc.e[i] = fc.e[i];
        sc.nbits_p = fc.nbits_p; sc.nbits_h = fc.nbits_h;
        uint8_t* dexp = temp_as<uint8_t>(64);
        bool ok = hipMemcpyAsync(dexp, sc.e, 64, hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        sc.dexp = dexp;
        sc.flag = new_flag(s);
        sc.kq = schoof_p_mod(l); sc.cost = schoof_pow_cost();
#ifdef ECFFT_TEST_HOOKS
        sc.pi2 = (uint32_t)schoof_pi2_force();
#endif
        if (schoof_leaves(l) == 1) {
            long long* dn = temp_as<long long>(count);
            schoof_small_launch(sc, A, B, nullptr, 0, l, dn, count, s);
            ok = hipMemcpyAsync(t_out, dn, count * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess && ok;
        } else {
            gcd_flag_ = new_flag(s);
            for (size_t p = 0; p < count && ok; ++p) {
                const TempMark mark = temps_mark();
                ok = schoof_one_large(sc, A + p, B + p, l, &t_out[p], s);
                temps_release(mark);
            }
        }
        int hflag = 0;
        ok = ok && hipMemcpyAsync(&hflag, sc.flag, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess && ok;
        *defect = hflag != 0;
        if (done) temps_done(); else temps_release(entry);
        return ok;
    }

    // coefficients of the reciprocal computed by k_series_base before the Newton steps take over (K0).  64 = one wave per pair: a
    // Newton step at p <= 64 costs a lift + EXIT in the latency regime, the recurrence's 63 tree sums a few us.
    static constexpr size_t kSeriesBase = 64;
    // poly_mul without releasing the temporaries (the division holds its own across several products); operand rows of len
    // coefficients at a row stride of ld (>= len) elements
    bool poly_mul_body(const E* a, size_t na, size_t lda, const E* b, size_t nb, size_t ldb, E* out, size_t count, hipStream_t s) {
        const size_t nc = na + nb - 1;
        const size_t N = mul_leaves(na, nb);
        const int nops = (a == b && na == nb && lda == ldb) ? 1 : 2;
        const E* src[2] = {a, b};
        const size_t len[2] = {na, nb}, ld[2] = {lda, ldb};
        PolyEvals<F> ev[2];
        E* Y = nullptr;
        bool ok = lift_operands(src, len, ld, nops, N, count, ev, Y, s);
        const size_t total = count * N;
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (nops + 1.0) * (double)total, k_poly_pointwise<F>, dim3(nblocks(total)), dim3(kBlock), 0, s,
                     Y, ev[0], ev[1], rinv_table(), ilog2(N), total);
        return exit_rows(Y, out, nc, N, count, ok, s);
    }
    // EXIT_N of count rows of Y, keeping the first nc coefficients of each (the others are zero) in out (count x nc)
    bool exit_rows(E* Y, E* out, size_t nc, size_t N, size_t count, bool ok, hipStream_t s) {
        if (nc == N) ok = exit(Y, out, N, count, s) && ok;
        else {
            ok = exit(Y, Y, N, count, s) && ok;                  // coefficients nc .. N-1 are zero: keep the first nc of each row
            ok = ok && hipMemcpy2DAsync(out, nc * sizeof(E), Y, N * sizeof(E), nc * sizeof(E), count, hipMemcpyDeviceToDevice, s) == hipSuccess;
        }
        return ok;
    }
    // k_series_base on count rows (grid chunks of at most 2^16 pairs)
    void series_base(const E* f, size_t ldf, size_t nf, E* out, size_t ldo, size_t p0, size_t count, int* flag, hipStream_t s) {
        const E r1 = crate_one();
        for_chunks(count, [&](size_t c0, size_t c) {
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 2.0 * (double)(c * p0), (k_series_base<F, (int)kSeriesBase>), dim3((unsigned)c),
                         dim3((unsigned)kSeriesBase), 0, s, out + c0 * ldo, ldo, f + c0 * ldf, ldf, nf, (uint32_t)p0, rinv_, r1, flag);
        });
    }
    // 1/f mod x^k (f: count rows of nf coefficients at a stride of ldf) into out (count x k); raises *flag on a zero f[0]
    bool inv_series_body(const E* f, size_t nf, size_t ldf, E* out, size_t k, size_t count, int* flag, hipStream_t s) {
        unsigned t = 0;
        while (((k + ((size_t)1 << t) - 1) >> t) > kSeriesBase) ++t;
        size_t p = (k + ((size_t)1 << t) - 1) >> t;
        E* buf[2] = {t ? temp(count * k) : nullptr, t > 1 ? temp(count * k) : nullptr};
        const E* g = t ? buf[0] : out;
        series_base(f, ldf, nf, t ? buf[0] : out, t ? p : k, p, count, flag, s);
        bool ok = true;
        for (int side = 1; t > 0; --t, side ^= 1) {
            const size_t p2 = (k + ((size_t)1 << (t - 1)) - 1) >> (t - 1);
            E* dst = t == 1 ? out : buf[side];
            ok = newton_step(f, nf, ldf, g, p, dst, p2, count, s) && ok;
            g = dst; p = p2;
        }
        return ok;
    }
    // g (count x p, p coefficients of 1/f) -> out (count x p2) = g (2 - f g) mod x^p2: f mod x^p2 and g entered at their own size
    // and lifted to N = next_pow2(2p + p2 - 2) on the joint launches of poly_mul, k_newton_pointwise, one batched EXIT_N.
    // deg(g^2 f) < N, so nothing wraps.
    bool newton_step(const E* f, size_t nf, size_t ldf, const E* g, size_t p, E* out, size_t p2, size_t count, hipStream_t s) {
        const size_t N = next_pow2(2 * p + p2 - 2);
        const E* src[2] = {f, g};
        const size_t len[2] = {nf < p2 ? nf : p2, p}, ld[2] = {ldf, p};
        PolyEvals<F> ev[2];
        E* Y = nullptr;
        bool ok = lift_operands(src, len, ld, 2, N, count, ev, Y, s);
        const E R = crate_one(), r2 = F::mul(R, R);
        const size_t total = count * N;
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 3.0 * (double)total, k_newton_pointwise<F>, dim3(nblocks(total)), dim3(kBlock), 0, s,
                     Y, ev[0], ev[1], F::add(r2, r2), F::to_table(F::mul(rinv_, rinv_)), ilog2(N), total);
        return exit_rows(Y, out, p2, N, count, ok, s);
    }
    int* new_flag(hipStream_t s) {
        int* flag = temp_as<int>(1);
        (void)hipMemsetAsync(flag, 0, sizeof(int), s);
        return flag;
    }
    bool finish_flagged(bool ok, const int* flag, bool* singular, hipStream_t s) {
        int h = 0;
        ok = ok && hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = finish_api(s) && ok;
        *singular = h != 0;
        return ok;
    }
    // The lifting half of poly_mul: the nops operands (src[i]: count rows of len[i] coefficients at a row stride of ld[i]) entered
    // at their own size and lifted to N, sharing the launches from the size at which they meet; ev[i] reads operand i's evaluations
    // on the leaves of T_N (the last lift's interleave), Y is a free count x N buffer.  Takes temporaries.
    bool lift_operands(const E* const* src, const size_t* len, const size_t* ld, int nops, size_t N, size_t count, PolyEvals<F>* ev, E*& Y,
                       hipStream_t s) {
        const size_t h = N / 2;
        const size_t m[2] = {next_pow2(len[0]), next_pow2(len[1])};
        // count rows of n coefficients (row stride ldp) -> count rows of mm, zero-padded
        auto pad = [&](E* dst, const E* p, size_t n, size_t ldp, size_t mm) {
            const size_t mask = mm - 1; const unsigned lm = ilog2(mm);
            foreach_n(s, count * mm, [=] __device__(size_t i) { const size_t j = i & mask; dst[i] = j < n ? p[(i >> lm) * ldp + j] : F::zero(); });
        };
        bool ok = true;
        int slot[2] = {-1, -1}, nl = 0;                           // lifted operands: slot q of the joint buffer
        for (int i = 0; i < nops; ++i) {
            if (m[i] < N) { slot[i] = nl++; continue; }
            E* P = temp(count * N);                               // longer than N/2: ENTER_N of the zero-padded vector
            if (len[i] == N && ld[i] == N) ok = enter(src[i], P, N, count, s) && ok;
            else { pad(P, src[i], len[i], ld[i], N); ok = enter(P, P, N, count, s) && ok; }
            ev[i] = PolyEvals<F>{P, P + 1, N, 2u};
        }
        E *U = nullptr, *V = nullptr;
        const E* cur = nullptr;
        if (nl) {
            // joint layout at size mm: slot q holds its operand's count vectors at [q*count*mm, (q+1)*count*mm)
            U = temp(count * N); V = temp(count * N);
            E* X = temp(nl * count * h);
            size_t hi = 0;
            for (int i = 0; i < nops; ++i) if (slot[i] >= 0 && m[i] > hi) hi = m[i];
            int nbig = 0, q0 = -1;
            for (int i = 0; i < nops; ++i)
                if (slot[i] >= 0 && m[i] == hi) { pad(U + slot[i] * count * hi, src[i], len[i], ld[i], hi); ++nbig; if (q0 < 0) q0 = slot[i]; }
            ok = enter(U + q0 * count * hi, U + q0 * count * hi, hi, nbig * count, s) && ok;   // the slots at `hi` are adjacent
            for (int i = 0; i < nops; ++i) {
                if (slot[i] < 0 || m[i] == hi) continue;
                // the shorter operand alone up to `hi`: ping-pong in V (each half holds count*h >= count*hi/2), last lift into its slot
                E* c = V;
                pad(V, src[i], len[i], ld[i], m[i]);
                ok = enter(V, V, m[i], count, s) && ok;
                for (size_t mm = m[i]; mm < hi; mm *= 2) {
                    E* dst = 2 * mm == hi ? U + slot[i] * count * hi : (c == V ? V + count * h : V);
                    ok = lift_step(c, dst, X, mm, count, s) && ok;
                    c = dst;
                }
            }
            E* c = U;
            for (size_t mm = hi; mm < h; mm *= 2) { E* dst = c == U ? V : U; ok = lift_step(c, dst, X, mm, nl * count, s) && ok; c = dst; }
            ok = extend_api(c, X, h, nl * count, 1, s) && ok;      // the last lift's EXTEND; its interleave is k_poly_pointwise's load
            cur = c;
            for (int i = 0; i < nops; ++i)
                if (slot[i] >= 0) ev[i] = PolyEvals<F>{cur + slot[i] * count * h, X + slot[i] * count * h, h, 1u};
        }
        if (nops == 1) ev[1] = ev[0];
        Y = nl ? (cur == U ? V : U) : temp(count * N);
        return ok;
    }

    // ecfft_poly_eval_points (no reference counterpart): out[b*m + i] = f_b(points[i]) for `count` polynomials of nf coefficients
    // (f: count x nf, crate form) at m arbitrary points shared by all of them.  Subproduct tree of the points in groups of
    // G = max(B, next_pow2(nf)) (subproduct_tree), a remainder tree down to nodes of B = kEvalLeaf points (remainder_descent), Horner
    // at the leaves (k_eval_leaves).  G == B: no tree, f itself is every block's remainder.  Device pointers; asynchronous on `s`
    // (every node is monic, so nothing can fail on the data).  Caller holds lock() and checks the tree rule (G <= size() if G > B).
    bool poly_eval_points(const E* f, size_t nf, const E* points, size_t m, E* out, size_t count, hipStream_t s) {
        const bool ok = eval_points_body(f, nf, points, m, out, count, s);
        temps_done();
        return ok && hipGetLastError() == hipSuccess;
    }
    // poly_eval_points without its end of call: the temporaries stay the caller's
    bool eval_points_body(const E* f, size_t nf, const E* points, size_t m, E* out, size_t count, hipStream_t s) {
        const size_t B = kEvalLeaf, G = eval_group(nf), P = (m + G - 1) / G * G;
        bool ok = true;
        const E* rem = f;
        size_t ld_poly = nf, ld_row = 0, nc = nf;
        if (G > B) {
            SubproductTree st;
            ok = subproduct_tree(points, m, G, st, s) && ok;
            E* R = temp(count * P);
            ok = remainder_descent(f, nf, st, count, R, s) && ok;
            rem = R; ld_poly = P; ld_row = B; nc = B;
        }
        const size_t rows = count * (P / B);
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * ((double)rows * nc + (double)count * m + (double)m), (k_eval_leaves<F, (int)kEvalLeaf>),
                     dim3(nblocks(rows * B)), dim3(kBlock), 0, s, out, rem, ld_poly, ld_row, (uint32_t)nc, points, m, P / B, rows,
                     rinv_table());
        return ok;
    }
    // leaf size B of the remainder tree: a node of B points is evaluated by Horner (B multiplies per point) instead of descending
    static constexpr size_t kEvalLeaf = 64;
    static size_t eval_group(size_t nf) { return nf <= kEvalLeaf ? kEvalLeaf : next_pow2(nf); }
    // Per-level node data of the subproduct tree of npts points (a multiple of G, in groups of G): level k holds the npts / d nodes
    // of d = B << k points (d = B .. G/2) laid end to end, each as M^ (its monic node polynomial M on the 2d leaves of T_2d, from the
    // vanish recursion) and G^ (g = 1/rev(M) mod x^d, lifted to T_2d): 2 npts elements each per level.  Temporaries of the call.
    struct NodeLevel { size_t d; E* Mh; E* Gh; };
    struct SubproductTree { size_t npts = 0, G = 0; std::vector<NodeLevel> lv; };
    // Phase A of ecfft_poly_eval_points: the vanish recursion over all groups at once up to nodes of G/2 points (a level is one
    // pointwise pass and one batched MEXTEND, vanish_step), keeping the levels d >= B; then per kept level one batched EXIT_2d of M^
    // (M's coefficients), one batched inv_series_body of rev(M) mod x^d over all nodes (rev(M)(0) = 1: never singular) and one lift.
    bool subproduct_tree(const E* points, size_t m, size_t G, SubproductTree& st, hipStream_t s) {
        const size_t P = (m + G - 1) / G * G;
        const unsigned lB = ilog2(kEvalLeaf), lG = ilog2(G);
        st.npts = P; st.G = G; st.lv.clear();
        for (unsigned r = lB; r < lG; ++r) st.lv.push_back({(size_t)1 << r, temp(2 * P), temp(2 * P)});
        const TempMark mark = temps_mark();
        E* Q = temp(2 * P); E* Q2 = temp(2 * P); E* q0 = temp(P); E* q1 = temp(P);
        vanish_base(points, m, Q, P, s, true);                   // the padding points of the last group are 0
        for (unsigned r = 1; r < lG; ++r) {
            E* dst = r >= lB ? st.lv[r - lB].Mh : Q2;
            vanish_step(r, Q, dst, q0, q1, P, s, true);
            if (r >= lB) Q = dst; else { Q2 = Q; Q = dst; }
        }
        bool ok = true;
        E* Mc = temp(2 * P); E* rv = temp(P); E* g = temp(P);
        int* flag = new_flag(s);                                 // k_series_base's flag: never raised, every node is monic
        for (const NodeLevel& L : st.lv) {
            const size_t d = L.d, nodes = P / d;
            const unsigned ld = ilog2(d);
            ok = exit(L.Mh, Mc, 2 * d, nodes, s) && ok;
            foreach_n(s, P, [=] __device__(size_t i) { const size_t n = i >> ld, j = i & (d - 1); rv[i] = Mc[(n << (ld + 1)) + d - j]; });
            const TempMark lvl = temps_mark();
            ok = inv_series_body(rv, d, d, g, d, nodes, flag, s) && ok;
            ok = lift_rows(g, d, nodes, L.Gh, s) && ok;
            temps_release(lvl);
        }
        temps_release(mark);
        return ok;
    }
    // Phase B: the remainders of count polynomials at every node of B points (rem: count x P, rows of B).  Per level, children of
    // d points (parents of 2d coefficients; the top parent is f itself, read at a row stride of 0 by every group):
    //   t   = rev(parent) mod x^d, lifted once per parent;
    //   q_c = rev((t g_c) mod x^d): k_tree_pointwise against G^_c (both siblings read their parent's t), one batched EXIT_2d;
    //   r_c = (parent mod x^d) - (M_c q_c mod x^d): q_c lifted, k_tree_pointwise against M^_c (deg M_c q_c < 2d: nothing wraps),
    //         one batched EXIT_2d and the subtraction.
    bool remainder_descent(const E* f, size_t nf, const SubproductTree& st, size_t count, E* rem, hipStream_t s) {
        const size_t P = st.npts;
        E* A = temp(count * P); E* C = temp(count * P); E* t = temp(count * P / 2); E* q = temp(count * P); E* Y = temp(2 * count * P);
        const TE rinv = rinv_table();
        const E* par = f;
        size_t ldb = nf, ldr = 0, plen = nf;                     // parent row (b, p) at par + b*ldb + p*ldr, plen coefficients
        bool ok = true;
        for (size_t k = st.lv.size(); k-- > 0;) {
            const NodeLevel& L = st.lv[k];
            const size_t d = L.d, nodes = P / d, npar = nodes / 2, rows = count * nodes, total = rows * 2 * d;
            const unsigned ld = ilog2(d);
            E* dst = k == 0 ? rem : (par == A ? C : A);
            const TempMark lvl = temps_mark();
            foreach_n(s, count * npar * d, [=] __device__(size_t i) {
                const size_t pr = i >> ld, j = i & (d - 1), b = pr / npar, p = pr - b * npar, c = 2 * d - 1 - j;
                t[i] = c < plen ? par[b * ldb + p * ldr + c] : F::zero();
            });
            PolyEvals<F> ev[2];
            ok = lift_evals(t, d, count * npar, ev, s) && ok;
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 2.5 * (double)total, k_tree_pointwise<F>, dim3(nblocks(total)), dim3(kBlock), 0, s,
                         Y, ev[0], 1u, (const E*)L.Gh, nodes, rinv, ld + 1, total);
            ok = exit(Y, Y, 2 * d, rows, s) && ok;
            foreach_n(s, rows * d, [=] __device__(size_t i) { const size_t r = i >> ld, j = i & (d - 1); q[i] = Y[(r << (ld + 1)) + d - 1 - j]; });
            ok = lift_evals(q, d, rows, ev, s) && ok;
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * 3.0 * (double)total, k_tree_pointwise<F>, dim3(nblocks(total)), dim3(kBlock), 0, s,
                         Y, ev[0], 0u, (const E*)L.Mh, nodes, rinv, ld + 1, total);
            ok = exit(Y, Y, 2 * d, rows, s) && ok;
            foreach_n(s, rows * d, [=] __device__(size_t i) {
                const size_t r = i >> ld, j = i & (d - 1), b = r / nodes, p = (r - b * nodes) >> 1;
                const E a = j < plen ? par[b * ldb + p * ldr + j] : F::zero();
                dst[i] = F::canon(F::sub(a, F::canon(Y[(r << (ld + 1)) + j])));
            });
            temps_release(lvl);
            par = dst; ldb = P; ldr = d; plen = d;
        }
        return ok;
    }
    // count rows of d coefficients (a power of two) -> their evaluations on the 2d leaves of T_2d as poly_mul's last lift leaves them
    // (ENTER_d, EXTEND_d onto S1: even / odd halves); takes temporaries
    bool lift_evals(const E* src, size_t d, size_t count, PolyEvals<F>* ev, hipStream_t s) {
        const E* srcs[2] = {src, src};
        const size_t len[2] = {d, d}, ld[2] = {d, d};
        E* Y = nullptr;
        return lift_operands(srcs, len, ld, 1, 2 * d, count, ev, Y, s);
    }
    // ... materialised in natural leaf order (dst: count x 2d)
    bool lift_rows(const E* src, size_t d, size_t count, E* dst, hipStream_t s) {
        PolyEvals<F> ev[2];
        const bool ok = lift_evals(src, d, count, ev, s);
        materialise(ev[0], 2 * d, count, dst, s);
        return ok;
    }

    // ecfft_poly_interpolate (no reference counterpart): out (count x m) = the coefficients of the f_b of degree < m with
    // f_b(points[i]) = values[b*m + i], for m pairwise distinct points shared by all `count` value vectors.  Lagrange form
    // f = sum_i c_i M / (x - x_i), M = prod (x - x_i), c_i = y_i / M'(x_i), on ONE group of P = max(B, next_pow2(m)) points of
    // eval_points' subproduct tree, the last k = P - m of them the pad point 0 with weight 0: the padded sum is x^k f.
    //   weights (once per call): M from the two top nodes (interp_weights), M'(x_i) by one remainder descent + k_eval_leaves, inverted;
    //   leaves: k_interp_leaves gives every block of B points its numerator's B coefficients, one lift brings them to T_2B;
    //   ascent: per level k_interp_combine (N^ = N^_l M^_r + N^_r M^_l on T_2d) and one batched EXTEND onto S1 of T_4d for the next
    //           level's odd half; one batched EXIT_P at the top, the output is that row shifted down by k.
    // P == B: k_interp_leaves is the whole interpolation, no transform.  Device pointers; synchronous (the flag of a zero weight
    // denominator is read back: *repeated = two equal points).  Caller holds lock() and checks the tree rule (P <= size() if P > B).
    bool poly_interpolate(const E* points, size_t m, const E* values, E* out, size_t count, bool* repeated, hipStream_t s) {
        int* flag = new_flag(s);
        const bool ok = interpolate_body(points, m, values, out, count, flag, nullptr, s);
        return finish_flagged(ok, flag, repeated, s);
    }
    // poly_interpolate without its end of call: *flag is raised for two equal points, the temporaries stay the caller's.  m0 (may be
    // null; needs P > B, m > kEvalLeaf): m + 1 coefficients that receive M = prod (x - x_i), which the weights pass through.
    bool interpolate_body(const E* points, size_t m, const E* values, E* out, size_t count, int* flag, E* m0, hipStream_t s) {
        const size_t B = kEvalLeaf, P = eval_group(m), k = P - m, rpv = P / B, rows = count * rpv;
        const TE rinv = rinv_table();
        bool ok = true;
        SubproductTree st;
        E* w = temp(m);                                          // plain 1 / M'(x_i)
        if (P > B) {
            ok = subproduct_tree(points, m, P, st, s) && ok;
            ok = interp_weights(points, m, st, w, flag, m0, s) && ok;
        } else {
            const E ri = rinv_;                                  // M'(x_i) = prod_{j != i} (x_i - x_j) over the m real points
            foreach_n(s, m, [=] __device__(size_t i) {
                const E xi = points[i];
                E acc = F::one();
                for (size_t j = 0; j < m; ++j) if (j != i) acc = F::mul(acc, F::mul(F::sub(xi, points[j]), ri));
                acc = F::canon(acc);
                if (F::is_zero(acc)) *flag = 1;
                w[i] = acc;
            });
            batch_inv(w, w, m, s);
        }
        E* leaf = P > B ? temp(count * P) : (k ? temp(count * P) : out);
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * ((double)rows * B + (double)count * m + 2.0 * (double)m), (k_interp_leaves<F, (int)kEvalLeaf>),
                     dim3(nblocks(rows * B)), dim3(kBlock), 0, s, leaf, values, (const E*)w, points, m, rpv, rows, rinv);
        const E* top = leaf;                                     // count rows of P coefficients of x^k f_b
        if (P > B) {
            E* Y[2] = {temp(count * P), st.lv.size() > 1 ? temp(count * P) : nullptr};
            E* X = st.lv.size() > 1 ? temp(count * P) : nullptr;
            const TempMark mark = temps_mark();                  // the lift's temporaries are read by the first level only
            PolyEvals<F> ev[2];
            ok = lift_evals(leaf, B, rows, ev, s) && ok;
            PolyEvals<F> cur = ev[0];
            for (size_t lvl = 0; lvl < st.lv.size(); ++lvl) {
                const NodeLevel& L = st.lv[lvl];
                const size_t d = L.d, nodes = P / d, total = count * P;           // count * nodes / 2 parents of 2d evaluations
                E* dst = Y[lvl & 1];
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (2.0 * (double)total + 2.0 * (double)P), k_interp_combine<F>, dim3(nblocks(total)),
                             dim3(kBlock), 0, s, dst, cur, (const E*)L.Mh, nodes, rinv, ilog2(d) + 1, total);
                if (lvl == 0) temps_release(mark);
                if (2 * d < P) {
                    ok = extend_api(dst, X, 2 * d, count * nodes / 2, 1, s) && ok;
                    cur = PolyEvals<F>{dst, X, 2 * d, 1u};
                }
                top = dst;
            }
            E* T = const_cast<E*>(top);
            if (k == 0) ok = exit(T, out, P, count, s) && ok; else ok = exit(T, T, P, count, s) && ok;
        }
        if (k)
            ok = ok && hipMemcpy2DAsync(out, m * sizeof(E), top + k, P * sizeof(E), m * sizeof(E), count, hipMemcpyDeviceToDevice, s) == hipSuccess;
        return ok;
    }
    // ---- ecfft_rs_decode: Reed-Solomon decoding by Gao's algorithm ----
    // code lengths up to this run a received word per workgroup (k_rs_decode_small), on any tree: g0 has m + 1 <= kGcdSmall coefficients
    static constexpr size_t kRsSmall = kGcdSmall - 1;
    static size_t rs_leaves(size_t m) { return m <= kRsSmall ? 1 : next_pow2(2 * m + 1); }
    // message (count x k) = the coefficients of the f_b, deg f_b < k, that differ from values (count x m) on at most (m - k) / 2 of
    // the m pairwise distinct points, n_errors[b] (host) the number of those positions; a zero row and -1 where there is none.
    // g0 = prod (x - x_i), g1 = the interpolant of the row, (r, ., t) = the partial row of (g0, g1) with stop = ceil((m + k) / 2),
    // f = r / t: the word decodes iff the division is exact and deg f < k, and then n_errors = deg t.
    // rs_decode_erasures without a mask, in coefficient form: one driver serves both.
    bool rs_decode(const E* points, size_t m, const E* values, size_t k, E* message, long long* n_errors, size_t count, bool* repeated,
                   hipStream_t s) {
        return rs_decode_erasures(points, m, values, nullptr, k, message, false, n_errors, count, repeated, s);
    }
    // What the small-regime rows over m <= kRsSmall points share (k_rs_prepare): g0 (m + 1), np and invd (m x m each)
    void rs_prepare_launch(const E* points, size_t m, E* np, E* g0, E* invd, int* flag, hipStream_t s) {
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * (2.0 * (double)m * (double)m + 2.0 * (double)m), (k_rs_prepare<F, (int)kGcdSmall>), dim3((unsigned)m),
                     dim3((unsigned)kGcdSmall), 0, s, points, (uint32_t)m, np, g0, invd, rinv_, crate_one(), flag);
    }
    // k_rs_decode_small over c <= 2^16 rows behind rs_prepare_launch: msg (c x k), derr (c verdicts, device)
    void rs_small_launch(const E* values, size_t m, size_t k, const E* np, const E* g0, const E* invd, E* msg, long long* derr, size_t c,
                         hipStream_t s) {
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * ((double)c * (double)(m + k) + 2.0 * (double)m * (double)m), (k_rs_decode_small<F, (int)kGcdSmall>),
                     dim3((unsigned)c), dim3((unsigned)kGcdSmall), 0, s, values, (uint32_t)m, (uint32_t)k, (int32_t)((m + k + 1) / 2), np, g0, invd, msg,
                     derr, crate_one());
    }
    // ---- ecfft_rs_encode / ecfft_rs_decode_erasures: the systematic codec ----
    // Above kRsSmall the encoder interpolates at the first k points and evaluates k coefficients at the other m - k
    static size_t rs_encode_leaves(size_t m, size_t k) { return m <= kRsSmall || k <= kEvalLeaf ? 1 : eval_group(k); }
    // *repeated = two of the m points are equal: fully reduced copies sorted on the host (the large regime's check over ALL points,
    // which no single interpolation of that regime covers).  Drains s.
    bool rs_points_repeat(const E* points, size_t m, bool* repeated, hipStream_t s) {
        E* c = temp(m);
        foreach_n(s, m, [=] __device__(size_t i) { c[i] = F::canon(points[i]); });
        std::vector<E> h(m);
        if (hipMemcpyAsync(h.data(), c, m * sizeof(E), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return false;
        auto less = [](const E& a, const E& b) { return std::memcmp(&a, &b, sizeof(E)) < 0; };
        std::sort(h.begin(), h.end(), less);
        *repeated = false;
        for (size_t i = 1; i < m; ++i) if (std::memcmp(&h[i - 1], &h[i], sizeof(E)) == 0) *repeated = true;
        return true;
    }
    // codeword (count x m) = data (count x k, fully reduced) followed by the m - k values at points[k..m) of the f_b of degree < k
    // with f_b(points[i]) = data[b][i], i < k.
    //   m <= kRsSmall: k_rs_encode_prepare (the (m - k) x k matrix of the Lagrange basis at the parity points, shared by the rows),
    //     then k_rs_encode_small, G / (m - k) rows per workgroup.
    //   otherwise interpolate_body at the first k points and eval_points_body at the others, for all rows at once.
    // Synchronous; *repeated = two equal points among all m.  Caller holds lock() and checks the tree rule (rs_encode_leaves).
    bool rs_encode(const E* points, size_t m, const E* data, size_t k, E* codeword, size_t count, bool* repeated, hipStream_t s) {
        const size_t npar = m - k;
        int* flag = new_flag(s);
        bool ok = true, rep = false;
        if (m <= kRsSmall) {
            constexpr int G = (int)kGcdSmall;
            E* gt = temp(npar ? npar * k : 1);
            ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * ((double)m + (double)npar * (double)k), (k_rs_encode_prepare<F, G>), dim3((unsigned)(npar ? npar : 1)),
                         dim3(G), 0, s, points, (uint32_t)m, (uint32_t)k, gt, flag);
            const size_t rpb = npar ? (size_t)G / npar : (size_t)G, blocks = (count + rpb - 1) / rpb;
            for_chunks(blocks, [&](size_t c0, size_t c) {
                const size_t b0 = c0 * rpb;
                ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * ((double)(count - b0) * (double)(m + k) + (double)npar * (double)k), (k_rs_encode_small<F, G>),
                             dim3((unsigned)c), dim3(G), 0, s, data + b0 * k, (uint32_t)m, (uint32_t)k, (const E*)gt, codeword + b0 * m, count - b0,
                             (uint32_t)rpb);
            });
        } else {
            ok = rs_points_repeat(points, m, &rep, s);
            if (ok && !rep) {
                E* coef = temp(count * k); E* par = temp(npar ? count * npar : 1);
                if (npar) {
                    ok = interpolate_body(points, k, data, coef, count, flag, nullptr, s);
                    ok = eval_points_body(coef, k, points + k, npar, par, count, s) && ok;
                }
                foreach_n(s, count * m, [=] __device__(size_t idx) {
                    const size_t b = idx / m, i = idx - b * m;
                    codeword[idx] = i < k ? F::canon(data[b * k + i]) : par[b * npar + (i - k)];
                });
            }
        }
        ok = finish_flagged(ok, flag, repeated, s);
        *repeated = *repeated || rep;
        return ok;
    }
    // One row of the large regime after its interpolation: g0 (mm + 1 coefficients), g1 (mm), the partial row with `stop`, the exact
    // division; msg (k coefficients, zeroed by the caller) and *verdict are written on success only.
    bool rs_decode_row(const E* g0, size_t mm, const E* g1, size_t k, size_t stop, E* r, E* t, E* msg, long long* verdict, hipStream_t s) {
        const TempMark mark = temps_mark();
        long long deg[3] = {-1, -1, -1};
        bool ok = gcd_partial_pair(g0, mm + 1, g1, mm, stop, r, mm + 1, nullptr, mm, t, mm + 1, deg, s);
        const long long dq = deg[0] - deg[2];
        if (ok && deg[0] < 0) {
            *verdict = deg[2];                                   // r = 0: f = 0
        } else if (ok && deg[2] >= 0 && dq >= 0 && dq < (long long)k) {
            const size_t lr = (size_t)deg[0] + 1, lt = (size_t)deg[2] + 1, lrem = lt - 1;
            E* q = temp((size_t)dq + 1); E* rem = temp(lrem ? lrem : 1);
            size_t nz = 0;
            ok = divrem_body(r, lr, t, lt, q, lrem ? rem : nullptr, 1, gcd_flag_, s) && gcd_row_lens(rem, lrem, lrem, 1, &nz, s);
            if (ok && nz == 0) {
                *verdict = deg[2];
                ok = hipMemcpyAsync(msg, q, ((size_t)dq + 1) * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
            }
        }
        temps_release(mark);
        return ok;
    }
    // The driver of ecfft_rs_decode and ecfft_rs_decode_erasures.  out (count x k coefficients, or count x m symbols of the
    // re-encoded codeword for codeword == true) and n_errors (host) of Gao's decoder on the kept positions of every row: erased
    // (count x m bytes, may be null) marks the lost symbols, whose values are never read.  A row with fewer than k kept symbols,
    // or without a codeword in its radius floor((m' - k) / 2), is zero and -1.
    //   m <= kRsSmall: rs_prepare_launch over all m points, then ONE launch for all rows: k_rs_decode_small for coefficients without
    //     a mask, else k_rs_decode_ee_small (byte-equal where both apply).
    //   otherwise the rows without erasure go together through one interpolate_body (g0 from its weights pass), then rs_decode_row
    //     each; a row with erasures is compacted on the device to its kept points and values and decoded as a code of length m':
    //     through rs_prepare_launch and rs_small_launch when m' <= kRsSmall, else interpolate_body and rs_decode_row.  The re-encoded
    //     codeword is eval_points_body of all decoded rows at all m points.  Two equal points: with a mask no single interpolation
    //     sees all m points, so rs_points_repeat sorts them first; without one the interpolation of the clean rows raises the flag,
    //     which is read back before the row loop.  No row is decoded once a repeat is known.
    // Synchronous; *repeated = two equal points among all m.  Caller holds lock() and checks the tree rule (rs_leaves).
    bool rs_decode_erasures(const E* points, size_t m, const E* values, const uint8_t* erased, size_t k, E* out, bool codeword,
                            long long* n_errors, size_t count, bool* repeated, hipStream_t s) {
        int* flag = new_flag(s);
        bool ok = true, rep = false;
        std::vector<long long> herr(count, -1);
        std::vector<std::vector<uint32_t>> kept;                 // host sources of asynchronous uploads: alive to the end of the call
        E* g0 = temp(m + 1);
        if (m <= kRsSmall) {
            E* np = temp(m * m); E* invd = temp(m * m);
            long long* derr = temp_as<long long>(count);
            const size_t no = codeword ? m : k;
            rs_prepare_launch(points, m, np, g0, invd, flag, s);
            for_chunks(count, [&](size_t c0, size_t c) {
                if (!erased && !codeword) rs_small_launch(values + c0 * m, m, k, np, g0, invd, out + c0 * k, derr + c0, c, s);
                else ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * ((double)c * (double)(m + no) + 2.0 * (double)m * (double)m),
                             (k_rs_decode_ee_small<F, (int)kGcdSmall>), dim3((unsigned)c), dim3((unsigned)kGcdSmall), 0, s, values + c0 * m,
                             erased ? erased + c0 * m : (const uint8_t*)nullptr, points, (uint32_t)m, (uint32_t)k, (const E*)np, (const E*)g0,
                             (const E*)invd, out + c0 * no, codeword ? 1u : 0u, derr + c0, rinv_, crate_one());
            });
            ok = hipMemcpyAsync(herr.data(), derr, count * sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess;
        } else {
            std::vector<uint8_t> mask;
            if (erased) {
                mask.resize(count * m);
                ok = hipMemcpyAsync(mask.data(), erased, count * m, hipMemcpyDeviceToHost, s) == hipSuccess;
                ok = rs_points_repeat(points, m, &rep, s) && ok; // drains s: the masks are here
            }
            E* coef = codeword ? temp(count * k) : out;
            ok = ok && hipMemsetAsync(coef, 0, count * k * sizeof(E), s) == hipSuccess;
            std::vector<size_t> clean;
            kept.resize(count);
            for (size_t p = 0; p < count; ++p) {
                for (size_t i = 0; erased && i < m; ++i) if (!mask[p * m + i]) kept[p].push_back((uint32_t)i);
                if (!erased || kept[p].size() == m) clean.push_back(p);
            }
            gcd_flag_ = new_flag(s);
            E* r = temp(m + 1); E* t = temp(m + 1);
            if (ok && !rep && !clean.empty()) {
                const size_t nc = clean.size();
                const E* cv = values;
                if (nc < count) {
                    E* g = temp(nc * m);
                    for (size_t i = 0; i < nc && ok; ++i)
                        ok = hipMemcpyAsync(g + i * m, values + clean[i] * m, m * sizeof(E), hipMemcpyDeviceToDevice, s) == hipSuccess;
                    cv = g;
                }
                E* g1 = temp(nc * m);
                ok = ok && interpolate_body(points, m, cv, g1, nc, flag, g0, s);
                if (!erased) {                                   // no sort ran: this interpolation met all m points
                    int h = 0;
                    ok = ok && hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
                    rep = h != 0;
                }
                for (size_t i = 0; i < nc && ok && !rep; ++i)
                    ok = rs_decode_row(g0, m, g1 + i * m, k, (m + k + 1) / 2, r, t, coef + clean[i] * k, &herr[clean[i]], s);
            }
            if (ok && !rep && clean.size() < count) {
                E* cp = temp(m); E* cy = temp(m); E* g1 = temp(m);
                uint32_t* didx = temp_as<uint32_t>(m);
                long long* derr = temp_as<long long>(1);
                for (size_t p = 0; p < count && ok; ++p) {
                    const size_t mk = kept[p].size();
                    if (mk == m || mk < k) continue;
                    const TempMark mark = temps_mark();
                    const E* row = values + p * m;
                    ok = hipMemcpyAsync(didx, kept[p].data(), mk * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess;
                    foreach_n(s, mk, [=] __device__(size_t i) { const uint32_t j = didx[i]; cp[i] = points[j]; cy[i] = row[j]; });
                    if (mk <= kRsSmall) {
                        E* np = temp(mk * mk); E* invd = temp(mk * mk);
                        rs_prepare_launch(cp, mk, np, g0, invd, flag, s);
                        rs_small_launch(cy, mk, k, np, g0, invd, coef + p * k, derr, 1, s);
                        ok = ok && hipMemcpyAsync(&herr[p], derr, sizeof(long long), hipMemcpyDeviceToHost, s) == hipSuccess
                                && hipStreamSynchronize(s) == hipSuccess;
                    } else {
                        ok = ok && interpolate_body(cp, mk, cy, g1, 1, flag, g0, s);
                        ok = ok && rs_decode_row(g0, mk, g1, k, (mk + k + 1) / 2, r, t, coef + p * k, &herr[p], s);
                    }
                    temps_release(mark);
                }
            }
            if (codeword && ok && !rep) ok = eval_points_body(coef, k, points, m, out, count, s);
        }
        ok = finish_flagged(ok, flag, repeated, s);
        *repeated = *repeated || rep;
        for (size_t p = 0; p < count; ++p) n_errors[p] = herr[p];
        return ok;
    }
    // The weights of ecfft_poly_interpolate: w[i] = 1 / M'(points[i]) in PLAIN form for i < m; raises *flag if some M'(x_i) is zero
    // (a repeated point).  The padded top polynomial Mp = x^k M has degree exactly P and does not fit T_P; with the two top nodes
    // M_l = x^(P/2) + A, M_r = x^(P/2) + B (one batched EXIT_P of the top level's M^): Mp = x^P + x^(P/2) (A + B) + A B, and A B
    // has < P coefficients: one product on T_P.  M'_j = (j + 1) Mp_{k+j+1}, the plain constant j + 1 keeps the crate form.
    // m0 (may be null): m + 1 coefficients that receive M itself, Mp's coefficients from k up, in crate form.
    bool interp_weights(const E* points, size_t m, const SubproductTree& st, E* w, int* flag, E* m0, hipStream_t s) {
        const size_t P = st.npts, h = P / 2, k = P - m, B = kEvalLeaf;
        const TempMark mark = temps_mark();
        E* Mc = temp(2 * P); E* AB = temp(P); E* dM = temp(m); E* rem = temp(P);
        bool ok = exit(st.lv.back().Mh, Mc, P, 2, s);
        ok = poly_mul_body(Mc, h, P, Mc + P, h, P, AB, 1, s) && ok;              // P - 1 coefficients
        const E r1 = crate_one();
        auto mp = [=] __device__(size_t c) {                                     // coefficient c <= P of Mp, not reduced
            if (c == P) return r1;
            E v = c < P - 1 ? AB[c] : F::zero();
            if (c >= h) v = F::add(v, F::add(F::canon(Mc[c - h]), F::canon(Mc[P + c - h])));
            return v;
        };
        foreach_n(s, m, [=] __device__(size_t j) { dM[j] = F::canon(F::mul(mp(k + j + 1), F::from_u32((uint32_t)(j + 1)))); });
        if (m0) foreach_n(s, m + 1, [=] __device__(size_t j) { m0[j] = F::canon(mp(k + j)); });
        ok = remainder_descent(dM, m, st, 1, rem, s) && ok;
        ECFFT_LAUNCH(KC_POINTWISE, sizeof(E) * ((double)P + 2.0 * (double)m), (k_eval_leaves<F, (int)kEvalLeaf>), dim3(nblocks(P)),
                     dim3(kBlock), 0, s, w, (const E*)rem, P, B, (uint32_t)B, points, m, P / B, P / B, rinv_table());
        const E ri = rinv_;
        foreach_n(s, m, [=] __device__(size_t i) {
            const E v = F::canon(F::mul(w[i], ri));
            if (F::is_zero(v)) *flag = 1;
            w[i] = v;
        });
        batch_inv(w, w, m, s);
        temps_release(mark);
        return ok;
    }

    // ------------------------------------------------------------------------------------------
    // Public wrappers of the remaining FFTree algorithms on USER data (crate representation),
    // composed from the same EXTEND kernels.  Device pointers; synchronous (they drain `s` before returning
    // because they use temporaries).  Caller holds lock().
    // ------------------------------------------------------------------------------------------
    bool api_mextend(const E* in, E* out, size_t e, size_t count, int target, hipStream_t s) {     // src/fftree.rs:138-141
        b_mextend(ilog2(e) + 1, in, out, count, target, s, true);
        return finish_api(s);
    }
    // redc_z0 / redc_z1 (src/fftree.rs:264-275): evals, a: n entries
    bool api_redc(const E* evals, const E* a, E* out, size_t n, int moiety, hipStream_t s) {
        unsigned l = ilog2(n); size_t e = n / 2;
        E* a0i = temp(e); E* a1 = temp(e);
        plain_halves(a, a0i, a1, e, s);
        batch_inv(a0i, a0i, e, s);                                          // the reference inverts a0 on every call (:235)
        b_redc(l, evals, a0i, a1, out, moiety, s);
        return finish_api(s);
    }
    // modular_reduce (src/fftree.rs:286-289)
    bool api_modular_reduce(const E* evals, const E* a, const E* c, E* out, size_t n, hipStream_t s) {
        unsigned l = ilog2(n); size_t e = n / 2;
        E* a0i = temp(e); E* a1 = temp(e); E* cp = temp(n);
        plain_halves(a, a0i, a1, e, s);
        batch_inv(a0i, a0i, e, s);
        { const E rinv = rinv_; foreach_n(s, n, [=] __device__(size_t i) { cp[i] = F::mul(c[i], rinv); }); }
        b_modular_reduce(l, evals, a0i, a1, cp, out, s);
        return finish_api(s);
    }
    // vanish (src/fftree.rs:313-316): nd domain points -> 2*nd evaluations on the leaves of T_{2 nd}
    bool api_vanish(const E* dom, E* out, size_t nd, hipStream_t s) {
        b_vanish(ilog2(nd) + 1, dom, out, s, true);
        return finish_api(s);
    }
    // degree (src/fftree.rs:169-198).  The reference's recursion is data dependent (g1 == e1 ? recurse on e0 : recurse on t0);
    // here every level computes BOTH candidates and a device-side flag selects between them, so the whole descent is
    // enqueued without a single host round trip (was: one stream synchronise per level) and the degree is read back once.
    bool api_degree(const E* evals, size_t n, hipStream_t s, size_t* degree) {
        unsigned long long hdeg = 0;
        if (n > 1) {
            E* cur = temp(n); E* e0 = temp(n / 2); E* e1 = temp(n / 2); E* g1 = temp(n / 2);
            unsigned long long* acc = temp_as<unsigned long long>(2);   // {degree, flag}
            (void)hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), s);
            (void)hipMemcpyAsync(cur, evals, n * sizeof(E), hipMemcpyDeviceToDevice, s);
            for (size_t m = n; m >= 2; m >>= 1) {
                unsigned l = ilog2(m); size_t e = m / 2;
                const Tree& T = trees_[l];
                foreach_n(s, e, [=] __device__(size_t i) { e0[i] = cur[2 * i]; e1[i] = cur[2 * i + 1]; });
                b_extend(l, e0, g1, 1, 1, s);                               // :180
                const E* zi = T.z0_inv_s1;
                foreach_n(s, e, [=] __device__(size_t i) {                  // :181 (flag) and :187-189 (t1, kept in e1)
                    E d = F::sub(e1[i], g1[i]);
                    if (!F::is_zero(d)) atomicOr(acc + 1, 1ull);
                    e1[i] = F::mul(d, zi[i]);
                });
                b_extend(l, e1, g1, 1, 0, s);                               // t0 (:190)
                foreach_n(s, e, [=] __device__(size_t i) { cur[i] = acc[1] ? g1[i] : e0[i]; });   // :182 / :191
                foreach_n(s, 1, [=] __device__(size_t) { if (acc[1]) acc[0] += (unsigned long long)e; acc[1] = 0; });
            }
            if (hipMemcpyAsync(&hdeg, acc, sizeof(hdeg), hipMemcpyDeviceToHost, s) != hipSuccess) { temps_done(); return false; }
        }
        bool ok = finish_api(s);
        *degree = (size_t)hdeg;
        return ok;
    }

    // The reference's own (un-normalised) matrices of T_m, rebuilt on demand for export (src/fftree.rs:341-363):
    // R = [[v0, s0 v0], [v1, s1 v1]], v_j = v(s_j)^(d/2-1), D = R^-1; identity where d == 1.  out: 4*m elements on the
    // device, row-major Mat2x2 in BinaryTree heap order, crate representation.  Synchronous.
    // standard = true: plain (standard-form) residues instead of the crate's in-memory form — what ark-serialize writes
    bool export_matrices(unsigned log_m, bool decompose, E* out, hipStream_t s, bool standard = false) {
        size_t m = (size_t)1 << log_m, N = N_, stride = N_ / m;
        const E* f = f_; const E* den = den_;
        foreach_n(s, m, [=] __device__(size_t idx) {
            E one = standard ? F::one() : F::to_mont(F::one()), zero = F::zero();
            E r00 = one, r01 = zero, r10 = zero, r11 = one;
            size_t d = 1; unsigned k = 0;
            if (idx >= 2) {                                   // layer k occupies [d, 2d), d = m >> (k+1)
                unsigned lg = 63 - __clzll((unsigned long long)idx);
                d = (size_t)1 << lg; k = (unsigned)(__ffsll((unsigned long long)m) - 1) - 1 - lg;
            }
            if (idx >= 2 && d >= 2) {
                size_t j = idx - d, lay = N >> k;
                E s0 = f[lay + j * stride], s1 = f[lay + (j + d) * stride];
                uint64_t ex = d / 2 - 1;
                E v0 = F::pow_u64(F::mul_add(den[2 * k + 1], s0, den[2 * k]), ex);
                E v1 = F::pow_u64(F::mul_add(den[2 * k + 1], s1, den[2 * k]), ex);
                E a = v0, b = F::mul(s0, v0), c = v1, dd = F::mul(s1, v1);
                if (decompose) {
                    E di = F::inv(F::sub(F::mul(a, dd), F::mul(b, c)));
                    r00 = F::mul(dd, di); r01 = F::mul(F::neg(b), di); r10 = F::mul(F::neg(c), di); r11 = F::mul(a, di);
                } else { r00 = a; r01 = b; r10 = c; r11 = dd; }
                if (!standard) { r00 = F::to_mont(r00); r01 = F::to_mont(r01); r10 = F::to_mont(r10); r11 = F::to_mont(r11); }
            }
            out[4 * idx] = r00; out[4 * idx + 1] = r01; out[4 * idx + 2] = r10; out[4 * idx + 3] = r11;
        });
        return hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }

    // f of T_m (BinaryTree<F>, 2m entries, heap order; entry 0 unused = 0): every (N/m)-th element of each layer of the top
    // tree's point set (src/fftree.rs:471-478), gathered on the device.  out: 2m elements on the device, plain.  Synchronous.
    bool gather_f(unsigned log_m, E* out, hipStream_t s) const {
        if (!f_) return false;
        const size_t m = (size_t)1 << log_m, N = N_, stride = N_ / m;
        const E* f = f_;
        foreach_n(s, 2 * m, [=] __device__(size_t idx) {
            if (idx == 0) { out[0] = F::zero(); return; }
            const unsigned lg = 63 - __clzll((unsigned long long)idx);     // layer with 2^lg points: idx in [2^lg, 2^(lg+1))
            const size_t sz = (size_t)1 << lg, j = idx - sz;
            out[idx] = f[(N / m) * sz + j * stride];                       // that layer of the top tree has N*sz/m points
        });
        return hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }

    // out[i] = f(x[i], y[i], T[t_off + i*t_stride]) with T one of the reference's plain tables of T_m (data x
    // plain table needs no Montgomery correction).  mode 0: x*T   1: x*T + y   2: y - x*T   3: (y - x)*T.
    // The pointwise steps of the multi-GPU ENTER / EXIT are built from this (Python model: tests/split_model.py).
    bool table_fma(E* out, const E* x, const E* y, size_t cnt, unsigned log_m, int which, size_t t_off, size_t t_stride, int mode, hipStream_t s) const {
        const Tree& T = trees_[log_m];
        const E* tbl = nullptr; size_t len = 0;
        switch (which) {
            case 3: tbl = T.xnn; len = T.m; break;           // ECFFT_TBL_XNN_S
            case 4: tbl = T.xnn_inv; len = T.m; break;
            case 5: tbl = T.z0_s1; len = T.e; break;
            case 6: tbl = T.z1_s0; len = T.e; break;
            case 7: tbl = T.z0_inv_s1; len = T.e; break;
            case 8: tbl = T.z1_inv_s0; len = T.e; break;
            case 9: tbl = T.z0z0; len = T.m; break;
            case 10: tbl = T.z1z1; len = T.m; break;
            default: return false;
        }
        if (cnt && t_off + (cnt - 1) * t_stride >= len) return false;
        if (mode < 0 || mode > 3 || (mode != 0 && !y)) return false;
        foreach_n(s, cnt, [=] __device__(size_t i) {
            E t = tbl[t_off + i * t_stride];
            E r;
            if (mode == 0) r = F::mul(t, x[i]);
            else if (mode == 1) r = F::mul_add(t, x[i], y[i]);
            else if (mode == 2) r = F::sub(y[i], F::mul(t, x[i]));
            else r = F::mul(t, F::sub(y[i], x[i]));
            out[i] = r;
        });
        return hipGetLastError() == hipSuccess;
    }

    E* scratch() const { return scratch_; }

private:
    // ---- memory ----
    E* take(size_t n) {
        size_t a = (n + 7) & ~(size_t)7;
        if (arena_used_ + a > arena_cap_) { fprintf(stderr, "ecfft: internal error: table arena overflow\n"); throw DeviceAllocError(); }   // sized exactly in build(); unreachable
        E* p = arena_ + arena_used_; arena_used_ += a; return p;
    }
    static constexpr size_t kTeElems = sizeof(TE) / sizeof(E);
    static_assert(sizeof(TE) % sizeof(E) == 0, "table element must be a whole number of field elements");
    // n table constants in the arena, filled from the plain values src[0..n)
    TE* to_tables(const E* src, size_t n, hipStream_t s) {
        TE* d = reinterpret_cast<TE*>(take(n * kTeElems));
        foreach_n(s, n, [=] __device__(size_t i) { d[i] = F::to_table(src[i]); });
        return d;
    }
    // construction temporaries come from one slab (bump-allocated, reset after every tree); anything that does not fit,
    // and every temporary of the public algorithm wrappers, is an individual allocation released by finish_api()
    E* temp(size_t n) {
        size_t a = (n + 7) & ~(size_t)7;
        if (slab_ && slab_used_ + a <= slab_cap_) { E* q = slab_ + slab_used_; slab_used_ += a; return q; }
        // pooled individual allocations: finish_api() / build_tree() hand them back to the pool instead of freeing them,
        // so repeated algorithm calls (ecfft_redc, ecfft_degree, ...) do not hipMalloc / hipFree every time.  Best fit, but a
        // request never takes a block more than 4x its size (or 64 KiB): the 16-byte accumulator of ecfft_degree used to grab
        // a multi-GiB block and force a fresh allocation for the next large request.
        size_t bytes = (a ? a : 8) * sizeof(E);
        const size_t cap_fit = bytes * 4 > ((size_t)64 << 10) ? bytes * 4 : ((size_t)64 << 10);
        int best = -1;
        for (size_t i = 0; i < pool_.size(); ++i)
            if (!pool_[i].busy && pool_[i].bytes >= bytes && pool_[i].bytes <= cap_fit && (best < 0 || pool_[i].bytes < pool_[(size_t)best].bytes)) best = (int)i;
        if (best >= 0) { pool_[(size_t)best].busy = true; pool_[(size_t)best].idle_calls = 0; return (E*)pool_[(size_t)best].p; }
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            temps_trim(0);                                    // give back every idle pooled block and try once more
            if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "ecfft: temporary allocation of %zu bytes failed\n", bytes); throw DeviceAllocError(); }
        }
        pool_.push_back({p, bytes, true, false, 0});
        return (E*)p;
    }
    // n objects of T in a temporary (rounded up to whole elements)
    template <class T> T* temp_as(size_t n) { return reinterpret_cast<T*>(temp((n * sizeof(T) + sizeof(E) - 1) / sizeof(E))); }
    // one workgroup per row of `count` rows: fn(first row, rows) per launch of at most 2^16 workgroups
    template <class Fn> static void for_chunks(size_t count, Fn&& fn) {
        for (size_t c0 = 0; c0 < count; c0 += (size_t)1 << 16) fn(c0, count - c0 < ((size_t)1 << 16) ? count - c0 : (size_t)1 << 16);
    }
    // End of a call: every pooled temporary becomes reusable.  The pool is bounded: idle blocks beyond `keep` bytes in total
    // (twice the transform scratch, at least 256 MiB) are returned to the device, largest first — one large ecfft_vanish /
    // ecfft_degree no longer pins 6-10 n elements of HBM for the life of the context (ecfft_ctx_trim returns all of it).  Pinned blocks (the temporaries of a sharded transform whose shape the ranks have agreed on) are never trimmed.
    void temps_done() {
        for (auto& b : pool_) { if (!b.busy) ++b.idle_calls; b.busy = false; }
        size_t keep = 2 * scratch_cap_ * sizeof(E);
        if (keep < ((size_t)256 << 20)) keep = (size_t)256 << 20;
        temps_trim(keep);                                    // rare: hipFree waits for the device
    }
    // Temporaries taken after a mark can be handed back before the call ends, so that each level of a multi-level call reuses the
    // previous level's: every later use is enqueued on the call's stream, after the kernels that read them.
    using TempMark = std::vector<const void*>;
    TempMark temps_mark() const { TempMark busy; for (const auto& b : pool_) if (b.busy) busy.push_back(b.p); return busy; }
    void temps_release(const TempMark& mark) {
        for (auto& b : pool_)
            if (b.busy && std::find(mark.begin(), mark.end(), (const void*)b.p) == mark.end()) b.busy = false;
    }
    size_t pool_bytes() const { size_t t = 0; for (const auto& b : pool_) t += b.bytes; return t; }
    // frees idle, unpinned blocks: those idle for > max_idle calls, then the largest ones until the idle total is <= keep bytes
    void temps_trim(size_t keep, unsigned max_idle = ~0u) {
        for (size_t i = 0; i < pool_.size();) {
            if (!pool_[i].busy && !pool_[i].pinned && pool_[i].idle_calls > max_idle) { (void)hipFree(pool_[i].p); pool_[i] = pool_.back(); pool_.pop_back(); }
            else ++i;
        }
        for (;;) {
            size_t idle = 0; int big = -1;
            for (size_t i = 0; i < pool_.size(); ++i)
                if (!pool_[i].busy && !pool_[i].pinned) { idle += pool_[i].bytes; if (big < 0 || pool_[i].bytes > pool_[(size_t)big].bytes) big = (int)i; }
            if (idle <= keep || big < 0) break;
            (void)hipFree(pool_[(size_t)big].p); pool_[(size_t)big] = pool_.back(); pool_.pop_back();
        }
    }
    void temps_free() { for (auto& b : pool_) (void)hipFree(b.p); pool_.clear(); }
    void release() {
        temps_free();
        full_cyclic_free();
        if (arena_) (void)hipFree(arena_);
        if (slab_) { (void)hipFree(slab_); slab_ = nullptr; slab_cap_ = slab_used_ = 0; }
        if (scratch_) (void)hipFree(scratch_);
        if (d_trees_) (void)hipFree(d_trees_);
        d_trees_ = nullptr;
        for (int i = 0; i < nside_; ++i) { (void)hipStreamDestroy(sides_[i]); (void)hipEventDestroy(ev_fork_[i]); (void)hipEventDestroy(ev_join_[i]); }
        nside_ = 0;
        arena_ = nullptr; scratch_ = nullptr;
    }

    bool ensure_scratch(size_t nt) {
        const size_t need = scratch_need(nt, kSplitDepth) > 5 * nt ? scratch_need(nt, kSplitDepth) : 5 * nt;
        if (scratch_cap_ >= need) return true;
        if (scratch_) { (void)hipDeviceSynchronize(); (void)hipFree(scratch_); scratch_ = nullptr; scratch_cap_ = 0; }
        if (hipMalloc(&scratch_, need * sizeof(E)) != hipSuccess) { fprintf(stderr, "ecfft: scratch allocation of %zu elements failed\n", need); return false; }
        scratch_cap_ = need;
        return true;
    }
    bool finish_api(hipStream_t s) {
        bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        temps_done();
        return ok;
    }
    // user table a (crate representation, 2e entries) -> plain even entries (to be inverted) and plain odd entries
    void plain_halves(const E* a, E* a_even, E* a_odd, size_t e, hipStream_t s) {
        const E rinv = rinv_;
        foreach_n(s, e, [=] __device__(size_t i) { a_even[i] = F::mul(a[2 * i], rinv); a_odd[i] = F::mul(a[2 * i + 1], rinv); });
    }

    // ---- construction-time device primitives (plain data) ----
    // out[i] = 1/in[i]; chunks share one Fermat inversion (Montgomery's trick).  Zero entries stay zero and do not disturb
    // their neighbours, like ark_ff::batch_inversion (used at src/fftree.rs:235, 331-333, 409-414).  The inversion is a
    // dependent chain of ~270 multiplies, i.e. its LATENCY is what a call costs; the chunk length grows with n so that at most
    // one wave per SIMD runs such a chain (more waves would only share the issue slots and stretch every chain), and the
    // prefix products live in `out` / a temporary instead of per-thread arrays (round 2: 528 B of scratch per thread).
    // Several independent arrays in ONE launch (the inversion chain's latency is paid once, not once per table).
    struct InvSeg { const E* in; E* out; size_t n; };
    struct InvSegs { const E* in[6]; E* out[6]; E* pre[6]; size_t n[6], first[7]; int k; };
    void batch_inv(const E* in, E* out, size_t n, hipStream_t s) { const InvSeg g{in, out, n}; batch_inv_multi(&g, 1, s); }
    void batch_inv_multi(const InvSeg* segs, int k, hipStream_t s) {
        size_t total = 0;
        for (int j = 0; j < k; ++j) total += segs[j].n;
        if (!total || k > 6) return;
        size_t CH = 8;
        while (CH < 64 && (total + CH - 1) / CH + (size_t)k > (size_t)65536) CH *= 2;
        InvSegs g{}; g.k = 0; g.first[0] = 0;
        for (int j = 0; j < k; ++j) {
            if (!segs[j].n) continue;
            const int q = g.k++;
            g.in[q] = segs[j].in; g.out[q] = segs[j].out; g.n[q] = segs[j].n;
            g.pre[q] = (segs[j].in == segs[j].out) ? temp(segs[j].n) : segs[j].out;   // in-place calls keep their inputs until the backward pass
            g.first[q + 1] = g.first[q] + (segs[j].n + CH - 1) / CH;                  // chunks never straddle two arrays
        }
        foreach_n(s, g.first[g.k], [=] __device__(size_t t) {
            int q = 0;
            while (q + 1 < g.k && t >= g.first[q + 1]) ++q;
            const E* in = g.in[q]; E* out = g.out[q]; E* pre = g.pre[q];
            const size_t n = g.n[q], b = (t - g.first[q]) * CH, cnt = (b + CH <= n) ? CH : n - b;
            E acc = F::one();
            for (size_t i = 0; i < cnt; ++i) { const E v = in[b + i]; pre[b + i] = acc; if (!F::is_zero(v)) acc = F::mul(acc, v); }
            acc = F::inv(acc);
            for (size_t i = cnt; i-- > 0;) {
                const E v = in[b + i];
                if (F::is_zero(v)) { out[b + i] = F::zero(); continue; }
                const E r = F::mul(acc, pre[b + i]);
                acc = F::mul(acc, v);
                out[b + i] = r;
            }
        });
    }
    void ew_mul(E* out, const E* a, const E* b, size_t n, hipStream_t s) {
        foreach_n(s, n, [=] __device__(size_t i) { out[i] = F::mul(a[i], b[i]); });
    }
    // FFTree::extend for construction (whole-vector form with pre/post scaling)
    void b_extend(unsigned log_m, const E* in, E* out, size_t count, int target, hipStream_t s) {
        extend(in, out, trees_[log_m].e, count, target, s);
    }
    // mextend (src/fftree.rs:128-141)
    // The compositions below run on PLAIN data during construction (mont = false) and on user data in the crate's
    // Montgomery form for the public wrappers (mont = true): tables that are ADDED to data are converted with to_mont,
    // data x data products get the extra factor R^-1 (rinv_), data x table products need nothing.
    void b_mextend(unsigned log_m, const E* in, E* out, size_t count, int target, hipStream_t s, bool mont = false) {
        const Tree& T = trees_[log_m];
        b_extend(log_m, in, out, count, target, s);
        const E* z = target == 1 ? T.z0_s1 : T.z1_s0;
        size_t mask = T.e - 1;
        foreach_n(s, T.e * count, [=] __device__(size_t i) { E zz = z[i & mask]; out[i] = F::add(out[i], mont ? F::to_mont(zz) : zz); });
    }
    // redc_impl (src/fftree.rs:232-259); a0inv/a1: e PLAIN entries; evals/out: m entries
    void b_redc(unsigned log_m, const E* evals, const E* a0inv, const E* a1, E* out, int moiety, hipStream_t s) {
        const Tree& T = trees_[log_m];
        size_t e = T.e;
        E* t0 = temp(e); E* h1 = temp(e);
        foreach_n(s, e, [=] __device__(size_t i) { t0[i] = F::mul(evals[2 * i], a0inv[i]); });
        b_extend(log_m, t0, t0, 1, 1 - moiety, s);                           // g1 = extend_impl(t0, opposite moiety)  (:239-245)
        const E* zinv = moiety == 0 ? T.z0_inv_s1 : T.z1_inv_s0;            // :247-250
        foreach_n(s, e, [=] __device__(size_t i) {
            h1[i] = F::mul(F::sub(evals[2 * i + 1], F::mul(t0[i], a1[i])), zinv[i]);
        });
        b_extend(log_m, h1, t0, 1, moiety, s);                               // h0 = extend_impl(h1, moiety)  (:256)
        foreach_n(s, e, [=] __device__(size_t i) { out[2 * i] = t0[i]; out[2 * i + 1] = h1[i]; });
    }
    void b_redc_s0(unsigned log_m, const E* evals, const E* a0inv, const E* a1, E* out, hipStream_t s) { b_redc(log_m, evals, a0inv, a1, out, 0, s); }
    // modular_reduce_impl (src/fftree.rs:277-281); c PLAIN
    void b_modular_reduce(unsigned log_m, const E* evals, const E* a0inv, const E* a1, const E* c, E* out, hipStream_t s) {
        size_t m = trees_[log_m].m;
        E* h = temp(m);
        b_redc_s0(log_m, evals, a0inv, a1, h, s);
        ew_mul(h, h, c, m, s);
        b_redc_s0(log_m, h, a0inv, a1, out, s);
    }
    // vanish_impl (src/fftree.rs:291-308), bottom-up: dom has e = m/2 entries, out m entries
    void b_vanish(unsigned log_m, const E* dom, E* out, hipStream_t s, bool mont = false) {
        const Tree& T = trees_[log_m];
        size_t e = T.e, m = T.m;
        E* Q = temp(m); E* Q2 = temp(m); E* q0 = temp(e); E* q1 = temp(e);
        vanish_base(dom, e, Q, e, s, mont);
        unsigned le = ilog2(e);
        for (unsigned r = 1; r <= le; ++r) {
            E* dstQ = (r == le) ? out : Q2;
            vanish_step(r, Q, dstQ, q0, q1, e, s, mont);
            E* t = Q; Q = Q2; Q2 = t;
        }
        if (le == 0) (void)hipMemcpyAsync(out, Q, m * sizeof(E), hipMemcpyDeviceToDevice, s);
    }
    // the leaves of the vanish recursion: Q[2i], Q[2i+1] = (x - dom[i]) on the two leaves of T_2 for e points, dom[i] = 0 for i >= nd
    void vanish_base(const E* dom, size_t nd, E* Q, size_t e, hipStream_t s, bool mont) {
        const E* f = f_; size_t N = N_;
        foreach_n(s, e, [=] __device__(size_t i) {        // T_2 leaves are the top tree's leaves 0 and N/2
            E l0 = f[N], l1 = f[N + N / 2];
            if (mont) { l0 = F::to_mont(l0); l1 = F::to_mont(l1); }
            const E x = i < nd ? dom[i] : F::zero();
            Q[2 * i] = F::sub(x, l0); Q[2 * i + 1] = F::sub(x, l1);
        });
    }
    // one level of the vanish recursion (src/fftree.rs:291-308) over e points (a multiple of 2^r): Q holds, per block of 2^(r-1)
    // points, their product on the 2^r leaves of T_(2^r); dst gets, per block of 2^r points, their product on the leaves of
    // T_(2^(r+1)) — the pointwise product of two sibling blocks is the product on S0 = T_(2^r), MEXTEND gives S1.  q0, q1: e each.
    void vanish_step(unsigned r, const E* Q, E* dst, E* q0, E* q1, size_t e, hipStream_t s, bool mont) {
        const size_t bs = (size_t)1 << r;                   // size of the blocks being merged
        const E rinv = rinv_;
        foreach_n(s, e, [=] __device__(size_t g) {
            size_t b = g >> r, i = g & (bs - 1);
            E pr = F::mul(Q[(2 * b) * bs + i], Q[(2 * b + 1) * bs + i]);
            q0[g] = mont ? F::mul(pr, rinv) : pr;
        });
        b_mextend(r + 1, q0, q1, e >> r, 1, s, mont);
        foreach_n(s, e, [=] __device__(size_t g) { dst[2 * g] = q0[g]; dst[2 * g + 1] = q1[g]; });
    }

    // matrix-core tables of the innermost 16-point map (mfma_blk16.h), per source parity: 32-byte fields, trees with e >= 16
    static size_t blk16_elems(unsigned l) { return (sizeof(E) == 32 && l >= 5) ? 2 * (Blk16::kArenaElems + 8) : 0; }
    void build_blk16(Tree& T, hipStream_t s) {
        T.blk16_A[0] = T.blk16_A[1] = nullptr; T.blk16_K[0] = T.blk16_K[1] = nullptr;
        if constexpr (sizeof(E) == 32) {
            if (T.e < 16 || mfma_off_) return;
            Blk16BuildArgs ba[2];
            for (int sg = 0; sg < 2; ++sg) {
                uint8_t* A = reinterpret_cast<uint8_t*>(take(Blk16::kArenaElems));
                unsigned long long* K = reinterpret_cast<unsigned long long*>(A + Blk16::kABytes);
                ba[sg] = {T.np0[sg], T.dinv[sg], T.p0[1 - sg], T.p1[1 - sg], T.inner[sg], A, K};
                T.blk16_A[sg] = A; T.blk16_K[sg] = K;
            }
            hipLaunchKernelGGL(k_blk16_build, dim3(2), dim3(256), 0, s, ba[0], ba[1], T.e);       // both source parities in one launch
        }
    }

    // The four lowest levels of ENTER and of EXIT as ONE 16 x 16 map each for the matrix cores (LevelTables::low16_A, read by the
    // 1024-element low-level kernels): every 16-block of a transform goes through the same levels on the same tables, so the maps
    // are the images of the 16 unit vectors under this context's own level code (16 transforms of 16 points in one batched call).
    static size_t low16_elems() { return sizeof(E) == 32 ? 2 * (Blk16::kArenaElems + 8) + 2 * (Blk16::kArenaElems32 + 8) : 0; }   // + the two low32 maps
    bool build_low16(unsigned l_top, hipStream_t s) {
        if constexpr (sizeof(E) == 32) {
            if (l_top < kLogLowSmall || mfma_off_ || low16_off_) return true;
            Tree& T = trees_[4];
            E* I = temp(256); E* O = temp(256);
            foreach_n(s, 256, [=] __device__(size_t j) { I[j] = ((j >> 4) == (j & 15)) ? F::one() : F::zero(); });
            for (int dir = 0; dir < 2; ++dir) {
                if (dir == 0) enter_levels(I, O, 16, 16, s, scratch_, 1, 4); else exit_levels(I, O, 16, 16, s, scratch_, 4, 1);
                uint8_t* A = reinterpret_cast<uint8_t*>(take(Blk16::kArenaElems));
                unsigned long long* K = reinterpret_cast<unsigned long long*>(A + Blk16::kABytes);
                hipLaunchKernelGGL(k_blk16_from_matrix, dim3(1), dim3(256), 0, s, O, A, K, true);
                T.low16_A[dir] = A; T.low16_K[dir] = K;
            }
            // round 4: the FIVE lowest levels as one 32 x 32 map per 32-block, for the 1024-element low-level kernels (low32_mask_:
            // bit 0 ENTER, bit 1 EXIT) — the images of the 32 unit vectors under the level code (32 transforms of 32 points)
            if (l_top >= kLogLow && low32_mask_) {
                Tree& T5 = trees_[5];
                E* I32 = temp(1024); E* O32 = temp(1024); E* CS = temp(1024);
                foreach_n(s, 1024, [=] __device__(size_t j) { I32[j] = ((j >> 5) == (j & 31)) ? F::one() : F::zero(); });
                for (int dir = 0; dir < 2; ++dir) {
                    if (!((low32_mask_ >> dir) & 1u)) continue;
                    if (dir == 0) enter_levels(I32, O32, 32, 32, s, scratch_, 1, 5); else exit_levels(I32, O32, 32, 32, s, scratch_, 5, 1);
                    uint8_t* A = reinterpret_cast<uint8_t*>(take(Blk16::kArenaElems32));
                    unsigned long long* K = reinterpret_cast<unsigned long long*>(A + Blk16::kABytes32);
                    hipLaunchKernelGGL(k_blk32_expand, dim3(4), dim3(256), 0, s, (const E*)O32, A, CS, true);
                    hipLaunchKernelGGL(k_blk32_seeds, dim3(1), dim3(32), 0, s, (const E*)CS, K);
                    T5.low32_A[dir] = A; T5.low32_K[dir] = K;
                }
            }
        }
        return hipGetLastError() == hipSuccess;
    }

    bool build_tree(unsigned l, hipStream_t s) {
        Tree& T = trees_[l];
        size_t m = (size_t)1 << l, e = m / 2;
        T.m = m; T.e = e; T.log_m = l;
        const E* f = f_; size_t N = N_; size_t stride = N_ / m;
        // symmetric basis: the stage tables hold sigma_k = (x - c1_k)/(x - c2_k) of the layer points instead of the points
        // (then p1 = -p0), and the weights carry one factor (s_k - c2_k) per layer more; every derived table follows from these
        const bool sym = sym_; const E* crit = crit_;
        T.xnn = take(m); T.xnn_inv = take(m);
        {
            E* xnn = T.xnn; uint64_t ex = m / 2;
            foreach_n(s, m, [=] __device__(size_t j) { xnn[j] = F::pow_u64(f[N + j * stride], ex); });
            if (l == 0) batch_inv(T.xnn, T.xnn_inv, m, s);      // otherwise inverted together with the stage tables below
        }
        if (l == 0) return true;
        unsigned le = ilog2(e);
        size_t es = e > 1 ? e : 1;
        // plain values first (temporaries), then the kernels' table form in the arena
        E *hp0[2], *hp1[2], *hnp0[2], *hdinv[2], *hw[2], *hwinv[2];
        for (int sg = 0; sg < 2; ++sg) {
            hp0[sg] = temp(es); hp1[sg] = temp(es); hnp0[sg] = temp(es); hdinv[sg] = temp(es);
            hw[sg] = temp(es); hwinv[sg] = temp(es);
            E *p0 = hp0[sg], *p1 = hp1[sg], *np0 = hnp0[sg], *dinv = hdinv[sg];
            if (e > 1) {
                // entry g of the concatenated stage tables: stage k = number of leading ones ... computed by scan
                foreach_n(s, e - 1, [=] __device__(size_t g) {
                    // stage k occupies [e - 2h, e - h), h = e >> (k+1)
                    size_t rem = e - g;                       // in (h, 2h]
                    unsigned k = 0; size_t h = e >> 1;
                    while (rem <= h) { h >>= 1; ++k; }
                    size_t i = g - (e - 2 * h);
                    size_t lay = N >> k;                      // offset (= size) of layer k in the top tree
                    E a = f[lay + (2 * i + sg) * stride];
                    E b = f[lay + (2 * i + sg + 2 * h) * stride];
                    if (sym) {      // u = a - c1, v = a - c2 and 2uv: ONE inverse gives sigma(a) = u/v and -1/(2 sigma(a)) below
                        const E u = F::sub(a, crit[2 * k]), v = F::sub(a, crit[2 * k + 1]), uv = F::mul(u, v);
                        p0[g] = u; p1[g] = v; dinv[g] = F::add(uv, uv);
                        return;
                    }
                    p0[g] = a; p1[g] = b; np0[g] = F::neg(a); dinv[g] = F::sub(b, a);
                });
            }
            // normalisation weights W(s) of the leaves of parity sg (DESIGN.md "Normalised butterflies")
            E* w = hw[sg]; const E* den = den_;
            foreach_n(s, e, [=] __device__(size_t i) {
                size_t j = 2 * i + sg;
                E U = F::one(), C = F::one();
                for (unsigned b = 0; b + 1 < le; ++b) {
                    size_t lsz = m >> b;                      // |L_b| of T_m
                    E sb = f[(N >> b) + (j & (lsz - 1)) * stride];
                    E V = F::mul_add(den[2 * b + 1], sb, den[2 * b]);
                    C = F::mul(C, V);
                    U = F::mul(F::sqr(U), C);
                }
                if (sym) {      // W' = W * prod over ALL le layers of (s_b - c2_b)
                    for (unsigned b = 0; b < le; ++b) {
                        size_t lsz = m >> b;
                        U = F::mul(U, F::sub(f[(N >> b) + (j & (lsz - 1)) * stride], crit[2 * b + 1]));
                    }
                }
                w[i] = U;
            });
        }
        E *xq = nullptr, *xqi = nullptr;                        // X^(m/4) on the leaves of T_m and its inverse (src/fftree.rs:328-330), used below
        if (l >= 2) { xq = temp(m); xqi = temp(m); E* q = xq; uint64_t ex = m / 4; foreach_n(s, m, [=] __device__(size_t j) { q[j] = F::pow_u64(f[N + j * stride], ex); }); }
        {   // 1/xnn_s, 1/(s1 - s0) and 1/W of both parities, 1/X^(m/4): six independent arrays, ONE inversion launch
            const InvSeg segs[6] = {{T.xnn, T.xnn_inv, m}, {hdinv[0], hdinv[0], e - 1}, {hdinv[1], hdinv[1], e - 1}, {hw[0], hwinv[0], e}, {hw[1], hwinv[1], e},
                                    {xq, xqi, l >= 2 ? m : 0}};
            batch_inv_multi(segs, 6, s);
        }
        if (sym && e > 1) {     // r = 1/(2uv): sigma(a) = 2 u^2 r, sigma(b) = -sigma(a), 1/(sigma(b) - sigma(a)) = -v^2 r
            for (int sg = 0; sg < 2; ++sg) {
                E *p0 = hp0[sg], *p1 = hp1[sg], *np0 = hnp0[sg], *dinv = hdinv[sg];
                foreach_n(s, e - 1, [=] __device__(size_t g) {
                    const E u = p0[g], v = p1[g], r = dinv[g];
                    const E u2 = F::sqr(u), sg0 = F::mul(F::add(u2, u2), r), nsg = F::neg(sg0);
                    p0[g] = sg0; p1[g] = nsg; np0[g] = nsg; dinv[g] = F::neg(F::mul(F::sqr(v), r));
                });
            }
        }
        // merged innermost stage pair (h = 1, stage k = le-1): out_j = a + c_j*(b - a) with
        // c_j = (p_j^target - p_0^source) / (p_1^source - p_0^source), table offset e-2 (kernels.h)
        for (int sg = 0; sg < 2; ++sg) {
            E* in = temp(2);
            if (e > 1) {
                const E *sp0 = hp0[sg] + (e - 2), *sdi = hdinv[sg] + (e - 2), *tp0 = hp0[1 - sg] + (e - 2), *tp1 = hp1[1 - sg] + (e - 2);
                foreach_n(s, 1, [=] __device__(size_t) {
                    in[0] = F::mul(F::sub(tp0[0], sp0[0]), sdi[0]);
                    in[1] = F::mul(F::sub(tp1[0], sp0[0]), sdi[0]);
                });
            } else {
                (void)hipMemsetAsync(in, 0, 2 * sizeof(E), s);
            }
            T.inner[sg] = to_tables(in, 2, s);
        }
        for (int sg = 0; sg < 2; ++sg) {   // c0t = np0 * dinv (pair-split decompose, kernels.h lds_extend_core)
            E* c0 = temp(es);
            if (e > 1) { const E *n0 = hnp0[sg], *di = hdinv[sg]; foreach_n(s, e - 1, [=] __device__(size_t g) { c0[g] = F::mul(n0[g], di[g]); }); }
            else (void)hipMemsetAsync(c0, 0, sizeof(E), s);
            if (e > 1) (void)hipMemsetAsync(c0 + (e - 1), 0, sizeof(E), s);
            T.c0t[sg] = to_tables(c0, es, s);
        }
        for (int sg = 0; sg < 2; ++sg) {
            if (e == 1) {   // no butterfly stage: the (never read) stage tables still get defined contents
                (void)hipMemsetAsync(hp0[sg], 0, sizeof(E), s); (void)hipMemsetAsync(hp1[sg], 0, sizeof(E), s);
                (void)hipMemsetAsync(hnp0[sg], 0, sizeof(E), s); (void)hipMemsetAsync(hdinv[sg], 0, sizeof(E), s);
            }
            T.p0[sg] = to_tables(hp0[sg], es, s); T.p1[sg] = to_tables(hp1[sg], es, s);
            T.np0[sg] = to_tables(hnp0[sg], es, s); T.dinv[sg] = to_tables(hdinv[sg], es, s);
            T.w[sg] = to_tables(hw[sg], es, s); T.winv[sg] = to_tables(hwinv[sg], es, s);
        }
        build_blk16(T, s);
        T.z0_s1 = take(es); T.z1_s0 = take(es); T.z0_inv_s1 = take(es); T.z1_inv_s0 = take(es);
        T.z0z0 = take(m); T.z1z1 = take(m);
        if (l == 1) {                                          // base cases src/fftree.rs:399-403, 454-458
            E *z0 = T.z0_s1, *z1 = T.z1_s0, *zz0 = T.z0z0, *zz1 = T.z1z1;
            foreach_n(s, 1, [=] __device__(size_t) {
                E s0 = f[N], s1 = f[N + stride];
                z0[0] = F::sub(s1, s0); z1[0] = F::sub(s0, s1);
                zz0[0] = zz0[1] = F::sqr(s0); zz1[0] = zz1[1] = F::sqr(s1);
            });
        } else {
            const Tree& S = trees_[l - 1];
            // z0_s1 (src/fftree.rs:386-393)
            E* a = temp(e); E* b = temp(e);
            {
                const E *sz0 = S.z0_s1, *sz1 = S.z1_s0;
                foreach_n(s, e / 2, [=] __device__(size_t i) {
                    a[2 * i] = F::zero(); a[2 * i + 1] = sz0[i];
                    b[2 * i] = sz1[i]; b[2 * i + 1] = F::zero();
                });
            }
            b_extend(l, a, a, 1, 1, s);
            b_extend(l, b, b, 1, 1, s);
            ew_mul(T.z0_s1, a, b, e, s);
            // z1_s0 = vanish(S1)[even]  (src/fftree.rs:396-397)
            E* s1 = temp(e); E* van = temp(m);
            foreach_n(s, e, [=] __device__(size_t i) { s1[i] = f[N + (2 * i + 1) * stride]; });
            b_vanish(l, s1, van, s);
            { E* z1 = T.z1_s0; foreach_n(s, e, [=] __device__(size_t i) { z1[i] = van[2 * i]; }); }
        }
        { const InvSeg segs[2] = {{T.z0_s1, T.z0_inv_s1, e}, {T.z1_s0, T.z1_inv_s0, e}}; batch_inv_multi(segs, 2, s); }
        if (l >= 2) {
            const Tree& S = trees_[l - 1];
            // a0inv / a1 views of xnn_s for REDC on this tree and on the subtree
            E* xa0i = temp(e); E* xa1 = temp(e);
            { const E *xi = T.xnn_inv, *x = T.xnn; foreach_n(s, e, [=] __device__(size_t i) { xa0i[i] = xi[2 * i]; xa1[i] = x[2 * i + 1]; }); }
            E* sxa0i = temp(e / 2 ? e / 2 : 1); E* sxa1 = temp(e / 2 ? e / 2 : 1);
            { const E *xi = S.xnn_inv, *x = S.xnn; foreach_n(s, e / 2, [=] __device__(size_t i) { sxa0i[i] = xi[2 * i]; sxa1[i] = x[2 * i + 1]; }); }
            // X^(m/4) tables on the leaves of T_m (src/fftree.rs:328-330)
            E* xqa0i = temp(e); E* xqa1 = temp(e);
            foreach_n(s, e, [=] __device__(size_t i) { xqa0i[i] = xqi[2 * i]; xqa1[i] = xq[2 * i + 1]; });
            // z0z0_rem_xnn_s (src/fftree.rs:418-446)
            E* sq = temp(e); E* zz0 = temp(e); E* zz1 = temp(e); E* zz = temp(m); E* tmp = temp(m); E* dr = temp(m);
            ew_mul(sq, S.z0z0, S.z1z1, e, s);                                       // :421-423
            b_modular_reduce(l - 1, sq, sxa0i, sxa1, S.z0z0, zz0, s);               // :424-425
            b_extend(l, zz0, zz1, 1, 1, s);                                         // :426
            foreach_n(s, e, [=] __device__(size_t i) { zz[2 * i] = zz0[i]; zz[2 * i + 1] = zz1[i]; });
            {
                const E *z0s1 = T.z0_s1, *xnn = T.xnn;
                foreach_n(s, m, [=] __device__(size_t i) {                           // :430-438
                    E z0 = (i & 1) ? z0s1[i / 2] : F::zero();
                    E y = F::sub(z0, xnn[i]);
                    tmp[i] = F::mul(F::sub(F::sqr(y), zz[i]), xqi[i]);
                });
            }
            b_modular_reduce(l, tmp, xqa0i, xqa1, zz, dr, s);                        // :439-440
            { E* o = T.z0z0; foreach_n(s, m, [=] __device__(size_t i) { o[i] = F::mul_add(xq[i], dr[i], zz[i]); }); } // :441-446
            // z1z1_rem_xnn_s (src/fftree.rs:449-452)
            {
                const E *z1s0 = T.z1_s0, *xnn = T.xnn;
                foreach_n(s, m, [=] __device__(size_t i) {
                    E z1 = (i & 1) ? F::zero() : z1s0[i / 2];
                    tmp[i] = F::sqr(F::sub(z1, xnn[i]));
                });
            }
            b_modular_reduce(l, tmp, xa0i, xa1, T.z0z0, T.z1z1, s);
        }
        // fused pointwise tables of the hot path
        {
            E *xe = temp(es), *w1x = temp(es), *A1 = temp(es), *B1 = temp(es), *NB2 = temp(es), *C1 = temp(es), *D1 = temp(es), *xie = temp(es);
            const E *xnn = T.xnn, *xi = T.xnn_inv, *w1 = hw[1], *wi0 = hwinv[0], *wi1 = hwinv[1], *zi = T.z0_inv_s1, *c = T.z0z0;
            foreach_n(s, e, [=] __device__(size_t i) {
                E xo = xnn[2 * i + 1], xiev = xi[2 * i], z = zi[i];
                xe[i] = xnn[2 * i];
                w1x[i] = F::mul(w1[i], xo);
                xie[i] = xiev;
                A1[i] = F::mul(xiev, wi0[i]);
                B1[i] = F::mul(z, wi1[i]);
                NB2[i] = F::neg(F::mul(xo, z));
                C1[i] = F::mul(c[2 * i], xiev);
                D1[i] = F::mul(c[2 * i + 1], z);
            });
            T.xe = to_tables(xe, es, s); T.w1x = to_tables(w1x, es, s); T.xie = to_tables(xie, es, s);
            // a context holds ONE fused EXIT set per tree: the Z1 set where exit_levels runs the three-core form, the Z0 set where
            // it runs the four-core form; the trees k_exit_low covers (at most 2^kLogLow leaves) keep both: its loop runs the
            // context's form on the Z1 set, and the four-core kernel under a three-core driver (ECFFT_EXIT_LOW_CORES=4, A/B) the Z0 set
            if (!exit3_ || l <= kLogLow) {
                T.A1 = to_tables(A1, es, s); T.B1 = to_tables(B1, es, s); T.NB2 = to_tables(NB2, es, s); T.C1 = to_tables(C1, es, s); T.D1 = to_tables(D1, es, s);
            }
            if (exit3_) {
                // reduction over Z1 (c' = z1z1_rem_xnn_s): t1~ = e1 (xinv_odd/W1); h0~ = e0 (z1inv/W0) - g0~ (x_even z1inv);
                // t1'~ = h1~ (c'_odd xinv_odd); u0 = H (c'_even z1inv W0) - g0'~ (x_even z1inv W0)
                const E *w0 = hw[0], *z1i = T.z1_inv_s0, *c1 = T.z1z1;
                foreach_n(s, e, [=] __device__(size_t i) {
                    const E xev = xnn[2 * i], xiod = xi[2 * i + 1], z = z1i[i], zw = F::mul(z, w0[i]);
                    A1[i] = F::mul(xiod, wi1[i]);
                    B1[i] = F::mul(z, wi0[i]);
                    NB2[i] = F::neg(F::mul(xev, z));
                    C1[i] = F::mul(c1[2 * i + 1], xiod);
                    D1[i] = F::mul(c1[2 * i], zw);
                    xe[i] = F::neg(F::mul(xev, zw));       // xe is in its table form already: the temporary is free
                });
                T.zA1 = to_tables(A1, es, s); T.zB1 = to_tables(B1, es, s); T.zNB2 = to_tables(NB2, es, s); T.zC1 = to_tables(C1, es, s);
                T.zD1 = to_tables(D1, es, s); T.zNB3 = to_tables(xe, es, s);
            }
        }
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) { fprintf(stderr, "ecfft: kernel launch failed: %s\n", hipGetErrorString(err)); return false; }
        // temporaries are only needed until the stream drains; free them per tree to bound memory
        if (hipStreamSynchronize(s) != hipSuccess) return false;
        temps_free();
        slab_used_ = 0;
        return true;
    }

    HostTree<F> host_;
    E rinv_ = F::inv(F::to_mont(F::one()));   // R^-1 as a plain residue (1 for M31)
    static E crate_one() { return F::to_mont(F::one()); }   // R, the crate's 1
    TE rinv_table() const { return F::to_table(rinv_); }    // R^-1 in the form the table multiply takes
    size_t N_ = 0; unsigned L_ = 0; int device_ = 0;
    E* arena_ = nullptr; size_t arena_cap_ = 0, arena_used_ = 0;
    E* f_ = nullptr; E* den_ = nullptr; E* scratch_ = nullptr; size_t scratch_cap_ = 0;
    E* slab_ = nullptr; size_t slab_cap_ = 0, slab_used_ = 0;
    std::vector<Tree> trees_;
    Tree* d_trees_ = nullptr;
    struct PoolBuf { void* p; size_t bytes; bool busy; bool pinned; unsigned idle_calls; };
    std::set<uint64_t> agreed_shapes_;                // (op, variant, world, len) of the collective calls the ranks have voted on
    bool fail_next_collective_ = false;
    std::vector<PoolBuf> pool_;
    std::mutex mu_;
    mutable Profiler prof_;
    hipStream_t sides_[kMaxSides] = {}; hipEvent_t ev_fork_[kMaxSides] = {}, ev_join_[kMaxSides] = {}; int nside_ = 0;
    bool bad_points_ = false;
    int shard_kind_ = kShardNone;                           // sharded EXTEND-only / ENTER-only context (build_*_shard)
    unsigned shard_log_p_ = 0, shard_rank_ = 0;
    std::vector<ShardSet> sets_;                            // per tree: the rank's share of its EXTEND tables (shard contexts)
    const Tree* ovr_tree_ = nullptr; const ShardSet* ovr_set_ = nullptr;   // temporary share of one tree (sharded EXIT build)
    mutable double tblw_ = 1.0;     // weight of table bytes in the algorithmic-byte accounting (see enter())
    mutable std::map<uint64_t, TE*> full_cyc_; mutable size_t full_cyc_bytes_ = 0;   // compact cyclic tables of a FULL context (full_cyclic_table)
    bool full_cyc_off_ = ab_env("ECFFT_NO_FULL_CYCLIC") != nullptr;      // A/B switch: one-stage launches with stride-P table reads
    // bit 0: ENTER levels 1..5, bit 1: EXIT levels 5..1 as one 32-point map (low32).  OFF by default: measured on MI355X (profiles/r04/low32_ab.txt)
    // the 32-point phase costs what it removes — level 5 is four 16-point phases + five pointwise steps (~35 us per tile), the phase
    // streams 1 MiB of matrices per tile and runs twice the MFMAs of low16 (k_exit_low 1.63 -> 1.65-1.69 ms, k_enter_low 0.66 -> 0.66)
    unsigned low32_mask_ = ab_env("ECFFT_LOW32") ? (unsigned)atoi(ab_env("ECFFT_LOW32")) : 0u;
    bool low16_off_ = ab_env("ECFFT_NO_LOW16") != nullptr;             // A/B switch: the four lowest ENTER / EXIT levels as VALU sweeps
    bool mfma_off_ = ab_env("ECFFT_NO_MFMA") != nullptr;                // A/B switch: innermost stages on the VALU instead of the matrix cores
    unsigned small_min_logc_ = ab_env("ECFFT_SMALL_MIN_LOGC") ? (unsigned)atoi(ab_env("ECFFT_SMALL_MIN_LOGC")) : 1u;   // log2 of the shortest column-tile row of a small launch (rows of 2 elements: 7 stages in one pass; A/B knob)
    bool in_halves_ = false;                                            // enqueueing the two-halves schedule of one transform (caller holds lock())
    Tree pair_full_{}; bool have_pair_full_ = false;                    // EXIT-shard contexts: the full tree T_2c (c = n / world) of the redundant pair level
    // full contexts: split EXITs of at most 2^this run every top level redundantly after one all-gather (0: never) — api_exit_split
    unsigned gather_max_log_ = ab_env("ECFFT_SPLIT_GATHER_MAX_LOG") ? (unsigned)atoi(ab_env("ECFFT_SPLIT_GATHER_MAX_LOG")) : 21u;
    // link striping of the big pairwise exchanges (Transport::exchange_striped): staging of the call in flight; A/B switches (test builds)
    mutable void* stripe_stage_ = nullptr; mutable size_t stripe_bytes_ = 0;
    struct StripeScope { const DeviceChain* ch; StripeScope(const DeviceChain* c, void* p, size_t b) : ch(c) { ch->stripe_stage_ = p; ch->stripe_bytes_ = p ? b : 0; }
                         ~StripeScope() { ch->stripe_stage_ = nullptr; ch->stripe_bytes_ = 0; } };
    bool stripe_off_ = ab_env("ECFFT_NO_STRIPE") != nullptr;
    size_t stripe_gain_ = ab_env("ECFFT_STRIPE_MIN_GAIN") ? (size_t)atoll(ab_env("ECFFT_STRIPE_MIN_GAIN")) : ~(size_t)0;
    bool q2_split_ = ab_env("ECFFT_SPLIT_Q2_SPLIT") != nullptr;        // A/B switch (full contexts): the pair level of a split EXIT as four split EXTENDs
    bool col256_off_ = ab_env("ECFFT_NO_COL256") != nullptr;            // A/B switch: small column passes on the generic kernels (pair-split LDS sweeps)
    bool row256_off_ = ab_env("ECFFT_NO_ROW256") != nullptr;            // A/B switch: small row passes on the generic kernel (pair-split LDS sweeps)
    bool ef_small_off_ = ab_env("ECFFT_NO_SMALL_TILES") != nullptr;   // A/B switch for the small-launch tile rule
    // EXIT levels of exit_levels: three EXTEND cores (reduction over Z1) unless the build (-DECFFT_EXIT_CORES=4) or the A/B switch asks
    // for the reference's four; exit3_ = the form this context's tables were built for (full contexts whose leaves are all non-zero)
    bool exit4_ = ECFFT_EXIT_CORES == 4 || ab_env("ECFFT_EXIT_FOUR_CORES") != nullptr;
    bool exit3_ = false;
    bool exit_low4_ = ab_env("ECFFT_EXIT_LOW_FOUR_CORES") != nullptr;   // A/B switch: k_exit_low keeps four cores per level in a three-core context
    // symmetric butterflies: sym_ = this context's stage tables and weights are written in the symmetric basis (the
    // library's own tree of a 32-byte field, full contexts only); the row and column passes of the full-size regime then run
    // sym_bfly unless the A/B switch keeps the general kernels on the symmetric tables.  -DECFFT_SYM_BFLY=0 builds the general basis
    // throughout, ECFFT_NO_SYM_BFLY=1 selects it per context in the hooks build.
    E* crit_ = nullptr;                                                 // critical points (c1, c2) of the maps, per layer
    bool sym_ = false;
    bool sym_off_ = ab_env("ECFFT_NO_SYM_BFLY") != nullptr;
    bool sym_general_kernels_ = ab_env("ECFFT_SYM_BFLY_GENERAL_KERNELS") != nullptr;
    bool sym_kernels() const { return sym_ && !sym_general_kernels_; }
    bool low_general_kernels_ = ab_env("ECFFT_LOW_GENERAL_KERNELS") != nullptr;   // A/B switch: general low-level kernels under symmetric row and column passes
    // (a context of the four-core A/B form, exit4_, keeps the general low-level kernels as well: it is the reference form throughout)
    bool low_sym_enter() const { return sym_kernels() && !low_general_kernels_ && !exit4_; }
    bool low_sym_exit() const { return low_sym_enter() && exit_low_cores() == 3; }
    // ENTER level 11 on the compile-time row engine (extend_core): full contexts of a 32-byte field whose tree has matrix-core tables
    bool enter_l11_generic_ = ab_env("ECFFT_ENTER_L11_GENERIC") != nullptr;   // A/B switch: that level on the run-time-tile row kernel
    bool enter_l11_tuned(const Tree& T, int srcpar) const { return kEnterL11 && !enter_l11_generic_ && !mfma_off_ && !shard_mode() && T.blk16_A[srcpar] != nullptr; }
};

}  // namespace ecfft
