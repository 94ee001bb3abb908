// Search for a curve y^2 = x(x^2 + a x + bb) whose group has a large cyclic 2-subgroup: the reference's find_curve
// (src/find_curve.rs:224-246, FIND_CURVE of ECFFT part II) and cyclic_two_sylow_subgroup (:190-218) with its
// helpers half_point_x / fi_roots / roots / double_point_x (:11-56).
//
// One body for both fields.  The Sylow computation is cut into STEPS (sylow_bb_square, sylow_disc_nonsquare, sylow_order4,
// sylow_halve), each __host__ __device__ and templated on the field.  sylow_host runs them one after another for one curve (the
// CPU baseline, tests/cpp/curve_host.cpp under the sanitizers); on the GPU each step is one STAGE kernel over a dense device
// queue: half the candidates die at every test, so a thread per candidate would leave most lanes of a wave idle inside
// exponentiations of ~270 multiplies.  A stage reads queue entries 0 .. len-1, and every wave appends its survivors to the next
// queue with one ballot and one vector atomic add; the host reads the new length between stages.  Every launch therefore runs
// full waves except the tail of its queue.
//
// Conventions that make the result bit-exact (include/ecfft_hip.h): every square root is v^((p+1)/4) (F::sqrt_canon; both
// fields have p = 3 mod 4), accepted when its square is v, so 0 counts as a square; the two roots of a quadratic are tried in
// the order (-b + s)/2, (-b - s)/2.  Nothing needs an inversion: 1/2 is a constant and double_point_x is only tested for None.
// Everything is in PLAIN form, like host_curve.h.
#pragma once
#include <stdint.h>
#include "field_secp256k1.h"
#include "field_m31.h"

namespace ecfft {
namespace curve {

// ---- the candidate stream (include/ecfft_hip.h ecfft_find_curve_candidate) -------------------------------------------
__host__ __device__ static inline uint64_t stream_word(uint64_t seed, uint64_t c) {
    uint64_t z = seed + (c + 1) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// the element made of the words c0 .. c0+3 (secp256k1: 256 bits < 2p, one conditional subtraction) or of word c0 (M31)
template <class F>
__host__ __device__ static inline typename F::elem stream_elem(uint64_t seed, uint64_t c0) {
    if constexpr (sizeof(typename F::elem) == 4) {
        const uint32_t v = (uint32_t)stream_word(seed, c0) & 0x7FFFFFFFu;
        return v == M31::P ? 0u : v;
    } else {
        uint32_t s[8];
        for (int j = 0; j < 4; ++j) { const uint64_t w = stream_word(seed, c0 + j); s[2 * j] = (uint32_t)w; s[2 * j + 1] = (uint32_t)(w >> 32); }
        return Secp256k1::finish(s, 0);
    }
}
constexpr uint64_t kMaxIndex = 1ull << 60;        // 8 * index + 7 stays inside 64 bits

// ---- the steps of cyclic_two_sylow_subgroup ---------------------------------------------------------------------------
template <class F>
struct Cand {                  // one live candidate: its curve, the x-coordinate reached so far and where it came from
    typename F::elem a, bb, acc;
    uint64_t idx;
};

template <class F>
__host__ __device__ static inline bool is_square(const typename F::elem& v, typename F::elem* root) {
    const typename F::elem r = F::sqrt_canon(v);
    *root = r;
    return F::eq(F::sqr(r), v);
}
template <class F>
__host__ __device__ static inline typename F::elem dbl(const typename F::elem& v) { return F::add(v, v); }
// x (x^2 + a x + bb): y^2 of the point with that x
template <class F>
__host__ __device__ static inline typename F::elem rhs(const typename F::elem& x, const typename F::elem& a, const typename F::elem& bb) {
    return F::mul(x, F::add(F::mul(F::add(x, a), x), bb));
}

// step 0: bb = b^2 with b != 0 (acc <- b).  bb = 0 is a singular curve: 0, where the reference asserts.
template <class F>
__host__ __device__ static inline bool sylow_bb_square(Cand<F>& c) {
    if (F::is_zero(c.bb)) return false;
    return is_square<F>(c.bb, &c.acc);
}
// step 1: the discriminant a^2 - 4 bb is no square, so (0, 0) is the only point of order 2 and the 2-Sylow subgroup is cyclic
// (:195).  A zero discriminant is a singular curve: 0.
template <class F>
__host__ __device__ static inline bool sylow_disc_nonsquare(const Cand<F>& c) {
    typename F::elem s;
    const typename F::elem disc = F::sub(F::sqr(c.a), dbl<F>(dbl<F>(c.bb)));
    return !is_square<F>(disc, &s);                                  // sqrt_canon(0) = 0 squares to 0: rejected too
}
// step 2: the point of order 4 (:197-205): x = b when a + 2b is a square, else -b (then a - 2b is one, because their product is
// the discriminant, no square).  false = the reference's (1, 0) exit: double_point_x is None, y^2 = 0.
template <class F>
__host__ __device__ static inline bool sylow_order4(Cand<F>& c) {
    typename F::elem s;
    const typename F::elem b = c.acc;
    if (!is_square<F>(F::add(c.a, dbl<F>(b)), &s)) c.acc = F::neg(b);
    return !F::is_zero(rhs<F>(c.acc, c.a, c.bb));
}
// step 3, once per halving round: half_point_x (:25-31).  true: acc <- the x of a half point.
template <class F>
__host__ __device__ static inline bool sylow_halve(Cand<F>& c, const typename F::elem& half) {
    using E = typename F::elem;
    const E qx = c.acc;
    E ds, sd;
    if (!is_square<F>(F::add(F::mul(F::add(qx, c.a), qx), c.bb), &ds)) return false;       // delta = qx^2 + a qx + bb (:51-52)
    // fi_roots(1).or_else(fi_roots(2)): x^2 + cx x + bb with cx = -(2 qx -/+ 2 sqrt(delta)); the SECOND polynomial is tried only
    // when the first has no roots, not when its roots fail the test below
    E mb = dbl<F>(F::sub(qx, ds));                                                         // -cx for i = 1
    const E bb4 = dbl<F>(dbl<F>(c.bb));
    if (!is_square<F>(F::sub(F::sqr(mb), bb4), &sd)) {
        mb = dbl<F>(F::add(qx, ds));                                                       // -cx for i = 2
        if (!is_square<F>(F::sub(F::sqr(mb), bb4), &sd)) return false;
    }
    E s;
    const E r0 = F::mul(F::add(mb, sd), half);
    if (is_square<F>(rhs<F>(r0, c.a, c.bb), &s)) { c.acc = r0; return true; }
    const E r1 = F::mul(F::sub(mb, sd), half);
    if (is_square<F>(rhs<F>(r1, c.a, c.bb), &s)) { c.acc = r1; return true; }
    return false;
}

// halving rounds any curve can survive: the group has fewer than 2p + 2 points, so n < 8 * bytes + 2
template <class F> constexpr unsigned kMaxRounds = 8 * F::kBytes + 2;

// cyclic_two_sylow_subgroup for one curve: n (0 = not cyclic, bb no square or a singular curve) and the x of a point of order 2^n
template <class F>
__host__ static inline uint32_t sylow_host(const typename F::elem& a, const typename F::elem& bb, const typename F::elem& half,
                                           typename F::elem* x) {
    Cand<F> c{a, bb, F::zero(), 0};
    *x = F::zero();
    if (!sylow_bb_square<F>(c) || !sylow_disc_nonsquare<F>(c)) return 0;
    if (!sylow_order4<F>(c)) return 1;
    uint32_t n = 2;
    for (unsigned r = 0; r < kMaxRounds<F> && sylow_halve<F>(c, half); ++r) ++n;
    *x = c.acc;
    return n;
}

#if defined(__HIPCC__)
// ---- the stages ---------------------------------------------------------------------------------------------------------
enum { STAGE_BB = 0, STAGE_DISC = 1, STAGE_ORDER4 = 2, STAGE_HALVE = 3 };
enum { FLAG_QUEUE_FULL = 1 };

template <class F>
struct StageArgs {
    const Cand<F>* in; Cand<F>* out;         // queues (STAGE_BB has no input queue: it reads the source below)
    unsigned in_len, cap;                    // entries to read; capacity of `out` (>= in_len: a stage never makes candidates)
    unsigned* out_len;                       // zero before the launch
    unsigned* flags;
    // source of STAGE_BB: the arrays a_in / bb_in (entry i is curve base + i), or the stream `seed` from index `base` when they are null
    const typename F::elem *a_in, *bb_in;
    uint64_t seed, base;
    // where a candidate that dies with n >= 1 is recorded: per curve (n_out / x_out, entry idx - base; zero-filled before, so
    // n = 0 writes nothing) and / or the smallest index with n >= k_min (`best`)
    uint32_t* n_out; typename F::elem* x_out;
    unsigned long long* best;
    uint32_t k_min;
    uint32_t n_now;                          // what a candidate that dies in this launch has reached
    typename F::elem half;
};

template <class F>
__device__ static inline void record(const StageArgs<F>& g, const Cand<F>& c, uint32_t n, const typename F::elem& x) {
    if (g.n_out) { g.n_out[c.idx - g.base] = n; g.x_out[c.idx - g.base] = x; }
    if (g.best && n >= g.k_min) atomicMin(g.best, (unsigned long long)c.idx);
}

template <class F, int STAGE>
__global__ __launch_bounds__(256) void k_stage(const StageArgs<F> g) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    const bool active = i < g.in_len;                     // idle lanes of the tail stay for the ballot
    Cand<F> c;
    bool keep = false;
    if (active) {
        if constexpr (STAGE == STAGE_BB) {
            c.idx = g.base + i;
            if (g.a_in) { c.a = g.a_in[i]; c.bb = g.bb_in[i]; }
            else { c.a = stream_elem<F>(g.seed, 8 * c.idx); c.bb = stream_elem<F>(g.seed, 8 * c.idx + 4); }
            keep = sylow_bb_square<F>(c);
        } else {
            c = g.in[i];
            if constexpr (STAGE == STAGE_DISC) keep = sylow_disc_nonsquare<F>(c);
            else if constexpr (STAGE == STAGE_ORDER4) { keep = sylow_order4<F>(c); if (!keep) record<F>(g, c, 1, F::zero()); }
            else { const typename F::elem x = c.acc; keep = sylow_halve<F>(c, g.half); if (!keep) record<F>(g, c, g.n_now, x); }
        }
    }
    // append the wave's survivors: one ballot, one atomic add by its first surviving lane
    const unsigned long long m = __ballot(keep);
    if (m == 0) return;
    const unsigned lane = __lane_id();
    const int leader = __ffsll((long long)m) - 1;
    unsigned first = 0;
    if ((int)lane == leader) first = atomicAdd(g.out_len, (unsigned)__popcll(m));
    first = __shfl(first, leader);
    if (keep) {
        const unsigned pos = first + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (pos < g.cap) g.out[pos] = c;
        else atomicOr(g.flags, (unsigned)FLAG_QUEUE_FULL);
    }
}
#endif  // __HIPCC__

}  // namespace curve
}  // namespace ecfft
