// HIP kernels of the ECFFT hot path (gfx950).  Field-generic: F = ecfft::Secp256k1 or ecfft::M31.
//
// All butterflies are the NORMALISED form derived in DESIGN.md ("Normalised butterflies"): the
// reference's 2x2 matrices (src/fftree.rs:355-362)
//      R = [[v0, s0*v0], [v1, s1*v1]],   D = R^-1,   v_j = v(s_j)^(d/2-1)
// factor as R = diag(v0, v1) * [[1, s0], [1, s1]].  Carrying the diagonal as a per-point weight W
// (W_k(s) = v_k(s)^(h_k-1) * W_{k+1}(psi_k(s))) turns every stage into
//      recombine:  (A, B) -> (A + s0*B, A + s1*B)                       2 field muls, was 4
//      decompose:  (a, b) -> q1 = (b - a)/(s1 - s0), q0 = a - s0*q1      2 field muls, was 4
// with one multiply by 1/W on the way in and by W on the way out of an EXTEND (both folded into the
// neighbouring pointwise tables).  Field elements are canonical residues, so the re-association is
// bit-exact against the reference.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <type_traits>
#include "mfma_blk16.h"
#include "curve_points.h"

namespace ecfft {

constexpr int kBlock = 256;

// Workgroup barrier that publishes LDS writes only: __syncthreads() also drains the vector-memory counter (s_waitcnt vmcnt(0)),
// which would turn every table request issued ahead of the barrier into a wait AT the barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// Round 6: sweeps whose pairs stay inside one wave's own 128-element span (one pair per thread, pair distance <= 64: the wave that
// wrote an element is the only one that reads it next) need no WORKGROUP barrier between them.  LDS operations of one wave execute
// in issue order, so a wavefront-scope fence (no instruction; it only stops the compiler from moving LDS accesses across it) is all
// the ordering there is to ask for.  ECFFT_WAVE_LOCAL: 0 = workgroup barrier everywhere (rounds 1-5), 1 = wavefront fence,
// 2 = s_waitcnt lgkmcnt(0) without the s_barrier (A/B forms; profiles/r06/wave_local_ab.txt).
#ifndef ECFFT_WAVE_LOCAL
#define ECFFT_WAVE_LOCAL 1
#endif
__device__ __forceinline__ void wave_local_sync() {
#if ECFFT_WAVE_LOCAL == 2
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#elif ECFFT_WAVE_LOCAL == 1
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    asm volatile("" ::: "memory");
#else
    lds_barrier();
#endif
}
// pair distance 2^lh of a one-pair-per-thread sweep (idx = ((tid >> lh) << (lh + 1)) + (tid & (h - 1))): wave-local iff h <= 64
__device__ __forceinline__ constexpr bool wave_local_lh(int lh) { return ECFFT_WAVE_LOCAL != 0 && lh <= 6; }
#ifndef ECFFT_RADIX_LDSBAR
#define ECFFT_RADIX_LDSBAR 1                 // 4-byte engine: the barrier behind the early table requests is LDS-only
#endif

// Value ranges: inside a kernel (registers, LDS) field elements may be in the field's LAZY range (F::tmul / F::tmul_add /
// F::sub keep them there: [0, p] for M31, canonical for secp256k1); every store to HBM goes through F::canon(), so all
// arrays between launches, and everything the caller sees, are canonical residues.
// ---------------------------------------------------------------------------------------------
// streaming butterfly stages (one launch per stage).  On the hot path only the cyclic shards of a
// multi-GPU split EXTEND use them (log2 P stages with strided tables); everything else is fused below.
// buf holds `npairs*2` elements = count vectors of length e laid end to end; h = pair distance.
// ---------------------------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(kBlock) void k_decompose_stage(typename F::elem* __restrict__ buf,
                                                             const typename F::telem* __restrict__ np0,
                                                             const typename F::telem* __restrict__ dinv,
                                                             uint32_t log_h, size_t npairs, uint32_t tstride, uint32_t toff) {
    // tstride/toff: table entry of local pair index i is i*tstride + toff (cyclic shards of a split EXTEND; 1/0 otherwise)
    size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= npairs) return;
    size_t h = (size_t)1 << log_h;
    size_t i = g & (h - 1);
    size_t idx = ((g >> log_h) << (log_h + 1)) + i;
    i = i * tstride + toff;
    typename F::elem a = buf[idx], b = buf[idx + h];
    typename F::elem q1 = F::tmul(dinv[i], F::sub(b, a));
    typename F::elem q0 = F::tmul_add(np0[i], q1, a);
    buf[idx] = F::canon(q0);
    buf[idx + h] = F::canon(q1);
}

template <class F>
__global__ __launch_bounds__(kBlock) void k_recombine_stage(typename F::elem* __restrict__ buf,
                                                             const typename F::telem* __restrict__ p0,
                                                             const typename F::telem* __restrict__ p1,
                                                             uint32_t log_h, size_t npairs, uint32_t tstride, uint32_t toff) {
    size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= npairs) return;
    size_t h = (size_t)1 << log_h;
    size_t i = g & (h - 1);
    size_t idx = ((g >> log_h) << (log_h + 1)) + i;
    i = i * tstride + toff;
    typename F::elem a = buf[idx], b = buf[idx + h];
    buf[idx] = F::canon(F::tmul_add(p0[i], b, a));
    buf[idx + h] = F::canon(F::tmul_add(p1[i], b, a));
}

// ---------------------------------------------------------------------------------------------
// Fused load / store operators.  Every pointwise step of ENTER / EXIT that sits between two EXTEND
// cores is folded into the first load or the last store of the neighbouring fused-stage kernel, so it
// costs no HBM pass of its own.  `pos` is the element's position in the work buffer (count vectors of
// length e laid end to end), i = pos mod e.
// ---------------------------------------------------------------------------------------------
enum { LD_PLAIN = 0, LD_SCALE = 1 };
enum { ST_PLAIN = 0, ST_SCALE = 1, ST_AXPBY = 2, ST_EXIT_SPLIT = 3, ST_ENTER = 4, ST_EXIT3 = 5 };

template <class F>
struct IoDesc {
    using E = typename F::elem;
    using TE = typename F::telem;
    // load:  x = [ld_tbl[i] *] src[src_stride*pos + src_off]
    //        ld_tr_logp > 0: src holds the P = 2^ld_tr_logp chunks of an all-to-all, source-rank major, and position pos of the
    //        block shard is element pos / P of chunk pos mod P:  src[(pos mod P)*tr_chunk + pos / P]   (split EXTEND)
    const E* src; uint32_t src_stride, src_off; int ld_mode; const TE* ld_tbl; uint32_t ld_tr_logp, st_tr_logp; size_t tr_chunk;
    // store: ST_PLAIN  dst[pos] = x
    //        ST_SCALE  dst[pos] = st_a[i]*x
    //        ST_AXPBY  r = st_a[i]*x + st_b[i]*aux[aux_stride*pos + aux_off]; dst[pos] = r; aux_out[pos] = r (if set)
    //        ST_EXIT_SPLIT  u0 = st_a[i]*x; v0 = st_b[i]*(aux[2*pos] - u0); dst[b*2e + i] = u0; dst[b*2e + e + i] = v0  (b = pos / e)
    //        ST_ENTER  (pair operator, ENTER loop C src/fftree.rs:155-159 in normalised form; x = U1~ at pos = b*2e + i, y = V1~ at
    //                  pos + e, both still in the tile; aux = the level's input blocks [u0 | v0])
    //                  dst[b*2e + 2i] = aux[b*2e + i] + st_a[i]*aux[b*2e + e + i];  dst[b*2e + 2i + 1] = st_c[i]*x + st_b[i]*y
    //        ST_EXIT3  (ST_AXPBY followed by ST_EXIT_SPLIT: the last store of the three-core EXIT level)
    //                  u0 = st_a[i]*x + st_b[i]*aux[aux_stride*pos + aux_off]; v0 = st_c[i]*(aux2[2*pos] - u0); dst as for ST_EXIT_SPLIT
    E* dst; int st_mode; const TE* st_a; const TE* st_b; const E* aux; uint32_t aux_stride, aux_off; E* aux_out; const TE* st_c;
    const E* aux2;       // ST_EXIT3: the level's input (even positions)
    uint32_t nt_st;      // != 0: non-temporal stores of the pass's results (data_st; launches of the latency regime)
};

// Result stores of the fused passes (32-byte fields) go through data_st: two explicit 16-byte vector stores, non-temporal when the host
// sets IoDesc::nt_st for the launch (DeviceChain::kNtStoreMaxLog; wave-uniform branch).  Round 6, measured on MI355X
// (profiles/r06/nt_data_ab.txt): the NON-TEMPORAL store itself buys nothing — flag set for launches <= 2^17 .. 2^19: +-0.3 % against the flag
// never set; set everywhere: +1.5 .. +3 % from 2^20 on (the next pass wants the results in cache); non-temporal LOADS of the tile data
// lose everywhere — so the shipped library never sets the flag.  What DOES pay is this form of the store: with it hipcc allocates the
// latency-regime column kernels differently (k_stages_col256 77 -> 101 VGPRs, k_stages_col_mid256 102 -> 94; same instructions, more loads
// in flight) and single transforms of 2^12 .. 2^19 run 0.7 - 3.2 % faster than with a plain `dst[pos] = x` (2^16 -0.7 %, 2^17 -1.5 %,
// 2^18 -1.4 %, 2^19 -3.2 %; >= 2^20 and batches unchanged), interleaved on one box against the previous sources.
typedef uint32_t nt_v4u __attribute__((ext_vector_type(4)));
template <class E>
__device__ __forceinline__ void data_st(E* p, const E& x, uint32_t nt) {
    if constexpr (sizeof(E) == 32) {
        if (nt) {                                                        // wave-uniform
            nt_v4u* q = reinterpret_cast<nt_v4u*>(p);
            nt_v4u a = {x.l[0], x.l[1], x.l[2], x.l[3]}, b = {x.l[4], x.l[5], x.l[6], x.l[7]};
            __builtin_nontemporal_store(a, q); __builtin_nontemporal_store(b, q + 1);
            return;
        }
    }
    *p = x;
}
template <class F>
__device__ __forceinline__ typename F::elem io_load(const IoDesc<F>& io, size_t pos, size_t emask) {
    typename F::elem v = io.ld_tr_logp ? io.src[(pos & (((size_t)1 << io.ld_tr_logp) - 1)) * io.tr_chunk + (pos >> io.ld_tr_logp)]
                                       : io.src[(size_t)io.src_stride * pos + io.src_off];
    if (io.ld_mode == LD_SCALE) v = F::tmul(io.ld_tbl[pos & emask], v);
    return v;
}
template <class F>
__device__ __forceinline__ void io_store(const IoDesc<F>& io, size_t pos, uint32_t log_e, const typename F::elem& x) {
    using E = typename F::elem;
    const size_t emask = ((size_t)1 << log_e) - 1, i = pos & emask;
    switch (io.st_mode) {
        case ST_PLAIN:   // st_tr_logp > 0: the mirror image of the transposed load — scatter into the send chunks of an all-to-all
            if (io.st_tr_logp) io.dst[(pos & (((size_t)1 << io.st_tr_logp) - 1)) * io.tr_chunk + (pos >> io.st_tr_logp)] = F::canon(x);
            else data_st(&io.dst[pos], F::canon(x), io.nt_st);
            break;
        case ST_SCALE: data_st(&io.dst[pos], F::canon(F::tmul(io.st_a[i], x)), io.nt_st); break;
        case ST_AXPBY: {
            E r = F::canon(F::tmul_add(io.st_a[i], x, F::tmul(io.st_b[i], io.aux[(size_t)io.aux_stride * pos + io.aux_off])));
            data_st(&io.dst[pos], r, io.nt_st);
            if (io.aux_out) io.aux_out[pos] = r;
            break;
        }
        case ST_EXIT3: {
            E u0 = F::canon(F::tmul_add(io.st_a[i], x, F::tmul(io.st_b[i], io.aux[(size_t)io.aux_stride * pos + io.aux_off])));
            E v0 = F::canon(F::tmul(io.st_c[i], F::sub(io.aux2[2 * pos], u0)));
            size_t base = (pos >> log_e) << (log_e + 1);
            data_st(&io.dst[base + i], u0, io.nt_st);
            data_st(&io.dst[base + ((size_t)1 << log_e) + i], v0, io.nt_st);
            break;
        }
        default: {  // ST_EXIT_SPLIT
            E u0 = F::canon(F::tmul(io.st_a[i], x));
            E v0 = F::canon(F::tmul(io.st_b[i], F::sub(io.aux[2 * pos], u0)));
            size_t base = (pos >> log_e) << (log_e + 1);
            data_st(&io.dst[base + i], u0, io.nt_st);
            data_st(&io.dst[base + ((size_t)1 << log_e) + i], v0, io.nt_st);
        }
    }
}

// the store operator of one EXTEND core followed by the load operator of the next one, applied to a value in flight
// (ST_PLAIN / ST_SCALE / ST_AXPBY only; side output aux_out is written): used where two cores are fused in one launch
template <class F>
__device__ __forceinline__ typename F::elem io_mid(const IoDesc<F>& io, size_t pos, size_t emask, const typename F::elem& x) {
    using E = typename F::elem;
    const size_t i = pos & emask;
    E r = x;
    if (io.st_mode == ST_SCALE) r = F::tmul(io.st_a[i], x);
    else if (io.st_mode == ST_AXPBY) {
        r = F::canon(F::tmul_add(io.st_a[i], x, F::tmul(io.st_b[i], io.aux[(size_t)io.aux_stride * pos + io.aux_off])));
        if (io.aux_out) io.aux_out[pos] = r;
    }
    if (io.ld_mode == LD_SCALE) r = F::tmul(io.ld_tbl[i], r);
    return r;
}

// table entry `idx` of a table whose base pointer is wave-uniform: 32-bit BYTE offset, so the load is "SGPR base + 32-bit lane
// offset" (global_load ... v_off, s[base:base+1]) instead of a 64-bit per-lane address built with v_lshl_add_u64
// The pointer is also cast to the GLOBAL address space: table pointers that were themselves loaded from memory (LevelTables) are
// generic, and generic (flat_load) accesses count against the LDS counter as well as the vector-memory one.
template <class TE>
__device__ __forceinline__ TE ldt(const TE* __restrict__ base, uint32_t idx) {
#ifdef ECFFT_EXP_NO_TABLE_LOADS      // experiment: constants made up in registers (no VMEM) — the bound of what free table loads could reach
    { TE r; uint32_t* w = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
      for (int k = 0; k < (int)(sizeof(TE) / 4); ++k) w[k] = (idx + 0x01010101u * (uint32_t)k) >> (sizeof(TE) == 4 ? 2 : 1);
      return r; }
#endif
    typedef const __attribute__((address_space(1))) char* gchar;
    if constexpr (sizeof(TE) == 4) {
        typedef const __attribute__((address_space(1))) TE* gte;
        return *(gte)((gchar)(reinterpret_cast<const char*>(base)) + (size_t)(idx * (uint32_t)sizeof(TE)));
    } else {
        // multi-word constants (secp256k1: 64 bytes): 16-byte global loads; 64-bit offset (tables may exceed 4 GiB)
        static_assert(sizeof(TE) % 16 == 0, "table constants are whole 16-byte words");
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(1))) u32x4* gq;
        const gq p = (gq)((gchar)(reinterpret_cast<const char*>(base)) + (size_t)idx * sizeof(TE));
        TE r;
        u32x4* rp = reinterpret_cast<u32x4*>(&r);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(TE) / 16); ++k) rp[k] = p[k];
        return r;
    }
}
// ---------------------------------------------------------------------------------------------
// Tile load / store for 4-byte fields, four consecutive elements ("quad") at a time.  The element-at-a-time loops of the
// generic kernels compile to a loop that waits for every 4-byte load before issuing the next one — 16 serial HBM round
// trips per thread for an 8192-element tile.  Here a thread issues ALL its 16-byte loads (data, strided gathers, operator
// tables) first, then computes, then stores 16 bytes per instruction.  `pos_of(j)` maps the LDS index j (a multiple of 4,
// j..j+3 contiguous in LDS) to the position of the quad in the work buffer (contiguous there too).
// Preconditions checked by vio_ok(): e >= 4, 16-byte aligned pointers, strides as produced by the level drivers.
// ---------------------------------------------------------------------------------------------
struct Quad { uint32_t v[4]; };
#ifdef ECFFT_EXP_TILE_IO_L2       // experiment: every tile load / store of the 4-byte vector paths lands in one 64 KiB window (cache resident):
#define ECFFT_DPOS(p) ((p) & (size_t)0x3FFF)      // the work stays, the HBM latency and bandwidth go — what a perfect prefetch ring could reach
#else
#define ECFFT_DPOS(p) (p)
#endif
__device__ __forceinline__ Quad ldq(const uint32_t* p) { uint4 t = *reinterpret_cast<const uint4*>(p); return Quad{{t.x, t.y, t.z, t.w}}; }
__device__ __forceinline__ void stq(uint32_t* p, const Quad& q) { *reinterpret_cast<uint4*>(p) = make_uint4(q.v[0], q.v[1], q.v[2], q.v[3]); }
// four consecutive 4-byte table entries starting at entry idx (16-byte aligned), uniform base pointer in the GLOBAL address space + 32-bit byte offset (see ldt below)
__device__ __forceinline__ Quad ldq_tab(const uint32_t* __restrict__ base, uint32_t idx) {
    typedef const __attribute__((address_space(1))) char* gchar;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4* gq;
    const u32x4 t = *(gq)((gchar)(reinterpret_cast<const char*>(base)) + (size_t)(idx * 4u));
    return Quad{{t.x, t.y, t.z, t.w}};
}
// four elements at p[stride*k + off], k = 0..3, stride 1 (off 0) or 2 (off 0 / 1)
__device__ __forceinline__ Quad ldq_strided(const uint32_t* p, uint32_t stride, uint32_t off) {
    if (stride == 1) return ldq(p);
    uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 4);
    return off ? Quad{{a.y, a.w, b.y, b.w}} : Quad{{a.x, a.z, b.x, b.z}};
}
template <class F>
__device__ __forceinline__ bool vio_ok(const IoDesc<F>& io, uint32_t log_e) {
    if constexpr (sizeof(typename F::elem) != 4) return false;
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    bool ok = log_e >= 2 && io.ld_tr_logp == 0 && io.st_tr_logp == 0 && al(io.src) && al(io.dst) && ((io.src_stride == 1 && io.src_off == 0) || (io.src_stride == 2 && io.src_off < 2));
    if (io.ld_mode == LD_SCALE) ok = ok && al(io.ld_tbl);
    if (io.st_mode == ST_SCALE || io.st_mode == ST_AXPBY || io.st_mode == ST_EXIT_SPLIT) ok = ok && al(io.st_a);
    if (io.st_mode == ST_AXPBY || io.st_mode == ST_EXIT_SPLIT) ok = ok && al(io.st_b) && al(io.aux) && ((io.aux_stride == 1 && io.aux_off == 0) || (io.aux_stride == 2 && io.aux_off < 2));
    if (io.st_mode == ST_AXPBY && io.aux_out) ok = ok && al(io.aux_out);
    if (io.st_mode == ST_EXIT_SPLIT) ok = ok && io.aux_stride == 2 && io.aux_off == 0;
    if (io.st_mode == ST_EXIT3) ok = ok && al(io.st_a) && al(io.st_b) && al(io.st_c) && al(io.aux) && al(io.aux2) && io.aux_stride == 1 && io.aux_off == 0;
    return ok;
}
template <class F, int NQ, int BLK, class PosFn>
__device__ __forceinline__ void vio_load(const IoDesc<F>& io, size_t emask, typename F::elem* tile, PosFn pos_of, uint32_t tid0) {
    const uint32_t tid = tid0;   // callers that split a tile into batches pass tid + batch*NQ*BLK (quad c of the batch = index 4*(tid + c*BLK))
    Quad d[NQ], t[NQ];
#pragma unroll
    for (int c = 0; c < NQ; ++c) { const size_t pos = pos_of(4u * (tid + (uint32_t)c * BLK)); d[c] = ldq_strided(io.src + (size_t)io.src_stride * ECFFT_DPOS(pos), io.src_stride, io.src_off); }
    if (io.ld_mode == LD_SCALE) {
#pragma unroll
        for (int c = 0; c < NQ; ++c) { const size_t pos = pos_of(4u * (tid + (uint32_t)c * BLK)); t[c] = ldq_tab(io.ld_tbl, (uint32_t)(pos & emask)); }
#pragma unroll
        for (int c = 0; c < NQ; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) d[c].v[k] = F::tmul(t[c].v[k], d[c].v[k]);
    }
#pragma unroll
    for (int c = 0; c < NQ; ++c) stq(tile + 4u * (tid + (uint32_t)c * BLK), d[c]);
}
// ST_EXIT3 on quads, two at a time (five operands per quad: more in flight would spill)
template <class F, int NQ, int BLK, class PosFn>
__device__ __forceinline__ void vio_store_exit3(const IoDesc<F>& io, uint32_t log_e, const typename F::elem* tile, PosFn pos_of, uint32_t tid) {
    const size_t e = (size_t)1 << log_e, emask = e - 1;
    static_assert(NQ % 2 == 0, "quads are taken two at a time");
#pragma unroll 1
    for (int c0 = 0; c0 < NQ; c0 += 2) {
        Quad x[2], a[2], b[2], t[2], y[2], z[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint32_t j = 4u * (tid + (uint32_t)(c0 + c) * BLK);
            const size_t pos = pos_of(j); const uint32_t i = (uint32_t)(pos & emask);
            x[c] = ldq(tile + j);
            a[c] = ldq_tab(io.st_a, i); b[c] = ldq_tab(io.st_b, i); t[c] = ldq_tab(io.st_c, i);
            y[c] = ldq(io.aux + ECFFT_DPOS(pos));
            z[c] = ldq_strided(io.aux2 + 2 * ECFFT_DPOS(pos), 2, 0);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const size_t pos = pos_of(4u * (tid + (uint32_t)(c0 + c) * BLK));
            Quad r, r2;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r.v[k] = F::canon(F::tmul_add(a[c].v[k], x[c].v[k], F::tmul(b[c].v[k], y[c].v[k])));
                r2.v[k] = F::canon(F::tmul(t[c].v[k], F::sub(z[c].v[k], r.v[k])));
            }
            const size_t bs = (pos >> log_e) << (log_e + 1), i = pos & emask;
            stq(io.dst + ECFFT_DPOS(bs + i), r); stq(io.dst + ECFFT_DPOS(bs + e + i), r2);
        }
    }
}
template <class F, int NQ, int BLK, class PosFn>
__device__ __forceinline__ void vio_store(const IoDesc<F>& io, uint32_t log_e, const typename F::elem* tile, PosFn pos_of, uint32_t tid) {
    const size_t e = (size_t)1 << log_e, emask = e - 1;
    const int m = io.st_mode;
    if (m == ST_EXIT3) { vio_store_exit3<F, NQ, BLK>(io, log_e, tile, pos_of, tid); return; }
    Quad x[NQ], a[NQ], b[NQ], y[NQ];
#pragma unroll
    for (int c = 0; c < NQ; ++c) x[c] = ldq(tile + 4u * (tid + (uint32_t)c * BLK));
    if (m != ST_PLAIN) {
#pragma unroll
        for (int c = 0; c < NQ; ++c) { const size_t pos = pos_of(4u * (tid + (uint32_t)c * BLK)); a[c] = ldq_tab(io.st_a, (uint32_t)(pos & emask)); }
    }
    if (m == ST_AXPBY || m == ST_EXIT_SPLIT) {
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
            const size_t pos = pos_of(4u * (tid + (uint32_t)c * BLK));
            b[c] = ldq_tab(io.st_b, (uint32_t)(pos & emask));
            y[c] = ldq_strided(io.aux + (size_t)io.aux_stride * ECFFT_DPOS(pos), io.aux_stride, io.aux_off);
        }
    }
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
        const size_t pos = pos_of(4u * (tid + (uint32_t)c * BLK));
        Quad r, r2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (m == ST_PLAIN) r.v[k] = F::canon(x[c].v[k]);
            else if (m == ST_SCALE) r.v[k] = F::canon(F::tmul(a[c].v[k], x[c].v[k]));
            else if (m == ST_AXPBY) r.v[k] = F::canon(F::tmul_add(a[c].v[k], x[c].v[k], F::tmul(b[c].v[k], y[c].v[k])));
            else { r.v[k] = F::canon(F::tmul(a[c].v[k], x[c].v[k])); r2.v[k] = F::canon(F::tmul(b[c].v[k], F::sub(y[c].v[k], r.v[k]))); }
        }
        if (m == ST_EXIT_SPLIT) {
            const size_t bs = (pos >> log_e) << (log_e + 1), i = pos & emask;
            stq(io.dst + ECFFT_DPOS(bs + i), r); stq(io.dst + ECFFT_DPOS(bs + e + i), r2);
        } else {
            stq(io.dst + ECFFT_DPOS(pos), r);
            if (m == ST_AXPBY && io.aux_out) stq(io.aux_out + ECFFT_DPOS(pos), r);
        }
    }
}

// io_mid on quads, in place in LDS: the store operator of one EXTEND core (ST_PLAIN / ST_SCALE / ST_AXPBY, side output
// aux_out written) followed by the load operator of the next (LD_PLAIN / LD_SCALE)
template <class F, int NQ, int BLK, class PosFn>
__device__ __forceinline__ void vio_mid(const IoDesc<F>& io, uint32_t log_e, typename F::elem* tile, PosFn pos_of, uint32_t tid) {
    const size_t emask = ((size_t)1 << log_e) - 1;
    Quad x[NQ], a[NQ], b[NQ], y[NQ], l[NQ];
    const int m = io.st_mode;
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
        const size_t pos = pos_of(4u * (tid + (uint32_t)c * BLK)), i = pos & emask;
        x[c] = ldq(tile + 4u * (tid + (uint32_t)c * BLK));
        if (m != ST_PLAIN) a[c] = ldq_tab(io.st_a, (uint32_t)i);
        if (m == ST_AXPBY) { b[c] = ldq_tab(io.st_b, (uint32_t)i); y[c] = ldq_strided(io.aux + (size_t)io.aux_stride * pos, io.aux_stride, io.aux_off); }
        if (io.ld_mode == LD_SCALE) l[c] = ldq_tab(io.ld_tbl, (uint32_t)i);
    }
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
        const size_t pos = pos_of(4u * (tid + (uint32_t)c * BLK));
        Quad r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t v = x[c].v[k];
            if (m == ST_SCALE) v = F::tmul(a[c].v[k], v);
            else if (m == ST_AXPBY) v = F::canon(F::tmul_add(a[c].v[k], v, F::tmul(b[c].v[k], y[c].v[k])));
            r.v[k] = v;
        }
        if (m == ST_AXPBY && io.aux_out) stq(io.aux_out + pos, r);
        if (io.ld_mode == LD_SCALE) {
#pragma unroll
            for (int k = 0; k < 4; ++k) r.v[k] = F::tmul(l[c].v[k], r.v[k]);
        }
        stq(tile + 4u * (tid + (uint32_t)c * BLK), r);
    }
}

// ENTER combine (ST_ENTER) on quads: NQ quads of pairs per thread; for quad c: ju / jv = LDS indices of U1~ / V1~, i = pair
// index inside the block (multiple of 4), bb = position of the block [u0 | v0] in the level's input / output
template <class F, int NQ, class IdxFn>
__device__ __forceinline__ void vio_enter_store(const typename F::elem* tile, const typename F::elem* __restrict__ src, typename F::elem* __restrict__ dst,
                                                const typename F::telem* __restrict__ xe, const typename F::telem* __restrict__ w1,
                                                const typename F::telem* __restrict__ w1x, size_t e, IdxFn idx, int cbase = 0) {
    // cbase: first quad of this batch (callers run several small batches: 7 live quads per pair-quad is 28 VGPRs)
    Quad u0[NQ], v0[NQ], tx[NQ], tw[NQ], twx[NQ], U[NQ], V[NQ];
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
        uint32_t ju, jv; size_t i, bb; idx(cbase + c, ju, jv, i, bb);
        u0[c] = ldq(src + ECFFT_DPOS(bb + i)); v0[c] = ldq(src + ECFFT_DPOS(bb + e + i));
        tx[c] = ldq_tab(xe, (uint32_t)i); tw[c] = ldq_tab(w1, (uint32_t)i); twx[c] = ldq_tab(w1x, (uint32_t)i);
        U[c] = ldq(tile + ju); V[c] = ldq(tile + jv);
    }
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
        uint32_t ju, jv; size_t i, bb; idx(cbase + c, ju, jv, i, bb);
        Quad lo, hi;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t ev = F::canon(F::tmul_add(tx[c].v[k], v0[c].v[k], u0[c].v[k]));
            const uint32_t od = F::canon(F::tmul_add(twx[c].v[k], V[c].v[k], F::tmul(tw[c].v[k], U[c].v[k])));
            if (k < 2) { lo.v[2 * k] = ev; lo.v[2 * k + 1] = od; } else { hi.v[2 * (k - 2)] = ev; hi.v[2 * (k - 2) + 1] = od; }
        }
        stq(dst + ECFFT_DPOS(bb + 2 * i), lo); stq(dst + ECFFT_DPOS(bb + 2 * i + 4), hi);
    }
}

// ---------------------------------------------------------------------------------------------
// LDS-fused butterfly stages, "row kernel".  One workgroup owns a contiguous tile of 2^log_tile
// elements (<= 64 KiB of LDS: 2048 secp256k1 / 16384 M31 elements), loads it once, runs every
// decompose stage k in [k_first, log e) and then every recombine stage back down to k_first in LDS,
// and stores it once: 2*(log e - k_first) stages for one HBM round trip.  Stage k_first has pair
// distance h = e >> (k_first+1) with 2h <= tile and tiles are tile-aligned, so a butterfly's table
// index is its local pair index mod h: every tile of a level reads the SAME h-entry table prefix
// (L2-resident per XCD).
// ---------------------------------------------------------------------------------------------
#ifndef ECFFT_BLOCK_LDS
#define ECFFT_BLOCK_LDS 512
#endif
constexpr int kBlockLds = ECFFT_BLOCK_LDS;   // threads per workgroup of the LDS-fused kernels
#ifndef ECFFT_BLOCK_ROW
#define ECFFT_BLOCK_ROW ECFFT_BLOCK_LDS
#endif
constexpr int kBlockRow = ECFFT_BLOCK_ROW;   // ... of the row kernel (k_stages_lds)
#ifndef ECFFT_ROW_PIPE
#define ECFFT_ROW_PIPE 1                     // row-kernel sweeps request the next sweep's table constants before the barrier
#endif
#ifndef ECFFT_MIN_WAVES
#define ECFFT_MIN_WAVES 4                    // waves per SIMD the register allocator must leave room for
#endif

// ---------------------------------------------------------------------------------------------
// One butterfly stage over an LDS-resident array: `npairs` pairs at distance h = 2^lh, table entry = pair index mod h.
// DEC: (a, b) -> (a + ta*q1, q1) with q1 = tb*(b - a)   [ta = np0, tb = dinv];   else (a, b) -> (a + ta*b, a + tb*b) [p0, p1].
// 4-byte fields (M31) take 4 consecutive pairs per lane with 128-bit LDS and table accesses whenever h >= 4 (the pairs,
// their partners and their table entries are then contiguous and 16-byte aligned): 4x fewer memory instructions and
// index computations.  No trailing barrier.
// ---------------------------------------------------------------------------------------------
// PAIR-SPLIT form (32-byte fields, sweeps with at most BLK/2 pairs — the small tiles of latency-bound launches): threads
// [0, npairs) produce the LOW output of every pair, threads [npairs, 2*npairs) the HIGH one, ONE multiply each (decompose through
// tc = np0*dinv, which makes its two products independent), so a sweep costs one multiply of latency instead of two dependent
// ones and twice as many SIMDs work.  Both roles read (a, b); a barrier separates those reads from the in-place writes.
template <class F, bool DEC, int BLK = kBlockLds>
__device__ __forceinline__ void stage_sweep(typename F::elem* a_, const typename F::telem* __restrict__ ta, const typename F::telem* __restrict__ tb,
                                            uint32_t lh, uint32_t npairs, uint32_t tid, const typename F::telem* __restrict__ tc = nullptr) {
    using E = typename F::elem;
    const uint32_t h = 1u << lh;
    if constexpr (sizeof(E) == 32) {
        if (2 * npairs <= (uint32_t)BLK && (!DEC || tc)) {
            const bool act = tid < 2 * npairs, hi = tid >= npairs;
            const uint32_t g = hi ? tid - npairs : tid, i = g & (h - 1), idx = ((g >> lh) << (lh + 1)) + i;
            E x, y; typename F::telem t;
            if (act) { x = a_[idx]; y = a_[idx + h]; t = DEC ? (hi ? ldt(tb, i) : ldt(tc, i)) : (hi ? ldt(tb, i) : ldt(ta, i)); }
            __syncthreads();
            if (act) {
                if (DEC) { const E d = F::sub(y, x); if (hi) a_[idx + h] = F::tmul(t, d); else a_[idx] = F::tmul_add(t, d, x); }
                else a_[idx + (hi ? h : 0)] = F::tmul_add(t, y, x);
            }
            return;
        }
    }
    if constexpr (sizeof(E) == 4) {
        if (lh >= 2 && (npairs & 3u) == 0) {
            for (uint32_t g4 = tid; g4 < (npairs >> 2); g4 += BLK) {
                const uint32_t g = g4 << 2, i = g & (h - 1), idx = ((g >> lh) << (lh + 1)) + i;
                uint4 va = *reinterpret_cast<const uint4*>(a_ + idx), vb = *reinterpret_cast<const uint4*>(a_ + idx + h);
                const uint4 v0 = *reinterpret_cast<const uint4*>(ta + i), v1 = *reinterpret_cast<const uint4*>(tb + i);
                uint32_t xa[4] = {va.x, va.y, va.z, va.w}, xb[4] = {vb.x, vb.y, vb.z, vb.w};
                const uint32_t t0[4] = {v0.x, v0.y, v0.z, v0.w}, t1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (DEC) { E q1 = F::tmul(t1[c], F::sub(xb[c], xa[c])); xa[c] = F::tmul_add(t0[c], q1, xa[c]); xb[c] = q1; }
                    else { E o0 = F::tmul_add(t0[c], xb[c], xa[c]), o1 = F::tmul_add(t1[c], xb[c], xa[c]); xa[c] = o0; xb[c] = o1; }
                }
                *reinterpret_cast<uint4*>(a_ + idx) = make_uint4(xa[0], xa[1], xa[2], xa[3]);
                *reinterpret_cast<uint4*>(a_ + idx + h) = make_uint4(xb[0], xb[1], xb[2], xb[3]);
            }
            return;
        }
    }
    for (uint32_t g = tid; g < npairs; g += BLK) {
        const uint32_t i = g & (h - 1), idx = ((g >> lh) << (lh + 1)) + i;
        E a = a_[idx], b = a_[idx + h];
        if (DEC) { E q1 = F::tmul(ldt(tb, i), F::sub(b, a)); a_[idx] = F::tmul_add(ldt(ta, i), q1, a); a_[idx + h] = q1; }
        else { a_[idx] = F::tmul_add(ldt(ta, i), b, a); a_[idx + h] = F::tmul_add(ldt(tb, i), b, a); }
    }
}


// ---------------------------------------------------------------------------------------------
// Register-resident multi-stage engine for 4-byte fields (M31).  A 4-byte element leaves most of the register file
// idle in the one-stage-per-LDS-round-trip sweeps above, and rocprofv3 showed the M31 row kernel waiting, not issuing
// (51 % of wave-cycles in s_waitcnt / s_barrier, one VALU instruction per 5.4 cycles per SIMD): every sweep paid a
// barrier, an LDS round trip and a dependent L2 table load for 14-17 arithmetic instructions per pair.  Here a thread
// keeps EPT = 16 (or 8) elements in registers and runs NS = 1..3 consecutive stages on them per LDS round trip
// ("radix-2^NS step": groups of 2^NS elements spaced by the smallest pair distance of the step), the table constants of
// the whole step are requested BEFORE the barrier that publishes the previous step (they do not depend on the data), and
// the lowest log2(EPT) decompose stages, the merged innermost stage and the first log2(EPT) recombine stages run on EPT
// consecutive elements in one visit with wave-uniform (scalar) table constants.  25 sweeps of an 8192-element tile become
// 7 visits.
// ---------------------------------------------------------------------------------------------
template <class F, bool DEC>
__device__ __forceinline__ void bfly(typename F::elem& a, typename F::elem& b, const typename F::telem& t0, const typename F::telem& t1) {
    using E = typename F::elem;
    if (DEC) { E q1 = F::tmul(t1, F::sub(b, a)); a = F::tmul_add(t0, q1, a); b = q1; }
    else { E o0 = F::tmul_add(t0, b, a), o1 = F::tmul_add(t1, b, a); a = o0; b = o1; }
}

// SYMMETRIC butterfly: on tables written in the coordinate sigma = (x - c1)/(x - c2) of each layer (c1, c2 the
// critical points of its map) the two pre-images of a point have p1 = -p0, so np0 = p1 and dinv = -1/(2 p0), and the general forms
//      recombine (A, B) -> (A + p0 B, A + p1 B)         decompose (a, b) -> q1 = dinv (b - a), q0 = a + np0 q1
// are  recombine (A, B) -> (A + m, A - m), m = p0 B     decompose (a, b) -> q1 = dinv (b - a), q0 = (a + b)/2
// ONE multiply and one constant (t = dinv | p0) per pair.  Same residues, canonical: the same bits as the general form.
// Written with modular subtractions only (18 instructions each for the 32-byte field, where a modular addition is over 40):
// (a + b)/2 = b - (b - a)/2 with the difference the multiply needs anyway, A - m = A - ((A + m) - A) with the addition inside the multiply.
template <class F, bool DEC>
__device__ __forceinline__ void sym_bfly(typename F::elem& a, typename F::elem& b, const typename F::telem& t) {
    using E = typename F::elem;
    if (DEC) { const E d = F::sub(b, a); a = F::sub(b, F::half(d)); b = F::tmul(t, d); }
    else { const E o0 = F::tmul_add(t, b, a); b = F::sub(a, F::sub(o0, a)); a = o0; }
}

// NS stages on NG groups of 2^NS elements: group g = LDS positions pbase[g] + j*pstride (j < 2^NS).  Stage s' < NS pairs
// (j, j + 2^s') and reads table entry (e - 2*(tstride << s')) + tbase[g] + (j mod 2^s')*tstride of ta / tb.
// DEC runs s' = NS-1 .. 0 (large distance first), recombine 0 .. NS-1.  Starts with the barrier that makes the previous
// step's LDS writes visible (after the table loads have been issued); does NOT end with one.
template <class F, int NS, bool DEC, int NG>
__device__ __forceinline__ void radix_step(typename F::elem* a, const typename F::telem* __restrict__ ta, const typename F::telem* __restrict__ tb,
                                           uint32_t e, const uint32_t (&pbase)[NG], uint32_t pstride, const uint32_t (&tbase)[NG], uint32_t tstride,
                                           uint32_t halves = 1, uint32_t hstride = 0) {
    // all table offsets are 32-bit (tables of one tree have < 2^31 entries): uniform base pointer + 32-bit lane offset.
    // halves > 1: the same step on `halves` arrays `hstride` elements apart that use the SAME table entries (two vectors of a
    // batched EXTEND): the constants are loaded once
    using E = typename F::elem;
    using TE = typename F::telem;
    constexpr int G = 1 << NS;
    TE t0[NG][G - 1], t1[NG][G - 1];                        // stage s' occupies [2^s' - 1, 2^(s'+1) - 1)
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int sp = 0; sp < NS; ++sp) {
            const uint32_t off = e - 2 * (tstride << sp) + tbase[g];
#pragma unroll
            for (int m = 0; m < (1 << sp); ++m) { t0[g][(1 << sp) - 1 + m] = ldt(ta, off + (uint32_t)m * tstride); t1[g][(1 << sp) - 1 + m] = ldt(tb, off + (uint32_t)m * tstride); }
        }
    }
    if (ECFFT_RADIX_LDSBAR) lds_barrier(); else __syncthreads();          // the constants requested above stay in flight across it
#pragma unroll 1
    for (uint32_t hf = 0; hf < halves; ++hf, a += hstride) {
        E x[NG][G];
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int j = 0; j < G; ++j) x[g][j] = a[pbase[g] + (uint32_t)j * pstride];
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            const int sp = DEC ? NS - 1 - st : st;
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int j = 0; j < G; ++j)
                    if (!(j & (1 << sp))) bfly<F, DEC>(x[g][j], x[g][j + (1 << sp)], t0[g][(1 << sp) - 1 + (j & ((1 << sp) - 1))], t1[g][(1 << sp) - 1 + (j & ((1 << sp) - 1))]);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int j = 0; j < G; ++j) a[pbase[g] + (uint32_t)j * pstride] = x[g][j];
    }
}

// `cnt` consecutive stages whose SMALLEST pair distance is 2^lh_low elements of a flat array (row layout: table entry =
// position mod pair distance), in radix-8 steps plus a radix-4 / radix-2 remainder.  DEC: lh_low + cnt - 1 down to lh_low.
template <class F, bool DEC, int EPT, int BLK>
__device__ __forceinline__ void flat_stages(typename F::elem* a, const typename F::telem* __restrict__ ta, const typename F::telem* __restrict__ tb,
                                            uint32_t e, uint32_t lh_low, uint32_t cnt, uint32_t tid) {
    // chunk sizes: as many 3s as possible, remainder first for DEC / last for recombine does not matter for correctness as
    // long as the order of stages is monotone; the chunks are walked from the far end for DEC
    uint32_t done = 0;
    while (done < cnt) {
        uint32_t ns = cnt - done >= 3 ? 3 : cnt - done;
        // DEC walks distances downwards: this chunk covers lh in [top - ns + 1, top], top = lh_low + cnt - 1 - done
        const uint32_t lo = DEC ? lh_low + cnt - done - ns : lh_low + done;
        const uint32_t hl = 1u << lo;
        auto run = [&](auto NSc) {
            constexpr int NS = decltype(NSc)::value;
            constexpr int NG = EPT >> NS;
            uint32_t pb[NG], tb0[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const uint32_t q = tid + (uint32_t)BLK * g, i0 = q & (hl - 1);
                pb[g] = ((q >> lo) << (lo + NS)) | i0; tb0[g] = i0;
            }
            radix_step<F, NS, DEC, NG>(a, ta, tb, e, pb, hl, tb0, hl);
        };
        if (ns == 3) run(std::integral_constant<int, 3>{}); else if (ns == 2) run(std::integral_constant<int, 2>{}); else run(std::integral_constant<int, 1>{});
        done += ns;
    }
}

// the lowest stages (pair distance < EPT) on EPT consecutive elements per thread: decompose lh = min(le, LOG_EPT)-1 .. 1, the
// merged innermost pair (h = 1), recombine 1 .. min(le, LOG_EPT)-1.  All table constants are wave-uniform.  Begins with a barrier.
template <class F, int EPT, int BLK>
__device__ __forceinline__ void tail_stages(typename F::elem* a, const typename F::telem* __restrict__ np0, const typename F::telem* __restrict__ dinv,
                                            const typename F::telem* __restrict__ p0, const typename F::telem* __restrict__ p1,
                                            const typename F::telem* __restrict__ inner, uint32_t e, uint32_t le, uint32_t tid) {
    using E = typename F::elem;
    static_assert(sizeof(E) == 4 && (EPT == 16 || EPT == 8), "4-byte fields, 8 or 16 elements per thread");
    constexpr int LOG_EPT = EPT == 16 ? 4 : 3;
    __syncthreads();
    if (le == 0) return;
    E x[EPT];
    uint4* va = reinterpret_cast<uint4*>(a + (size_t)tid * EPT);
#pragma unroll
    for (int q = 0; q < EPT / 4; ++q) { uint4 v = va[q]; x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w; }
#pragma unroll
    for (int lh = LOG_EPT - 1; lh >= 1; --lh) {
        if ((uint32_t)lh < le) {
            const uint32_t off = e - 2 * (1u << lh);
#pragma unroll
            for (int j = 0; j < EPT; ++j)
                if (!(j & (1 << lh))) bfly<F, true>(x[j], x[j + (1 << lh)], ldt(np0, off + (j & ((1 << lh) - 1))), ldt(dinv, off + (j & ((1 << lh) - 1))));
        }
    }
    {
        const typename F::telem c0 = ldt(inner, 0), c1 = ldt(inner, 1);
#pragma unroll
        for (int j = 0; j < EPT; j += 2) { E d = F::sub(x[j + 1], x[j]); E o0 = F::tmul_add(c0, d, x[j]); x[j + 1] = F::tmul_add(c1, d, x[j]); x[j] = o0; }
    }
#pragma unroll
    for (int lh = 1; lh < LOG_EPT; ++lh) {
        if ((uint32_t)lh < le) {
            const uint32_t off = e - 2 * (1u << lh);
#pragma unroll
            for (int j = 0; j < EPT; ++j)
                if (!(j & (1 << lh))) bfly<F, false>(x[j], x[j + (1 << lh)], ldt(p0, off + (j & ((1 << lh) - 1))), ldt(p1, off + (j & ((1 << lh) - 1))));
        }
    }
#pragma unroll
    for (int q = 0; q < EPT / 4; ++q) va[q] = make_uint4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}

// every in-tile stage of an EXTEND core on BLK*EPT LDS elements = vectors of length e laid end to end (or, for e larger
// than the tile, a tile-aligned piece of one: then only the stages with pair distance below 2^log_span = tile run here).
// Decompose from distance 2^(log_span-1) down, merged innermost pair, recombine back up.  Starts with a barrier, ends with one.
template <class F, int EPT, int BLK>
__device__ __forceinline__ void lds_extend_fast(typename F::elem* a, const typename F::telem* __restrict__ np0, const typename F::telem* __restrict__ dinv,
                                                const typename F::telem* __restrict__ p0, const typename F::telem* __restrict__ p1,
                                                const typename F::telem* __restrict__ inner, size_t e64, uint32_t log_span, uint32_t tid) {
    const uint32_t e = (uint32_t)e64;
    constexpr uint32_t LOG_EPT = EPT == 16 ? 4 : 3;
    const uint32_t upper = log_span > LOG_EPT ? log_span - LOG_EPT : 0;      // stages with pair distance >= EPT
    if (upper) flat_stages<F, true, EPT, BLK>(a, np0, dinv, e, LOG_EPT, upper, tid);
    tail_stages<F, EPT, BLK>(a, np0, dinv, p0, p1, inner, e, log_span, tid);
    if (upper) flat_stages<F, false, EPT, BLK>(a, p0, p1, e, LOG_EPT, upper, tid);
    __syncthreads();
}

// Row-kernel sweeps of a 32-byte field, one pair per thread (tile = 2 * BLK elements), with the two table constants of the NEXT
// sweep requested before the barrier that ends the current one (see col_stages_pipe).  Pair distances 2^lh_from .. 2^lh_to
// (downwards for DEC, upwards otherwise), table entry e - 2h + (pair index mod h).  Ends with a barrier.
// lh_after: pair-distance log of a one-pair-per-thread consumer that follows the last sweep (then the closing barrier is relaxed
// like the ones between wave-local sweeps), or 99 = the consumer reads other waves' elements.
// PIPE = false (SYM only, an A/B form): every sweep requests its own constant after the barrier, as the low kernels' sweeps did.
template <class F, bool DEC, bool SYM = false, bool PIPE = true>
__device__ __forceinline__ void row_stages_pipe(typename F::elem* tile, const typename F::telem* __restrict__ ta, const typename F::telem* __restrict__ tb,
                                                uint32_t e, int lh_from, int lh_to, uint32_t tid, int lh_after = 99) {
    using E = typename F::elem;
    using TE = typename F::telem;
    if (DEC ? lh_from < lh_to : lh_from > lh_to) return;
    auto geom = [&](int lh, uint32_t& idx, uint32_t& ti) {
        const uint32_t h = 1u << lh, i = tid & (h - 1);
        idx = ((tid >> lh) << (lh + 1)) + i; ti = e - 2 * h + i;
    };
    uint32_t idx, ti;
    geom(lh_from, idx, ti);
    if constexpr (SYM) {      // symmetric butterflies (sym_bfly below): ONE constant per pair, dinv (DEC) or p0
        const TE* __restrict__ tk = DEC ? tb : ta;
        TE nk;
        if constexpr (PIPE) nk = ldt(tk, ti);
#pragma unroll 1
        for (int lh = lh_from; DEC ? lh >= lh_to : lh <= lh_to; lh += DEC ? -1 : 1) {
            if constexpr (!PIPE) nk = ldt(tk, ti);
            const TE t = nk;
            const uint32_t lo = idx, up = idx + (1u << lh);
            E a = tile[lo], b = tile[up];
            sym_bfly<F, DEC>(a, b, t);
            tile[lo] = a; tile[up] = b;
            if (lh != lh_to) { geom(lh + (DEC ? -1 : 1), idx, ti); if constexpr (PIPE) nk = ldt(tk, ti); }
            const int nxt = lh != lh_to ? lh + (DEC ? -1 : 1) : lh_after;
            if (wave_local_lh(lh) && wave_local_lh(nxt)) wave_local_sync(); else lds_barrier();
        }
        return;
    }
    TE na = ldt(ta, ti), nb = ldt(tb, ti);
#pragma unroll 1
    for (int lh = lh_from; DEC ? lh >= lh_to : lh <= lh_to; lh += DEC ? -1 : 1) {
        const TE t0 = na, t1 = nb;
        const uint32_t lo = idx, up = idx + (1u << lh);
        const E a = tile[lo], b = tile[up];
        if (DEC) { const E q1 = F::tmul(t1, F::sub(b, a)); tile[lo] = F::tmul_add(t0, q1, a); tile[up] = q1; }
        else { const E o0 = F::tmul_add(t0, b, a), o1 = F::tmul_add(t1, b, a); tile[lo] = o0; tile[up] = o1; }
        if (lh != lh_to) { geom(lh + (DEC ? -1 : 1), idx, ti); na = ldt(ta, ti); nb = ldt(tb, ti); }
        const int nxt = lh != lh_to ? lh + (DEC ? -1 : 1) : lh_after;
        if (wave_local_lh(lh) && wave_local_lh(nxt)) wave_local_sync(); else lds_barrier();
    }
}

// Round 6, second form of the wave-local sweeps: the sweeps at pair distance 64 and 32 of a one-pair-per-thread
// row tile with the PAIR KEPT IN REGISTERS between them.  After the sweep at distance 64 lane l of a wave holds elements (l, l + 64)
// of the wave's 128-element span; the sweep at distance 32 wants (l, l + 32) in lanes < 32 and (l + 32, l + 64) in lanes >= 32: the
// upper half-wave's low elements trade places with the lower half-wave's high elements — one v_permlane32_swap per register (8 per
// pair); from distance 32 to 16 the same inside each half-wave: v_permlane16_swap.  No LDS write + read between the three sweeps.
// ECFFT_ROW_REGS: 0 = through LDS (row_stages_pipe), 1 = registers.  A/B: profiles/r06/row_regs_ab.txt.
#ifndef ECFFT_ROW_REGS
#define ECFFT_ROW_REGS 0
#endif
template <class E>
__device__ __forceinline__ void pair_swap32(E& a, E& b) {
#pragma unroll
    for (int w = 0; w < 8; ++w) { auto p = __builtin_amdgcn_permlane32_swap(a.l[w], b.l[w], false, false); a.l[w] = p[0]; b.l[w] = p[1]; }
}
template <class E>
__device__ __forceinline__ void pair_swap16(E& a, E& b) {
#pragma unroll
    for (int w = 0; w < 8; ++w) { auto p = __builtin_amdgcn_permlane16_swap(a.l[w], b.l[w], false, false); a.l[w] = p[0]; b.l[w] = p[1]; }
}
// decompose at distance 64, then 32: reads the pair (idx6, idx6 + 64) from the tile (published by a barrier), returns the pair
// (idx4, idx4 + 16), idx4 = ((tid >> 4) << 5) + (tid & 15), of the state after the distance-32 sweep — what the fused distance-16 sweep reads
template <class F>
__device__ __forceinline__ void row_regs_dec(const typename F::elem* tile, const typename F::telem* __restrict__ np0, const typename F::telem* __restrict__ dinv,
                                             uint32_t e, uint32_t tid, typename F::elem& a, typename F::elem& b) {
    const uint32_t l = tid & 63u, idx6 = ((tid >> 6) << 7) + l;
    typename F::telem t0 = ldt(np0, e - 128u + l), t1 = ldt(dinv, e - 128u + l);
    a = tile[idx6]; b = tile[idx6 + 64];
    bfly<F, true>(a, b, t0, t1);
    t0 = ldt(np0, e - 64u + (l & 31u)); t1 = ldt(dinv, e - 64u + (l & 31u));
    pair_swap32(a, b);
    bfly<F, true>(a, b, t0, t1);
    pair_swap16(a, b);
}
// recombine at distance 32, then 64, from the pair (idx4, idx4 + 16) after the distance-16 sweep; writes the pair (idx6, idx6 + 64) to the tile
template <class F>
__device__ __forceinline__ void row_regs_rec(typename F::elem* tile, const typename F::telem* __restrict__ p0, const typename F::telem* __restrict__ p1,
                                             uint32_t e, uint32_t tid, typename F::elem a, typename F::elem b) {
    const uint32_t l = tid & 63u, idx6 = ((tid >> 6) << 7) + l;
    typename F::telem t0 = ldt(p0, e - 64u + (l & 31u)), t1 = ldt(p1, e - 64u + (l & 31u));
    pair_swap16(a, b);
    bfly<F, false>(a, b, t0, t1);
    t0 = ldt(p0, e - 128u + l); t1 = ldt(p1, e - 128u + l);
    pair_swap32(a, b);
    bfly<F, false>(a, b, t0, t1);
    tile[idx6] = a; tile[idx6 + 64] = b;
}

template <class F, int LOG_TILE_CT, bool SYM = false>      // LOG_TILE_CT > 0: tile size known at compile time (loops unroll); 0: runtime log_tile
__global__ __launch_bounds__(kBlockRow, ECFFT_MIN_WAVES) void k_stages_lds(IoDesc<F> io,
                                                           const typename F::telem* __restrict__ np0,
                                                           const typename F::telem* __restrict__ dinv,
                                                           const typename F::telem* __restrict__ p0,
                                                           const typename F::telem* __restrict__ p1,
                                                           const typename F::telem* __restrict__ inner,
                                                           uint32_t log_e, uint32_t k_first, uint32_t log_tile,
                                                           const typename F::telem* __restrict__ c0t,
                                                           const uint8_t* __restrict__ blkA, const unsigned long long* __restrict__ blkK) {
    // blkA / blkK != nullptr (32-byte field, tiles of whole 1024-element sub-tiles, >= 4 in-tile stages): the stages with pair
    // distance <= 8 run on the int8 matrix cores as one 16 x 16 map per block (mfma_blk16.h) instead of 7 VALU sweeps
    // SYM (symmetric contexts of a 32-byte field): the pipelined sweeps and the fused sweeps at distance 16 run sym_bfly
    using E = typename F::elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char ecfft_smem[];
    E* tile = reinterpret_cast<E*>(ecfft_smem);
    if (LOG_TILE_CT > 0) log_tile = LOG_TILE_CT;
    const uint32_t T = 1u << log_tile, tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x << log_tile;
    const size_t e = (size_t)1 << log_e, emask = e - 1;
    constexpr bool kFast = sizeof(E) == 4 && LOG_TILE_CT > 0 && ((1u << (LOG_TILE_CT > 0 ? LOG_TILE_CT : 0)) % (kBlockRow * 16)) == 0;
    constexpr int kNQ = kFast ? (1 << (LOG_TILE_CT > 0 ? LOG_TILE_CT : 2)) / (4 * kBlockRow) : 1;
    bool vio = false;
    if constexpr (kFast) vio = vio_ok<F>(io, log_e);
    if constexpr (kFast) {
        if (vio) {
#ifndef ECFFT_EXP_NO_TILE_IO      // experiment (tools/experiments/README): compute only — the bound of what perfect tile prefetch could reach
#pragma unroll 1
            for (uint32_t b = 0; b < (uint32_t)kNQ / 4; ++b) vio_load<F, 4, kBlockRow>(io, emask, tile, [=](uint32_t j) { return base + j; }, tid + b * 4u * kBlockRow);
#endif
        }
    }
    if (!vio) {
#ifndef ECFFT_EXP_NO_TILE_IO
#pragma unroll
        for (uint32_t j = tid; j < T; j += kBlockRow) tile[j] = io_load<F>(io, base + j, emask);
#endif
    }
    __syncthreads();
    const uint32_t npairs = T >> 1;
    if constexpr (kFast) {
        // register-resident multi-stage engine, 8192 elements per call (a 64 KiB ST_ENTER tile is two independent halves)
#pragma unroll 1
        for (uint32_t o = 0; o < T; o += kBlockRow * 16)
            lds_extend_fast<F, 16, kBlockRow>(tile + o, np0, dinv, p0, p1, inner, e, log_e - k_first, tid);
    } else {
    // stages k_first .. log_e-2 (h >= 2); the two innermost stages (decompose h=1, recombine h=1) act on the
    // same pairs back to back and are merged into out_j = a + c_j*(b - a): 2 multiplies instead of 4
    const uint32_t k_inner = log_e ? log_e - 1 : 0;
    // the matrix-core form lives in the compile-time-tile instantiation only (1024-element tiles): its four 32 x 32 accumulators
    // next to the multiply's registers spill a few dwords in the run-time-tile instantiation, which the small tiles keep using
    constexpr bool kMfma = sizeof(E) == 32 && kBlockRow == 512 && LOG_TILE_CT == 10;
    bool mfma = false;
    if constexpr (kMfma) mfma = blkA != nullptr;
    const uint32_t k_dec_end = mfma ? log_e - 4 : k_inner;              // mfma: VALU sweeps only for pair distances >= 16
    // mfma with T == 1024 and a decompose sweep at distance 16 in this kernel: that sweep writes its results in operand form itself
    const bool fuse16 = mfma && T == (uint32_t)Blk16::kSub && k_first < k_dec_end;
    bool pipe = false;                                                  // one pair per thread: constants one sweep ahead
    if constexpr (sizeof(E) == 32 && ECFFT_ROW_PIPE) pipe = npairs == (uint32_t)kBlockRow && (e >> 31) == 0;
    // registers across the sweeps at distance 64 / 32 / 16 (ECFFT_ROW_REGS): the pipelined sweeps stop above distance 64
    const bool regs = ECFFT_ROW_REGS && sizeof(E) == 32 && pipe && fuse16 && log_e - k_first >= 7;
    if (pipe) {
        if constexpr (sizeof(E) == 32) row_stages_pipe<F, true, SYM>(tile, np0, dinv, (uint32_t)e, (int)(log_e - k_first) - 1, regs ? 7 : (int)(log_e - (k_dec_end - (fuse16 ? 1u : 0u))), tid, fuse16 && !regs ? 4 : 99);
    } else
    for (uint32_t k = k_first; k < k_dec_end - (fuse16 ? 1u : 0u); ++k) {
        const uint32_t lh = log_e - k - 1, h = 1u << lh;
        stage_sweep<F, true, kBlockRow>(tile, np0 + (e - 2 * (size_t)h), dinv + (e - 2 * (size_t)h), lh, npairs, tid, c0t ? c0t + (e - 2 * (size_t)h) : nullptr);
        __syncthreads();
    }
    if constexpr (kMfma) {
        if (mfma) {
            Blk16::APre pre;
            if (fuse16) {                                                // one pair per thread: (idx, idx + 16)
                const uint32_t i = tid & 15u, idx = ((tid >> 4) << 5) + i;
                E a, b;
                if constexpr (ECFFT_ROW_REGS && sizeof(E) == 32) { if (regs) row_regs_dec<F>(tile, np0, dinv, (uint32_t)e, tid, a, b); else { a = tile[idx]; b = tile[idx + 16]; } }
                else { a = tile[idx]; b = tile[idx + 16]; }
                E q0, q1;
                if constexpr (SYM) { q0 = a; q1 = b; sym_bfly<F, true>(q0, q1, ldt(dinv + (e - 32), i)); }
                else { q1 = F::tmul(ldt(dinv + (e - 32), i), F::sub(b, a)); q0 = F::tmul_add(ldt(np0 + (e - 32), i), q1, a); }
                __builtin_amdgcn_sched_barrier(0);
                pre = Blk16::prefetch(blkA, tid);                        // after the multiplies (they need the registers), before the barriers
                __builtin_amdgcn_sched_barrier(0);
                // operand form permutes chunks across threads' elements — inside 8-element groups (Blk16::phys), i.e. inside the wave's span
                if (ECFFT_WAVE_LOCAL) wave_local_sync(); else __syncthreads();
                Blk16::store_operand(tile, idx, q0); Blk16::store_operand(tile, idx + 16, q1);
                __syncthreads();
            } else {
                pre = Blk16::prefetch(blkA, tid);
                __builtin_amdgcn_sched_barrier(0);
                Blk16::to_operand_form<kBlockRow>(tile, T, tid);
            }
#ifndef ECFFT_EXP_SKIP_PHASE
#pragma unroll 1
            for (uint32_t o = 0; o < T; o += Blk16::kSub) {
                if (o) { pre = Blk16::prefetch(blkA, tid); __builtin_amdgcn_sched_barrier(0); }
                Blk16::phase(tile + o, blkA, blkK, tid, pre);
            }
#endif
            if (fuse16) {                                                // recombine sweep at distance 16, reading the swizzled results
                const uint32_t i = tid & 15u, idx = ((tid >> 4) << 5) + i;
                const E a = Blk16::load_swizzled(tile, idx), b = Blk16::load_swizzled(tile, idx + 16);
                E o0, o1;
                if constexpr (SYM) { o0 = a; o1 = b; sym_bfly<F, false>(o0, o1, ldt(p0 + (e - 32), i)); }
                else { o0 = F::tmul_add(ldt(p0 + (e - 32), i), b, a); o1 = F::tmul_add(ldt(p1 + (e - 32), i), b, a); }
                // the swizzled positions read above and the plain ones written below lie in the wave's own span; so do the pairs of the
                // recombine sweep at distance 32 that follows in the pipelined form
                bool done_regs = false;
                if constexpr (ECFFT_ROW_REGS && sizeof(E) == 32) {
                    if (regs) {      // distance 32 and 64 in registers; the swizzled positions read above lie in the wave's own span, like the ones written
                        if (ECFFT_WAVE_LOCAL) wave_local_sync(); else __syncthreads();
                        row_regs_rec<F>(tile, p0, p1, (uint32_t)e, tid, o0, o1);
                        lds_barrier();
                        done_regs = true;
                    }
                }
                if (!done_regs) {
                if (ECFFT_WAVE_LOCAL) wave_local_sync(); else __syncthreads();
                tile[idx] = o0; tile[idx + 16] = o1;
                if (ECFFT_WAVE_LOCAL && pipe && k_first + 1 < k_dec_end) wave_local_sync(); else __syncthreads();
                }
            } else {
                Blk16::from_swizzled<kBlockRow>(tile, T, tid);
            }
        }
    }
    if (log_e > 0 && !mfma) {
        if (sizeof(E) == 32 && 2 * npairs <= (uint32_t)kBlockRow) {        // pair-split merged innermost stage
            const bool act = tid < 2 * npairs, hi = tid >= npairs;
            const uint32_t g = hi ? tid - npairs : tid;
            E a, b; typename F::telem c;
            if (act) { a = tile[2 * g]; b = tile[2 * g + 1]; c = inner[hi ? 1 : 0]; }
            __syncthreads();
            if (act) tile[2 * g + (hi ? 1 : 0)] = F::tmul_add(c, F::sub(b, a), a);
        } else {
        const typename F::telem c0 = inner[0], c1 = inner[1];
#pragma unroll
        for (uint32_t g = tid; g < npairs; g += kBlockRow) {
            E a = tile[2 * g], b = tile[2 * g + 1];
            E d = F::sub(b, a);
            tile[2 * g] = F::tmul_add(c0, d, a);
            tile[2 * g + 1] = F::tmul_add(c1, d, a);
        }
        }
        __syncthreads();
    }
    if (pipe) {
        if constexpr (sizeof(E) == 32) row_stages_pipe<F, false, SYM>(tile, p0, p1, (uint32_t)e, regs ? 7 : (int)(log_e - (k_dec_end - (fuse16 ? 1u : 0u))), (int)(log_e - k_first) - 1, tid);
    } else
    for (uint32_t k = k_dec_end - (fuse16 ? 1u : 0u); k-- > k_first;) {
        const uint32_t lh = log_e - k - 1, h = 1u << lh;
        stage_sweep<F, false, kBlockRow>(tile, p0 + (e - 2 * (size_t)h), p1 + (e - 2 * (size_t)h), lh, npairs, tid);
        __syncthreads();
    }
    }
    if (io.st_mode == ST_ENTER) {
        // the tile holds whole [U1~ | V1~] blocks (2e <= T): combine them with the level's input and store interleaved
        if constexpr (kFast) {
            auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
            if (log_e >= 2 && al(io.aux) && al(io.dst) && al(io.st_a) && al(io.st_b) && al(io.st_c)) {
#ifdef ECFFT_EXP_NO_TILE_IO
                return;
#endif
#pragma unroll 1
                for (int cb = 0; cb < kNQ / 2; cb += 2)
                    vio_enter_store<F, 2>(tile, io.aux, io.dst, io.st_a, io.st_c, io.st_b, e, [=](int c, uint32_t& ju, uint32_t& jv, size_t& i, size_t& bb) {
                        const uint32_t g = 4u * (tid + (uint32_t)c * kBlockRow), ii = g & (uint32_t)emask, lb = (g >> log_e) << (log_e + 1);
                        ju = lb + ii; jv = lb + (uint32_t)e + ii; i = ii; bb = base + lb;
                    }, cb);
                return;
            }
        }
#ifdef ECFFT_EXP_NO_TILE_IO
        return;
#endif
        for (uint32_t g = tid; g < npairs; g += kBlockRow) {
            const uint32_t i = g & (uint32_t)emask, lb = (g >> log_e) << (log_e + 1);
            const size_t bb = base + lb;
            const E u0 = io.aux[bb + i], v0 = io.aux[bb + e + i];
            const E ev = F::tmul_add(io.st_a[i], v0, u0);
            const E od = F::tmul_add(io.st_b[i], tile[lb + (uint32_t)e + i], F::tmul(io.st_c[i], tile[lb + i]));
            io.dst[bb + 2 * i] = F::canon(ev);
            io.dst[bb + 2 * i + 1] = F::canon(od);
        }
        return;
    }
    if constexpr (kFast) {
        if (vio) {
#ifndef ECFFT_EXP_NO_TILE_IO
#pragma unroll 1
            for (uint32_t b = 0; b < (uint32_t)kNQ / 4; ++b) vio_store<F, 4, kBlockRow>(io, log_e, tile, [=](uint32_t j) { return base + j; }, tid + b * 4u * kBlockRow);
#endif
            return;
        }
    }
#ifndef ECFFT_EXP_NO_TILE_IO
#pragma unroll
    for (uint32_t j = tid; j < T; j += kBlockRow) io_store<F>(io, base + j, log_e, tile[j]);
#endif
}

// ---------------------------------------------------------------------------------------------
// Row kernel of ENTER level 11: the EXTEND of an ENTER level with e = 1024 and the level's combine (ST_ENTER), 32-byte fields with
// matrix-core tables.  ST_ENTER combines U1~ and V1~ of one [u0 | v0] block, so the workgroup owns the whole block: 2048 elements,
// 64 KiB of LDS.  The block's two 1024-element halves are independent EXTENDs on the same constants; each goes through the engine of
// k_stages_lds<F, 10, SYM> on a 1024-element tile: pipelined sweeps at pair distance 512 .. 32, the fused sweep at distance 16 into
// operand form, the matrix-core phase, the fused recombine at distance 16, pipelined sweeps back up to 512 — one pair per thread, so
// the register footprint is that kernel's.  BLK = 512: one half after the other (two workgroups per CU); BLK = 1024: threads 0..511
// take the first half and threads 512..1023 the second at the same time (one workgroup per CU, the same sixteen waves: a launch of
// one block per CU — the half-streams of a single transform of 2^20 — then runs four waves per SIMD instead of two).
// (k_stages_lds<F, 0> on a 2048-element tile, which served this level before, has neither the pipelined sweeps nor the matrix-core
// phase.)  Same operators, canonical residues: the same bytes.
// ---------------------------------------------------------------------------------------------
template <class F, bool SYM, int BLK>
__global__ __launch_bounds__(BLK, ECFFT_MIN_WAVES) void k_enter_l11(IoDesc<F> io,
                                                                   const typename F::telem* __restrict__ np0,
                                                                   const typename F::telem* __restrict__ dinv,
                                                                   const typename F::telem* __restrict__ p0,
                                                                   const typename F::telem* __restrict__ p1,
                                                                   const uint8_t* __restrict__ blkA, const unsigned long long* __restrict__ blkK) {
    using E = typename F::elem;
    static_assert(sizeof(E) == 32 && Blk16::kSub == 1024 && (BLK == 512 || BLK == 1024), "32-byte field, 1024-element matrix-core phases");
    extern __shared__ __attribute__((aligned(16))) unsigned char ecfft_smem[];
    E* const blk = reinterpret_cast<E*>(ecfft_smem);
    constexpr uint32_t e = 1024, log_e = 10;
    const size_t base = (size_t)blockIdx.x << (log_e + 1);
#pragma unroll
    for (uint32_t j = threadIdx.x; j < 2 * e; j += BLK) blk[j] = io_load<F>(io, base + j, (size_t)e - 1);
    __syncthreads();
#pragma unroll 1
    for (uint32_t sub = 0; sub < 1024u / BLK; ++sub) {
        // the thread index taken anew in every iteration: nothing that depends on it (pair positions, table constants, the prefetched
        // matrix rows) is carried in registers from one half to the other
        uint32_t tid = threadIdx.x & 511u;
        asm volatile("" : "+v"(tid));
        E* const tile = blk + (BLK == 1024 ? threadIdx.x >> 9 : sub) * e;
        row_stages_pipe<F, true, SYM>(tile, np0, dinv, e, (int)log_e - 1, 5, tid, 4);
        Blk16::APre pre;
        const uint32_t i = tid & 15u, idx = ((tid >> 4) << 5) + i;      // one pair per thread: (idx, idx + 16)
        {
            const E a = tile[idx], b = tile[idx + 16];
            E q0, q1;
            if constexpr (SYM) { q0 = a; q1 = b; sym_bfly<F, true>(q0, q1, ldt(dinv + (e - 32), i)); }
            else { q1 = F::tmul(ldt(dinv + (e - 32), i), F::sub(b, a)); q0 = F::tmul_add(ldt(np0 + (e - 32), i), q1, a); }
            __builtin_amdgcn_sched_barrier(0);
            pre = Blk16::prefetch(blkA, tid);                            // after the multiplies (they need the registers), before the barriers
            __builtin_amdgcn_sched_barrier(0);
            // operand form permutes chunks inside 8-element groups (Blk16::phys), i.e. inside the wave's own span
            if (ECFFT_WAVE_LOCAL) wave_local_sync(); else __syncthreads();
            Blk16::store_operand(tile, idx, q0); Blk16::store_operand(tile, idx + 16, q1);
            __syncthreads();
        }
        Blk16::phase(tile, blkA, blkK, tid, pre);
        {                                                                // recombine sweep at distance 16, reading the swizzled results
            const E a = Blk16::load_swizzled(tile, idx), b = Blk16::load_swizzled(tile, idx + 16);
            E o0, o1;
            if constexpr (SYM) { o0 = a; o1 = b; sym_bfly<F, false>(o0, o1, ldt(p0 + (e - 32), i)); }
            else { o0 = F::tmul_add(ldt(p0 + (e - 32), i), b, a); o1 = F::tmul_add(ldt(p1 + (e - 32), i), b, a); }
            // the swizzled positions read above and the plain ones written below lie in the wave's own span; so do the pairs of the
            // recombine sweep at distance 32 that follows
            if (ECFFT_WAVE_LOCAL) wave_local_sync(); else __syncthreads();
            tile[idx] = o0; tile[idx + 16] = o1;
            if (ECFFT_WAVE_LOCAL) wave_local_sync(); else __syncthreads();
        }
        row_stages_pipe<F, false, SYM>(tile, p0, p1, e, 5, (int)log_e - 1, tid);      // ends with a barrier
    }
    // the block holds [U1~ | V1~]: combine them with the level's input and store interleaved (ST_ENTER, as k_stages_lds)
    for (uint32_t i = threadIdx.x; i < e; i += BLK) {
        const E u0 = io.aux[base + i], v0 = io.aux[base + e + i];
        const E ev = F::tmul_add(io.st_a[i], v0, u0);
        const E od = F::tmul_add(io.st_b[i], blk[e + i], F::tmul(io.st_c[i], blk[i]));
        io.dst[base + 2 * i] = F::canon(ev);
        io.dst[base + 2 * i + 1] = F::canon(od);
    }
}

// forward declaration (defined with the low-level kernels below)
template <class F, int BLK, bool SWZ = false>
__device__ __forceinline__ void reg_extend32(typename F::elem* a, uint32_t len, uint32_t log_e, uint32_t k_first,
                                             const typename F::telem* __restrict__ c0t, const typename F::telem* __restrict__ dinv,
                                             const typename F::telem* __restrict__ p0, const typename F::telem* __restrict__ p1,
                                             const typename F::telem* __restrict__ inner, uint32_t tid,
                                             const uint8_t* __restrict__ blkA, const unsigned long long* __restrict__ blkK);

// ---------------------------------------------------------------------------------------------
// Row kernel of the LATENCY regime (32-byte fields, launches with fewer 1024-element tiles than CUs): 256-element
// tiles, 256 threads, ONE element per thread kept in registers through every in-tile stage (reg_extend32: cross-lane moves for
// pair distances < 64, LDS above), and — round 4 — the stages with pair distance <= 8 as one 16-point map per block on the
// matrix cores (v_mfma_i32_16x16x64_i8, Blk16::phase_n16_regs) when blkA != nullptr.  Same stages, same operators and the same
// results as k_stages_lds on a 256-element tile (ST_ENTER excepted: that operator needs whole [U | V] blocks and keeps the
// generic kernel).
// ---------------------------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(256, 2) void k_stages_row256(IoDesc<F> io,
                                                          const typename F::telem* __restrict__ dinv,
                                                          const typename F::telem* __restrict__ p0,
                                                          const typename F::telem* __restrict__ p1,
                                                          const typename F::telem* __restrict__ inner,
                                                          uint32_t log_e, uint32_t k_first,
                                                          const typename F::telem* __restrict__ c0t,
                                                          const uint8_t* __restrict__ blkA, const unsigned long long* __restrict__ blkK) {
    using E = typename F::elem;
    if constexpr (sizeof(E) == 32) {
        __shared__ E tile[256];
        const uint32_t tid = threadIdx.x;
        const size_t pos = ((size_t)blockIdx.x << 8) + tid;
        const size_t emask = ((size_t)1 << log_e) - 1;
        tile[tid] = io_load<F>(io, pos, emask);
        __syncthreads();
        reg_extend32<F, 256>(tile, 256u, log_e, k_first, c0t, dinv, p0, p1, inner, tid, blkA, blkK);
        io_store<F>(io, pos, log_e, tile[tid]);
    }
}

#ifndef ECFFT_COL_PAD
#define ECFFT_COL_PAD 0
#endif
// LDS row stride of a column tile: C elements + optional padding.  Unpadded, the small-distance stages make consecutive lane
// groups hit the same half of the 256-byte bank row (rows are 128 B at C = 4), a 4-way conflict on ds_read_b128 — but an
// A/B on MI355X (pad 0 / 1 / 2 rows) showed no difference: the kernel is bound by the modular multiply, not by LDS.
template <class E>
__host__ __device__ constexpr uint32_t col_row_stride(uint32_t C) { return C + (sizeof(E) == 4 ? 4u * ECFFT_COL_PAD : 1u * ECFFT_COL_PAD); }

// column-tile variant of stage_sweep: pair (row r, column cc) with partner d rows below; table entry ((r mod d) << log_hs) + c0 + cc
template <class F, bool DEC>
__device__ __forceinline__ void col_stage_sweep(typename F::elem* tile, const typename F::telem* __restrict__ pa, const typename F::telem* __restrict__ pb,
                                                uint32_t sft, uint32_t log_c, uint32_t log_hs, size_t c0, uint32_t npairs, uint32_t tid,
                                                const typename F::telem* __restrict__ pc = nullptr) {
    using E = typename F::elem;
    const uint32_t C = 1u << log_c, d = 1u << sft;
    if constexpr (sizeof(E) == 32) {
        if (2 * npairs <= (uint32_t)kBlockLds && (!DEC || pc)) {          // pair-split form, see stage_sweep
            const bool act = tid < 2 * npairs, hi = tid >= npairs;
            const uint32_t g = hi ? tid - npairs : tid, cc = g & (C - 1), pr = g >> log_c;
            const uint32_t r = ((pr >> sft) << (sft + 1)) | (pr & (d - 1));
            const size_t i = ((size_t)(r & (d - 1)) << log_hs) + c0 + cc;
            const uint32_t RS = col_row_stride<E>(C), lo = r * RS + cc, up = lo + d * RS;
            E x, y; typename F::telem t;
            if (act) { x = tile[lo]; y = tile[up]; t = DEC ? (hi ? pb[i] : pc[i]) : (hi ? pb[i] : pa[i]); }
            __syncthreads();
            if (act) {
                if (DEC) { const E dd = F::sub(y, x); if (hi) tile[up] = F::tmul(t, dd); else tile[lo] = F::tmul_add(t, dd, x); }
                else tile[hi ? up : lo] = F::tmul_add(t, y, x);
            }
            return;
        }
    }
    if constexpr (sizeof(E) == 4) {
        if (log_c >= 2) {
            for (uint32_t g4 = tid; g4 < (npairs >> 2); g4 += kBlockLds) {
                const uint32_t g = g4 << 2, cc = g & (C - 1), pr = g >> log_c;
                const uint32_t r = ((pr >> sft) << (sft + 1)) | (pr & (d - 1));
                const size_t i = ((size_t)(r & (d - 1)) << log_hs) + c0 + cc;
                const uint32_t RS = col_row_stride<E>(C), lo = r * RS + cc, hi = lo + d * RS;
                uint4 va = *reinterpret_cast<const uint4*>(tile + lo), vb = *reinterpret_cast<const uint4*>(tile + hi);
                const uint4 v0 = *reinterpret_cast<const uint4*>(pa + i), v1 = *reinterpret_cast<const uint4*>(pb + i);
                uint32_t xa[4] = {va.x, va.y, va.z, va.w}, xb[4] = {vb.x, vb.y, vb.z, vb.w};
                const uint32_t t0[4] = {v0.x, v0.y, v0.z, v0.w}, t1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (DEC) { E q1 = F::tmul(t1[c], F::sub(xb[c], xa[c])); xa[c] = F::tmul_add(t0[c], q1, xa[c]); xb[c] = q1; }
                    else { E o0 = F::tmul_add(t0[c], xb[c], xa[c]), o1 = F::tmul_add(t1[c], xb[c], xa[c]); xa[c] = o0; xb[c] = o1; }
                }
                *reinterpret_cast<uint4*>(tile + lo) = make_uint4(xa[0], xa[1], xa[2], xa[3]);
                *reinterpret_cast<uint4*>(tile + hi) = make_uint4(xb[0], xb[1], xb[2], xb[3]);
            }
            return;
        }
    }
    for (uint32_t g = tid; g < npairs; g += kBlockLds) {
        const uint32_t cc = g & (C - 1), pr = g >> log_c;
        const uint32_t r = ((pr >> sft) << (sft + 1)) | (pr & (d - 1));
        const size_t i = ((size_t)(r & (d - 1)) << log_hs) + c0 + cc;
        const uint32_t RS = col_row_stride<E>(C), lo = r * RS + cc, hi = lo + d * RS;
        E a = tile[lo], b = tile[hi];
        if (DEC) { E q1 = F::tmul(pb[i], F::sub(b, a)); tile[lo] = F::tmul_add(pa[i], q1, a); tile[hi] = q1; }
        else { tile[lo] = F::tmul_add(pa[i], b, a); tile[hi] = F::tmul_add(pb[i], b, a); }
    }
}

#ifndef ECFFT_COL_PIPE
#define ECFFT_COL_PIPE 1
#endif
// Column stages of a 32-byte field with the table constants ONE SWEEP AHEAD (round 3).  A column pass of a single transform is one
// workgroup per CU, and every sweep used to be "request two 64-byte constants from HBM / L2 -> wait -> two multiplies ->
// barrier": the top sweeps' constants are read once per launch, so their latency was paid R times in a row (48 % VALU-busy solo,
// profiles/r03).  Here the constants of sweep s+1 (they depend only on the thread's index) are requested right after the
// multiplies of sweep s, when the registers are free again, and fly across the LDS-only barrier and the next sweep's LDS reads.
// One pair per thread is pipelined (pair index tid); further pairs of the thread (two vectors per workgroup) load theirs in
// place as before.  Same arithmetic, same order: bit-identical.  Ends with a barrier.
template <class F, bool DEC, int BLK, bool SYM = false>
__device__ __forceinline__ void col_stages_pipe(typename F::elem* tile, const typename F::telem* __restrict__ ta, const typename F::telem* __restrict__ tb,
                                                uint32_t R, uint32_t log_c, uint32_t log_hs, size_t c0, size_t e, uint32_t tid, uint32_t npairs) {
    using E = typename F::elem;
    using TE = typename F::telem;
    const uint32_t C = 1u << log_c, RS = col_row_stride<E>(C);
    auto geom = [&](uint32_t st, uint32_t g, uint32_t& lo, uint32_t& up, uint32_t& ti) {
        const uint32_t sft = DEC ? R - 1 - st : st, d = 1u << sft;
        const uint32_t cc = g & (C - 1), pr = g >> log_c;
        const uint32_t r = ((pr >> sft) << (sft + 1)) | (pr & (d - 1));
        ti = (uint32_t)(e - 2 * (((size_t)1 << log_hs) << sft)) + ((r & (d - 1)) << log_hs) + (uint32_t)c0 + cc;
        lo = r * RS + cc; up = lo + d * RS;
    };
    uint32_t lo, up, ti;
    geom(0, tid, lo, up, ti);
    if constexpr (SYM) {      // symmetric butterflies: one constant per pair, dinv (DEC) or p0
        const TE* __restrict__ tk = DEC ? tb : ta;
        TE nk = ldt(tk, ti);
#pragma unroll 1
        for (uint32_t st = 0; st < R; ++st) {
            const TE t = nk;
            {
                E a = tile[lo], b = tile[up];
                sym_bfly<F, DEC>(a, b, t);
                tile[lo] = a; tile[up] = b;
            }
            for (uint32_t g = tid + BLK; g < npairs; g += BLK) {
                uint32_t l2, u2, i2; geom(st, g, l2, u2, i2);
                E a = tile[l2], b = tile[u2];
                sym_bfly<F, DEC>(a, b, ldt(tk, i2));
                tile[l2] = a; tile[u2] = b;
            }
            if (st + 1 < R) { geom(st + 1, tid, lo, up, ti); nk = ldt(tk, ti); }
            const uint32_t sft = DEC ? R - 1 - st : st, sft_n = DEC ? sft - 1 : sft + 1;
            if (st + 1 < R && wave_local_lh((int)(sft + log_c)) && wave_local_lh((int)(sft_n + log_c))) wave_local_sync(); else lds_barrier();
        }
        return;
    }
    TE na = ldt(ta, ti), nb = ldt(tb, ti);
#pragma unroll 1
    for (uint32_t st = 0; st < R; ++st) {
        const TE t0 = na, t1 = nb;
        const uint32_t lo0 = lo, up0 = up;
        {
            const E a = tile[lo0], b = tile[up0];
            if (DEC) { const E q1 = F::tmul(t1, F::sub(b, a)); tile[lo0] = F::tmul_add(t0, q1, a); tile[up0] = q1; }
            else { const E o0 = F::tmul_add(t0, b, a), o1 = F::tmul_add(t1, b, a); tile[lo0] = o0; tile[up0] = o1; }
        }
        for (uint32_t g = tid + BLK; g < npairs; g += BLK) {
            uint32_t l2, u2, i2; geom(st, g, l2, u2, i2);
            const E a = tile[l2], b = tile[u2];
            if (DEC) { const E q1 = F::tmul(ldt(tb, i2), F::sub(b, a)); tile[l2] = F::tmul_add(ldt(ta, i2), q1, a); tile[u2] = q1; }
            else { const E o0 = F::tmul_add(ldt(ta, i2), b, a), o1 = F::tmul_add(ldt(tb, i2), b, a); tile[l2] = o0; tile[u2] = o1; }
        }
        if (st + 1 < R) { geom(st + 1, tid, lo, up, ti); na = ldt(ta, ti); nb = ldt(tb, ti); }
        // pairs g in [64 q, 64 q + 64) of a stage with element distance (C << sft) <= 64 fill one aligned span of 128 elements, the same
        // span for every such stage: between two of them only the wave's own LDS traffic has to be ordered (wave_local_sync)
        const uint32_t sft = DEC ? R - 1 - st : st, sft_n = DEC ? sft - 1 : sft + 1;
        if (st + 1 < R && wave_local_lh((int)(sft + log_c)) && wave_local_lh((int)(sft_n + log_c))) wave_local_sync(); else lds_barrier();
    }
}

// The R stages of a column tile (2^R rows x C columns in LDS, row distance 2^s at stage k = kb - s; table entry
// ((row mod 2^s) << log_hs) + c0 + column, table base e - 2*(hs << s)).  DECOMPOSE runs s = R-1 .. 0, recombine 0 .. R-1.
// 4-byte fields with exactly 16 elements per thread use the register-resident radix steps (up to 3 stages per LDS round
// trip, table constants requested before the barrier); everything else sweeps one stage at a time.  Ends with a barrier.
template <class F, bool DEC, bool SYM = false>      // SYM: the pipelined sweeps of a 32-byte field run sym_bfly (the other forms stay general)
__device__ __forceinline__ void col_stages(typename F::elem* tile, const typename F::telem* __restrict__ ta, const typename F::telem* __restrict__ tb,
                                           uint32_t R, uint32_t log_c, uint32_t log_hs, size_t c0, size_t e, uint32_t tid, uint32_t halves = 1,
                                           const typename F::telem* __restrict__ tc = nullptr) {
    // halves = 2: two such tiles back to back in LDS that use the same table entries (k_stages_col_enter)
    using E = typename F::elem;
    const uint32_t C = 1u << log_c, T = C << R;
    if constexpr (sizeof(E) == 4 && ECFFT_COL_PAD == 0) {
        if (T == kBlockLds * 16) {
          {
            uint32_t done = 0;
            while (done < R) {
                const uint32_t ns = R - done >= 3 ? 3 : R - done;
                const uint32_t slo = DEC ? R - done - ns : done;              // lowest stage index s of this chunk
                auto run = [&](auto NSc) {
                    constexpr int NS = decltype(NSc)::value;
                    constexpr int NG = 16 >> NS;
                    uint32_t pb[NG], tb0[NG];
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const uint32_t q = tid + (uint32_t)kBlockLds * g, cc = q & (C - 1), rq = q >> log_c;
                        const uint32_t rlow = rq & ((1u << slo) - 1), rb = ((rq >> slo) << (slo + NS)) | rlow;
                        pb[g] = (rb << log_c) + cc; tb0[g] = (rlow << log_hs) + (uint32_t)c0 + cc;
                    }
                    radix_step<F, NS, DEC, NG>(tile, ta, tb, (uint32_t)e, pb, C << slo, tb0, (1u << log_hs) << slo, halves, T);
                };
                if (ns == 3) run(std::integral_constant<int, 3>{}); else if (ns == 2) run(std::integral_constant<int, 2>{}); else run(std::integral_constant<int, 1>{});
                done += ns;
            }
          }
            __syncthreads();
            return;
        }
    }
    const size_t hs = (size_t)1 << log_hs;
    if constexpr (sizeof(E) == 32 && ECFFT_COL_PIPE) {
        const uint32_t npairs = (halves * T) >> 1;
        if (npairs >= (uint32_t)kBlockLds && npairs % kBlockLds == 0 && (e >> 32) == 0) {     // at least one pair per thread (not the pair-split small tiles)
            col_stages_pipe<F, DEC, kBlockLds, SYM>(tile, ta, tb, R, log_c, log_hs, c0, e, tid, npairs);
            return;
        }
    }
    for (uint32_t st = 0; st < R; ++st) {
        const uint32_t sft = DEC ? R - 1 - st : st;
        const size_t h = hs << sft;
        col_stage_sweep<F, DEC>(tile, ta + (e - 2 * h), tb + (e - 2 * h), sft, log_c, log_hs, c0, (halves * T) >> 1, tid, tc ? tc + (e - 2 * h) : nullptr);   // pairs never cross a tile (row distance < 2^R)
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// LDS-fused butterfly stages, "column kernel": the R = kb-ka+1 consecutive stages ka..kb whose pair
// distances (h_ka = hs*2^(R-1) ... h_kb = hs) are too large for a contiguous tile.  A workgroup
// gathers 2^R rows spaced hs apart, 2^log_c contiguous elements each (>= 4 KiB per row for R <= 4 on
// secp256k1: fully coalesced), runs the R stages in LDS and scatters the rows back.  DECOMPOSE runs
// ka -> kb (large distance first), RECOMBINE kb -> ka.  Table index of the pair (row r, column c) at
// stage k: (r mod d)*hs + c_global with d = 2^(kb-k).
// ---------------------------------------------------------------------------------------------
template <class F, bool DECOMPOSE, int LOG_TILE_CT, bool SYM = false>     // LOG_TILE_CT > 0: log2(tile elements) known at compile time
__global__ __launch_bounds__(kBlockLds, ECFFT_MIN_WAVES) void k_stages_col(IoDesc<F> io,
                                                           const typename F::telem* __restrict__ ta,   // np0 | p0
                                                           const typename F::telem* __restrict__ tb,   // dinv | p1
                                                           uint32_t log_e, uint32_t ka, uint32_t kb, uint32_t log_c,
                                                           const typename F::telem* __restrict__ tc,    // np0*dinv (pair-split decompose) | unused
                                                           uint32_t log_v) {  // 4-byte fast path only: 2^log_v consecutive spans per workgroup
    // log_v = 1: two consecutive 2h_ka-spans (same column chunk) share one workgroup — every span of a stage reads the SAME table
    // entries, so their constants are loaded once for both (halves the table traffic of the HBM-bound column passes)
    using E = typename F::elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char ecfft_smem[];
    E* tile = reinterpret_cast<E*>(ecfft_smem);
    const uint32_t R = kb - ka + 1, tid = threadIdx.x;
    const uint32_t C = 1u << log_c, T = LOG_TILE_CT > 0 ? (1u << LOG_TILE_CT) : (C << R);
    const size_t e = (size_t)1 << log_e, emask = e - 1;
    const uint32_t log_hs = log_e - kb - 1;
    const size_t hs = (size_t)1 << log_hs;
    const uint32_t chunks_log = log_hs - log_c;                      // column chunks per 2h_ka block
    const size_t blk = ((size_t)blockIdx.x >> chunks_log) << log_v, chunk = (size_t)blockIdx.x & (((size_t)1 << chunks_log) - 1);
    const size_t B = (blk << (log_hs + R)) + (chunk << log_c);       // position of (row 0, col 0)
    const size_t c0 = (chunk << log_c);                              // column offset inside the hs-block
    constexpr bool kFast = sizeof(E) == 4 && ECFFT_COL_PAD == 0 && LOG_TILE_CT > 0 && (1u << (LOG_TILE_CT > 0 ? LOG_TILE_CT : 0)) == kBlockLds * 16;
    bool vio = false;
    if constexpr (kFast) vio = log_c >= 2 && vio_ok<F>(io, log_e);
    const uint32_t log_T = log_c + R;
    auto pos_of = [=](uint32_t j) { const uint32_t jj = j & (T - 1); return B + ((size_t)(j >> log_T) << (log_hs + R)) + ((size_t)(jj >> log_c) << log_hs) + (jj & (C - 1)); };
    if constexpr (kFast) {
        if (log_v && !vio) return;                                   // host only pairs spans on the vector path (never taken)
        if (vio) {
            // paired spans: two batches of four quads per thread (one batch of eight needs > 128 VGPRs and spills)
#ifndef ECFFT_EXP_NO_TILE_IO
#pragma unroll 1
            for (uint32_t b = 0; b < (1u << log_v); ++b) vio_load<F, 4, kBlockLds>(io, emask, tile, pos_of, tid + b * 4u * kBlockLds);
#endif
            __syncthreads();
            col_stages<F, DECOMPOSE>(tile, ta, tb, R, log_c, log_hs, c0, e, tid, 1u << log_v, nullptr);
#ifndef ECFFT_EXP_NO_TILE_IO
#pragma unroll 1
            for (uint32_t b = 0; b < (1u << log_v); ++b) vio_store<F, 4, kBlockLds>(io, log_e, tile, pos_of, tid + b * 4u * kBlockLds);
#endif
            return;
        }
    }
    if (!vio) {
#ifndef ECFFT_EXP_NO_TILE_IO
#pragma unroll
        for (uint32_t j = tid; j < T; j += kBlockLds) {
            uint32_t r = j >> log_c, cc = j & (C - 1);
            tile[r * col_row_stride<E>(C) + cc] = io_load<F>(io, B + ((size_t)r << log_hs) + cc, emask);
        }
#endif
    }
    __syncthreads();
    col_stages<F, DECOMPOSE, SYM>(tile, ta, tb, R, log_c, log_hs, c0, e, tid, 1, DECOMPOSE ? tc : nullptr);
#ifndef ECFFT_EXP_NO_TILE_IO
#pragma unroll
    for (uint32_t j = tid; j < T; j += kBlockLds) {
        uint32_t r = j >> log_c, cc = j & (C - 1);
        io_store<F>(io, B + ((size_t)r << log_hs) + cc, log_e, tile[r * col_row_stride<E>(C) + cc]);
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// Two consecutive EXTEND cores of an EXIT level meet at a column pass: core A ends with the recombine stages kb..ka,
// core B (opposite direction, SAME point set: A's target parity = B's source parity) starts with the decompose stages
// ka..kb on the same tiles, with only a pointwise step in between.  This kernel runs both halves on one tile residency:
// load, R recombine stages, io_mid (A's store operator + B's load operator), R decompose stages, store — one launch and
// one HBM round trip instead of two.
// ---------------------------------------------------------------------------------------------
template <class F, bool SYM = false>
__global__ __launch_bounds__(kBlockLds, ECFFT_MIN_WAVES) void k_stages_col_mid(IoDesc<F> io,
                                                               const typename F::telem* __restrict__ p0, const typename F::telem* __restrict__ p1,
                                                               const typename F::telem* __restrict__ np0, const typename F::telem* __restrict__ dinv,
                                                               uint32_t log_e, uint32_t ka, uint32_t kb, uint32_t log_c,
                                                               const typename F::telem* __restrict__ c0t, uint32_t log_v) {
    using E = typename F::elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char ecfft_smem[];
    E* tile = reinterpret_cast<E*>(ecfft_smem);
    const uint32_t R = kb - ka + 1, tid = threadIdx.x;
    const uint32_t C = 1u << log_c, T = C << R;
    const size_t e = (size_t)1 << log_e, emask = e - 1;
    const uint32_t log_hs = log_e - kb - 1;
    const size_t hs = (size_t)1 << log_hs;
    const uint32_t chunks_log = log_hs - log_c;
    const size_t blk = ((size_t)blockIdx.x >> chunks_log) << log_v, chunk = (size_t)blockIdx.x & (((size_t)1 << chunks_log) - 1);
    const size_t B = (blk << (log_hs + R)) + (chunk << log_c);
    const size_t c0 = (chunk << log_c);
    const uint32_t log_T = log_c + R;
    auto pos_of = [=](uint32_t j) { const uint32_t jj = j & (T - 1); return B + ((size_t)(j >> log_T) << (log_hs + R)) + ((size_t)(jj >> log_c) << log_hs) + (jj & (C - 1)); };
    bool vio = false;
    if constexpr (sizeof(E) == 4 && ECFFT_COL_PAD == 0) {
        IoDesc<F> chk = io; chk.src_stride = 1; chk.src_off = 0;           // this kernel reads src plainly and stores plainly
        const int m = io.st_mode;
        vio = T == kBlockLds * 16 && log_c >= 2 && (m == ST_PLAIN || m == ST_SCALE || m == ST_AXPBY) && vio_ok<F>(chk, log_e);
        if (log_v && !vio) return;                                   // host only pairs spans on the vector path (never taken)
        if (vio) {
            IoDesc<F> pl = io; pl.src_stride = 1; pl.src_off = 0; pl.ld_mode = LD_PLAIN; pl.st_mode = ST_PLAIN;
#pragma unroll 1
            for (uint32_t b = 0; b < (1u << log_v); ++b) vio_load<F, 4, kBlockLds>(pl, emask, tile, pos_of, tid + b * 4u * kBlockLds);
            __syncthreads();
            col_stages<F, false>(tile, p0, p1, R, log_c, log_hs, c0, e, tid, 1u << log_v);
#pragma unroll 1
            for (uint32_t b = 0; b < (2u << log_v); ++b) vio_mid<F, 2, kBlockLds>(io, log_e, tile, pos_of, tid + b * 2u * kBlockLds);   // 2 quads at a time: 4 spill
            __syncthreads();
            col_stages<F, true>(tile, np0, dinv, R, log_c, log_hs, c0, e, tid, 1u << log_v, nullptr);
#pragma unroll 1
            for (uint32_t b = 0; b < (1u << log_v); ++b) vio_store<F, 4, kBlockLds>(pl, log_e, tile, pos_of, tid + b * 4u * kBlockLds);
            return;
        }
    }
#ifndef ECFFT_EXP_NO_TILE_IO
    for (uint32_t j = tid; j < T; j += kBlockLds) {
        uint32_t r = j >> log_c, cc = j & (C - 1);
        tile[r * col_row_stride<E>(C) + cc] = io.src[B + ((size_t)r << log_hs) + cc];
    }
#endif
    __syncthreads();
    col_stages<F, false, SYM>(tile, p0, p1, R, log_c, log_hs, c0, e, tid);
#ifndef ECFFT_EXP_NO_MID
    for (uint32_t j = tid; j < T; j += kBlockLds) {
        uint32_t r = j >> log_c, cc = j & (C - 1);
        { const uint32_t q = r * col_row_stride<E>(C) + cc; tile[q] = io_mid<F>(io, B + ((size_t)r << log_hs) + cc, emask, tile[q]); }
    }
#endif
    __syncthreads();
    col_stages<F, true, SYM>(tile, np0, dinv, R, log_c, log_hs, c0, e, tid, 1, c0t);
#ifndef ECFFT_EXP_NO_TILE_IO
    for (uint32_t j = tid; j < T; j += kBlockLds) {
        uint32_t r = j >> log_c, cc = j & (C - 1);
        data_st(&io.dst[B + ((size_t)r << log_hs) + cc], F::canon(tile[r * col_row_stride<E>(C) + cc]), io.nt_st);
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// The LAST column pass of an ENTER level's EXTEND (recombine stages kb..0) fused with the level's combine step
// (src/fftree.rs:155-159).  The combine needs U1~[i] and V1~[i] — the same column of two ADJACENT vectors of the batched
// EXTEND — so one workgroup takes both vectors' column tiles: rows 0..2^R-1 = vector 2b (U), rows 2^R..2^(R+1)-1 = vector
// 2b+1 (V), R = kb+1, C columns each (64 KiB of LDS).  The stage sweeps never pair across the two halves (row distance
// <= 2^(R-1)) and both halves read the same table entries.  Store: even = u0 + xe*v0, odd = w1*U1~ + w1x*V1~, interleaved,
// straight to the level's output — the separate combine launch (3n element moves for 1.5n multiplies, HBM-bound) and the
// EXTEND's write + re-read of its result are gone.
// ---------------------------------------------------------------------------------------------
template <class F, bool SYM = false>
__global__ __launch_bounds__(kBlockLds, ECFFT_MIN_WAVES) void k_stages_col_enter(const typename F::elem* __restrict__ work, const typename F::elem* __restrict__ src,
                                                                 typename F::elem* __restrict__ dst,
                                                                 const typename F::telem* __restrict__ p0, const typename F::telem* __restrict__ p1,
                                                                 const typename F::telem* __restrict__ xe, const typename F::telem* __restrict__ w1,
                                                                 const typename F::telem* __restrict__ w1x,
                                                                 uint32_t log_e, uint32_t kb, uint32_t log_c) {
    using E = typename F::elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char ecfft_smem[];
    E* tile = reinterpret_cast<E*>(ecfft_smem);
    const uint32_t R = kb + 1, tid = threadIdx.x;
    const uint32_t C = 1u << log_c, T = C << (R + 1), RS = col_row_stride<E>(C);
    const size_t e = (size_t)1 << log_e;
    const uint32_t log_hs = log_e - R;                               // hs = e >> R: row spacing; 2^R rows span one vector
    const size_t hs = (size_t)1 << log_hs;
    const uint32_t chunks_log = log_hs - log_c;
    const size_t b = (size_t)blockIdx.x >> chunks_log, chunk = (size_t)blockIdx.x & (((size_t)1 << chunks_log) - 1);
    const size_t c0 = chunk << log_c;
    const size_t B = (b << (log_e + 1)) + c0;                        // position of (row 0, col 0) of the U vector
    bool vio = false;
    if constexpr (sizeof(E) == 4 && ECFFT_COL_PAD == 0) {
        auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
        vio = T == kBlockLds * 32 && log_c >= 2 && al(work) && al(src) && al(dst) && al(xe) && al(w1) && al(w1x);
        if (vio) {
#ifndef ECFFT_EXP_NO_TILE_IO
            Quad d[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint32_t j = 4u * (tid + (uint32_t)c * kBlockLds), r = j >> log_c, cc = j & (C - 1);
                d[c] = ldq(work + ECFFT_DPOS(B + ((size_t)(r >> R) << log_e) + ((size_t)(r & ((1u << R) - 1)) << log_hs) + cc));
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) stq(tile + 4u * (tid + (uint32_t)c * kBlockLds), d[c]);
#endif
            __syncthreads();
            col_stages<F, false>(tile, p0, p1, R, log_c, log_hs, c0, e, tid, 2);
#ifdef ECFFT_EXP_NO_TILE_IO
            return;
#endif
            const size_t bb0 = b << (log_e + 1);
#pragma unroll 1
            for (int cb = 0; cb < 4; cb += 2)
                vio_enter_store<F, 2>(tile, src, dst, xe, w1, w1x, e, [=](int c, uint32_t& ju, uint32_t& jv, size_t& i, size_t& bb) {
                    const uint32_t j = 4u * (tid + (uint32_t)c * kBlockLds), r = j >> log_c, cc = j & (C - 1);
                    ju = j; jv = j + (C << R); i = ((size_t)r << log_hs) + c0 + cc; bb = bb0;
                }, cb);
            return;
        }
    }
#ifndef ECFFT_EXP_NO_TILE_IO
#pragma unroll
    for (uint32_t j = tid; j < T; j += kBlockLds) {
        const uint32_t r = j >> log_c, cc = j & (C - 1);            // r < 2^(R+1): r >> R selects the vector
        tile[r * RS + cc] = work[B + ((size_t)(r >> R) << log_e) + ((size_t)(r & ((1u << R) - 1)) << log_hs) + cc];
    }
#endif
    __syncthreads();
    // the U rows and the V rows are two independent column tiles that read the same table entries
    col_stages<F, false, SYM>(tile, p0, p1, R, log_c, log_hs, c0, e, tid, 2);
#ifdef ECFFT_EXP_NO_TILE_IO
    return;
#endif
#pragma unroll
    for (uint32_t j = tid; j < (T >> 1); j += kBlockLds) {
        const uint32_t r = j >> log_c, cc = j & (C - 1);
        const size_t i = ((size_t)r << log_hs) + c0 + cc, bb = b << (log_e + 1);
        const E u0 = src[bb + i], v0 = src[bb + e + i];
        const E ev = F::tmul_add(xe[i], v0, u0);
        const E od = F::tmul_add(w1x[i], tile[((1u << R) + r) * RS + cc], F::tmul(w1[i], tile[r * RS + cc]));
        dst[bb + 2 * i] = F::canon(ev);
        dst[bb + 2 * i + 1] = F::canon(od);
    }
}

// ---------------------------------------------------------------------------------------------
// Whole low levels of ENTER / EXIT in LDS.  Level m <= tile only touches data inside one tile-aligned
// block, so the first log(tile) levels of ENTER (bottom-up) and the last log(tile) levels of EXIT
// (top-down) run in ONE launch with a single HBM round trip: every pre-scale, butterfly stage and
// pointwise step of those levels happens in LDS.  `LevelTables` is the per-tree table set of
// device_tree.h (DeviceChain::Tree), indexed by log2(m).
// ---------------------------------------------------------------------------------------------
template <class F>
struct LevelTables {
    using E = typename F::elem;
    using TE = typename F::telem;
    size_t m, e; unsigned log_m;
    // butterfly / fused pointwise constants, in the form the kernels multiply by (F::telem)
    TE *p0[2], *p1[2], *np0[2], *dinv[2];
    TE *w[2], *winv[2];
    TE *xe, *w1x, *A1, *B1, *NB2, *C1, *D1, *xie;
    TE *inner[2];   // inner[srcpar] = {c0, c1}: the merged innermost (h = 1) decompose+recombine stage, out_j = a + c_j*(b - a)
    TE *c0t[2];     // c0t[s] = np0[s]*dinv[s]: decompose as two INDEPENDENT multiplies, q0 = a + c0t*(b - a), q1 = dinv*(b - a) (pair-split sweeps)
    E *xnn, *xnn_inv, *z0_s1, *z1_s0, *z0_inv_s1, *z1_inv_s0, *z0z0, *z1z1;
    // blk16_A[srcpar] / blk16_K[srcpar]: the innermost 16-point map of an EXTEND from parity srcpar as int8 matrices + accumulator
    // seeds for the matrix cores (mfma_blk16.h); nullptr: the VALU sweeps run (4-byte fields, trees with e < 16, shard contexts)
    const uint8_t* blk16_A[2]; const unsigned long long* blk16_K[2];
    // low16_A / _K (only in the entry of the tree with 16 leaves): levels 1..4 of ENTER [0] and levels 4..1 of EXIT [1] of a 16-block
    // as ONE 16 x 16 map in the same form - every 16-block of a transform goes through the same four levels on the same tables
    const uint8_t* low16_A[2]; const unsigned long long* low16_K[2];
    // low32_A / _K (only in the entry of the tree with 32 leaves; round 4): levels 1..5 of ENTER [0] / 5..1 of EXIT [1] of a 32-block as
    // ONE 32 x 32 map (1 MiB of matrices each, Blk16::phase32); nullptr: low16 (or the level code) runs
    const uint8_t* low32_A[2]; const unsigned long long* low32_K[2];
    // three-core EXIT level (reduction over Z1, device_tree.h exit_levels): the Z1 counterparts of A1, B1, NB2, C1, D1 and the
    // coefficient of the last store; nullptr: the level runs the four-core form
    TE *zA1, *zB1, *zNB2, *zC1, *zD1, *zNB3;
};

// ---------------------------------------------------------------------------------------------
// Register-resident, one-element-per-thread stage engine for 32-byte fields in the latency regime (tiles of at most one
// element per thread).  The pair-split sweeps above pay an LDS round trip and TWO workgroup barriers per stage for ONE
// multiply of work; here thread `tid` keeps element `tid` of the tile in registers through every in-tile stage and fetches its
// partner tid ^ h with eight cross-lane moves whenever h < 64 (same wave: no LDS traffic, no barrier), through LDS otherwise.
// Roles are per lane: bit lh of tid says whether the thread produces the low or the high output of its pair — one multiply
// each, decompose through c0t = np0*dinv as in the pair-split form, the hi role as t*d + 0 so divergent lanes share ONE
// instruction stream.  Stages k_first .. log_e-1 of vectors of length e = 2^log_e laid end to end in a[0, len); tables are
// the per-tree bases (entry e - 2h + i).  `a` must have been published with a barrier; ends with a barrier.
// ---------------------------------------------------------------------------------------------
#ifndef ECFFT_REG_ENGINE
#define ECFFT_REG_ENGINE 1
#endif
#ifndef ECFFT_N16_DEPTH2W
#define ECFFT_N16_DEPTH2W 2     // units of constant matrices in flight in the two-wave 16x16x64 phases of k_exit_low<8,128> (1: 252 instead of 284 VGPRs, measured 0.6-1.2 % slower)
#endif
#ifndef ECFFT_CORE_OPAQUE_TID
#define ECFFT_CORE_OPAQUE_TID 1  // lds_extend_core: per-call opaque thread index (no hoisting of its LDS addresses out of the callers' level loops)
#endif
#ifndef ECFFT_LDS_SWZ
#define ECFFT_LDS_SWZ 1      // k_exit_low<10,512>: XOR-swizzled LDS layout of the 32-byte elements (A/B: -DECFFT_LDS_SWZ=0)
#endif
// LDS layout of an array of 32-byte elements that ds_read_b128 / ds_write_b128 reach without bank conflicts (round 4): the 16-byte
// chunks 2j, 2j + 1 of element j are XOR-ed with (j >> 3) & 3 inside their 256-byte row (16 chunks = all 64 banks).  A wave-wide
// access takes the same half of each element: in the plain layout the 16 lanes of one of ds_read_b128's groups hit every second bank
// quad twice for consecutive elements (2-way: the 2.1x of SQ_LDS_BANK_CONFLICT over active LDS cycles in k_exit_low) and every fourth
// one four times for the stride-2 de-interleaving reads; with the XOR both patterns cover all sixteen quads.
template <class F, bool SWZ>
__device__ __forceinline__ typename F::elem lds_get(const typename F::elem* a, uint32_t j) {
    if constexpr (SWZ && sizeof(typename F::elem) == 32) {
        const uint4* p = reinterpret_cast<const uint4*>(a);
        const uint32_t sx = (j >> 3) & 3u;
        const uint4 lo = p[(2 * j) ^ sx], hi = p[(2 * j + 1) ^ sx];
        typename F::elem r; r.l[0] = lo.x; r.l[1] = lo.y; r.l[2] = lo.z; r.l[3] = lo.w; r.l[4] = hi.x; r.l[5] = hi.y; r.l[6] = hi.z; r.l[7] = hi.w;
        return r;
    } else return a[j];
}
template <class F, bool SWZ>
__device__ __forceinline__ void lds_put(typename F::elem* a, uint32_t j, const typename F::elem& x) {
    if constexpr (SWZ && sizeof(typename F::elem) == 32) {
        uint4* p = reinterpret_cast<uint4*>(a);
        const uint32_t sx = (j >> 3) & 3u;
        p[(2 * j) ^ sx] = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
        p[(2 * j + 1) ^ sx] = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
    } else a[j] = x;
}
template <class F>
__device__ __forceinline__ typename F::elem lane_xor(const typename F::elem& x, uint32_t h) {
    typename F::elem r;
#pragma unroll
    for (int w = 0; w < 8; ++w) r.l[w] = (uint32_t)__shfl_xor((int)x.l[w], (int)h);
    return r;
}
template <class F>
__device__ __forceinline__ typename F::elem lane_sel(bool c, const typename F::elem& p, const typename F::elem& q) {
    typename F::elem r;
#pragma unroll
    for (int w = 0; w < 8; ++w) r.l[w] = c ? p.l[w] : q.l[w];
    return r;
}
// ---------------------------------------------------------------------------------------------
// Column passes of the LATENCY regime (round 4): 256-element column tiles (2^R rows x C columns), ONE element per thread kept in
// registers through the R stages — the column-tile counterpart of reg_extend32 / k_stages_row256.  Thread tid holds (row
// tid >> log_c, column tid & (C - 1)); its partner at stage s' (row distance d = 2^s') is thread tid ^ (d C): eight cross-lane
// moves when d C < 64, an LDS exchange otherwise.  One multiply per thread per stage (decompose through c0t = np0 dinv), the roles
// sharing one instruction stream as in reg_extend32.  Same arithmetic, same order as col_stage_sweep: bit-identical.
// `a`: 256 (or, two vectors per workgroup, 512) elements of LDS for the exchanges.
// ---------------------------------------------------------------------------------------------
template <class F, bool DEC>
__device__ __forceinline__ void reg_col_stages(typename F::elem& x, typename F::elem* a, uint32_t R, uint32_t log_c, uint32_t log_hs, uint32_t c0, uint32_t e,
                                               const typename F::telem* __restrict__ ta,     // DEC: c0t = np0*dinv | p0
                                               const typename F::telem* __restrict__ tb,     // DEC: dinv | p1
                                               uint32_t tid) {
    using E = typename F::elem;
    using TE = typename F::telem;
    static_assert(sizeof(E) == 32, "32-byte fields");
    const uint32_t cc = tid & ((1u << log_c) - 1), r = tid >> log_c;        // r may carry a vector-select bit above bit R - 1
    for (uint32_t st = 0; st < R; ++st) {
        const uint32_t sft = DEC ? R - 1 - st : st, d = 1u << sft, h = d << log_c;
        const bool hi = (r >> sft) & 1u;
        const uint32_t ti = (e - 2u * ((1u << log_hs) << sft)) + ((r & (d - 1)) << log_hs) + c0 + cc;
        const TE t = hi ? ldt(tb, ti) : ldt(ta, ti);
        E xp;
        if (h < 64) xp = lane_xor<F>(x, h);
        else { __syncthreads(); a[tid] = x; __syncthreads(); xp = a[tid ^ h]; }
        const E A = lane_sel<F>(hi, xp, x), B = lane_sel<F>(hi, x, xp);
        if (DEC) x = F::tmul_add(t, F::sub(B, A), lane_sel<F>(hi, F::zero(), A));     // lo: a + c0t*(b - a)   hi: dinv*(b - a)
        else x = F::tmul_add(t, B, A);                                               // a + p*b
    }
}

// k_stages_col for 256-element tiles: see reg_col_stages
template <class F, bool DECOMPOSE>
__global__ __launch_bounds__(256, 2) void k_stages_col256(IoDesc<F> io, const typename F::telem* __restrict__ ta, const typename F::telem* __restrict__ tb,
                                                          uint32_t log_e, uint32_t ka, uint32_t kb, uint32_t log_c) {
    using E = typename F::elem;
    if constexpr (sizeof(E) == 32) {
        __shared__ E xch[256];
        const uint32_t R = kb - ka + 1, tid = threadIdx.x;
        const uint32_t log_hs = log_e - kb - 1, chunks_log = log_hs - log_c;
        const size_t blk = (size_t)blockIdx.x >> chunks_log, chunk = (size_t)blockIdx.x & (((size_t)1 << chunks_log) - 1);
        const uint32_t c0 = (uint32_t)(chunk << log_c);
        const size_t pos = (blk << (log_hs + R)) + c0 + ((size_t)(tid >> log_c) << log_hs) + (tid & ((1u << log_c) - 1));
        E x = io_load<F>(io, pos, ((size_t)1 << log_e) - 1);
        reg_col_stages<F, DECOMPOSE>(x, xch, R, log_c, log_hs, c0, 1u << log_e, ta, tb, tid);
        io_store<F>(io, pos, log_e, x);
    }
}
// k_stages_col_mid for 256-element tiles
template <class F>
__global__ __launch_bounds__(256, 2) void k_stages_col_mid256(IoDesc<F> io, const typename F::telem* __restrict__ p0, const typename F::telem* __restrict__ p1,
                                                              const typename F::telem* __restrict__ c0t, const typename F::telem* __restrict__ dinv,
                                                              uint32_t log_e, uint32_t ka, uint32_t kb, uint32_t log_c) {
    using E = typename F::elem;
    if constexpr (sizeof(E) == 32) {
        __shared__ E xch[256];
        const uint32_t R = kb - ka + 1, tid = threadIdx.x;
        const uint32_t log_hs = log_e - kb - 1, chunks_log = log_hs - log_c;
        const size_t blk = (size_t)blockIdx.x >> chunks_log, chunk = (size_t)blockIdx.x & (((size_t)1 << chunks_log) - 1);
        const uint32_t c0 = (uint32_t)(chunk << log_c);
        const size_t pos = (blk << (log_hs + R)) + c0 + ((size_t)(tid >> log_c) << log_hs) + (tid & ((1u << log_c) - 1));
        E x = io.src[pos];
        reg_col_stages<F, false>(x, xch, R, log_c, log_hs, c0, 1u << log_e, p0, p1, tid);
        x = io_mid<F>(io, pos, ((size_t)1 << log_e) - 1, x);
        reg_col_stages<F, true>(x, xch, R, log_c, log_hs, c0, 1u << log_e, c0t, dinv, tid);
        data_st(&io.dst[pos], F::canon(x), io.nt_st);
    }
}
// k_stages_col_enter for 256-element tiles: 512 threads, thread tid < 256 holds the U element, tid >= 256 the V element of the same
// column position; the combine's odd output w1 U + w1x V is one multiply per thread and an addition
template <class F>
__global__ __launch_bounds__(512, 2) void k_stages_col_enter256(const typename F::elem* __restrict__ work, const typename F::elem* __restrict__ src,
                                                                typename F::elem* __restrict__ dst,
                                                                const typename F::telem* __restrict__ p0, const typename F::telem* __restrict__ p1,
                                                                const typename F::telem* __restrict__ xe, const typename F::telem* __restrict__ w1,
                                                                const typename F::telem* __restrict__ w1x,
                                                                uint32_t log_e, uint32_t kb, uint32_t log_c) {
    using E = typename F::elem;
    if constexpr (sizeof(E) == 32) {
        __shared__ E xch[512];
        const uint32_t R = kb + 1, tid = threadIdx.x;
        const uint32_t log_hs = log_e - R, chunks_log = log_hs - log_c;
        const size_t b = (size_t)blockIdx.x >> chunks_log, chunk = (size_t)blockIdx.x & (((size_t)1 << chunks_log) - 1);
        const uint32_t c0 = (uint32_t)(chunk << log_c);
        const uint32_t rf = tid >> log_c, v = rf >> R, r = rf & ((1u << R) - 1), cc = tid & ((1u << log_c) - 1);
        const size_t i = ((size_t)r << log_hs) + c0 + cc, bb = b << (log_e + 1), e = (size_t)1 << log_e;
        E x = work[bb + ((size_t)v << log_e) + i];
        reg_col_stages<F, false>(x, xch, R, log_c, log_hs, c0, 1u << log_e, p0, p1, tid);
        const E y = F::tmul(v ? ldt(w1x, (uint32_t)i) : ldt(w1, (uint32_t)i), x);
        __syncthreads();
        xch[tid] = y;
        __syncthreads();
        if (v) dst[bb + 2 * i] = F::canon(F::tmul_add(ldt(xe, (uint32_t)i), src[bb + e + i], src[bb + i]));
        else dst[bb + 2 * i + 1] = F::canon(F::add(xch[tid], xch[tid + 256]));
    }
}

template <class F, int BLK, bool SWZ>
__device__ __forceinline__ void reg_extend32(typename F::elem* a, uint32_t len, uint32_t log_e, uint32_t k_first,
                                             const typename F::telem* __restrict__ c0t, const typename F::telem* __restrict__ dinv,
                                             const typename F::telem* __restrict__ p0, const typename F::telem* __restrict__ p1,
                                             const typename F::telem* __restrict__ inner, uint32_t tid,
                                             const uint8_t* __restrict__ blkA, const unsigned long long* __restrict__ blkK) {
    // blkA != nullptr (len == BLK == 512, 256 or 128, log_e - k_first >= 4): the stages with pair distance <= 8 run on the matrix cores
    using E = typename F::elem;
    using TE = typename F::telem;
    static_assert(sizeof(E) == 32, "32-byte fields");
    const bool act = tid < len;                                             // len is a multiple of 64: wave-uniform
    const size_t e = (size_t)1 << log_e;
    // SWZ: `a` is read and written in the XOR-swizzled layout (lds_get / lds_put); the matrix-core phase uses its own operand layout
    E x = act ? lds_get<F, SWZ>(a, tid) : F::zero();
    auto partner = [&](uint32_t h) -> E {
        if (h < 64) return act ? lane_xor<F>(x, h) : x;
        __syncthreads();                                                    // readers of the previous LDS exchange are done
        if (act) lds_put<F, SWZ>(a, tid, x);
        __syncthreads();
        return act ? lds_get<F, SWZ>(a, tid ^ h) : x;
    };
    const uint32_t k_inner = log_e ? log_e - 1 : 0;
    bool mfma = false;
    if constexpr (BLK == 512 || BLK == 256 || BLK == 128) mfma = blkA != nullptr;
    const uint32_t k_dec_end = mfma ? log_e - 4 : k_inner;
    for (uint32_t k = k_first; k < k_dec_end; ++k) {
        const uint32_t lh = log_e - k - 1, h = 1u << lh;
        const bool hi = (tid >> lh) & 1u;
        const uint32_t off = (uint32_t)(e - 2 * (size_t)h) + (tid & (h - 1));
        TE t; if (act) t = hi ? ldt(dinv, off) : ldt(c0t, off);
        const E xp = partner(h);
        if (act) {
            const E A = lane_sel<F>(hi, xp, x), B = lane_sel<F>(hi, x, xp);
            x = F::tmul_add(t, F::sub(B, A), lane_sel<F>(hi, F::zero(), A));   // lo: a + c0t*(b - a)   hi: dinv*(b - a)
        }
    }
    if constexpr (BLK == 512 || BLK == 256 || BLK == 128) {
        if (mfma) {                                                         // len == BLK: every thread holds an element
            if constexpr (BLK == 512) x = Blk16::phase512_regs(a, x, blkA, blkK, tid);
            else x = Blk16::phase_n16_regs<BLK / 64, (BLK == 128 ? ECFFT_N16_DEPTH2W : 2)>(a, x, blkA, blkK, tid);   // small launches: v_mfma_i32_16x16x64_i8
        }
    }
    if (log_e > 0 && k_first <= k_inner && !mfma) {                         // merged innermost stage pair (h = 1)
        const bool hi = tid & 1u;
        TE t; if (act) t = ldt(inner, hi ? 1u : 0u);
        const E xp = partner(1);
        if (act) {
            const E A = lane_sel<F>(hi, xp, x), B = lane_sel<F>(hi, x, xp);
            x = F::tmul_add(t, F::sub(B, A), A);
        }
    }
    for (uint32_t k = k_dec_end; k-- > k_first;) {
        const uint32_t lh = log_e - k - 1, h = 1u << lh;
        const bool hi = (tid >> lh) & 1u;
        const uint32_t off = (uint32_t)(e - 2 * (size_t)h) + (tid & (h - 1));
        TE t; if (act) t = hi ? ldt(p1, off) : ldt(p0, off);
        const E xp = partner(h);
        if (act) {
            const E A = lane_sel<F>(hi, xp, x), B = lane_sel<F>(hi, x, xp);
            x = F::tmul_add(t, B, A);                                        // a + p*b
        }
    }
    __syncthreads();
    if (act) lds_put<F, SWZ>(a, tid, x);
    __syncthreads();
}

// PAIR-PER-THREAD engine of a 512-element EXTEND core on symmetric tables (k_exit_low<10,512,3,SYM>).  On the
// register engine above both lanes of a pair execute the multiply's instruction stream, so a one-multiply butterfly saves nothing
// there.  Here the VALU stages (pair distance 2^(log_e-1) .. 16 down, then up) run as sym_bfly sweeps on `a` in LDS, one pair per
// thread: 256 pairs on HALF of the workgroup (four waves, 64 consecutive pairs each, so sweeps at distance <= 64 stay inside the
// wave's own 128-element span); the other half only takes part in the barriers.  The sweeping half requests the next sweep's
// constant before the barrier, as row_stages_pipe does.  The matrix-core phase stays on all eight waves.  Same arithmetic on the
// same residues as the general form: the same bytes.  `a` published by a barrier; ends with one.
#ifndef ECFFT_EXIT_LOW_SYM
#define ECFFT_EXIT_LOW_SYM 1          // 0: k_exit_low<10,512,3> keeps the register engine in symmetric contexts (A/B)
#endif
// which four waves sweep: 0 = waves 0..3 (one sweeping wave per SIMD: waves w and w + 4 share one), 1 = the even waves (two on each
// of two SIMDs).  Measured (profiles/low_sym/low_sym_ab.txt): 0 gains 0.07 ms per step on the register engine, 1 nothing.
#ifndef ECFFT_EXIT_LOW_SYM_WAVES
#define ECFFT_EXIT_LOW_SYM_WAVES 0
#endif
template <class F, bool DEC, bool SWZ>
__device__ __forceinline__ void half_stages_pipe(typename F::elem* a, const typename F::telem* __restrict__ tk, uint32_t e, int lh_from, int lh_to,
                                                 uint32_t q, bool sw) {
    using E = typename F::elem;
    using TE = typename F::telem;
    auto geom = [&](int lh, uint32_t& idx, uint32_t& ti) {
        const uint32_t h = 1u << lh, i = q & (h - 1);
        idx = ((q >> lh) << (lh + 1)) + i; ti = e - 2 * h + i;
    };
    uint32_t idx = 0, ti = 0;
    TE nk;
    if (sw) { geom(lh_from, idx, ti); nk = ldt(tk, ti); }
#pragma unroll 1
    for (int lh = lh_from; DEC ? lh >= lh_to : lh <= lh_to; lh += DEC ? -1 : 1) {
        if (sw) {                                                           // wave-uniform
            const TE t = nk;
            const uint32_t lo = idx, up = idx + (1u << lh);
            E x = lds_get<F, SWZ>(a, lo), y = lds_get<F, SWZ>(a, up);
            sym_bfly<F, DEC>(x, y, t);
            lds_put<F, SWZ>(a, lo, x); lds_put<F, SWZ>(a, up, y);
            if (lh != lh_to) { geom(lh + (DEC ? -1 : 1), idx, ti); nk = ldt(tk, ti); }
        }
        const int nxt = lh != lh_to ? lh + (DEC ? -1 : 1) : 99;              // the phase / the caller reads other waves' elements
        if (wave_local_lh(lh) && wave_local_lh(nxt)) wave_local_sync(); else lds_barrier();
    }
}
template <class F, bool SWZ>
__device__ __forceinline__ void pair_extend512(typename F::elem* a, uint32_t log_e, const typename F::telem* __restrict__ dinv, const typename F::telem* __restrict__ p0,
                                               uint32_t tid, const uint8_t* __restrict__ blkA, const unsigned long long* __restrict__ blkK) {
    using E = typename F::elem;
    // log_e in 5 .. 9, 512 elements, 512 threads
    const bool sw = ECFFT_EXIT_LOW_SYM_WAVES ? ((tid >> 6) & 1u) == 0 : tid < 256u;
    const uint32_t q = ECFFT_EXIT_LOW_SYM_WAVES ? (((tid >> 7) << 6) | (tid & 63u)) : (tid & 255u);
    const uint32_t e = 1u << log_e;
    half_stages_pipe<F, true, SWZ>(a, dinv, e, (int)log_e - 1, 4, q, sw);
    E x = lds_get<F, SWZ>(a, tid);
    x = Blk16::phase512_regs(a, x, blkA, blkK, tid);                       // its first barrier: every read above is done
    __syncthreads();                                                        // the phase's swizzled results are read
    lds_put<F, SWZ>(a, tid, x);
    __syncthreads();
    half_stages_pipe<F, false, SWZ>(a, p0, e, 4, (int)log_e - 1, q, sw);
}

// every stage (decompose then recombine) of EXTEND on `len` LDS elements = len/e vectors of length e;
// srcpar = parity of the source moiety.  Ends with a barrier.
// SYM (symmetric tables): the one-pair-per-thread VALU sweeps next to a matrix-core phase (len == 2 * BLK == 1024,
// k_enter_low<10,512>'s cores) run the row kernel's engine: sym_bfly, ONE multiply and one constant per pair, the next sweep's
// constant requested before the barrier.  Every other path keeps the general form.
#ifndef ECFFT_ENTER_LOW_SYM
#define ECFFT_ENTER_LOW_SYM 1   // 0: k_enter_low keeps the general sweeps in symmetric contexts; 2: symmetric sweeps without the constant pipelining (A/B)
#endif
template <class F, int BLK = kBlockLds, bool SWZ = false, bool SYM = false>      // SWZ: `a` in the XOR-swizzled layout — only the register engine (len <= BLK) reads it that way
__device__ __forceinline__ void lds_extend_core(typename F::elem* a, uint32_t len, uint32_t log_e, const LevelTables<F>& T, int srcpar) {
    using E = typename F::elem;
    // The thread index is made opaque per call (32-byte fields): the callers run this core once per LEVEL in a loop, and with a
    // loop-invariant tid the compiler hoists every LDS address of the matrix-core phase's swizzled layout (16 xor-ed offsets and
    // more) out of that loop and keeps them alive across the 110-VGPR multiplies — k_enter_low<10,512> spilled 60 B for it.
    // Recomputing them per call costs a few dozen integer instructions per level.
    uint32_t tid_ = threadIdx.x;
#if ECFFT_CORE_OPAQUE_TID
    if constexpr (sizeof(E) == 32) asm volatile("" : "+v"(tid_));
#endif
    const uint32_t tid = tid_, npairs = len >> 1;
    const size_t e = (size_t)1 << log_e;
    const int tgt = 1 - srcpar;
    // matrix-core form of the stages with pair distance <= 8 (mfma_blk16.h): arrays of 512 (one element per thread) or of whole
    // 1024-element sub-tiles, vectors of >= 16 elements
    const uint8_t* bA = nullptr; const unsigned long long* bK = nullptr;
    if constexpr (sizeof(E) == 32 && BLK == 512) {
        if (log_e >= 4 && (len == 512u || (len & 1023u) == 0)) { bA = T.blk16_A[srcpar]; bK = T.blk16_K[srcpar]; }
    }
    if constexpr (sizeof(E) == 32 && (BLK == 256 || BLK == 128)) {          // latency variants: one element per thread
        if (log_e >= 4 && len == (uint32_t)BLK) { bA = T.blk16_A[srcpar]; bK = T.blk16_K[srcpar]; }
    }
    if constexpr (SYM && sizeof(E) == 32 && BLK == 512 && ECFFT_EXIT_LOW_SYM != 0) {
        // k_exit_low<10,512,3,SYM>'s half-tiles: symmetric pair-per-thread sweeps around the matrix-core phase
        if (len == (uint32_t)BLK && bA && log_e >= 5) { pair_extend512<F, SWZ>(a, log_e, T.dinv[srcpar], T.p0[tgt], tid, bA, bK); return; }
    }
    if constexpr (sizeof(E) == 32 && ECFFT_REG_ENGINE) {
        if (len <= (uint32_t)BLK && (len & 63u) == 0) {
            reg_extend32<F, BLK, SWZ>(a, len, log_e, 0, T.c0t[srcpar], T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.inner[srcpar], tid, len == (uint32_t)BLK ? bA : nullptr, bK);
            return;
        }
    }
    if constexpr (SWZ) __builtin_trap();      // unreachable: the callers that swizzle pass len == BLK
    if constexpr (sizeof(E) == 32) {
        if (len == BLK) {
            // PAIR-SPLIT sweeps (k_exit_low: half as many pairs as threads).  One butterfly = two multiplies; with one pair per
            // thread half the workgroup idles and every sweep costs two dependent 169-instruction multiplies.  Here waves 0..3
            // produce the LOW output of every pair and waves 4..7 the HIGH one, one multiply each (decompose through the extra
            // table c0t = np0*dinv, which makes its two products independent): a sweep costs one multiply of latency and all
            // eight waves issue.  Both roles read (a, b); a barrier separates the reads from the in-place writes.
            const uint32_t g = tid & (npairs - 1);
            const bool hi = tid >= npairs;                                  // wave-uniform: npairs is a multiple of 64
            const uint32_t k_inner = log_e ? log_e - 1 : 0;
            for (uint32_t k = 0; k < k_inner; ++k) {
                const uint32_t lh = log_e - k - 1, h = 1u << lh, i = g & (h - 1), idx = ((g >> lh) << (lh + 1)) + i;
                const size_t off = e - 2 * (size_t)h + i;
                const typename F::telem t = hi ? ldt(T.dinv[srcpar], (uint32_t)off) : ldt(T.c0t[srcpar], (uint32_t)off);
                const E x = a[idx], y = a[idx + h];
                __syncthreads();
                const E d = F::sub(y, x);
                if (hi) a[idx + h] = F::tmul(t, d); else a[idx] = F::tmul_add(t, d, x);
                __syncthreads();
            }
            if (log_e > 0) {
                const typename F::telem t = ldt(T.inner[srcpar], hi ? 1u : 0u);
                const E x = a[2 * g], y = a[2 * g + 1];
                __syncthreads();
                a[2 * g + (hi ? 1 : 0)] = F::tmul_add(t, F::sub(y, x), x);
                __syncthreads();
            }
            for (uint32_t k = k_inner; k-- > 0;) {
                const uint32_t lh = log_e - k - 1, h = 1u << lh, i = g & (h - 1), idx = ((g >> lh) << (lh + 1)) + i;
                const size_t off = e - 2 * (size_t)h + i;
                const typename F::telem t = hi ? ldt(T.p1[tgt], (uint32_t)off) : ldt(T.p0[tgt], (uint32_t)off);
                const E x = a[idx], y = a[idx + h];
                __syncthreads();
                a[idx + (hi ? h : 0)] = F::tmul_add(t, y, x);
                __syncthreads();
            }
            return;
        }
    }
    if constexpr (sizeof(E) == 4) {
        // callers have published `a` with a barrier; the engine starts with one of its own and ends with one
        if (len == BLK * 16) { lds_extend_fast<F, 16, BLK>(a, T.np0[srcpar], T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.inner[srcpar], e, log_e, tid); return; }
        if (len == BLK * 8) { lds_extend_fast<F, 8, BLK>(a, T.np0[srcpar], T.dinv[srcpar], T.p0[tgt], T.p1[tgt], T.inner[srcpar], e, log_e, tid); return; }
    }
    const uint32_t k_inner = log_e ? log_e - 1 : 0;
    bool mfma = false;
    if constexpr (sizeof(E) == 32 && BLK == 512) mfma = bA != nullptr && (len & 1023u) == 0;
    const uint32_t k_dec_end = mfma ? log_e - 4 : k_inner;
    // one-pair-per-thread sweeps (32-byte fields, at least one pair per thread): the sweeps at pair distance <= 64 stay inside the
    // wave's own span, and so does the merged innermost stage — no workgroup barrier between them (wave_local_sync)
    const bool wl = sizeof(E) == 32 && 2 * npairs > (uint32_t)BLK;
    bool symp = false;                                  // symmetric pipelined sweeps at pair distance 2^(log_e-1) .. 16
    if constexpr (SYM && sizeof(E) == 32 && BLK == 512) {
        symp = mfma && npairs == (uint32_t)BLK;
        // to_operand_form reads elements of other waves' spans: the last decompose sweep closes with a workgroup barrier (lh_after = 99)
        if (symp) row_stages_pipe<F, true, true, ECFFT_ENTER_LOW_SYM != 2>(a, T.np0[srcpar], T.dinv[srcpar], (uint32_t)e, (int)log_e - 1, 4, tid);
    }
    if (!symp)
    for (uint32_t k = 0; k < k_dec_end; ++k) {
        const uint32_t lh = log_e - k - 1, h = 1u << lh;
        stage_sweep<F, true, BLK>(a, T.np0[srcpar] + (e - 2 * (size_t)h), T.dinv[srcpar] + (e - 2 * (size_t)h), lh, npairs, tid, T.c0t[srcpar] + (e - 2 * (size_t)h));
        if (wl && wave_local_lh((int)lh) && (k + 1 < k_dec_end || !mfma)) wave_local_sync(); else __syncthreads();
    }
    if constexpr (sizeof(E) == 32 && BLK == 512) {
        if (mfma) {
            Blk16::APre pre = Blk16::prefetch(bA, tid);
            __builtin_amdgcn_sched_barrier(0);
            Blk16::to_operand_form<BLK>(a, len, tid);
#pragma unroll 1
            for (uint32_t o = 0; o < len; o += Blk16::kSub) {
                if (o) { pre = Blk16::prefetch(bA, tid); __builtin_amdgcn_sched_barrier(0); }
                Blk16::phase(a + o, bA, bK, tid, pre);
            }
            Blk16::from_swizzled<BLK>(a, len, tid);
        }
    }
    if (log_e > 0 && !mfma) {                           // merged innermost stage pair (h = 1)
        const typename F::telem c0 = ldt(T.inner[srcpar], 0u), c1 = ldt(T.inner[srcpar], 1u);
        for (uint32_t g = tid; g < npairs; g += BLK) {
            E x = a[2 * g], y = a[2 * g + 1];
            E d = F::sub(y, x);
            a[2 * g] = F::tmul_add(c0, d, x);
            a[2 * g + 1] = F::tmul_add(c1, d, x);
        }
        if (wl && ECFFT_WAVE_LOCAL && k_dec_end > 0) wave_local_sync(); else __syncthreads();
    }
    if constexpr (SYM && sizeof(E) == 32 && BLK == 512) {
        // from_swizzled ended with a workgroup barrier; the last recombine sweep ends the core with one
        if (symp) { row_stages_pipe<F, false, true, ECFFT_ENTER_LOW_SYM != 2>(a, T.p0[tgt], T.p1[tgt], (uint32_t)e, 4, (int)log_e - 1, tid); return; }
    }
    for (uint32_t k = k_dec_end; k-- > 0;) {
        const uint32_t lh = log_e - k - 1, h = 1u << lh;
        stage_sweep<F, false, BLK>(a, T.p0[tgt] + (e - 2 * (size_t)h), T.p1[tgt] + (e - 2 * (size_t)h), lh, npairs, tid);
        if (wl && k > 0 && wave_local_lh((int)lh + 1)) wave_local_sync(); else __syncthreads();
    }
}

// ENTER levels 1 .. log_tile (src/fftree.rs:143-161 for every block of size <= tile).  LDS: 2*tile elements.
// SYM (symmetric contexts of a 32-byte field, 1024-element tiles): the VALU sweeps of the EXTEND cores run sym_bfly (lds_extend_core)
template <class F, int LOG_TILE, int BLK = kBlockLds, bool SYM = false>
__global__ __launch_bounds__(BLK, (BLK >= 512 ? ECFFT_MIN_WAVES : 2)) void k_enter_low(typename F::elem* __restrict__ dst, const typename F::elem* __restrict__ src,
                                                          const LevelTables<F>* __restrict__ trees) {
    using E = typename F::elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char ecfft_smem[];
    constexpr uint32_t log_tile = LOG_TILE, T = 1u << LOG_TILE, npairs = T >> 1;
    constexpr bool kRoles = npairs * 2 == (uint32_t)BLK;    // latency variant: two threads per pair (one output each)
    constexpr int PAIRS = kRoles ? 1 : (int)(npairs / BLK);     // compile-time trip counts keep ev/od in registers
    static_assert(kRoles || (npairs >= (uint32_t)BLK && npairs % BLK == 0), "tile too small for the workgroup");
    const uint32_t tid = threadIdx.x;
    E* cur = reinterpret_cast<E*>(ecfft_smem);
    E* work = cur + T;
    const size_t base = (size_t)blockIdx.x << log_tile;
    constexpr bool kQuad = sizeof(E) == 4 && T % (4 * BLK) == 0;     // 4-byte fields: quad-vectorised, loads-first pointwise steps
    bool qio = false;                                                      // user pointers may be only element-aligned
    if constexpr (kQuad) qio = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    if constexpr (kQuad) {
        if (qio) {
            constexpr int NQ = (int)(T / (4 * BLK));
            Quad d[NQ];
#pragma unroll
            for (int c = 0; c < NQ; ++c) d[c] = ldq(src + base + 4u * (tid + (uint32_t)c * BLK));
#pragma unroll
            for (int c = 0; c < NQ; ++c) stq(cur + 4u * (tid + (uint32_t)c * BLK), d[c]);
        }
    }
    if (!qio) {
        for (uint32_t j = tid; j < T; j += BLK) cur[j] = src[base + j];
    }
    __syncthreads();
    uint32_t l_first = 1;
    if constexpr (sizeof(E) == 32 && LOG_TILE == 10 && BLK == 512) {
        // levels 1..5 on the matrix cores as one 32 x 32 map per 32-block (LevelTables::low32_A), else
        // levels 1..4 as one 16 x 16 map per 16-block (LevelTables::low16_A)
        const uint8_t* lA = trees[4].low16_A[0];
        const uint8_t* lA32 = trees[5].low32_A[0];
        if (lA32) {
            Blk16::to_operand_form32(cur, tid);
            Blk16::phase32(cur, lA32, trees[5].low32_K[0], tid);
            Blk16::from_swizzled32(cur, tid);
            l_first = 6;
        } else if (lA) {
            Blk16::APre pre = Blk16::prefetch(lA, tid);
            __builtin_amdgcn_sched_barrier(0);
            Blk16::to_operand_form<BLK>(cur, T, tid);
            Blk16::phase(cur, lA, trees[4].low16_K[0], tid, pre);
            Blk16::from_swizzled<BLK>(cur, T, tid);
            l_first = 5;
        }
    }
    if constexpr (sizeof(E) == 32 && LOG_TILE == 8 && BLK == 256) {
        // latency variant: the same map on the 16 blocks of the 256-element tile (v_mfma_i32_16x16x64_i8, mfma_blk16.h)
        const uint8_t* lA = trees[4].low16_A[0];
        if (lA) {
            Blk16::phase_n16<4, false>(cur, lA, trees[4].low16_K[0], tid, [&] { Blk16::to_operand_form<BLK>(cur, T, tid); });
            Blk16::from_swizzled<BLK>(cur, T, tid);
            l_first = 5;
        }
    }
    for (uint32_t l = l_first; l <= log_tile; ++l) {
        const LevelTables<F>& L = trees[l];
        const uint32_t le = l - 1, e = 1u << le;
        if constexpr (kQuad) {
            if (le >= 2) {
                constexpr int NQ = (int)(T / (4 * BLK)), NP = NQ / 2;
                {
                    Quad x[NQ], t[NQ];
                    const typename F::telem* wi = L.winv[0];
#pragma unroll
                    for (int c = 0; c < NQ; ++c) { const uint32_t j = 4u * (tid + (uint32_t)c * BLK); t[c] = ldq_tab(wi, j & (e - 1)); x[c] = ldq(cur + j); }
#pragma unroll
                    for (int c = 0; c < NQ; ++c) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) x[c].v[k] = F::tmul(t[c].v[k], x[c].v[k]);
                        stq(work + 4u * (tid + (uint32_t)c * BLK), x[c]);
                    }
                }
                __syncthreads();
                lds_extend_core<F, BLK>(work, T, le, L, 0);
                Quad lo[NP], hi[NP];
                {
                    Quad u0[NP], v0[NP], U1[NP], V1[NP], tx[NP], tw[NP], twx[NP];
                    const typename F::telem *xe = L.xe, *w1 = L.w[1], *w1x = L.w1x;
#pragma unroll
                    for (int c = 0; c < NP; ++c) {
                        const uint32_t g = 4u * (tid + (uint32_t)c * BLK), i = g & (e - 1), bb = (g >> le) << l;
                        tx[c] = ldq_tab(xe, (uint32_t)i); tw[c] = ldq_tab(w1, (uint32_t)i); twx[c] = ldq_tab(w1x, (uint32_t)i);
                        u0[c] = ldq(cur + bb + i); v0[c] = ldq(cur + bb + e + i); U1[c] = ldq(work + bb + i); V1[c] = ldq(work + bb + e + i);
                    }
#pragma unroll
                    for (int c = 0; c < NP; ++c)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const E ev = F::tmul_add(tx[c].v[k], v0[c].v[k], u0[c].v[k]);
                            const E od = F::tmul_add(twx[c].v[k], V1[c].v[k], F::tmul(tw[c].v[k], U1[c].v[k]));
                            if (k < 2) { lo[c].v[2 * k] = ev; lo[c].v[2 * k + 1] = od; } else { hi[c].v[2 * (k - 2)] = ev; hi[c].v[2 * (k - 2) + 1] = od; }
                        }
                }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < NP; ++c) {
                    const uint32_t g = 4u * (tid + (uint32_t)c * BLK), i = g & (e - 1), bb = (g >> le) << l;
                    stq(cur + bb + 2 * i, lo[c]); stq(cur + bb + 2 * i + 4, hi[c]);
                }
                __syncthreads();
                continue;
            }
        }
        for (uint32_t j = tid; j < T; j += BLK) work[j] = F::tmul(ldt(L.winv[0], j & (e - 1)), cur[j]);
        __syncthreads();
        lds_extend_core<F, BLK, false, SYM>(work, T, le, L, 0);
        // combine (:155-159): block [u0|v0] + extended [U1|V1] -> interleaved evaluations; results are held in
        // registers across the barrier because the interleaving store overwrites other threads' inputs
        if constexpr (kRoles) {
            const bool hi = tid >= npairs;
            const uint32_t g = hi ? tid - npairs : tid, i = g & (e - 1), bb = (g >> le) << l;
            E r;
            if (!hi) r = F::tmul_add(ldt(L.xe, i), cur[bb + e + i], cur[bb + i]);
            else r = F::tmul_add(ldt(L.w1x, i), work[bb + e + i], F::tmul(ldt(L.w[1], i), work[bb + i]));
            __syncthreads();
            cur[bb + 2 * i + (hi ? 1 : 0)] = r;
            __syncthreads();
            continue;
        }
        E ev[PAIRS], od[PAIRS];
#pragma unroll
        for (int c = 0; c < PAIRS; ++c) {
            uint32_t g = tid + (uint32_t)c * BLK, i = g & (e - 1), bb = (g >> le) << l;
            E u0 = cur[bb + i], v0 = cur[bb + e + i], U1 = work[bb + i], V1 = work[bb + e + i];
            ev[c] = F::tmul_add(ldt(L.xe, i), v0, u0);
            od[c] = F::tmul_add(ldt(L.w1x, i), V1, F::tmul(ldt(L.w[1], i), U1));
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < PAIRS; ++c) {
            uint32_t g = tid + (uint32_t)c * BLK, i = g & (e - 1), bb = (g >> le) << l;
            cur[bb + 2 * i] = ev[c]; cur[bb + 2 * i + 1] = od[c];
        }
        __syncthreads();
    }
    if constexpr (kQuad) {
        if (qio) {
            constexpr int NQ = (int)(T / (4 * BLK));
#pragma unroll
            for (int c = 0; c < NQ; ++c) {
                Quad q = ldq(cur + 4u * (tid + (uint32_t)c * BLK));
#pragma unroll
                for (int k = 0; k < 4; ++k) q.v[k] = F::canon(q.v[k]);
                stq(dst + base + 4u * (tid + (uint32_t)c * BLK), q);
            }
            return;
        }
    }
    for (uint32_t j = tid; j < T; j += BLK) dst[base + j] = F::canon(cur[j]);
}

// EXIT levels log_tile .. 1 (src/fftree.rs:200-224 with redc_impl :232-259 inlined, normalised form, see
// DeviceChain::exit).  LDS: cur (tile) + G (tile/2) + H (tile/2).
// CORES: the form of a level of the loop, uniform over the launch (the driver instantiates the context's form).
//   4  the reference's: reduction over Z0, four EXTEND cores (S0->S1, S1->S0, S0->S1, S1->S0) and five pointwise steps
//   3  reduction over Z1 (the z* tables): G = zA1 cur[odd]; core S1->S0; G = H = zNB2 G + zB1 cur[even]; core S0->S1; G = zC1 G;
//      core S1->S0; u0 = zNB3 G + zD1 H, v0 = xie (cur[even] - u0) — three cores, 7 multiplies per pair instead of 8
// The matrix-core maps of the lowest levels (low16 / low32) are exact linear maps of the whole levels and serve both forms.
// SYM (symmetric contexts of a 32-byte field, 1024-element tiles, CORES == 3): the cores' VALU stages run on pair_extend512
template <class F, int LOG_TILE, int BLK = kBlockLds, int CORES = 4, bool SYM = false>
__global__ __launch_bounds__(BLK, (BLK >= 512 ? ECFFT_MIN_WAVES : 1)) void k_exit_low(typename F::elem* __restrict__ dst, const typename F::elem* __restrict__ src,
                                                         const LevelTables<F>* __restrict__ trees) {
    using E = typename F::elem;
    static_assert(CORES == 3 || CORES == 4, "three or four EXTEND cores per level");
    constexpr bool k3 = CORES == 3;
    constexpr int par1 = k3 ? 1 : 0;                                        // source parity of the level's first core
    extern __shared__ __attribute__((aligned(16))) unsigned char ecfft_smem[];
    constexpr uint32_t log_tile = LOG_TILE, T = 1u << LOG_TILE, nh = T >> 1;
    constexpr int PAIRS = (int)(nh / BLK);
    static_assert(PAIRS >= 1 && nh % BLK == 0, "tile too small for the workgroup");
    const uint32_t tid = threadIdx.x;
    E* cur = reinterpret_cast<E*>(ecfft_smem);
    E* G = cur + T;
    E* H = G + nh;
    const size_t base = (size_t)blockIdx.x << log_tile;
    constexpr bool kQuad = sizeof(E) == 4 && nh % (4 * BLK) == 0;
    // cur / G / H in the XOR-swizzled layout (lds_get / lds_put: no bank conflicts for consecutive elements) — the 1024-element
    // variant of 32-byte fields, whose EXTEND cores run on the register engine
    constexpr bool kSwz = ECFFT_LDS_SWZ && sizeof(E) == 32 && LOG_TILE == 10 && BLK == 512;
    bool qio = false;                                                      // user pointers may be only element-aligned
    if constexpr (kQuad) qio = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    if constexpr (kQuad) {
        if (qio) {
            constexpr int NQ = (int)(T / (4 * BLK));
            Quad d[NQ];
#pragma unroll
            for (int c = 0; c < NQ; ++c) d[c] = ldq(src + base + 4u * (tid + (uint32_t)c * BLK));
#pragma unroll
            for (int c = 0; c < NQ; ++c) stq(cur + 4u * (tid + (uint32_t)c * BLK), d[c]);
        }
    }
    if (!qio) {
        for (uint32_t j = tid; j < T; j += BLK) lds_put<F, kSwz>(cur, j, src[base + j]);
    }
    __syncthreads();
    bool cur_swz = kSwz;                                                    // the final matrix-core phase leaves `cur` in the plain layout
    uint32_t l_last = 1;
    const uint8_t* lA = nullptr;
    const uint8_t* lA32 = nullptr;
    if constexpr (sizeof(E) == 32 && ((LOG_TILE == 10 && BLK == 512) || (LOG_TILE == 8 && BLK == 128))) { lA = trees[4].low16_A[1]; if (lA) l_last = 5; }
    if constexpr (sizeof(E) == 32 && LOG_TILE == 10 && BLK == 512) { lA32 = trees[5].low32_A[1]; if (lA32) l_last = 6; }
    for (uint32_t l = log_tile; l >= l_last; --l) {
        const LevelTables<F>& L = trees[l];
        const uint32_t le = l - 1, e = 1u << le;
        if constexpr (kQuad) {
            if (le >= 2) {
                // the level's pointwise steps on quads of the pair index g (loads first), the EXTEND cores between them
                constexpr int NP = (int)(nh / (4 * BLK));
                auto gq = [=](int c) { return 4u * (tid + (uint32_t)c * BLK); };
                auto tq = [=](const typename F::telem* t, int c) { return ldq_tab(t, gq(c) & (e - 1)); };
                auto evenq = [=](int c) { uint4 a = *reinterpret_cast<const uint4*>(cur + 2 * gq(c)), b = *reinterpret_cast<const uint4*>(cur + 2 * gq(c) + 4); return Quad{{a.x, a.z, b.x, b.z}}; };
                auto oddq = [=](int c) { uint4 a = *reinterpret_cast<const uint4*>(cur + 2 * gq(c)), b = *reinterpret_cast<const uint4*>(cur + 2 * gq(c) + 4); return Quad{{a.y, a.w, b.y, b.w}}; };
                {
                    Quad t[NP], x[NP];
#pragma unroll
                    for (int c = 0; c < NP; ++c) { t[c] = tq(k3 ? L.zA1 : L.A1, c); x[c] = k3 ? oddq(c) : evenq(c); }
#pragma unroll
                    for (int c = 0; c < NP; ++c) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) x[c].v[k] = F::tmul(t[c].v[k], x[c].v[k]);
                        stq(G + gq(c), x[c]);
                    }
                }
                __syncthreads();
                lds_extend_core<F, BLK>(G, nh, le, L, par1);
                {
                    Quad ta[NP], tb[NP], x[NP], y[NP];
#pragma unroll
                    for (int c = 0; c < NP; ++c) { ta[c] = tq(k3 ? L.zNB2 : L.NB2, c); tb[c] = tq(k3 ? L.zB1 : L.B1, c); x[c] = ldq(G + gq(c)); y[c] = k3 ? evenq(c) : oddq(c); }
#pragma unroll
                    for (int c = 0; c < NP; ++c) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) x[c].v[k] = F::tmul_add(ta[c].v[k], x[c].v[k], F::tmul(tb[c].v[k], y[c].v[k]));
                        stq(G + gq(c), x[c]); stq(H + gq(c), x[c]);
                    }
                }
                __syncthreads();
                lds_extend_core<F, BLK>(G, nh, le, L, 1 - par1);
                {
                    Quad t[NP], x[NP];
#pragma unroll
                    for (int c = 0; c < NP; ++c) { t[c] = tq(k3 ? L.zC1 : L.C1, c); x[c] = ldq(G + gq(c)); }
#pragma unroll
                    for (int c = 0; c < NP; ++c) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) x[c].v[k] = F::tmul(t[c].v[k], x[c].v[k]);
                        stq(G + gq(c), x[c]);
                    }
                }
                __syncthreads();
                lds_extend_core<F, BLK>(G, nh, le, L, par1);
                Quad uq[NP], vq[NP];
                if constexpr (k3) {
                    Quad ta[NP], tb[NP], tc[NP], x[NP], y[NP], z[NP];
#pragma unroll
                    for (int c = 0; c < NP; ++c) { ta[c] = tq(L.zNB3, c); tb[c] = tq(L.zD1, c); tc[c] = tq(L.xie, c); x[c] = ldq(G + gq(c)); y[c] = ldq(H + gq(c)); z[c] = evenq(c); }
#pragma unroll
                    for (int c = 0; c < NP; ++c)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            uq[c].v[k] = F::tmul_add(ta[c].v[k], x[c].v[k], F::tmul(tb[c].v[k], y[c].v[k]));
                            vq[c].v[k] = F::tmul(tc[c].v[k], F::sub(z[c].v[k], uq[c].v[k]));
                        }
                } else {
                    {
                        Quad ta[NP], tb[NP], x[NP], y[NP];
#pragma unroll
                        for (int c = 0; c < NP; ++c) { ta[c] = tq(L.NB2, c); tb[c] = tq(L.D1, c); x[c] = ldq(G + gq(c)); y[c] = ldq(H + gq(c)); }
#pragma unroll
                        for (int c = 0; c < NP; ++c) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) x[c].v[k] = F::tmul_add(ta[c].v[k], x[c].v[k], F::tmul(tb[c].v[k], y[c].v[k]));
                            stq(G + gq(c), x[c]);
                        }
                    }
                    __syncthreads();
                    lds_extend_core<F, BLK>(G, nh, le, L, 1);
                    Quad ta[NP], tb[NP], x[NP], y[NP];
#pragma unroll
                    for (int c = 0; c < NP; ++c) { ta[c] = tq(L.w[0], c); tb[c] = tq(L.xie, c); x[c] = ldq(G + gq(c)); y[c] = evenq(c); }
#pragma unroll
                    for (int c = 0; c < NP; ++c)
#pragma unroll
                        for (int k = 0; k < 4; ++k) { uq[c].v[k] = F::tmul(ta[c].v[k], x[c].v[k]); vq[c].v[k] = F::tmul(tb[c].v[k], F::sub(y[c].v[k], uq[c].v[k])); }
                }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < NP; ++c) {
                    const uint32_t g = gq(c), i = g & (e - 1), bb = (g >> le) << l;
                    stq(cur + bb + i, uq[c]); stq(cur + bb + e + i, vq[c]);
                }
                __syncthreads();
                continue;
            }
        }
        for (uint32_t g = tid; g < nh; g += BLK) lds_put<F, kSwz>(G, g, F::tmul(ldt(k3 ? L.zA1 : L.A1, g & (e - 1)), lds_get<F, kSwz>(cur, 2 * g + par1)));
        __syncthreads();
        lds_extend_core<F, BLK, kSwz, SYM && k3>(G, nh, le, L, par1);
        for (uint32_t g = tid; g < nh; g += BLK) {
            uint32_t i = g & (e - 1);
            E r = F::tmul_add(ldt(k3 ? L.zNB2 : L.NB2, i), lds_get<F, kSwz>(G, g), F::tmul(ldt(k3 ? L.zB1 : L.B1, i), lds_get<F, kSwz>(cur, 2 * g + 1 - par1)));
            lds_put<F, kSwz>(G, g, r); lds_put<F, kSwz>(H, g, r);
        }
        __syncthreads();
        lds_extend_core<F, BLK, kSwz, SYM && k3>(G, nh, le, L, 1 - par1);
        for (uint32_t g = tid; g < nh; g += BLK) lds_put<F, kSwz>(G, g, F::tmul(ldt(k3 ? L.zC1 : L.C1, g & (e - 1)), lds_get<F, kSwz>(G, g)));
        __syncthreads();
        lds_extend_core<F, BLK, kSwz, SYM && k3>(G, nh, le, L, par1);
        if constexpr (!k3) {
            for (uint32_t g = tid; g < nh; g += BLK) {
                uint32_t i = g & (e - 1);
                lds_put<F, kSwz>(G, g, F::tmul_add(ldt(L.NB2, i), lds_get<F, kSwz>(G, g), F::tmul(ldt(L.D1, i), lds_get<F, kSwz>(H, g))));
            }
            __syncthreads();
            lds_extend_core<F, BLK, kSwz, SYM && k3>(G, nh, le, L, 1);
        }
        E u[PAIRS], v[PAIRS];
#pragma unroll
        for (int c = 0; c < PAIRS; ++c) {
            uint32_t g = tid + (uint32_t)c * BLK, i = g & (e - 1);
            if constexpr (k3) u[c] = F::tmul_add(ldt(L.zNB3, i), lds_get<F, kSwz>(G, g), F::tmul(ldt(L.zD1, i), lds_get<F, kSwz>(H, g)));
            else u[c] = F::tmul(ldt(L.w[0], i), lds_get<F, kSwz>(G, g));
            v[c] = F::tmul(ldt(L.xie, i), F::sub(lds_get<F, kSwz>(cur, 2 * g), u[c]));
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < PAIRS; ++c) {
            uint32_t g = tid + (uint32_t)c * BLK, i = g & (e - 1), bb = (g >> le) << l;
            lds_put<F, kSwz>(cur, bb + i, u[c]); lds_put<F, kSwz>(cur, bb + e + i, v[c]);
        }
        __syncthreads();
    }
    if constexpr (sizeof(E) == 32 && LOG_TILE == 10 && BLK == 512) {
        if (lA32) {             // levels 5..1 on the matrix cores: one 32 x 32 map per 32-block
            if constexpr (kSwz) {                                          // (off by default: the plain layout first)
                const E x0 = lds_get<F, true>(cur, tid), x1 = lds_get<F, true>(cur, tid + 512);
                __syncthreads();
                cur[tid] = x0; cur[tid + 512] = x1;
                __syncthreads();
            }
            Blk16::to_operand_form32(cur, tid);
            Blk16::phase32(cur, lA32, trees[5].low32_K[1], tid);
            Blk16::from_swizzled32(cur, tid);
            cur_swz = false;
        } else
        if (lA) {               // levels 4..1 on the matrix cores: one 16 x 16 map per 16-block
            Blk16::APre pre = Blk16::prefetch(lA, tid);
            __builtin_amdgcn_sched_barrier(0);
            Blk16::to_operand_form<BLK, kSwz>(cur, T, tid);
            Blk16::phase(cur, lA, trees[4].low16_K[1], tid, pre);
            Blk16::from_swizzled<BLK>(cur, T, tid);
            cur_swz = false;
        }
    }
    if constexpr (sizeof(E) == 32 && LOG_TILE == 8 && BLK == 128) {
        if (lA) {               // latency variant: 16 blocks on two waves (v_mfma_i32_16x16x64_i8), two results per lane
            Blk16::phase_n16<2, false, ECFFT_N16_DEPTH2W>(cur, lA, trees[4].low16_K[1], tid, [&] { Blk16::to_operand_form<BLK>(cur, T, tid); });
            Blk16::from_swizzled<BLK>(cur, T, tid);
        }
    }
    if constexpr (kQuad) {
        if (qio) {
            constexpr int NQ = (int)(T / (4 * BLK));
#pragma unroll
            for (int c = 0; c < NQ; ++c) {
                Quad q = ldq(cur + 4u * (tid + (uint32_t)c * BLK));
#pragma unroll
                for (int k = 0; k < 4; ++k) q.v[k] = F::canon(q.v[k]);
                stq(dst + base + 4u * (tid + (uint32_t)c * BLK), q);
            }
            return;
        }
    }
    if (cur_swz) { for (uint32_t j = tid; j < T; j += BLK) dst[base + j] = F::canon(lds_get<F, kSwz>(cur, j)); }
    else for (uint32_t j = tid; j < T; j += BLK) dst[base + j] = F::canon(cur[j]);
}

// ---------------------------------------------------------------------------------------------
// pointwise scaling by a (strided) table: cyclic shards of a multi-GPU split EXTEND.  (The combine step of ENTER,
// src/fftree.rs:155-159, has no kernel of its own: it is the store operator of the level's last EXTEND pass — ST_ENTER in
// k_stages_lds, k_stages_col_enter.)
// ---------------------------------------------------------------------------------------------
// work[j] = src[j] * winv0[j mod e]
template <class F>
__global__ __launch_bounds__(kBlock) void k_scale_by_table(typename F::elem* dst,  // may alias src
                                                            const typename F::elem* src,
                                                            const typename F::telem* __restrict__ tbl,
                                                            size_t tbl_mask, size_t n, uint32_t tstride, uint32_t toff) {
    size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= n) return;
    dst[g] = F::canon(F::tmul(tbl[(g & tbl_mask) * tstride + toff], src[g]));
}

// ---------------------------------------------------------------------------------------------
// pointwise product of ecfft_poly_mul (no reference counterpart): out[b*N + j] = A_b(x_j) * B_b(x_j) * R^-1 on the N leaves of T_N,
// in the natural leaf order EXIT reads.  An operand's evaluations at the even leaves j = 2k and the odd leaves j = 2k+1 are read
// through two pointers, so the last lift of a zero-padded operand (ENTER_N(p | 0) = interleave(E, EXTEND_S1(E)), src/fftree.rs:
// 155-159 with v0 = v1 = 0) needs no interleave pass of its own: even = E, odd = EXTEND_S1(E), stride 1; an operand entered at the
// full size N is even = P, odd = P + 1, stride 2.  User data is x*R (secp256k1, R = 2^256; field_secp256k1.h), so the plain product
// of two operands carries R^2: the table multiply by R^-1 (rinv) puts it back in the crate's form.  M31 has R = 1.
// ---------------------------------------------------------------------------------------------
template <class F>
struct PolyEvals {
    const typename F::elem* even;   // evaluations at the leaves 2k of polynomial b: even[b*batch + k*stride]
    const typename F::elem* odd;    // ... at the leaves 2k + 1: odd[b*batch + k*stride]
    size_t batch;
    uint32_t stride;
};
template <class F>
__global__ __launch_bounds__(kBlock) void k_poly_pointwise(typename F::elem* __restrict__ out, PolyEvals<F> a, PolyEvals<F> b,
                                                           typename F::telem rinv, uint32_t log_n, size_t total) {
    using E = typename F::elem;
    const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= total) return;
    const size_t bi = g >> log_n, j = g & (((size_t)1 << log_n) - 1), k = j >> 1;
    const E* pa = (j & 1) ? a.odd : a.even;
    const E* pb = (j & 1) ? b.odd : b.even;
    E r = F::mul(pa[bi * a.batch + k * a.stride], pb[bi * b.batch + k * b.stride]);
    if constexpr (sizeof(E) == 32) r = F::tmul(rinv, r);
    out[g] = F::canon(r);
}

// ---------------------------------------------------------------------------------------------
// ecfft_poly_inv_series / ecfft_poly_divrem (division with remainder; the reference's utils::div_rem, src/utils.rs:184-193,
// runs ark-poly's schoolbook divide_with_q_and_r on the CPU).  The reciprocal 1/f mod x^k starts from the first p0 <= K0
// coefficients (k_series_base) and doubles its precision by Newton steps g' = g (2 - f g), each one pointwise product on the
// leaves of T_N (k_newton_pointwise).
// ---------------------------------------------------------------------------------------------
// One workgroup of K0 threads per pair: g_0 = 1/f_0, g_j = -g_0 * sum_{i=1..j} f_i g_{j-i} for j < p0 <= K0, on plain residues
// in LDS (one tree sum per coefficient).  f: row b at f + b*ldf, nf coefficients (crate form); out: row b at out + b*ldo, p0
// coefficients (crate form).  A pair with f_0 == 0 stores 1 to *flag (its row is then zero).  rinv = R^-1, r1 = R (plain).
template <class F, int K0>
__global__ __launch_bounds__(K0) void k_series_base(typename F::elem* __restrict__ out, size_t ldo, const typename F::elem* __restrict__ f,
                                                   size_t ldf, size_t nf, uint32_t p0, typename F::elem rinv, typename F::elem r1,
                                                   int* __restrict__ flag) {
    using E = typename F::elem;
    __shared__ E sf[K0], sg[K0], red[K0];
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    sf[t] = (t < p0 && t < nf) ? F::canon(F::mul(f[b * ldf + t], rinv)) : F::zero();
    __syncthreads();
    if (t == 0) {
        if (F::is_zero(sf[0])) *flag = 1;
        sg[0] = F::canon(F::inv(sf[0]));                 // inv(0) = 0: the row of a flagged pair stays zero
    }
    __syncthreads();
    const E g0 = sg[0];
    for (uint32_t j = 1; j < p0; ++j) {
        red[t] = (t >= 1 && t <= j) ? F::mul(sf[t], sg[j - t]) : F::zero();
        __syncthreads();
        for (uint32_t w = K0 / 2; w > 0; w >>= 1) {
            if (t < w) red[t] = F::add(red[t], red[t + w]);
            __syncthreads();
        }
        if (t == 0) sg[j] = F::canon(F::neg(F::mul(g0, red[0])));
        __syncthreads();
    }
    if (t < p0) out[b * ldo + t] = F::canon(F::mul(sg[t], r1));
}
// One Newton step's pointwise product on the N leaves of T_N: out = G (2 - F G), read like k_poly_pointwise (PolyEvals).  User
// data is x*R, so F::mul(F^, G^) carries R^2: subtracted from two_r2 = 2R^2 and multiplied by G^ it carries R^3, and one table
// multiply by rinv2 = R^-2 puts it back in the crate's form.  M31 has R = 1.
template <class F>
__global__ __launch_bounds__(kBlock) void k_newton_pointwise(typename F::elem* __restrict__ out, PolyEvals<F> f, PolyEvals<F> g,
                                                             typename F::elem two_r2, typename F::telem rinv2, uint32_t log_n, size_t total) {
    using E = typename F::elem;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const size_t bi = i >> log_n, j = i & (((size_t)1 << log_n) - 1), k = j >> 1;
    const E* pf = (j & 1) ? f.odd : f.even;
    const E* pg = (j & 1) ? g.odd : g.even;
    const E gv = pg[bi * g.batch + k * g.stride];
    E r = F::mul(F::sub(two_r2, F::mul(pf[bi * f.batch + k * f.stride], gv)), gv);
    if constexpr (sizeof(E) == 32) r = F::tmul(rinv2, r);
    out[i] = F::canon(r);
}
// remainder of ecfft_poly_divrem: r[b*nr + j] = a[b*lda + j] - p[b*ldp + j] for j < nr (p = (b mod x^nr)(q mod x^nr))
template <class F>
__global__ __launch_bounds__(kBlock) void k_divrem_sub(typename F::elem* __restrict__ r, size_t nr, const typename F::elem* __restrict__ a,
                                                       size_t lda, const typename F::elem* __restrict__ p, size_t ldp, size_t total) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const size_t bi = i / nr, j = i - bi * nr;
    r[i] = F::canon(F::sub(a[bi * lda + j], F::canon(p[bi * ldp + j])));
}

// ---------------------------------------------------------------------------------------------
// ecfft_poly_eval_points (multipoint evaluation at arbitrary points; no reference counterpart): a remainder tree over the
// subproduct tree of the points.  Every node of a level has the same degree d, so a level is one batched launch.
// ---------------------------------------------------------------------------------------------
// Pointwise product of a lifted operand with a cached node operand on the 2^log_n leaves of T_2d: out row i = A row (i >> a_shift)
// times node row (i mod nodes), both in the natural leaf order EXIT reads.  The node operand (M^ or G^ of the subproduct tree) is
// indexed by node, not by polynomial x node; a_shift = 1 lets both children of a parent read the parent's row.  Scaling as
// k_poly_pointwise: the plain product of two user-form operands carries R^2, one table multiply by R^-1 puts it back (M31: R = 1).
template <class F>
__global__ __launch_bounds__(kBlock) void k_tree_pointwise(typename F::elem* __restrict__ out, PolyEvals<F> a, uint32_t a_shift,
                                                           const typename F::elem* __restrict__ node, size_t nodes, typename F::telem rinv,
                                                           uint32_t log_n, size_t total) {
    using E = typename F::elem;
    const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= total) return;
    const size_t bi = g >> log_n, j = g & (((size_t)1 << log_n) - 1), k = j >> 1, ai = bi >> a_shift, ni = bi % nodes;
    const E* pa = (j & 1) ? a.odd : a.even;
    E r = F::mul(pa[ai * a.batch + k * a.stride], node[(ni << log_n) + j]);
    if constexpr (sizeof(E) == 32) r = F::tmul(rinv, r);
    out[g] = F::canon(r);
}
// The leaves of the remainder tree: row r of `rows_per_poly` rows per polynomial holds the remainder (nc <= B coefficients, crate
// form) of polynomial r / rows_per_poly at the B points of its leaf block; out[b*m + i] = that remainder at points[i], i < m.  One
// thread per point, B threads per row: the row is staged in LDS and read by all of them as a broadcast.  The point is brought to
// plain form once (x R^-1, one table multiply; M31: R = 1), so each Horner step is one F::mul and one F::add on the crate form.
// Row stride ld_row = 0: every row of a polynomial is the same (the no-tree path, where f itself is every block's remainder).
template <class F, int B>
__global__ __launch_bounds__(kBlock) void k_eval_leaves(typename F::elem* __restrict__ out, const typename F::elem* __restrict__ rem,
                                                        size_t ld_poly, size_t ld_row, uint32_t nc, const typename F::elem* __restrict__ points,
                                                        size_t m, size_t rows_per_poly, size_t rows, typename F::telem rinv) {
    static_assert(kBlock % B == 0, "a workgroup holds whole rows");
    using E = typename F::elem;
    __shared__ E sc[kBlock];
    const uint32_t t = threadIdx.x, lane = t % B;
    const size_t r = (size_t)blockIdx.x * (kBlock / B) + t / B;
    const size_t b = r / rows_per_poly, rr = r - b * rows_per_poly, i = rr * B + lane;
    sc[t] = (r < rows && lane < nc) ? rem[b * ld_poly + rr * ld_row + lane] : F::zero();
    __syncthreads();
    if (r >= rows || i >= m) return;
    E x = points[i];
    if constexpr (sizeof(E) == 32) x = F::tmul(rinv, x);
    const E* c = sc + (t - lane);
    E acc = F::zero();
    for (uint32_t j = nc; j-- > 0;) acc = F::add(F::mul(acc, x), c[j]);
    out[b * m + i] = F::canon(acc);
}

// ---------------------------------------------------------------------------------------------
// ecfft_poly_interpolate (interpolation from arbitrary points; no reference counterpart): the Lagrange form
// f = sum_i c_i M / (x - x_i), c_i = y_i / M'(x_i), combined upwards over the subproduct tree of the points: a node's numerator is
// N = N_l M_r + N_r M_l.  Every node of a level has the same degree, so a level is one batched launch.
// ---------------------------------------------------------------------------------------------
// The leaves of the combination, the mirror image of k_eval_leaves: row r of `rows_per_vec` rows per value vector holds the B
// coefficients (crate form) of N = sum_i c_i prod_{j != i} (x - x_j) over the B points of its leaf block, c_i = y[b*m + i] * w[i]
// (w: plain 1 / M'(x_i)); positions i >= m are the pad point 0 with c_i = 0.  One thread per coefficient, B steps over the block's
// points keeping (M_t, N_t): M_{t+1} = M_t (x - x_t), N_{t+1} = N_t (x - x_t) + c_t M_t — the neighbour coefficient through LDS,
// x_t and c_t as LDS broadcasts.  The point is brought to plain form once (as k_eval_leaves), M is a plain polynomial, N and c are
// in crate form: 3 multiplies per thread and step, none of them crate x crate.
template <class F, int B>
__global__ __launch_bounds__(kBlock) void k_interp_leaves(typename F::elem* __restrict__ out, const typename F::elem* __restrict__ values,
                                                          const typename F::elem* __restrict__ weights,
                                                          const typename F::elem* __restrict__ points, size_t m, size_t rows_per_vec,
                                                          size_t rows, typename F::telem rinv) {
    static_assert(kBlock % B == 0, "a workgroup holds whole rows");
    using E = typename F::elem;
    __shared__ E sx[kBlock], sc[kBlock], sm[kBlock], sn[kBlock];
    const uint32_t t = threadIdx.x, lane = t % B, base = t - lane;
    const size_t r = (size_t)blockIdx.x * (kBlock / B) + t / B;
    const size_t b = r / rows_per_vec, rr = r - b * rows_per_vec, i = rr * B + lane;
    const bool real = r < rows && i < m;
    E x = real ? points[i] : F::zero();
    if constexpr (sizeof(E) == 32) x = F::tmul(rinv, x);
    sx[t] = F::canon(x);
    sc[t] = real ? F::canon(F::mul(values[b * m + i], weights[i])) : F::zero();
    E M = lane == 0 ? F::one() : F::zero(), N = F::zero();
    for (int step = 0; step < B; ++step) {
        sm[t] = M; sn[t] = N;
        __syncthreads();
        const E xt = sx[base + step], ct = sc[base + step];
        const E Mp = lane ? sm[t - 1] : F::zero(), Np = lane ? sn[t - 1] : F::zero();
        __syncthreads();
        N = F::canon(F::add(F::sub(Np, F::mul(xt, N)), F::mul(ct, M)));
        M = F::canon(F::sub(Mp, F::mul(xt, M)));
    }
    if (r < rows) out[r * B + lane] = N;
}
// One level of the ascent in evaluation form: children of d points (2^log_n = 2d), parent row g >> log_n of `total >> log_n` rows
// (vector x parent node): N^_parent = N^_l M^_r + N^_r M^_l on the 2d leaves of T_2d in the natural leaf order EXIT reads
// (deg < 2d: nothing wraps).  The children's rows 2 row and 2 row + 1 are read through even / odd pointers like k_poly_pointwise,
// the node operands from the cached M^ of the level indexed by node (not by vector x node).  Both products carry R^2, so ONE
// table multiply by R^-1 on the sum puts the result back in the crate's form (M31: R = 1).
template <class F>
__global__ __launch_bounds__(kBlock) void k_interp_combine(typename F::elem* __restrict__ out, PolyEvals<F> a,
                                                           const typename F::elem* __restrict__ node, size_t nodes, typename F::telem rinv,
                                                           uint32_t log_n, size_t total) {
    using E = typename F::elem;
    const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= total) return;
    const size_t row = g >> log_n, j = g & (((size_t)1 << log_n) - 1), k = j >> 1, cl = 2 * row, nl = cl % nodes;
    const E* pa = (j & 1) ? a.odd : a.even;
    const E Nl = pa[cl * a.batch + k * a.stride], Nr = pa[(cl + 1) * a.batch + k * a.stride];
    const E Ml = node[(nl << log_n) + j], Mr = node[((nl + 1) << log_n) + j];
    E r = F::add(F::mul(Nl, Mr), F::mul(Nr, Ml));
    if constexpr (sizeof(E) == 32) r = F::tmul(rinv, r);
    out[g] = F::canon(r);
}

// ---------------------------------------------------------------------------------------------
// ecfft_poly_pow_mod (utils::pow_mod, src/utils.rs:194-211: square-and-multiply with a div_rem per step).  Above K coefficients a
// modular product is three products on T_N against operands whose evaluations are kept for the whole call (the base, the
// reciprocal g of the reversed modulus, the modulus); up to K the whole exponentiation of a residue runs in one workgroup.
// ---------------------------------------------------------------------------------------------
// The pad load of a lift: count rows of n coefficients at a row stride of ld -> count rows of 2^log_m, zero-padded.  rev: the
// row is read downwards from index `top` (dst[j] = src[top - j]), so rev(c) mod x^n and the reversal that turns the low half of
// a product into the quotient need no pass of their own.
template <class F>
__global__ __launch_bounds__(kBlock) void k_powmod_pad(typename F::elem* __restrict__ dst, const typename F::elem* __restrict__ src, size_t n,
                                                       size_t ld, uint32_t rev, size_t top, uint32_t log_m, size_t total) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const size_t b = i >> log_m, j = i & (((size_t)1 << log_m) - 1);
    dst[i] = j < n ? src[b * ld + (rev ? top - j : j)] : F::zero();
}
// Pointwise product of a lifted operand (PolyEvals, as k_poly_pointwise reads it) with an operand cached for the call in the
// natural leaf order EXIT reads (cached row r at cached + (r << log_n)); cached == nullptr squares the lifted operand.  Scaling
// as k_poly_pointwise: both operands are user-form evaluations, the plain product carries R^2 and one table multiply by R^-1
// puts it back in the crate's form (M31: R = 1).
template <class F>
__global__ __launch_bounds__(kBlock) void k_powmod_pointwise(typename F::elem* __restrict__ out, PolyEvals<F> a,
                                                             const typename F::elem* __restrict__ cached, typename F::telem rinv,
                                                             uint32_t log_n, size_t total) {
    using E = typename F::elem;
    const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= total) return;
    const size_t bi = g >> log_n, j = g & (((size_t)1 << log_n) - 1), k = j >> 1;
    const E* pa = (j & 1) ? a.odd : a.even;
    const E x = pa[bi * a.batch + k * a.stride];
    E r = F::mul(x, cached ? cached[g] : x);
    if constexpr (sizeof(E) == 32) r = F::tmul(rinv, r);
    out[g] = F::canon(r);
}
// The end of a modular product: res[b*d + j] = c[b*ld + j] - t[b*ld + j] for j < d (c: the product x y, t: (f mod x^d) q)
template <class F>
__global__ __launch_bounds__(kBlock) void k_powmod_sub(typename F::elem* __restrict__ res, size_t d, const typename F::elem* __restrict__ c,
                                                       const typename F::elem* __restrict__ t, size_t ld, size_t total) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / d, j = i - b * d;
    res[i] = F::canon(F::sub(F::canon(c[b * ld + j]), F::canon(t[b * ld + j])));
}
// The modular product of the small regimes (k_powmod_small, k_compose_small, roots_pow_scan): one workgroup of K threads per row,
// residues of d <= K coefficients in LDS rows of K, thread t owning coefficient t.  The modulus is made monic once (one Fermat
// inversion of its leading coefficient) and kept as PLAIN residues: f_t / f_d is the same number in either form.  A product brings
// its left operand to plain form (one table multiply by R^-1 per coefficient, M31: R = 1), so every inner multiply is plain x crate
// and stays crate: thread t sums the d terms of coefficients t and t + d of the schoolbook product (those with k <= t belong to the
// first; it switches accumulators at k = t + 1), then d - 1 elimination steps of the monic modulus fold coefficients 2d-2 .. d
// back.  The last thread never switches, because coefficient 2d - 1 does not exist: its sum is the low one.
//
// smod[t] = f[t] / f[d] as plain residues (zero from d on); a zero leading coefficient stores 1 to *flag.  The inverse passes
// through sx[0].  No barrier after the store: the caller loads its own rows first.
template <class F>
__device__ __forceinline__ void modmul_monic(typename F::elem* smod, typename F::elem* sx, const typename F::elem* __restrict__ f, uint32_t d,
                                             int* __restrict__ flag, uint32_t t) {
    using E = typename F::elem;
    if (t == 0) {
        const E lead = F::canon(f[d]);
        if (F::is_zero(lead)) *flag = 1;
        sx[0] = F::canon(F::inv(lead));                  // inv(0) = 0: a flagged row computes on a zero modulus, its result is not used
    }
    __syncthreads();
    const E linv = sx[0];
    __syncthreads();
    smod[t] = t < d ? F::canon(F::mul(f[t], linv)) : F::zero();
}
// sx = the left operand sres in plain form
template <class F>
__device__ __forceinline__ void modmul_plain(typename F::elem* sx, const typename F::elem* sres, const typename F::telem& rinv, uint32_t t) {
    using E = typename F::elem;
    E x = sres[t];
    if constexpr (sizeof(E) == 32) x = F::tmul(rinv, x);
    sx[t] = F::canon(x);
    __syncthreads();
}
// sprod[0 .. d) = sx y mod (x^d + smod) for the plain sx and any LDS row y of d crate-form coefficients (sprod: 2K entries)
template <class F>
__device__ __forceinline__ void modmul_reduce(typename F::elem* sprod, const typename F::elem* sx, const typename F::elem* y,
                                              const typename F::elem* smod, uint32_t d, uint32_t t) {
    using E = typename F::elem;
    if (t < d) {
        uint32_t k = 0;                                  // declared ahead of the sums: in the for statement, hipcc 7 counts the
                                                         // loop of k_powmod_small<M31> in a vector register (+4.5 % on a full GPU)
        E acc = F::zero(), lo = F::zero();
        for (; k < d; ++k) {
            if (k == t + 1) { lo = acc; acc = F::zero(); }
            const uint32_t j = k <= t ? t - k : t + d - k;
            acc = F::canon(F::mul_add(sx[k], y[j], acc));
        }
        if (t + 1 == d) { lo = acc; acc = F::zero(); }
        sprod[t] = lo;
        sprod[t + d] = acc;
    }
    __syncthreads();
    for (uint32_t k = 2 * d - 2; k >= d; --k) {
        if (t < d) sprod[k - d + t] = F::canon(F::sub(sprod[k - d + t], F::canon(F::mul(sprod[k], smod[t]))));
        __syncthreads();
    }
}
// a^exp mod f for residues of d <= K coefficients: one workgroup of K threads per pair, the whole left-to-right square-and-multiply
// in LDS on the product above.  a: row b at a + b*lda, na <= d coefficients (crate form); f: row b at f + b*(d+1), d + 1
// coefficients; exp: nbits bits, little-endian bytes, bit nbits-1 set (nbits == 0: the result is 1); out: count x d.  r1 = R, the
// crate's 1.
template <class F, int K>
__global__ __launch_bounds__(K) void k_powmod_small(typename F::elem* __restrict__ out, const typename F::elem* __restrict__ a, size_t lda,
                                                    uint32_t na, const typename F::elem* __restrict__ f, uint32_t d,
                                                    const uint8_t* __restrict__ exp, uint32_t nbits, typename F::telem rinv,
                                                    typename F::elem r1, int* __restrict__ flag) {
    using E = typename F::elem;
    __shared__ E sres[K], sbase[K], smod[K], sx[K], sprod[2 * K];
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    modmul_monic<F>(smod, sx, f + b * ((size_t)d + 1), d, flag, t);
    sbase[t] = t < na ? a[b * lda + t] : F::zero();
    sres[t] = sbase[t];
    __syncthreads();
    if (nbits == 0) {
        if (t < d) out[b * d + t] = t == 0 ? r1 : F::zero();
        return;
    }
    for (uint32_t i = nbits - 1; i-- > 0;) {
        const uint32_t passes = 1 + ((exp[i >> 3] >> (i & 7)) & 1);     // a squaring, then on a set bit a product with the base
        for (uint32_t pass = 0; pass < passes; ++pass) {
            modmul_plain<F>(sx, sres, rinv, t);
            modmul_reduce<F>(sprod, sx, pass ? sbase : sres, smod, d, t);   // sres = sres * y mod f
            if (t < d) sres[t] = sprod[t];
            __syncthreads();
        }
    }
    if (t < d) out[b * d + t] = sres[t];
}

// ---------------------------------------------------------------------------------------------
// ecfft_poly_compose_mod (no single reference counterpart: the composition of two residues, the Horner-like loop of
// examples/schoofs.rs:197-235 and the step x^(p^i) -> x^(p^(i+1)) of distinct-degree factorisation, utils.rs:52-78).  Up to K
// residue coefficients one workgroup runs the whole Horner scheme (k_compose_small); above that the host drives Brent-Kung baby
// and giant steps on the kept-modulus products of poly_pow_mod, and k_compose_rows is the dense matrix product between them
// (DESIGN.md 5.10).
// ---------------------------------------------------------------------------------------------
// f(g) mod h for residues of d <= K coefficients: one workgroup of K threads per triple, Horner in LDS on the product of
// k_powmod_small (modmul_*): res = f[nf-1], then for i = nf - 2 .. 0 res = res g mod h and res[0] += f[i]; nf is the only loop
// bound.  f: row b at f + b*nf; g: row b at g + b*ldg, ng <= d coefficients; h: row b at h + b*(d+1); out: count x d.
template <class F, int K>
__global__ __launch_bounds__(K) void k_compose_small(typename F::elem* __restrict__ out, const typename F::elem* __restrict__ f, uint32_t nf,
                                                     const typename F::elem* __restrict__ g, size_t ldg, uint32_t ng,
                                                     const typename F::elem* __restrict__ h, uint32_t d, typename F::telem rinv,
                                                     int* __restrict__ flag) {
    using E = typename F::elem;
    __shared__ E sres[K], sg[K], smod[K], sx[K], sprod[2 * K];
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    const E* fb = f + b * (size_t)nf;
    modmul_monic<F>(smod, sx, h + b * ((size_t)d + 1), d, flag, t);
    sg[t] = t < ng ? F::canon(g[b * ldg + t]) : F::zero();
    {
        E v = F::zero();
        if (t == 0) v = F::canon(fb[nf - 1]);
        sres[t] = v;
    }
    __syncthreads();
    for (uint32_t i = nf - 1; i-- > 0;) {
        modmul_plain<F>(sx, sres, rinv, t);
        modmul_reduce<F>(sprod, sx, sg, smod, d, t);
        if (t < d) {
            E v = sprod[t];
            if (t == 0) v = F::canon(F::add(v, F::canon(fb[i])));
            sres[t] = v;
        }
        __syncthreads();
    }
    if (t < d) out[b * d + t] = sres[t];
}
// The matrix product between the baby and the giant steps: C[i][b][j] = R^-1 sum_{t < k} f_b[i k + t] B[t][b][j] for i < kp, j < d
// (B: (k + 1) x count x d, the powers g^t mod h; C: kp x count x d; f: row b at f + b*nf; a term with i k + t >= nf is absent).
// Both factors are crate form, so the plain sum carries R^2 and one table multiply by R^-1 per output restores crate form (M31:
// R = 1).  A thread owns column j and TR rows i; the f-coefficients of the tile go through LDS TC columns of t at a time, so the
// inner loop is one coalesced load of B[t][b][j], reused by every row of the tile, and one F::mul_add per row.  Grid: (column
// blocks, row tiles, count).
template <class F> struct ComposeTile { static constexpr int TR = sizeof(typename F::elem) == 4 ? 8 : 4, TC = 32; };
template <class F>
__global__ __launch_bounds__(kBlock) void k_compose_rows(typename F::elem* __restrict__ C, const typename F::elem* __restrict__ B,
                                                         const typename F::elem* __restrict__ f, size_t nf, size_t k, size_t kp,
                                                         size_t d, size_t count, typename F::telem rinv) {
    using E = typename F::elem;
    constexpr int TR = ComposeTile<F>::TR, TC = ComposeTile<F>::TC;
    static_assert(TR * TC <= (int)kBlock, "one thread stages one coefficient");
    __shared__ E sf[TR * TC];
    const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x, i0 = (size_t)blockIdx.y * TR, b = blockIdx.z;
    const E* fb = f + b * nf;
    E acc[TR];
#pragma unroll
    for (int r = 0; r < TR; ++r) acc[r] = F::zero();
    for (size_t t0 = 0; t0 < k; t0 += TC) {
        if (threadIdx.x < (unsigned)(TR * TC)) {
            const size_t r = threadIdx.x / TC, t = t0 + threadIdx.x % TC, idx = (i0 + r) * k + t;
            sf[threadIdx.x] = (t < k && i0 + r < kp && idx < nf) ? F::canon(fb[idx]) : F::zero();
        }
        __syncthreads();
        if (j < d) {
            const size_t tn = k - t0 < (size_t)TC ? k - t0 : (size_t)TC;
            for (size_t tt = 0; tt < tn; ++tt) {
                const E bv = B[((t0 + tt) * count + b) * d + j];
#pragma unroll
                for (int r = 0; r < TR; ++r) acc[r] = F::canon(F::mul_add(sf[r * TC + tt], bv, acc[r]));
            }
        }
        __syncthreads();
    }
    if (j >= d) return;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        E v = acc[r];
        if constexpr (sizeof(E) == 32) v = F::tmul(rinv, v);
        if (i0 + r < kp) C[((i0 + r) * count + b) * d + j] = F::canon(v);
    }
}

// ---------------------------------------------------------------------------------------------
// ecfft_poly_gcd / ecfft_poly_xgcd (utils::gcd / utils::xgcd, src/utils.rs:132-182: one schoolbook div_rem per remainder on the
// CPU).  Up to G coefficients the whole remainder sequence of a pair runs in one workgroup (k_gcd_small); above that the host
// drives a half-GCD on the poly_mul and division bodies whose recursion ends in the same kernel.
// ---------------------------------------------------------------------------------------------
// The cross-multiplied remainder loop of k_gcd_small and k_roots_small on LDS rows, thread t owning coefficient t of every row:
// while deg R1 >= bound (and R1 != 0), steps
//     R0 <- lc(R1) R0 - lc(R0) x^k R1,   k = deg R0 - deg R1,
// until deg R0 < deg R1, then the rows swap.  The new degree is an atomicMax into sdeg[par], which the step before left at -1;
// the step resets the other entry, so the two alternate.  On entry d0 = deg R0, d1 = deg R1 (-1: zero) and both sdeg are -1 behind
// a barrier.  cof != 0 applies the same combination to the cofactor rows (S0, T0), (S1, T1), touched below their lengths c0, c1
// only; cof == 0 ignores them.  Returns the number of swaps.  Every thread takes the same path through every barrier: d0, d1 come
// from LDS after a barrier, bound and cof are the same for the workgroup.
template <class F>
__device__ __forceinline__ int gcd_remainder_loop(typename F::elem*& R0, typename F::elem*& R1, int& d0, int& d1, typename F::elem*& S0,
                                                  typename F::elem*& S1, typename F::elem*& T0, typename F::elem*& T1, int& c0, int& c1,
                                                  uint32_t cof, int bound, int* sdeg, uint32_t t) {
    using E = typename F::elem;
    int swaps = 0;
    uint32_t par = 0;                                        // sdeg[par] == -1 receives the next step's degree
    while (d1 >= 0 && d1 >= bound) {
        while (d0 >= d1) {
            const uint32_t k = (uint32_t)(d0 - d1);
            const E lr = R0[d0], lb = R1[d1];
            __syncthreads();                                 // everyone holds lr (thread d0 clears it) and the previous step's degree
            if (t == 0) sdeg[par ^ 1] = -1;
            if ((int)t < d0) {
                E v = F::mul(lb, R0[t]);
                if (t >= k) v = F::sub(v, F::mul(lr, R1[t - k]));
                v = F::canon(v);
                R0[t] = v;
                if (!F::is_zero(v)) atomicMax(&sdeg[par], (int)t);
            } else if ((int)t == d0) {
                R0[t] = F::zero();
            }
            if (cof) {
                const int cn = c0 > c1 + (int)k ? c0 : c1 + (int)k;
                if ((int)t < cn) {
                    E u = F::mul(lb, S0[t]), w = F::mul(lb, T0[t]);
                    if (t >= k) { u = F::sub(u, F::mul(lr, S1[t - k])); w = F::sub(w, F::mul(lr, T1[t - k])); }
                    S0[t] = F::canon(u); T0[t] = F::canon(w);
                }
                c0 = cn;
            }
            __syncthreads();
            d0 = sdeg[par];
            par ^= 1;
        }
        { E* x = R0; R0 = R1; R1 = x; x = S0; S0 = S1; S1 = x; x = T0; T0 = T1; T1 = x; }
        { int x = d0; d0 = d1; d1 = x; x = c0; c0 = c1; c1 = x; }
        ++swaps;
    }
    return swaps;
}
// The remainder sequence of one pair in one workgroup of G threads, entirely in LDS: thread t owns coefficient t of the two
// remainders (R0, R1) and of the two cofactor rows (S0, T0), (S1, T1), with R_i = S_i a + T_i b throughout.  a: row p at
// a + p*lda, na <= G coefficients; b likewise; high zero coefficients are allowed and either row may be zero — the true degrees
// are found here.  No inversion per quotient: gcd_remainder_loop's steps are cross-multiplied (a quotient of degree q takes q + 1
// of them), so each row is a non-zero scalar multiple of the Euclidean algorithm's row, which changes no degree.
// The multiplies are plain products of stored numbers; with the cofactor rows started from the crate's 1 (r1 = R; M31: R = 1)
// the relation R_i = S_i a + T_i b holds in the crate's arithmetic (x y / R) whatever the scalars are, so the Montgomery factor
// needs no bookkeeping until the end.  The loop runs while deg R1 >= bound (and R1 != 0).
//   leaf == 0 (bound = 0: to the end): R0 is a multiple of the gcd.  With c = R / lc(R0) — the one inversion of the pair —
//     g = c R0 is the monic gcd in crate form and (s, t) = c (S0, T0) its cofactors: the scalars of the row cancel in c.  g: row p
//     of ng coefficients, s: ns, t: nt (either may be null), zero-padded; deg_out[p] = deg g, -1 for a = b = 0 (all rows zero).
//   leaf != 0 (the leaf of the half-GCD): mat + 4 p ldm receives the rows S0, T0, S1, T1 (nm coefficients each at a stride of
//     ldm) and info + 8 p the numbers deg R0, deg R1, the lengths of the two cofactor rows and the count of row swaps (0: the
//     matrix is the identity).
// cof == 0 skips the cofactor rows (gcd only).  Cofactor row i is touched below its length only: deg S_i, T_i grow as deg R_i falls.
template <class F, int G>
__global__ __launch_bounds__(G) void k_gcd_small(const typename F::elem* __restrict__ a, size_t lda, uint32_t na,
                                                 const typename F::elem* __restrict__ b, size_t ldb, uint32_t nb, int32_t bound,
                                                 uint32_t leaf, uint32_t cof, typename F::elem* __restrict__ g, uint32_t ng,
                                                 typename F::elem* __restrict__ s, uint32_t ns, typename F::elem* __restrict__ tt,
                                                 uint32_t nt, long long* __restrict__ deg_out, typename F::elem* __restrict__ mat,
                                                 size_t ldm, uint32_t nm, int32_t* __restrict__ info, typename F::elem r1) {
    using E = typename F::elem;
    __shared__ E buf[6 * G];
    __shared__ E snorm;
    __shared__ int sdeg[2];
    const uint32_t t = threadIdx.x;
    const size_t p = blockIdx.x;
    E *R0 = buf, *R1 = buf + G, *S0 = buf + 2 * G, *S1 = buf + 3 * G, *T0 = buf + 4 * G, *T1 = buf + 5 * G;
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    {
        E va = F::zero(), vb = F::zero(), one = F::zero();
        if (t < na) va = F::canon(a[p * lda + t]);
        if (t < nb) vb = F::canon(b[p * ldb + t]);
        if (t == 0) one = r1;
        R0[t] = va; R1[t] = vb;
        if (!F::is_zero(va)) atomicMax(&sdeg[0], (int)t);
        if (!F::is_zero(vb)) atomicMax(&sdeg[1], (int)t);
        S0[t] = one; T0[t] = F::zero(); S1[t] = F::zero(); T1[t] = one;
    }
    __syncthreads();
    int d0 = sdeg[0], d1 = sdeg[1], c0 = 1, c1 = 1;
    __syncthreads();
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    const int swaps = gcd_remainder_loop<F>(R0, R1, d0, d1, S0, S1, T0, T1, c0, c1, cof, bound, sdeg, t);
    if (leaf) {
        if (t < nm) {
            E* m = mat + p * 4 * ldm;
            m[t] = S0[t]; m[ldm + t] = T0[t]; m[2 * ldm + t] = S1[t]; m[3 * ldm + t] = T1[t];
        }
        if (t == 0) {
            int32_t* o = info + p * 8;
            o[0] = d0; o[1] = d1; o[2] = c0; o[3] = c1; o[4] = swaps;
        }
        return;
    }
    if (t == 0) {
        E c = F::zero();
        if (d0 >= 0) c = F::canon(F::mul(F::inv(R0[d0]), r1));
        snorm = c;
        if (deg_out) deg_out[p] = d0;
    }
    __syncthreads();
    const E c = snorm;
    if (t < ng) g[p * ng + t] = F::canon(F::mul(R0[t], c));
    if (s && t < ns) s[p * ns + t] = F::canon(F::mul(S0[t], c));
    if (tt && t < nt) tt[p * nt + t] = F::canon(F::mul(T0[t], c));
}
// ecfft_poly_xgcd_partial in one workgroup: k_gcd_small's rows and prologue, the loop stopped at bound = stop, and another
// epilogue.  Every swap of gcd_remainder_loop is one row of the classical sequence (the first one, with deg a < deg b, its own
// swap), so when the loop ends R1 is a scalar multiple of the first row r_j, j >= 1, with deg r_j < stop, and (S1, T1) of its
// cofactors.  The scale is taken out by the one inversion of the pair: c = R / lc(T1), or R / lc(S1) where T1 = 0 (the row
// (a, 1, 0)), so that t (else s) is monic.  r: row p of ng coefficients, s: ns (may be null), t: nt, zero-padded; deg_out + 3 p
// (may be null) receives deg r, deg s, deg t, -1 for a zero row.
template <class F, int G>
__global__ __launch_bounds__(G) void k_xgcd_partial_small(const typename F::elem* __restrict__ a, size_t lda, uint32_t na,
                                                          const typename F::elem* __restrict__ b, size_t ldb, uint32_t nb, int32_t stop,
                                                          typename F::elem* __restrict__ r, uint32_t ng, typename F::elem* __restrict__ s,
                                                          uint32_t ns, typename F::elem* __restrict__ tt, uint32_t nt,
                                                          long long* __restrict__ deg_out, typename F::elem r1) {
    using E = typename F::elem;
    __shared__ E buf[6 * G];
    __shared__ E snorm;
    __shared__ int sdeg[2];
    const uint32_t t = threadIdx.x;
    const size_t p = blockIdx.x;
    E *R0 = buf, *R1 = buf + G, *S0 = buf + 2 * G, *S1 = buf + 3 * G, *T0 = buf + 4 * G, *T1 = buf + 5 * G;
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    {
        E va = F::zero(), vb = F::zero(), one = F::zero();
        if (t < na) va = F::canon(a[p * lda + t]);
        if (t < nb) vb = F::canon(b[p * ldb + t]);
        if (t == 0) one = r1;
        R0[t] = va; R1[t] = vb;
        if (!F::is_zero(va)) atomicMax(&sdeg[0], (int)t);
        if (!F::is_zero(vb)) atomicMax(&sdeg[1], (int)t);
        S0[t] = one; T0[t] = F::zero(); S1[t] = F::zero(); T1[t] = one;
    }
    __syncthreads();
    int d0 = sdeg[0], d1 = sdeg[1], c0 = 1, c1 = 1;
    __syncthreads();
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    gcd_remainder_loop<F>(R0, R1, d0, d1, S0, S1, T0, T1, c0, c1, 1u, stop, sdeg, t);
    __syncthreads();
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    // the rows were all written at the start and are zero above their lengths: the true degrees of the two cofactors
    if (!F::is_zero(S1[t])) atomicMax(&sdeg[0], (int)t);
    if (!F::is_zero(T1[t])) atomicMax(&sdeg[1], (int)t);
    __syncthreads();
    const int ds = sdeg[0], dt = sdeg[1];
    if (t == 0) {
        E c = F::zero();
        if (dt >= 0) c = F::canon(F::mul(F::inv(T1[dt]), r1));
        else if (ds >= 0) c = F::canon(F::mul(F::inv(S1[ds]), r1));
        snorm = c;
        if (deg_out) { deg_out[3 * p] = d1; deg_out[3 * p + 1] = ds; deg_out[3 * p + 2] = dt; }
    }
    __syncthreads();
    const E c = snorm;
    if (t < ng) r[p * ng + t] = F::canon(F::mul(R1[t], c));
    if (s && t < ns) s[p * ns + t] = F::canon(F::mul(S1[t], c));
    if (t < nt) tt[p * nt + t] = F::canon(F::mul(T1[t], c));
}
// ---------------------------------------------------------------------------------------------
// ecfft_rs_decode, small regime (m <= G - 1 points): Gao's decoder, a received word per workgroup.
// ---------------------------------------------------------------------------------------------
// What the rows of a call share, from the m points (crate form), in one launch of m workgroups of G threads:
//   block 0: the Newton basis N_i = prod_{l < i} (x - x_l), i < m, as PLAIN coefficients (np + i m + t, t <= i; thread t owns
//            coefficient t through the m steps N_{i+1} = x N_i - x_i N_i), and g0 = N_m in crate form (m + 1 coefficients);
//   block j >= 1: the PLAIN inverse denominators of lag j, invd[j m + i] = 1 / (x_i - x_{i-j}) for j <= i < m: every pair of
//            points meets in exactly one of them, so a zero difference (two equal points) raises *flag.
// rinv = R^-1, r1 = R (M31: both 1): x R^-1 is the plain value of a crate-form x, and R / d the plain inverse of a crate-form d.
template <class F, int G>
__global__ __launch_bounds__(G) void k_rs_prepare(const typename F::elem* __restrict__ points, uint32_t m, typename F::elem* __restrict__ np,
                                                  typename F::elem* __restrict__ g0, typename F::elem* __restrict__ invd,
                                                  typename F::elem rinv, typename F::elem r1, int* __restrict__ flag) {
    using E = typename F::elem;
    __shared__ E row[G];
    const uint32_t t = threadIdx.x, j = blockIdx.x;
    if (j) {
        if (t >= j && t < m) {
            const E d = F::canon(F::sub(F::canon(points[t]), F::canon(points[t - j])));
            E v = F::zero();
            if (F::is_zero(d)) *flag = 1;
            else v = F::canon(F::mul(F::inv(d), r1));
            invd[(size_t)j * m + t] = v;
        }
        return;
    }
    E cur = F::zero();
    if (t == 0) cur = F::one();
    for (uint32_t i = 0; i < m; ++i) {
        if (t <= i) np[(size_t)i * m + t] = cur;
        row[t] = cur;
        __syncthreads();
        const E xi = F::canon(F::mul(F::canon(points[i]), rinv));
        E lo = F::zero();
        if (t) lo = row[t - 1];
        cur = F::canon(F::sub(lo, F::canon(F::mul(xi, cur))));
        __syncthreads();
    }
    if (t <= m) g0[t] = F::canon(F::mul(cur, r1));
}
// The two decoders below are one body between a prologue and an epilogue of their own: rs_interpolant (step 1), then rs_gao_finish
// (steps 2 and 3).  One received word of m <= G - 1 symbols per workgroup, everything in LDS, thread t owning coefficient t of
// every row:
//   1. the interpolant g1: Newton's divided differences (m - 1 steps of one multiply by k_rs_prepare's inverse denominators; a
//      thread keeps its own entry in a register and reads its neighbour's through two alternating rows, one barrier a step),
//      then coefficient t of sum_i dd_i N_i as a sum over the basis rows in global memory — no sequential Horner;
//   2. gcd_remainder_loop on (g0, g1) with bound = stop = ceil((m + k) / 2), the S rows aliased to the T rows (only the cofactor
//      of g1 is needed): R1 = c r and T1 = c t for the wanted row (r, s, t) of the sequence and some scalar c;
//   3. f = R1 / T1 by long division with T1 made monic as PLAIN numbers (one inversion, u = 1 / lc(T1)): the quotient of the
//      stored numbers is lc(T1) times the plain f, so u R brings its coefficients to crate form.  The word decodes iff the
//      remainder is zero and deg f < k, and then its verdict is deg t; else -1.
// Step 1: mine = the thread's symbol (zero from m up, and for a lost one); returns coefficient t of g1.  A, B: the two alternating
// rows, dd: the row that holds the divided differences for the sum.  All three are free behind the closing barrier, and sdeg is
// -1, -1 there.
template <class F>
__device__ __forceinline__ typename F::elem rs_interpolant(typename F::elem mine, uint32_t m, const typename F::elem* __restrict__ np,
                                                           const typename F::elem* __restrict__ invd, typename F::elem* dd,
                                                           typename F::elem* A, typename F::elem* B, int* sdeg, uint32_t t) {
    using E = typename F::elem;
    for (uint32_t j = 1; j < m; ++j) {
        A[t] = mine;
        __syncthreads();
        if (t >= j && t < m) mine = F::canon(F::mul(F::canon(F::sub(mine, A[t - 1])), invd[(size_t)j * m + t]));
        E* x = A; A = B; B = x;
    }
    __syncthreads();
    dd[t] = mine;
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    E acc = F::zero();
    if (t < m)
        for (uint32_t i = t; i < m; ++i) acc = F::canon(F::mul_add(np[(size_t)i * m + t], dd[i], acc));
    __syncthreads();
    return acc;
}
// Steps 2 and 3 on the thread's coefficients va of R0 (deg R0 = d0) and acc of R1 = g1, behind rs_interpolant's closing barrier:
// sets up the four rows, and owns sdeg and *snorm from there on.  Returns the thread's coefficient of f in crate form — zero from
// deg f + 1 up, and everywhere for a word that does not decode — and the word's verdict.  No barrier closes it: other threads may
// still read the R rows, the two T rows are free.
template <class F>
__device__ __forceinline__ typename F::elem rs_gao_finish(typename F::elem va, typename F::elem acc, int d0, int stop, uint32_t k,
                                                          typename F::elem r1, typename F::elem* R0, typename F::elem* R1,
                                                          typename F::elem* T0, typename F::elem* T1, typename F::elem* snorm, int* sdeg,
                                                          uint32_t t, long long& verdict) {
    using E = typename F::elem;
    {
        E one = F::zero();
        if (t == 0) one = r1;
        R0[t] = va; R1[t] = acc;
        if (!F::is_zero(acc)) atomicMax(&sdeg[1], (int)t);
        T0[t] = F::zero(); T1[t] = one;
    }
    __syncthreads();
    int d1 = sdeg[1], c0 = 1, c1 = 1;
    __syncthreads();
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    E *S0 = T0, *S1 = T1;
    gcd_remainder_loop<F>(R0, R1, d0, d1, S0, S1, T0, T1, c0, c1, 1u, stop, sdeg, t);
    __syncthreads();
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    if (!F::is_zero(T1[t])) atomicMax(&sdeg[0], (int)t);     // written whole at the start and zero above its length
    __syncthreads();
    const int dt = sdeg[0], dq = d1 - dt;
    bool good = dt >= 0 && (d1 < 0 || (dq >= 0 && dq < (int)k));
    if (good && d1 >= 0) {
        if (t == 0) *snorm = F::canon(F::inv(T1[dt]));
        __syncthreads();
        if ((int)t < dt) T1[t] = F::canon(F::mul(T1[t], *snorm));
        __syncthreads();
        for (int i = dq; i >= 0; --i) {
            const E qi = R1[i + dt];
            if ((int)t < dt) R1[i + (int)t] = F::canon(F::sub(R1[i + (int)t], F::canon(F::mul(qi, T1[t]))));
            __syncthreads();
        }
        if ((int)t < dt && !F::is_zero(R1[t])) atomicMax(&sdeg[1], (int)t);
        __syncthreads();
        good = sdeg[1] < 0;
    }
    E v = F::zero();
    if (good && d1 >= 0 && (int)t <= dq) v = F::canon(F::mul(R1[dt + (int)t], F::canon(F::mul(*snorm, r1))));
    verdict = good ? dt : -1;
    return v;
}
// ecfft_rs_decode's kernel: the shared body on k_rs_prepare's g0.  message row p (k coefficients) = f, zero-padded, n_err[p] = the
// verdict; a word that does not decode leaves a zero row.
template <class F, int G>
__global__ __launch_bounds__(G) void k_rs_decode_small(const typename F::elem* __restrict__ values, uint32_t m, uint32_t k, int32_t stop,
                                                       const typename F::elem* __restrict__ np, const typename F::elem* __restrict__ g0,
                                                       const typename F::elem* __restrict__ invd, typename F::elem* __restrict__ message,
                                                       long long* __restrict__ n_err, typename F::elem r1) {
    using E = typename F::elem;
    __shared__ E buf[4 * G];
    __shared__ E snorm;
    __shared__ int sdeg[2];
    const uint32_t t = threadIdx.x;
    const size_t p = blockIdx.x;
    E *R0 = buf, *R1 = buf + G, *T0 = buf + 2 * G, *T1 = buf + 3 * G;
    E mine = F::zero();
    if (t < m) mine = F::canon(values[p * m + t]);
    const E acc = rs_interpolant<F>(mine, m, np, invd, R0, T0, T1, sdeg, t);
    E va = F::zero();
    if (t <= m) va = g0[t];
    long long verdict;
    const E v = rs_gao_finish<F>(va, acc, (int)m, stop, k, r1, R0, R1, T0, T1, &snorm, sdeg, t, verdict);
    if (t < k) message[p * k + t] = v;
    if (t == 0) n_err[p] = verdict;
}
// ecfft_rs_decode_erasures, small regime: the shared body with a mask per row (erased + p m, may be null: no erasure; a non-zero
// byte marks a lost symbol, whose stored value is never read) behind the same k_rs_prepare over ALL m points.
// With K the kept positions, m' = |K| and g0' = prod_{i in K} (x - x_i): the interpolant over all m points of the row with its
// erased symbols read as 0 is congruent mod g0' to the interpolant over K, and the remainder sequence of (g0', g1) is the swap row,
// g1 mod g0' with cofactor 1, then the rows of the punctured code's own pair.  So rs_interpolant stays as it is, and rs_gao_finish
// takes another first operand and bound: R0 = g0' (deg m'), stop' = ceil((m' + k) / 2).
//   g0': a row without erasure takes the shared g0.  Otherwise the product over the kept points, the recurrence of k_rs_prepare's
//     block 0 with the erased points skipped (m' steps on PLAIN coefficients, then R for crate form; the mask is in LDS, so every
//     thread skips the same steps; the plain points are staged once in a free LDS row and the coefficient row alternates between
//     two rows: one multiply and one barrier a step).  The two loops stay apart: block 0 keeps one row and pays a second barrier a
//     step, which this kernel has the rows to avoid.
//   m' < k: the row fails before any work.
//   form == 0: out row p = the k coefficients of f, as k_rs_decode_small's message.  form != 0: out row p = the m symbols f(x_i),
//     thread i by Horner on the plain x_i = x_i R^-1 (k steps, no barrier); a failed row is zero in both forms.
template <class F, int G>
__global__ __launch_bounds__(G) void k_rs_decode_ee_small(const typename F::elem* __restrict__ values, const uint8_t* __restrict__ erased,
                                                          const typename F::elem* __restrict__ points, uint32_t m, uint32_t k,
                                                          const typename F::elem* __restrict__ np, const typename F::elem* __restrict__ g0,
                                                          const typename F::elem* __restrict__ invd, typename F::elem* __restrict__ out,
                                                          uint32_t form, long long* __restrict__ n_err, typename F::elem rinv,
                                                          typename F::elem r1) {
    using E = typename F::elem;
    __shared__ E buf[4 * G];
    __shared__ E snorm;
    __shared__ int sdeg[2];
    __shared__ uint8_t smask[G];
    const uint32_t t = threadIdx.x;
    const size_t p = blockIdx.x;
    const uint32_t no = form ? m : k;                        // symbols of an output row
    E *R0 = buf, *R1 = buf + G, *T0 = buf + 2 * G, *T1 = buf + 3 * G;
    const bool lost = erased && t < m && erased[p * m + t] != 0;
    smask[t] = lost ? 1 : 0;
    const uint32_t mk = (uint32_t)__syncthreads_count(t < m && !lost);          // m', and smask is visible
    if (mk < k) {
        if (t < no) out[p * no + t] = F::zero();
        if (t == 0) n_err[p] = -1;
        return;
    }
    E mine = F::zero();
    if (t < m && !lost) mine = F::canon(values[p * m + t]);
    const E acc = rs_interpolant<F>(mine, m, np, invd, R0, T0, T1, sdeg, t);
    E va = F::zero();
    if (mk == m) {
        if (t <= m) va = g0[t];
    } else {
        E cur = F::zero(), x = F::zero();
        if (t == 0) cur = F::one();
        if (t < m) x = F::canon(F::mul(F::canon(points[t]), rinv));
        T0[t] = x;                                           // the plain points; read behind the first step's barrier
        E *A = R0, *B = R1;                                  // two alternating rows, one barrier a step, as the divided differences
        for (uint32_t i = 0; i < m; ++i) {
            if (smask[i]) continue;
            A[t] = cur;
            __syncthreads();
            E lo = F::zero();
            if (t) lo = A[t - 1];
            cur = F::canon(F::sub(lo, F::canon(F::mul(T0[i], cur))));
            E* y = A; A = B; B = y;
        }
        __syncthreads();
        if (t <= mk) va = F::canon(F::mul(cur, r1));
    }
    long long verdict;
    const E v = rs_gao_finish<F>(va, acc, (int)mk, (int)((mk + k + 1) / 2), k, r1, R0, R1, T0, T1, &snorm, sdeg, t, verdict);
    if (t == 0) n_err[p] = verdict;
    if (!form) {
        if (t < k) out[p * k + t] = v;
        return;
    }
    T0[t] = v;                                               // f in crate form, zero from k up; the cofactor rows are done
    __syncthreads();
    if (t < m) {
        const E x = F::canon(F::mul(F::canon(points[t]), rinv));
        E y = T0[k - 1];
        for (uint32_t i = k - 1; i-- > 0;) y = F::canon(F::mul_add(y, x, T0[i]));
        out[p * m + t] = y;
    }
}
// ecfft_rs_encode, small regime: with shared points a systematic encoder is ONE linear map, parity = G data, with
// G[j][i] = L_i(x_{k+j}) for the Lagrange basis L_i of the first k points.  Block j < max(m - k, 1), thread i < k:
//   den_i = prod_{l < k, l != i} (x_i - x_l), num_i = prod_{l < k, l != i} (x_{k+j} - x_l): both carry R^(k-1), so num_i / den_i is
//   the PLAIN number G[j][i], and plain x crate stays crate.  Stored transposed, gt[i (m - k) + j]: the encode kernel's threads run
//   along j.  Every pair of points meets in a zero test: two of the first k in den_i (every block), x_{k+j} and any other point in
//   block j's comparison of thread t < m, t != k + j.  Equal points raise *flag.  k == m: one block, the zero tests only.
template <class F, int G>
__global__ __launch_bounds__(G) void k_rs_encode_prepare(const typename F::elem* __restrict__ points, uint32_t m, uint32_t k,
                                                         typename F::elem* __restrict__ gt, int* __restrict__ flag) {
    using E = typename F::elem;
    __shared__ E sx[G];
    const uint32_t t = threadIdx.x, j = blockIdx.x, npar = m - k;
    E x = F::zero();
    if (t < m) x = F::canon(points[t]);
    sx[t] = x;
    __syncthreads();
    if (t >= m) return;
    const bool par = k + j < m;
    E y = F::zero();
    if (par) {
        y = sx[k + j];
        if (t != k + j && F::is_zero(F::canon(F::sub(y, x)))) *flag = 1;
    }
    if (t >= k) return;
    E den = F::one(), num = F::one();
    for (uint32_t l = 0; l < k; ++l) {
        if (l == t) continue;
        const E xl = sx[l];
        den = F::canon(F::mul(den, F::canon(F::sub(x, xl))));
        num = F::canon(F::mul(num, F::canon(F::sub(y, xl))));
    }
    if (F::is_zero(den)) { *flag = 1; return; }
    if (par) gt[(size_t)t * npar + j] = F::canon(F::mul(num, F::inv(den)));
}
// codeword row b (m symbols) = data row b (k symbols, fully reduced), then parity[j] = sum_i G[j][i] data[b][i], j < npar = m - k.
// A workgroup takes rpb = max(1, G / npar) rows: thread t is parity j = t mod npar of row t / npar, so a wave's loads of gt are
// contiguous and a row's data symbol is one address for all its threads.  gt: k_rs_encode_prepare's, i-major.
template <class F, int G>
__global__ __launch_bounds__(G) void k_rs_encode_small(const typename F::elem* __restrict__ data, uint32_t m, uint32_t k,
                                                       const typename F::elem* __restrict__ gt, typename F::elem* __restrict__ codeword,
                                                       size_t count, uint32_t rpb) {
    using E = typename F::elem;
    const uint32_t t = threadIdx.x, npar = m - k;
    const size_t b0 = (size_t)blockIdx.x * rpb;
    const size_t rows = count - b0 < (size_t)rpb ? count - b0 : (size_t)rpb;
    if (npar) {
        const uint32_t r = t / npar, j = t - r * npar;
        if (r < rows) {
            const E* d = data + (b0 + r) * k;
            E acc = F::zero();
            for (uint32_t i = 0; i < k; ++i) acc = F::canon(F::mul_add(gt[(size_t)i * npar + j], F::canon(d[i]), acc));
            codeword[(b0 + r) * m + k + j] = acc;
        }
    }
    for (size_t idx = t; idx < rows * k; idx += G) {
        const size_t r = idx / k, i = idx - r * k;
        codeword[(b0 + r) * m + i] = F::canon(data[(b0 + r) * k + i]);
    }
}
// Rows of different lengths gathered into one zero-padded block: dst row r (blockIdx.y) of n coefficients = rows.p[r] below
// rows.len[r].  The operands of the batched products of the half-GCD (matrix entries, remainders) live in separate buffers.
template <class F>
struct GcdRows { const typename F::elem* p[8]; size_t len[8]; };
template <class F>
__global__ __launch_bounds__(kBlock) void k_gcd_gather(typename F::elem* __restrict__ dst, GcdRows<F> rows, size_t n) {
    using E = typename F::elem;
    const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = blockIdx.y;
    E v = F::zero();
    if (j < rows.len[r]) v = rows.p[r][j];
    dst[(size_t)r * n + j] = v;
}
// Sums of pairs of product rows: out row r (blockIdx.y) of ldo coefficients = base_r + sign (P_{2r} [+ P_{2r+1}]) below np, zero
// above — base == nullptr: none; single != 0: one product per row (P_r); sign != 0 subtracts.  The 2x2 matrix times vector, matrix
// times matrix and quotient steps of the half-GCD after their batched products (rows of P: np coefficients).
template <class F>
__global__ __launch_bounds__(kBlock) void k_gcd_combine(typename F::elem* __restrict__ out, size_t ldo, const typename F::elem* __restrict__ P,
                                                        size_t np, GcdRows<F> base, uint32_t has_base, uint32_t single, uint32_t sign) {
    using E = typename F::elem;
    const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= ldo) return;
    const uint32_t r = blockIdx.y;
    E v = F::zero();
    if (j < np) {
        if (single) v = F::canon(P[(size_t)r * np + j]);
        else v = F::canon(F::add(F::canon(P[(size_t)(2 * r) * np + j]), F::canon(P[(size_t)(2 * r + 1) * np + j])));
    }
    if (sign) v = F::canon(F::neg(v));
    if (has_base && j < base.len[r]) v = F::canon(F::add(v, F::canon(base.p[r][j])));
    out[(size_t)r * ldo + j] = v;
}

// ---------------------------------------------------------------------------------------------
// ecfft_poly_find_roots (utils::find_roots, src/utils.rs:25-44).  A polynomial or factor of degree <= K is finished by ONE
// workgroup (k_roots_small); above that the host drives rounds on the poly_pow_mod / gcd / division bodies that end in the same
// kernel, and k_roots_rank puts the roots in ascending order of their standard form.
// ---------------------------------------------------------------------------------------------
// sres (e residues, crate form) = (x + c)^exp mod h for the monic h of degree e >= 2 whose low e coefficients smod holds as PLAIN
// residues; exp: nbits >= 1 bits, bit nbits - 1 set.  k_powmod_small's scan: a squaring is its product (modmul_*); "multiply by
// the base" is a shift, a scale by the plain integer c and ONE elimination step: x r + c r - r_{e-1} h.
template <class F, int K>
__device__ __forceinline__ void roots_pow_scan(typename F::elem* sres, typename F::elem* sx, typename F::elem* sprod,
                                               const typename F::elem* smod, uint32_t e, uint32_t c, const uint8_t* __restrict__ exp,
                                               uint32_t nbits, const typename F::telem& rinv, const typename F::elem& r1, uint32_t t) {
    using E = typename F::elem;
    const E cE = F::from_u32(c);
    {
        E v = F::zero();
        if (t == 1) v = r1;
        if (t == 0 && c) v = F::canon(F::mul(cE, r1));
        sres[t] = v;
    }
    __syncthreads();
    for (uint32_t i = nbits - 1; i-- > 0;) {
        modmul_plain<F>(sx, sres, rinv, t);
        modmul_reduce<F>(sprod, sx, sres, smod, e, t);
        if (t < e) sres[t] = sprod[t];
        __syncthreads();
        if ((exp[i >> 3] >> (i & 7)) & 1) {
            E v = F::zero();
            if (t < e) {
                const E top = sres[e - 1];
                if (t) v = sres[t - 1];
                if (c) v = F::canon(F::add(v, F::canon(F::mul(cE, sres[t]))));
                v = F::canon(F::sub(v, F::canon(F::mul(top, smod[t]))));
            }
            __syncthreads();
            if (t < e) sres[t] = v;
            __syncthreads();
        }
    }
}
// The remainder sequence of (R0, R1), deg R0 = d0 >= deg R1, to its end: gcd_remainder_loop without cofactors, after the degree
// of R1 is found below d0.  Rows of K + 1 entries; nothing above a row's degree is read.  On return R0 is a non-zero multiple of
// the gcd and the result its degree.  sdeg: two ints.
template <class F, int K>
__device__ __forceinline__ int roots_gcd_rows(typename F::elem*& R0, typename F::elem*& R1, int d0, int* sdeg, uint32_t t) {
    using E = typename F::elem;
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    if ((int)t < d0 && !F::is_zero(R1[t])) atomicMax(&sdeg[1], (int)t);
    __syncthreads();
    int d1 = sdeg[1];
    __syncthreads();
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    E* none = nullptr;
    int c = 0;
    gcd_remainder_loop<F>(R0, R1, d0, d1, none, none, none, none, c, c, 0u, 0, sdeg, t);
    return d0;
}
// quo[0 .. e - du] = A / u for the monic A of degree e (low e plain coefficients in a) and the monic u of degree du <= e (low du
// plain coefficients in u): synthetic division, no inversion.  work: e + 1 entries; quo[e - du] = 1.  a, u, quo, work
// are four different rows.
template <class F>
__device__ __forceinline__ void ddf_div_monic(typename F::elem* quo, typename F::elem* work, const typename F::elem* a, int e,
                                              const typename F::elem* u, int du, uint32_t t) {
    using E = typename F::elem;
    if ((int)t < e) work[t] = a[t];
    if (t == 0) work[e] = F::one();
    __syncthreads();
    for (int k = e - du; k >= 0; --k) {
        const E qk = work[k + du];
        if ((int)t < du) work[k + t] = F::canon(F::sub(work[k + t], F::canon(F::mul(qk, u[t]))));
        if (t == 0) quo[k] = qk;
        __syncthreads();
    }
}
// The prologue of the small factorisation kernels, one workgroup of K threads per row: the true degree d of the row fb (nin <= K + 1
// coefficients, crate form, untrimmed; thread t looks at coefficient t, thread 0 also at coefficient K of a full row) through
// sdeg[0], returned to every thread from behind a barrier: -1 for the zero row.  For d >= 1 the row is made monic: srow[t] = the
// PLAIN residue f_t / f_d, zero from d on, each thread writing its own entry (no barrier after it).  The inversion and the row are
// done for every d >= 1, whatever the caller then rejects (k_edf_small: a degree its dd does not divide).
template <class F, int K>
__device__ __forceinline__ int small_row_monic(const typename F::elem* __restrict__ fb, uint32_t nin, typename F::elem* srow,
                                               typename F::elem* snorm, int* sdeg, uint32_t t) {
    using E = typename F::elem;
    if (t == 0) sdeg[0] = -1;
    __syncthreads();
    E mine = F::zero();
    if (t < nin) mine = F::canon(fb[t]);
    if (!F::is_zero(mine)) atomicMax(&sdeg[0], (int)t);
    if (t == 0 && nin == K + 1 && !F::is_zero(F::canon(fb[K]))) atomicMax(&sdeg[0], K);
    __syncthreads();
    const int d = sdeg[0];
    if (d >= 1) {
        if (t == 0) *snorm = F::canon(F::inv(F::canon(fb[d])));
        __syncthreads();
        E v = F::zero();
        if ((int)t < d) v = F::canon(F::mul(mine, *snorm));
        srow[t] = v;
    }
    return d;
}
// The tail of a successful split in k_roots_small and k_edf_small: the top stack entry h (degree e at stack + base, its plain
// residues also in smod) has met a multiple R0 of its proper factor of degree du.  u = R0 / lc(R0) (sx) by the one inversion of the
// split, v = h / u (sres) by ddf_div_monic on sprod; the entry becomes u and v is pushed above it.  Ends behind a barrier.
template <class F>
__device__ __forceinline__ void split_push(typename F::elem* stack, int* stk_deg, int* stk_off, int sp, int base, int e,
                                           const typename F::elem* R0, int du, typename F::elem* snorm, typename F::elem* sx,
                                           typename F::elem* sres, typename F::elem* sprod, const typename F::elem* smod, uint32_t t) {
    if (t == 0) *snorm = F::canon(F::inv(R0[du]));
    __syncthreads();
    if ((int)t < du) sx[t] = F::canon(F::mul(R0[t], *snorm));
    __syncthreads();
    ddf_div_monic<F>(sres, sprod, smod, e, sx, du, t);
    if ((int)t < du) stack[base + t] = sx[t];
    if ((int)t < e - du) stack[base + du + t] = sres[t];
    if (t == 0) { stk_deg[sp - 1] = du; stk_deg[sp] = e - du; stk_off[sp] = base + du; }
    __syncthreads();
}
// All roots of one polynomial, or of one factor, of degree <= K in one workgroup of K threads, everything in LDS.  Block b reads
// nin <= K + 1 coefficients (crate form, untrimmed, any non-zero leading coefficient) at in + b*ldin and writes its roots, in crate
// form and in NO particular order, from out + b*ldout on; desc != nullptr gives block b the triple (input offset, input length,
// output offset) instead.  n_out[b] (may be null) = the number of roots, -1 for the zero polynomial.
//   frob != 0: the row is first replaced by g = gcd(f, x^p - x mod f), the product of its distinct linear factors (x^p - x is the
//     squarefree product of ALL x - a).  Otherwise the row is taken to be such a product already.
//   Then a stack of monic factors, kept as PLAIN residues without their leading 1 (at most K coefficients in all): a factor
//   x + a yields the root -a; a factor h of degree e >= 2 is split by the next shift c = c0, c0 + 1, ... (one counter per
//   workgroup, incremented after every attempt; p is odd): w = (x + c)^((p-1)/2) mod h, u = gcd(h, w - 1), v = h / u, a success
//   when 0 < deg u < e.  u is made monic by the one inversion of the split; the exact division by the monic u needs none.
// Loop bounds are fixed at launch: the exponents' bit counts, degrees <= K, and kCap consecutive failed shifts of one factor,
// after which *flag = 1 and the workgroup stops (a bug must not spin it; for distinct roots the chance is below 2^-63).
// exp_p / exp_h: p and (p-1)/2 as little-endian bytes with their top bits set.  rinv = R^-1 (table form), r1 = R (M31: both 1).
template <class F, int K>
__global__ __launch_bounds__(K) void k_roots_small(const typename F::elem* __restrict__ in, size_t ldin, uint32_t nin,
                                                   typename F::elem* __restrict__ out, size_t ldout, const uint32_t* __restrict__ desc,
                                                   long long* __restrict__ n_out, uint32_t frob, uint32_t c0,
                                                   const uint8_t* __restrict__ exp_p, uint32_t nbits_p,
                                                   const uint8_t* __restrict__ exp_h, uint32_t nbits_h, typename F::telem rinv,
                                                   typename F::elem r1, int* __restrict__ flag) {
    using E = typename F::elem;
    constexpr uint32_t kCap = 64;
    __shared__ E stack[K], smod[K], sres[K], sx[K], sprod[2 * K], rows[2 * (K + 1)];
    __shared__ E snorm;
    __shared__ int sdeg[2], stk_deg[K], stk_off[K];
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    const E* fb = in + b * ldin;
    E* ob = out + b * ldout;
    if (desc) { fb = in + desc[3 * b]; nin = desc[3 * b + 1]; ob = out + desc[3 * b + 2]; }
    // ---- the true degree, and the row made monic (plain residues f_t / f_d) ----
    const int d = small_row_monic<F, K>(fb, nin, smod, &snorm, sdeg, t);
    if (d <= 0) {
        if (t == 0 && n_out) n_out[b] = d;                   // the zero polynomial: -1; a non-zero constant: no roots
        return;
    }
    stack[t] = smod[t];
    if (t == 0) { stk_deg[0] = d; stk_off[0] = 0; }
    __syncthreads();
    E* R0 = rows;
    E* R1 = rows + K + 1;
    if (frob && d >= 2) {
        // g = gcd(f, x^p - x mod f); the scan's base is x (c = 0)
        roots_pow_scan<F, K>(sres, sx, sprod, smod, (uint32_t)d, 0u, exp_p, nbits_p, rinv, r1, t);
        if ((int)t < d) {
            E v = sres[t];
            if (t == 1) v = F::canon(F::sub(v, r1));
            R1[t] = v;
            R0[t] = smod[t];
        }
        if (t == 0) R0[d] = F::one();
        const int dg = roots_gcd_rows<F, K>(R0, R1, d, sdeg, t);
        if (dg <= 0) {                                       // deg g = 0: no root in the field (g != 0: f != 0)
            if (t == 0 && n_out) n_out[b] = 0;
            return;
        }
        if (t == 0) { snorm = F::canon(F::inv(R0[dg])); stk_deg[0] = dg; }
        __syncthreads();
        if ((int)t < dg) stack[t] = F::canon(F::mul(R0[t], snorm));
        __syncthreads();
    }
    // ---- the splitting recursion on the stack ----
    int sp = 1;
    uint32_t c = c0, fails = 0, nout = 0;
    while (sp > 0) {
        const int e = stk_deg[sp - 1], base = stk_off[sp - 1];
        if (e == 1) {
            if (t == 0) ob[nout] = F::canon(F::neg(F::canon(F::mul(stack[base], r1))));
            ++nout; --sp;
            continue;
        }
        {
            E v = F::zero();
            if ((int)t < e) v = stack[base + t];
            smod[t] = v;
        }
        __syncthreads();
        roots_pow_scan<F, K>(sres, sx, sprod, smod, (uint32_t)e, c, exp_h, nbits_h, rinv, r1, t);
        R0 = rows; R1 = rows + K + 1;
        if ((int)t < e) {
            E v = sres[t];
            if (t == 0) v = F::canon(F::sub(v, r1));
            R1[t] = v;
            R0[t] = smod[t];
        }
        if (t == 0) R0[e] = F::one();
        const int du = roots_gcd_rows<F, K>(R0, R1, e, sdeg, t);
        ++c;
        if (du <= 0 || du >= e) {
            if (++fails >= kCap) { if (t == 0) *flag = 1; break; }
            continue;
        }
        fails = 0;
        split_push<F>(stack, stk_deg, stk_off, sp, base, e, R0, du, &snorm, sx, sres, sprod, smod, t);
        ++sp;
    }
    if (t == 0 && n_out) n_out[b] = (long long)nout;
}
// a < b as standard-form integers (ark's Ord on Fp)
template <class F>
__device__ __forceinline__ bool roots_less(const typename F::elem& a, const typename F::elem& b) {
    if constexpr (sizeof(typename F::elem) == 4) return a < b;
    else {
        bool lt = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) if (a.l[i] != b.l[i]) lt = a.l[i] < b.l[i];
        return lt;
    }
}
// Row r (blockIdx.y) of dst (ldd elements) = the n distinct roots of row r of src (lds apart, crate form, any order) in ascending
// order of their standard form, zero above: rank(i) = the number of roots smaller than root i is a permutation, so each root is
// scattered to its rank.  n = n_dev[r] (negative: 0) or n_fixed.  Standard form is one table multiply by R^-1 (M31: R = 1); the
// others pass through LDS in tiles of kBlock.
template <class F>
__global__ __launch_bounds__(kBlock) void k_roots_rank(typename F::elem* __restrict__ dst, size_t ldd, const typename F::elem* __restrict__ src,
                                                       size_t lds, const long long* __restrict__ n_dev, long long n_fixed,
                                                       typename F::telem rinv) {
    using E = typename F::elem;
    __shared__ E tile[kBlock];
    const uint32_t t = threadIdx.x;
    const size_t r = blockIdx.y, i = (size_t)blockIdx.x * kBlock + t;
    long long nn = n_dev ? n_dev[r] : n_fixed;
    if (nn < 0) nn = 0;
    const size_t n = (size_t)nn < ldd ? (size_t)nn : ldd;
    const E* sr = src + r * lds;
    E mine = F::zero(), ms = F::zero();
    if (i < n) {
        mine = F::canon(sr[i]);
        ms = mine;
        if constexpr (sizeof(E) == 32) ms = F::tmul(rinv, ms);
        ms = F::canon(ms);
    }
    size_t rank = 0;
    for (size_t j0 = 0; j0 < n; j0 += kBlock) {
        __syncthreads();
        if (j0 + t < n) {
            E v = F::canon(sr[j0 + t]);
            if constexpr (sizeof(E) == 32) v = F::tmul(rinv, v);
            tile[t] = F::canon(v);
        }
        __syncthreads();
        const uint32_t m = n - j0 < (size_t)kBlock ? (uint32_t)(n - j0) : (uint32_t)kBlock;
        if (i < n)
            for (uint32_t j = 0; j < m; ++j) rank += roots_less<F>(tile[j], ms) ? 1u : 0u;
    }
    if (i < n) dst[r * ldd + rank] = mine;
    else if (i < ldd) dst[r * ldd + i] = F::zero();
}

// ---------------------------------------------------------------------------------------------
// ecfft_poly_squarefree / ecfft_poly_distinct_degree (utils::square_free_factors and utils::distinct_degree_factors,
// src/utils.rs:46-78, the latter with x^(p^i) where the reference takes x^(p i)).  A polynomial of degree <= K is finished by ONE
// workgroup (k_ddf_small) on the pieces of k_roots_small and the Horner loop of k_compose_small; above that the host drives the
// same loop on the poly_pow_mod / gcd / division bodies and a kept composition.
// ---------------------------------------------------------------------------------------------
// gcd_remainder_loop without cofactors on (R0, R1) with deg R0 = d0 known and R1 scanned below n1 coefficients: unlike
// roots_gcd_rows, deg R1 may exceed d0 (the loop swaps first).  On return R0 is a non-zero multiple of the gcd (R1 = 0: R0 itself)
// and the result its degree.
template <class F>
__device__ __forceinline__ int ddf_gcd_rows(typename F::elem*& R0, typename F::elem*& R1, int d0, int n1, int* sdeg, uint32_t t) {
    using E = typename F::elem;
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    if ((int)t < n1 && !F::is_zero(R1[t])) atomicMax(&sdeg[1], (int)t);
    __syncthreads();
    int d1 = sdeg[1];
    __syncthreads();
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    E* none = nullptr;
    int c = 0;
    gcd_remainder_loop<F>(R0, R1, d0, d1, none, none, none, none, c, c, 0u, 0, sdeg, t);
    return d0;
}
// The squarefree part (mode 1) or the distinct-degree factors (mode 0) of one polynomial of degree <= K in one workgroup of K
// threads, everything in LDS.  Block b reads nin <= K + 1 coefficients (crate form, untrimmed, any non-zero leading coefficient)
// at in + b*ldin.
//   s = f / gcd(f, f') on the monic f (plain residues): f'_j = (j + 1) f_(j+1) with the plain integer j + 1, which is non-zero in
//     the field because p > K; so f' = 0 only for constants and there is no p-th-power case.
//   mode 1: out + b*ldout receives the nw <= K + 1 low coefficients of the monic s in crate form (its leading 1 included where it
//     fits, zero above); deg_out[b*lddeg] = deg s, 0 for a non-zero constant (s = 1), -1 for the zero polynomial (a zero row).
//   mode 0: h_1 = x^p mod s (roots_pow_scan, base x); then for i = 1, 2, ... while deg f* >= 2i (f* = s at first): g = gcd(f*,
//     h_i - x) is the product of the irreducible factors of degree i; a g of positive degree is made monic, appended and divided
//     out; h_(i+1) = h_i(h_1) mod s by Horner (deg s - 1 products of modmul_*), skipped when the loop is about to end.  What is
//     left of f* has no factor of degree <= i and degree < 2(i + 1), so it is irreducible: g_(deg f*).  out + b*ldout receives
//     nw <= K entries: the g_d of positive degree in ascending d, each as its low deg g_d coefficients (crate form), then zeros;
//     deg_out[b*lddeg + d - 1] = deg g_d for d <= nw (zero polynomial: -1, 0, 0, ...).
// Loop bounds are fixed at launch: the bit count of p and degrees <= K.  Every thread takes every barrier: degrees come from LDS
// behind a barrier (gcd_remainder_loop).  exp_p: p as little-endian bytes, bit nbits_p - 1 set; rinv = R^-1 (table form), r1 = R.
template <class F, int K>
__global__ __launch_bounds__(K) void k_ddf_small(const typename F::elem* __restrict__ in, size_t ldin, uint32_t nin,
                                                 typename F::elem* __restrict__ out, size_t ldout, uint32_t nw,
                                                 long long* __restrict__ deg_out, size_t lddeg, uint32_t mode,
                                                 const uint8_t* __restrict__ exp_p, uint32_t nbits_p, typename F::telem rinv,
                                                 typename F::elem r1) {
    using E = typename F::elem;
    __shared__ E smod[K], sfs[K], sh1[K], shi[K], sres[K], sx[K], squo[K + 1], sout[K], sprod[2 * K], rows[2 * (K + 1)];
    __shared__ E snorm;
    __shared__ int sdeg[2], sdegs[K];
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    const E* fb = in + b * ldin;
    E* ob = out + b * ldout;
    long long* db = deg_out + b * lddeg;
    // ---- the true degree, and the row made monic (plain residues f_t / f_d) ----
    sout[t] = F::zero();
    sdegs[t] = 0;
    const int d = small_row_monic<F, K>(fb, nin, smod, &snorm, sdeg, t);
    int ds = d;                                              // deg s
    if (d >= 1) __syncthreads();
    if (d >= 2) {
        // ---- s = f / gcd(f, f') ----
        E* R0 = rows;
        E* R1 = rows + K + 1;
        if ((int)t < d) {
            R0[t] = smod[t];
            E v = F::from_u32(t + 1);
            if ((int)t + 1 < d) v = F::canon(F::mul(v, smod[t + 1]));
            R1[t] = v;
        }
        if (t == 0) R0[d] = F::one();
        const int dg = roots_gcd_rows<F, K>(R0, R1, d, sdeg, t);
        if (dg > 0) {
            if (t == 0) snorm = F::canon(F::inv(R0[dg]));
            __syncthreads();
            if ((int)t < dg) sx[t] = F::canon(F::mul(R0[t], snorm));
            __syncthreads();
            ddf_div_monic<F>(squo, sprod, smod, d, sx, dg, t);
            ds = d - dg;
            {
                E v = F::zero();
                if ((int)t < ds) v = squo[t];
                __syncthreads();
                smod[t] = v;
            }
            __syncthreads();
        }
    }
    if (mode) {
        if (t < nw) {
            E v = F::zero();
            if ((int)t < ds) v = F::canon(F::mul(smod[t], r1));
            if ((int)t == ds) v = r1;
            ob[t] = v;
        }
        if (t == 0 && nw == K + 1) { E v = F::zero(); if (ds == K) v = r1; ob[K] = v; }
        if (t == 0) db[0] = ds;
        return;
    }
    int e = ds < 0 ? 0 : ds;                                 // deg f*
    uint32_t pos = 0;                                        // coefficients appended so far
    if (ds >= 2) {
        sfs[t] = smod[t];
        __syncthreads();
        roots_pow_scan<F, K>(sres, sx, sprod, smod, (uint32_t)ds, 0u, exp_p, nbits_p, rinv, r1, t);
        {
            E v = F::zero();
            if ((int)t < ds) v = sres[t];
            sh1[t] = v;
            shi[t] = v;
        }
        __syncthreads();
        for (int i = 1; e >= 2 * i; ++i) {
            E* R0 = rows;
            E* R1 = rows + K + 1;
            if ((int)t < e) R0[t] = sfs[t];
            if (t == 0) R0[e] = F::one();
            {
                E v = shi[t];
                if (t == 1) v = F::canon(F::sub(v, r1));
                R1[t] = v;
            }
            const int dg = ddf_gcd_rows<F>(R0, R1, e, ds, sdeg, t);
            if (dg > 0) {
                if (t == 0) { snorm = F::canon(F::inv(R0[dg])); sdegs[i - 1] = dg; }
                __syncthreads();
                if ((int)t < dg) {
                    const E v = F::canon(F::mul(R0[t], snorm));
                    sx[t] = v;
                    sout[pos + t] = F::canon(F::mul(v, r1));
                }
                __syncthreads();
                if (dg < e) {
                    ddf_div_monic<F>(squo, sprod, sfs, e, sx, dg, t);
                    if ((int)t < e - dg) sfs[t] = squo[t];
                    __syncthreads();
                }
                pos += (uint32_t)dg;
                e -= dg;
            }
            if (e < 2 * (i + 1)) break;
            // h_(i+1) = h_i(h_1) mod s
            {
                E v = F::zero();
                if (t == 0) v = shi[ds - 1];
                sres[t] = v;
            }
            __syncthreads();
            for (int j = ds - 1; j-- > 0;) {
                modmul_plain<F>(sx, sres, rinv, t);
                modmul_reduce<F>(sprod, sx, sh1, smod, (uint32_t)ds, t);
                if ((int)t < ds) {
                    E v = sprod[t];
                    if (t == 0) v = F::canon(F::add(v, shi[j]));
                    sres[t] = v;
                }
                __syncthreads();
            }
            if ((int)t < ds) shi[t] = sres[t];
            __syncthreads();
        }
    } else if (ds == 1) {
        sfs[t] = smod[t];
        __syncthreads();
    }
    if (e > 0) {
        if ((int)t < e) sout[pos + t] = F::canon(F::mul(sfs[t], r1));
        if (t == 0) sdegs[e - 1] = e;
    }
    if (t == 0 && d < 0) sdegs[0] = -1;
    __syncthreads();
    if (t < nw) { ob[t] = sout[t]; db[t] = sdegs[t]; }
}
// Yun's squarefree decomposition f = lc prod_i a_i^i (a_i monic, squarefree, pairwise coprime) of one polynomial of degree <= K in
// one workgroup of K threads, everything in LDS (ecfft_poly_squarefree_decompose; the first step of ecfft_poly_factor).  Block b
// reads nin <= K + 1 coefficients (crate form, untrimmed, any non-zero leading coefficient) at in + b*ldin.
//   The state is the monic b (sb, plain residues without the leading 1, degree db) and a row sd of degree < db.  One step takes
//   u = gcd(b, sd) (roots_gcd_rows; sd = 0 leaves u = b), made monic by the one inversion of the step, and where deg u > 0 divides
//   it out of both: b <- b / u and c = sd / u.  sd is not monic, but b + sd is, of degree db, and u divides both, so
//   (b + sd) / u = b / u + sd / u: two runs of ddf_div_monic and a subtraction.  Then sd <- c - b', with b'_j = (j + 1) b_(j+1) on the
//   plain integer j + 1 as in k_ddf_small (p > K: derivatives vanish for constants only, there is no p-th-power case).
//   Step 0 starts from b = f, sd = f': u = a_0 = gcd(f, f') is not an output, and leaves b = f / a_0, sd = f' / a_0 - b'.  Step
//   i >= 1 yields a_i = u; a step that meets sd = 0 yields a_i = b and ends the loop.  A squarefree f has a_0 = 1, so sd = f' - f' =
//   0 and step 1 is its last.  i never exceeds deg f.
//   out + b*ldout receives nw <= K entries: the a_i of positive degree in ascending i, each as its low deg a_i coefficients (crate
//   form; the layout of k_ddf_small's g_d), then zeros; deg_out[b*lddeg + i - 1] = deg a_i for i <= nw (the zero polynomial: -1, 0,
//   0, ...; a non-zero constant: zeros); lead[b] (lead may be null) = the leading coefficient, 0 for the zero polynomial.
// Loop bounds are fixed at launch: at most K + 1 steps on degrees <= K.  Every thread takes every barrier: degrees come from LDS
// behind a barrier (gcd_remainder_loop), and pos + db <= deg f holds throughout, so nothing is written past sout.  r1 = R.
template <class F, int K>
__global__ __launch_bounds__(K) void k_yun_small(const typename F::elem* __restrict__ in, size_t ldin, uint32_t nin,
                                                 typename F::elem* __restrict__ out, size_t ldout, uint32_t nw,
                                                 long long* __restrict__ deg_out, size_t lddeg, typename F::elem* __restrict__ lead,
                                                 typename F::elem r1) {
    using E = typename F::elem;
    __shared__ E sb[K], sd[K], sx[K], squo[K + 1], scq[K + 1], sout[K], swork[K + 1], rows[2 * (K + 1)];
    __shared__ E snorm;
    __shared__ int sdeg[2], sdegs[K];
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    const E* fb = in + b * ldin;
    E* ob = out + b * ldout;
    long long* dgb = deg_out + b * lddeg;
    sout[t] = F::zero();
    sdegs[t] = 0;
    // ---- the true degree, and the row made monic (plain residues f_t / f_n) ----
    const int n = small_row_monic<F, K>(fb, nin, sb, &snorm, sdeg, t);
    if (t == 0 && lead) lead[b] = n >= 0 ? F::canon(fb[n]) : F::zero();
    int db = n < 0 ? 0 : n;                                  // deg b
    uint32_t pos = 0;                                        // coefficients appended so far
    if (n >= 1) {
        __syncthreads();
        {
            E v = F::zero();                                 // sd = f'
            if ((int)t < n) {
                v = F::from_u32(t + 1);
                if ((int)t + 1 < n) v = F::canon(F::mul(v, sb[t + 1]));
            }
            sd[t] = v;
        }
        __syncthreads();
        for (int i = 0; i <= K && db > 0; ++i) {
            E* R0 = rows;
            E* R1 = rows + K + 1;
            if ((int)t < db) { R0[t] = sb[t]; R1[t] = sd[t]; }
            if (t == 0) R0[db] = F::one();
            const int du = roots_gcd_rows<F, K>(R0, R1, db, sdeg, t);
            E c = sd[t];                                     // deg u = 0: c = sd
            if (du > 0) {
                if (i > 0 && du == db) {                     // sd = 0: a_i = b, the last one
                    if ((int)t < db) sout[pos + t] = F::canon(F::mul(sb[t], r1));
                    if (t == 0) sdegs[i - 1] = db;
                    break;
                }
                if (t == 0) snorm = F::canon(F::inv(R0[du]));
                __syncthreads();
                if ((int)t < du) {
                    const E v = F::canon(F::mul(R0[t], snorm));
                    sx[t] = v;
                    if (i > 0) sout[pos + t] = F::canon(F::mul(v, r1));
                }
                if (t == 0 && i > 0) sdegs[i - 1] = du;
                if ((int)t < db) sd[t] = F::canon(F::add(sd[t], sb[t]));
                __syncthreads();
                ddf_div_monic<F>(squo, swork, sb, db, sx, du, t);
                ddf_div_monic<F>(scq, swork, sd, db, sx, du, t);
                if (i > 0) pos += (uint32_t)du;
                db -= du;
                E bq = F::zero();
                c = F::zero();
                if ((int)t < db) { bq = squo[t]; c = F::canon(F::sub(scq[t], bq)); }
                sb[t] = bq;
                __syncthreads();
            }
            {
                E v = F::zero();                             // sd <- c - b'
                if ((int)t < db) {
                    E m = F::from_u32(t + 1);
                    if ((int)t + 1 < db) m = F::canon(F::mul(m, sb[t + 1]));
                    v = F::canon(F::sub(c, m));
                }
                sd[t] = v;
            }
            __syncthreads();
        }
    }
    if (t == 0 && n < 0) sdegs[0] = -1;
    __syncthreads();
    if (t < nw) { ob[t] = sout[t]; dgb[t] = sdegs[t]; }
}

// ---------------------------------------------------------------------------------------------
// ecfft_poly_equal_degree (utils::equal_degree_factorization, src/utils.rs:82-113, with the splitting element taken through the
// norm).  A polynomial or factor of degree <= K is finished by ONE workgroup (k_edf_small); above that the host drives rounds on
// the kept modulus and the poly_pow_mod / gcd / division bodies that end in the same kernel, and k_edf_rank puts the factors in
// their canonical order.
// ---------------------------------------------------------------------------------------------
// sres (e residues, crate form) = sbase^exp mod h for the monic h of degree e whose low e coefficients smod holds as PLAIN
// residues and a general base of e crate-form coefficients in LDS: k_powmod_small's scan on its product (modmul_*).  exp: nbits
// >= 1 bits, bit nbits - 1 set.
template <class F>
__device__ __forceinline__ void edf_pow_scan(typename F::elem* sres, typename F::elem* sx, typename F::elem* sprod,
                                             const typename F::elem* sbase, const typename F::elem* smod, uint32_t e,
                                             const uint8_t* __restrict__ exp, uint32_t nbits, const typename F::telem& rinv, uint32_t t) {
    sres[t] = sbase[t];
    __syncthreads();
    for (uint32_t i = nbits - 1; i-- > 0;) {
        const uint32_t passes = 1 + ((exp[i >> 3] >> (i & 7)) & 1);     // a squaring, then on a set bit a product with the base
        for (uint32_t pass = 0; pass < passes; ++pass) {
            modmul_plain<F>(sx, sres, rinv, t);
            modmul_reduce<F>(sprod, sx, pass ? sbase : sres, smod, e, t);
            if (t < e) sres[t] = sprod[t];
            __syncthreads();
        }
    }
}
// The monic irreducible factors of degree dd of one polynomial, or of one factor, of degree n <= K in one workgroup of K threads.
// Block b reads nin <= K + 1 coefficients (crate form, untrimmed, any non-zero leading coefficient) at in + b*ldin, taken to be a
// squarefree product of r = n / dd irreducibles of degree dd, and writes them, each as its low dd coefficients in crate form and
// in NO particular order, from out + b*ldout on; desc != nullptr gives block b the triple (input offset, input length, output
// offset) instead.  n_out[b] (may be null) = r; -1 for the zero polynomial, 0 for a non-zero constant, -2 where dd does not
// divide n (nothing is written in these three cases).  n = dd: the row itself, made monic.
//   Otherwise h_1 = x^p mod g (roots_pow_scan, base x) and h_i = h_(i-1)(h_1) mod g for i = 2 .. dd - 1 by Horner's loop of
//   k_compose_small, as k_ddf_small takes them; the dd - 1 residues go to the block's global workspace ws + b*ldws (row i - 1 at a
//   stride of n; thread t writes and later reads element t only), because they are read once per attempt and do not fit in LDS.
//   Then a stack of monic factors as in k_roots_small: a factor of degree dd is written out; a factor h of degree e > dd is
//   attacked with the next shift c = c0, c0 + 1, ... (one counter per workgroup): the norm N_c = prod_{i<dd} (h_i + c) mod g
//   (dd - 1 products, h_0 = x), reduced modulo h by synthetic division; w = N_c^((p-1)/2) mod h (edf_pow_scan), which is
//   (x + c)^((p^dd - 1)/2); u = gcd(h, w - 1), v = h / u, a success when 0 < deg u < e.
// Loop bounds are fixed at launch: the exponents' bit counts, degrees <= K, dd <= K and kCap consecutive failed shifts of one
// factor, after which *flag = 1 and the workgroup stops; so does a split whose degree dd does not divide (an input outside the
// precondition).  Every thread takes every barrier: degrees come from LDS behind a barrier.
template <class F, int K>
__global__ __launch_bounds__(K) void k_edf_small(const typename F::elem* __restrict__ in, size_t ldin, uint32_t nin, uint32_t dd,
                                                 typename F::elem* __restrict__ out, size_t ldout, const uint32_t* __restrict__ desc,
                                                 long long* __restrict__ n_out, typename F::elem* __restrict__ ws, size_t ldws,
                                                 uint32_t c0, const uint8_t* __restrict__ exp_p, uint32_t nbits_p,
                                                 const uint8_t* __restrict__ exp_h, uint32_t nbits_h, typename F::telem rinv,
                                                 typename F::elem r1, int* __restrict__ flag) {
    using E = typename F::elem;
    constexpr uint32_t kCap = 64;
    __shared__ E sg[K], stack[K], smod[K], sbase[K], sres[K], sx[K], sprod[2 * K], rows[2 * (K + 1)];
    __shared__ E snorm;
    __shared__ int sdeg[2], stk_deg[K], stk_off[K];
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    const E* fb = in + b * ldin;
    E* ob = out + b * ldout;
    E* wb = ws + b * ldws;
    if (desc) { fb = in + desc[3 * b]; nin = desc[3 * b + 1]; ob = out + desc[3 * b + 2]; }
    // ---- the true degree, and the row made monic (plain residues g_t / g_n) ----
    const int n = small_row_monic<F, K>(fb, nin, sg, &snorm, sdeg, t);
    if (n <= 0 || (uint32_t)n % dd != 0) {
        if (t == 0 && n_out) n_out[b] = n <= 0 ? n : -2;
        return;
    }
    __syncthreads();
    const uint32_t r = (uint32_t)n / dd;
    if (r == 1) {
        if (t < dd) ob[t] = F::canon(F::mul(sg[t], r1));
        if (t == 0 && n_out) n_out[b] = 1;
        return;
    }
    // ---- h_1 .. h_(dd-1) modulo g, into the workspace; stack doubles as h_i and sbase as h_1 until the recursion starts ----
    if (dd >= 2) {
        roots_pow_scan<F, K>(sres, sx, sprod, sg, (uint32_t)n, 0u, exp_p, nbits_p, rinv, r1, t);
        {
            E v = F::zero();
            if ((int)t < n) { v = sres[t]; wb[t] = v; }
            sbase[t] = v;
            stack[t] = v;
        }
        __syncthreads();
        for (uint32_t i = 2; i < dd; ++i) {
            {
                E v = F::zero();
                if (t == 0) v = stack[n - 1];
                sres[t] = v;
            }
            __syncthreads();
            for (int j = n - 1; j-- > 0;) {
                modmul_plain<F>(sx, sres, rinv, t);
                modmul_reduce<F>(sprod, sx, sbase, sg, (uint32_t)n, t);
                if ((int)t < n) {
                    E v = sprod[t];
                    if (t == 0) v = F::canon(F::add(v, stack[j]));
                    sres[t] = v;
                }
                __syncthreads();
            }
            if ((int)t < n) { const E v = sres[t]; stack[t] = v; wb[(size_t)(i - 1) * (uint32_t)n + t] = v; }
            __syncthreads();
        }
    }
    stack[t] = sg[t];
    if (t == 0) { stk_deg[0] = n; stk_off[0] = 0; }
    __syncthreads();
    // ---- the splitting recursion on the stack ----
    int sp = 1;
    uint32_t c = c0, fails = 0, nout = 0;
    while (sp > 0) {
        const int e = stk_deg[sp - 1], base = stk_off[sp - 1];
        if ((uint32_t)e == dd) {
            if (t < dd) ob[(size_t)nout * dd + t] = F::canon(F::mul(stack[base + t], r1));
            ++nout; --sp;
            continue;
        }
        const E cR = F::canon(F::mul(F::from_u32(c), r1));
        // N_c = (x + c) prod_i (h_i + c) mod g
        {
            E v = F::zero();
            if ((int)t < e) v = stack[base + t];
            smod[t] = v;
            v = F::zero();
            if (t == 0) v = cR;
            if (t == 1) v = r1;
            sres[t] = v;
        }
        __syncthreads();
        for (uint32_t i = 1; i < dd; ++i) {
            {
                E v = F::zero();
                if ((int)t < n) v = wb[(size_t)(i - 1) * (uint32_t)n + t];
                if (t == 0) v = F::canon(F::add(v, cR));
                sbase[t] = v;
            }
            modmul_plain<F>(sx, sres, rinv, t);
            modmul_reduce<F>(sprod, sx, sbase, sg, (uint32_t)n, t);
            if ((int)t < n) sres[t] = sprod[t];
            __syncthreads();
        }
        // N_c mod h: the remainder side of the synthetic division by the monic h, in place
        for (int k = n - 1 - e; k >= 0; --k) {
            const E qk = sres[k + e];
            if ((int)t < e) sres[k + t] = F::canon(F::sub(sres[k + t], F::canon(F::mul(qk, smod[t]))));
            __syncthreads();
        }
        {
            E v = F::zero();
            if ((int)t < e) v = sres[t];
            __syncthreads();
            sbase[t] = v;
        }
        __syncthreads();
        edf_pow_scan<F>(sres, sx, sprod, sbase, smod, (uint32_t)e, exp_h, nbits_h, rinv, t);
        E* R0 = rows;
        E* R1 = rows + K + 1;
        if ((int)t < e) {
            E v = sres[t];
            if (t == 0) v = F::canon(F::sub(v, r1));
            R1[t] = v;
            R0[t] = smod[t];
        }
        if (t == 0) R0[e] = F::one();
        const int du = roots_gcd_rows<F, K>(R0, R1, e, sdeg, t);
        ++c;
        if (du <= 0 || du >= e) {
            if (++fails >= kCap) { if (t == 0) *flag = 1; break; }
            continue;
        }
        if ((uint32_t)du % dd != 0) { if (t == 0) *flag = 1; break; }
        fails = 0;
        split_push<F>(stack, stk_deg, stk_off, sp, base, e, R0, du, &snorm, sx, sres, sprod, smod, t);
        ++sp;
    }
    if (t == 0 && n_out) n_out[b] = (long long)nout;
}
// Row r (blockIdx.y) of dst (ldd elements) = the n distinct factors of row r of src (lds apart, dd crate-form coefficients each,
// any order) in ascending lexicographic order of (c_0, .., c_(dd-1)) as standard-form integers, zero above: k_roots_rank for rows
// of dd elements.  stdf holds src in standard form (same layout), converted once per element before the launch; the compare exits
// at the first differing coefficient.  Thread i < n scatters factor i to dd * rank(i); the threads from n dd on zero the tail.
// n = n_dev[r] (negative: 0) or n_fixed.
template <class F>
__global__ __launch_bounds__(kBlock) void k_edf_rank(typename F::elem* __restrict__ dst, size_t ldd, const typename F::elem* __restrict__ src,
                                                     const typename F::elem* __restrict__ stdf, size_t lds, uint32_t dd,
                                                     const long long* __restrict__ n_dev, long long n_fixed) {
    using E = typename F::elem;
    const size_t r = blockIdx.y, i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    long long nn = n_dev ? n_dev[r] : n_fixed;
    if (nn < 0) nn = 0;
    const size_t n = (size_t)nn < ldd / dd ? (size_t)nn : ldd / dd;
    const E* sr = src + r * lds;
    const E* ss = stdf + r * lds;
    if (i < n) {
        const E* me = ss + i * dd;
        size_t rank = 0;
        for (size_t j = 0; j < n; ++j) {
            const E* o = ss + j * dd;
            bool lt = false;
            for (uint32_t k = 0; k < dd; ++k) {
                const E a = o[k], m = me[k];
                if (roots_less<F>(a, m)) { lt = true; break; }
                if (roots_less<F>(m, a)) break;
            }
            rank += lt ? 1u : 0u;
        }
        for (uint32_t k = 0; k < dd; ++k) dst[r * ldd + rank * dd + k] = F::canon(sr[i * dd + k]);
    } else if (i >= n * dd && i < ldd) {
        dst[r * ldd + i] = F::zero();
    }
}

// ---------------------------------------------------------------------------------------------
// ecfft_curve_trace_mod (frobenius_trace_mod_l, examples/schoofs.rs:76-138): the trace of Frobenius of y^2 = x^3 + A x + B modulo
// a small prime l, in the ring F_p[x]/(h) that starts at h = psi_l made monic.  A modulus of degree <= K is finished by ONE
// workgroup (k_schoof_small), everything in LDS, on the pieces of k_roots_small / k_edf_small / k_compose_small.
// ---------------------------------------------------------------------------------------------
// What the workgroup shares: LDS rows of K entries, thread t owning coefficient t of every row, every row in crate form, fully
// reduced and zero from d on.  An endomorphism is a pair of rows (a, b) standing for (a(x), b(x) y).
template <class F, int K>
struct SchoofWg {
    using E = typename F::elem;
    using TE = typename F::telem;
    E *smod, *sx, *sprod, *sres, *fx, *num, *rr, *iv, *tz, *a3, *b3, *rows, *snorm;
    int* sdeg;                                               // [0], [1]: gcd_remainder_loop's degrees; [2]: a vote
    TE rinv;
    E r1, cA;
    uint32_t d, t;

    // crate x crate -> crate for scalars
    __device__ __forceinline__ E cmul(const E& a, const E& b) const {
        E v = F::mul(a, b);
        if constexpr (sizeof(E) == 32) v = F::tmul(rinv, v);
        return F::canon(v);
    }
    // dst = a b mod h (dst may be a or b)
    __device__ __forceinline__ void mm(E* dst, const E* a, const E* b) {
        modmul_plain<F>(sx, a, rinv, t);
        modmul_reduce<F>(sprod, sx, b, smod, d, t);
        E v = F::zero();
        if (t < d) v = sprod[t];
        dst[t] = v;
        __syncthreads();
    }
    // dst = a b mod x^K without a modulus (psi_l from the recurrence: every product there has at most 61 coefficients)
    __device__ __forceinline__ void pmul(E* dst, const E* a, const E* b) {
        modmul_plain<F>(sx, a, rinv, t);
        E acc = F::zero();
        for (uint32_t i = 0; i <= t; ++i) acc = F::canon(F::mul_add(sx[i], b[t - i], acc));
        __syncthreads();
        dst[t] = acc;
        __syncthreads();
    }
    // does pred hold at every coefficient below d?  The same answer in every thread.
    __device__ __forceinline__ bool all(bool pred) {
        if (t == 0) sdeg[2] = 0;
        __syncthreads();
        if (t < d && !pred) sdeg[2] = 1;
        __syncthreads();
        const bool r = sdeg[2] == 0;
        __syncthreads();
        return r;
    }
    __device__ __forceinline__ bool eq(const E* a, const E* b) { return all(F::eq(a[t], b[t])); }
    __device__ __forceinline__ bool negeq(const E* a, const E* b) { return all(F::is_zero(F::canon(F::add(a[t], b[t])))); }
    // dst = c(g) mod h for the d coefficients of the row c: Horner's loop of k_compose_small (dst is neither c nor g)
    __device__ __forceinline__ void compose(E* dst, const E* c, const E* g) {
        {
            E v = F::zero();
            if (t == 0) v = c[d - 1];
            dst[t] = v;
        }
        __syncthreads();
        for (uint32_t i = d - 1; i-- > 0;) {
            mm(dst, dst, g);
            if (t == 0) dst[0] = F::canon(F::add(dst[0], c[i]));
            __syncthreads();
        }
    }
    // The remainder sequence of (h, e) for the row e whose coefficient t is `den` (zero from d on), with the cofactor of e:
    // gcd_remainder_loop with its S rows aliased to the T rows (the cofactor of h is never needed, and both get the same values).
    // Returns deg gcd (d itself for e = 0); R0 is a non-zero multiple of the gcd and R0 = T0 e mod h.
    __device__ __forceinline__ int gcd_h(const E& den, E*& R0, E*& T0) {
        R0 = rows;
        E* R1 = rows + K + 1;
        T0 = iv;
        E* T1 = tz;
        if (t < 2) sdeg[t] = -1;
        __syncthreads();
        if (t < d) R0[t] = smod[t];
        if (t == 0) R0[d] = F::one();
        R1[t] = den;
        if (!F::is_zero(den)) atomicMax(&sdeg[1], (int)t);
        {
            E o = F::zero();
            if (t == 0) o = r1;
            T0[t] = F::zero(); T1[t] = o;
        }
        __syncthreads();
        int d0 = (int)d, d1 = sdeg[1], c0 = 1, c1 = 1;
        __syncthreads();
        if (t < 2) sdeg[t] = -1;
        __syncthreads();
        E *S0 = T0, *S1 = T1;
        gcd_remainder_loop<F>(R0, R1, d0, d1, S0, S1, T0, T1, c0, c1, 1u, 0, sdeg, t);
        return d0;
    }
    // the modulus becomes R0 / lc(R0), of degree dg: plain residues, zero from dg on
    __device__ __forceinline__ void remodulus(const E* R0, int dg) {
        if (t == 0) *snorm = F::canon(F::inv(R0[dg]));
        __syncthreads();
        E v = F::zero();
        if ((int)t < dg) v = F::canon(F::mul(R0[t], *snorm));
        __syncthreads();
        smod[t] = v;
        d = (uint32_t)dg;
        __syncthreads();
    }
    // (a3, b3) = (a1, b1) + (a2, b2), the reference's Add (schoofs.rs:237-273) with the case it lacks.  Returns 0: done; 1: the
    // sum is the point at infinity (a1 = a2, b1 = -b2); 2: a denominator was not invertible and the modulus is now the proper
    // factor gcd(denominator, h) — with a1 = a2 and b1 != +-b2 the factor gcd(b1 - b2, h), else gcd(b1 + b2, h); 3: neither is
    // proper, or a denominator is zero (a defect: for an odd prime l it cannot happen).  a3, b3 are none of the operands.
    __device__ __forceinline__ int add(const E* a1, const E* b1, const E* a2, const E* b2) {
        E den;
        E *R0, *T0;
        if (eq(a1, a2)) {
            if (negeq(b1, b2)) return 1;
            if (eq(b1, b2)) {                                // the tangent: (3 a1^2 + A) / (2 f b1)
                mm(num, a1, a1);
                E v = F::canon(F::mul(F::from_u32(3), num[t]));
                if (t == 0) v = F::canon(F::add(v, cA));
                num[t] = v;
                mm(rr, fx, b1);
                den = F::canon(F::add(rr[t], rr[t]));
            } else {
                for (int sgn = 0; sgn < 2; ++sgn) {
                    den = sgn ? F::canon(F::add(b1[t], b2[t])) : F::canon(F::sub(b1[t], b2[t]));
                    const int dg = gcd_h(den, R0, T0);
                    if (dg > 0 && dg < (int)d) { remodulus(R0, dg); return 2; }
                }
                return 3;
            }
        } else {                                             // the chord: (b1 - b2) / (a1 - a2)
            num[t] = F::canon(F::sub(b1[t], b2[t]));
            den = F::canon(F::sub(a1[t], a2[t]));
        }
        const int dg = gcd_h(den, R0, T0);
        if (dg < 0 || dg >= (int)d) return 3;
        if (dg > 0) { remodulus(R0, dg); return 2; }
        if (t == 0) *snorm = F::canon(F::mul(F::inv(R0[0]), r1));   // the one inversion of the sum, as k_gcd_small normalises
        __syncthreads();
        {
            E v = F::zero();
            if (t < d) v = F::canon(F::mul(T0[t], *snorm));
            a3[t] = v;
        }
        __syncthreads();
        mm(rr, num, a3);                                     // the slope r
        mm(a3, rr, rr);
        mm(a3, a3, fx);                                      // r^2 y^2
        {
            const E v = F::canon(F::sub(F::canon(F::sub(a3[t], a1[t])), a2[t]));
            a3[t] = v;
            b3[t] = F::canon(F::sub(a1[t], v));
        }
        __syncthreads();
        mm(b3, rr, b3);
        b3[t] = F::canon(F::sub(b3[t], b1[t]));
        __syncthreads();
        return 0;
    }
    __device__ __forceinline__ void copy(E* dst, const E* src) {
        E v = F::zero();
        if (t < d) v = src[t];
        dst[t] = v;
    }
};
// t mod l for one curve per workgroup of K threads, with #E = p + 1 - t.  Block b takes the curve (A[b], B[b]) (crate form) and
// writes t_out[b]: -1 for a singular curve (4 A^3 + 27 B^2 = 0), else the residue in [0, l).  kq = p mod l.
//   l = 2: the residue is 0 iff f = x^3 + A x + B has a root, i.e. gcd(x^p - x mod f, f) != 1 (roots_pow_scan, base x).
//   mod_in != nullptr (l odd): the first modulus is block b's row of nmod <= K + 1 coefficients at mod_in + b*nmod, a monic factor
//     of psi_l in crate form that the large regime hands down after a split; psi_l is not built.
//   l = 3, 5, 7, 11: psi_l is built here from the closed forms of psi_3, psi_4 and the recurrence (schoofs.rs:368-431) by
//     products without a modulus (at most 61 coefficients), so the call needs no transform and no other launch.  Then attempts
//     on a monic modulus h of degree d, at first psi_l / l:
//       f mod h from x mod h by two products; pi = (x^p, f^((p-1)/2)) (roots_pow_scan, base x; edf_pow_scan, base f);
//       pi^2 = (pi_a(pi_a), pi_b(pi_a) pi_b) by Horner's loop where d - 1 < pow_cost, the products of one power with p, else
//       (pi_a^p, pi_b^p pi_b); pi2 = 1 / 2 force the power / the composition (the test-build hook);
//       Q = [kq](x, y) by kq - 1 sums with (x, y); E = pi^2 + Q — the point at infinity gives 0; then j pi for j = 1, 2, ...,
//       each from the last by one sum with pi, compared with E: the j that matches, 0 if none does below l.
//     A sum whose denominator is not invertible replaces h by a proper factor (SchoofWg::add) and the attempt starts over: every
//     non-zero point of E[l] gives the same residue.  Degrees fall strictly, so there are at most d + 1 attempts; d = 1 is an
//     attempt like any other (a root of psi_l says nothing about its y, so there is no shortcut).
// A defect (SchoofWg::add's 3) stores 1 to *flag and gives 0.  Every thread takes every barrier: all decisions come from LDS
// behind a barrier.
// LDS: 20 rows of K and the two remainder rows of K + 1: smod, sx, sprod (2), sres, fx, x, 1, pi (2), pi^2 then E (2), Q then
// j pi (2), num, r, the cofactor rows (2), the sum (2) = 22 K + 2 elements, and snorm and three ints beside them; secp256k1 at
// K = 64: 45164 bytes of the 65536 a workgroup gets.  The rows from fx on serve the psi recurrence first.
template <class F, int K>
__global__ __launch_bounds__(K) void k_schoof_small(const typename F::elem* __restrict__ A, const typename F::elem* __restrict__ B,
                                                    const typename F::elem* __restrict__ mod_in, uint32_t nmod, uint32_t l,
                                                    uint32_t kq, long long* __restrict__ t_out, uint32_t pi2,
                                                    uint32_t pow_cost, const uint8_t* __restrict__ exp_p, uint32_t nbits_p,
                                                    const uint8_t* __restrict__ exp_h, uint32_t nbits_h, typename F::telem rinv,
                                                    typename F::elem r1, int* __restrict__ flag) {
    using E = typename F::elem;
    constexpr int NR = 20;
    __shared__ E buf[NR * K + 2 * (K + 1)];
    __shared__ E snorm;
    __shared__ int sdeg[3];
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    SchoofWg<F, K> w;
    w.smod = buf; w.sx = buf + K; w.sprod = buf + 2 * K; w.sres = buf + 4 * K; w.fx = buf + 5 * K;
    E *xr = buf + 6 * K, *one = buf + 7 * K, *pa = buf + 8 * K, *pb = buf + 9 * K, *ea = buf + 10 * K, *eb = buf + 11 * K;
    E *qa = buf + 12 * K, *qb = buf + 13 * K;
    w.num = buf + 14 * K; w.rr = buf + 15 * K; w.iv = buf + 16 * K; w.tz = buf + 17 * K; w.a3 = buf + 18 * K; w.b3 = buf + 19 * K;
    w.rows = buf + NR * K; w.snorm = &snorm; w.sdeg = sdeg; w.rinv = rinv; w.r1 = r1; w.t = t; w.d = 3;
    const E cA = F::canon(A[b]), cB = F::canon(B[b]);
    w.cA = cA;
    if (t == 0) {
        const E a3 = w.cmul(w.cmul(cA, cA), cA), b2 = w.cmul(cB, cB);
        const E disc = F::canon(F::add(F::canon(F::mul(F::from_u32(4), a3)), F::canon(F::mul(F::from_u32(27), b2))));
        sdeg[2] = F::is_zero(disc) ? 1 : 0;
    }
    __syncthreads();
    const bool singular = sdeg[2] != 0;
    __syncthreads();
    if (singular) {
        if (t == 0) t_out[b] = -1;
        return;
    }
    // f = x^3 + A x + B as a row
    E* frow = w.fx;
    {
        E v = F::zero();
        if (t == 0) v = cB;
        if (t == 1) v = cA;
        if (t == 3) v = r1;
        frow[t] = v;
    }
    __syncthreads();
    if (l == 2) {
        modmul_plain<F>(w.sx, frow, rinv, t);
        {
            E v = F::zero();
            if (t < 3) v = w.sx[t];
            w.smod[t] = v;
        }
        __syncthreads();
        roots_pow_scan<F, K>(w.sres, w.sx, w.sprod, w.smod, 3u, 0u, exp_p, nbits_p, rinv, r1, t);
        E den = F::zero();
        if (t < 3) den = w.sres[t];
        if (t == 1) den = F::canon(F::sub(den, r1));
        E *R0, *T0;
        const int dg = w.gcd_h(den, R0, T0);
        if (t == 0) t_out[b] = dg > 0 ? 0 : 1;
        return;
    }
    if (mod_in) {
        // ---- the modulus is given: a monic factor of psi_l in crate form, nmod = degree + 1 coefficients ----
        const uint32_t dm = nmod - 1;
        E v = F::zero();
        if (t < dm) v = F::canon(mod_in[b * (size_t)nmod + t]);
        w.num[t] = v;
        __syncthreads();
        modmul_plain<F>(w.sx, w.num, rinv, t);
        w.smod[t] = w.sx[t];
        w.d = dm;
        __syncthreads();
    } else {
        // ---- psi_l, not monic, into hrow; then the modulus ----
        E *F2 = buf + 6 * K, *p3 = buf + 7 * K, *p4 = buf + 8 * K, *c3 = buf + 9 * K, *p5 = buf + 10 * K, *c4 = buf + 11 * K;
        E *p7 = buf + 12 * K, *p6 = buf + 13 * K, *tA = buf + 14 * K, *tB = buf + 15 * K;
        auto sc = [&](uint32_t k, const E& v) { return F::canon(F::mul(F::from_u32(k), v)); };
        {
            E v3 = F::zero(), v4 = F::zero();
            if (t == 0) {
                const E aa = w.cmul(cA, cA), ab = w.cmul(cA, cB), bb = w.cmul(cB, cB), aaa = w.cmul(aa, cA);
                p3[0] = F::canon(F::neg(aa)); p3[1] = sc(12, cB); p3[2] = sc(6, cA); p3[3] = F::zero(); p3[4] = sc(3, r1);
                p4[0] = F::canon(F::neg(F::canon(F::add(sc(2, aaa), sc(16, bb)))));
                p4[1] = F::canon(F::neg(sc(8, ab))); p4[2] = F::canon(F::neg(sc(10, aa))); p4[3] = sc(40, cB); p4[4] = sc(10, cA);
                p4[5] = F::zero(); p4[6] = sc(2, r1);
            }
            if (t >= 5) p3[t] = v3;
            if (t >= 7) p4[t] = v4;
        }
        __syncthreads();
        const E* hrow = p3;
        if (l >= 5) {
            w.pmul(F2, frow, frow);
            F2[t] = sc(16, F2[t]);
            w.pmul(c3, p3, p3);
            w.pmul(c3, c3, p3);                              // psi_3^3
            w.pmul(p5, F2, p4);
            p5[t] = F::canon(F::sub(p5[t], c3[t]));          // psi_5 = 16 f^2 psi_4 psi_2^3 - psi_1 psi_3^3
            __syncthreads();
            hrow = p5;
        }
        if (l >= 7) {
            w.pmul(c4, p4, p4);                              // psi_4^2
            w.pmul(tA, c4, p4);
            w.pmul(tA, tA, F2);
            w.pmul(p7, p5, c3);
            p7[t] = F::canon(F::sub(p7[t], tA[t]));          // psi_7 = psi_5 psi_3^3 - 16 f^2 psi_2 psi_4^3
            __syncthreads();
            hrow = p7;
        }
        if (l == 11) {
            tA[t] = F::canon(F::sub(p5[t], c4[t]));
            __syncthreads();
            w.pmul(p6, p3, tA);                              // psi_6 = psi_3 (psi_5 psi_2^2 - psi_1 psi_4^2)
            w.pmul(tA, p5, p5);
            w.pmul(tA, tA, p5);
            w.pmul(tA, tA, p7);                              // psi_7 psi_5^3
            w.pmul(tB, p6, p6);
            w.pmul(tB, tB, p6);
            w.pmul(tB, tB, p4);
            w.pmul(tB, tB, F2);                              // 16 f^2 psi_4 psi_6^3
            tA[t] = F::canon(F::sub(tA[t], tB[t]));          // psi_11
            __syncthreads();
            hrow = tA;
        }
        const uint32_t dl = (l * l - 1) / 2;
        if (t == 0) snorm = F::canon(F::inv(hrow[dl]));
        __syncthreads();
        {
            E v = F::zero();
            if (t < dl) v = F::canon(F::mul(hrow[t], snorm));
            w.smod[t] = v;
        }
        w.d = dl;
        __syncthreads();
    }
    // ---- attempts ----
    long long res = 0;
    for (int attempt = 0; attempt <= K; ++attempt) {
        const uint32_t d = w.d;
        // x, 1 and f modulo h
        {
            E vx = F::zero(), v1 = F::zero();
            if (d == 1) { if (t == 0) vx = F::canon(F::neg(F::canon(F::mul(w.smod[0], r1)))); }
            else if (t == 1) vx = r1;
            if (t == 0) v1 = r1;
            xr[t] = vx; one[t] = v1;
        }
        __syncthreads();
        w.mm(w.fx, xr, xr);
        w.mm(w.fx, w.fx, xr);
        {
            E v = F::canon(F::add(w.fx[t], w.cmul(cA, xr[t])));
            if (t == 0) v = F::canon(F::add(v, cB));
            w.fx[t] = v;
        }
        __syncthreads();
        // pi
        if (d >= 2) {
            roots_pow_scan<F, K>(w.sres, w.sx, w.sprod, w.smod, d, 0u, exp_p, nbits_p, rinv, r1, t);
            w.copy(pa, w.sres);
        } else {
            w.copy(pa, xr);                                  // a constant is its own p-th power
        }
        __syncthreads();
        edf_pow_scan<F>(w.sres, w.sx, w.sprod, w.fx, w.smod, d, exp_h, nbits_h, rinv, t);
        w.copy(pb, w.sres);
        __syncthreads();
        // pi^2
        if (pi2 == 2 || (pi2 == 0 && d - 1 < pow_cost)) {
            w.compose(ea, pa, pa);
            w.compose(w.num, pb, pa);
            w.mm(eb, w.num, pb);
        } else {
            edf_pow_scan<F>(w.sres, w.sx, w.sprod, pa, w.smod, d, exp_p, nbits_p, rinv, t);
            w.copy(ea, w.sres);
            __syncthreads();
            edf_pow_scan<F>(w.sres, w.sx, w.sprod, pb, w.smod, d, exp_p, nbits_p, rinv, t);
            w.mm(eb, w.sres, pb);
        }
        // Q = [kq](x, y)
        w.copy(qa, xr); w.copy(qb, one);
        __syncthreads();
        int st = 0;
        for (uint32_t i = 1; i < kq && st == 0; ++i) {
            st = w.add(qa, qb, xr, one);
            if (st == 0) { w.copy(qa, w.a3); w.copy(qb, w.b3); __syncthreads(); }
        }
        if (st == 2) continue;
        if (st != 0) { if (t == 0) *flag = 1; break; }       // [i](x, y) is never the point at infinity below l
        // E = pi^2 + Q
        st = w.add(ea, eb, qa, qb);
        if (st == 2) continue;
        if (st == 1) break;                                  // pi^2 + [p] = O: the trace is 0 modulo l
        if (st == 3) { if (t == 0) *flag = 1; break; }
        w.copy(ea, w.a3); w.copy(eb, w.b3);
        w.copy(qa, pa); w.copy(qb, pb);
        __syncthreads();
        // j pi
        for (uint32_t j = 1; j < l; ++j) {
            if (w.eq(qa, ea) && w.eq(qb, eb)) { res = (long long)j; break; }
            if (j + 1 == l) break;
            st = w.add(qa, qb, pa, pb);
            if (st != 0) break;
            w.copy(qa, w.a3); w.copy(qb, w.b3);
            __syncthreads();
        }
        if (st == 2) continue;
        if (st == 3 && t == 0) *flag = 1;
        break;
    }
    if (t == 0) t_out[b] = res;
}

// ---------------------------------------------------------------------------------------------
// Points of short-Weierstrass curves y^2 = x^3 + A x + B (curve_points.h has the group law): ecfft_curve_point_mul,
// ecfft_curve_point_two_adicity and the scan of ecfft_curve_find_generator.  One thread per row, workgroups of one wave (a row is
// a chain of thousands of dependent multiplies, so a small call spreads over as many CUs as it has waves); no LDS, no scratch.
// Curves and points arrive in crate form and are taken to plain form here (secp256k1: one multiply by rinv = 2^-256; M31: the
// crate's form is the plain one), results go back the same way.
// ---------------------------------------------------------------------------------------------
constexpr int kPointBlock = 64;
enum { POINT_FLAG_OFF_CURVE = 1, POINT_FLAG_SINGULAR = 2, POINT_FLAG_BAD_ORDER = 4 };

template <class F>
__device__ __forceinline__ typename F::elem point_to_plain(const typename F::elem& v, const typename F::elem& rinv) {
    if constexpr (sizeof(typename F::elem) == 32) return F::mul(v, rinv);
    else return F::canon(v);
}
// row i of a point call: its curve (plain) and its base (plain; inf = the point at infinity).  false: a singular curve or a
// point off its curve, flagged
template <class F>
__device__ __forceinline__ bool point_load(const typename F::elem* __restrict__ A, const typename F::elem* __restrict__ B, uint32_t ncurves,
                                           const typename F::elem* __restrict__ P, const uint8_t* __restrict__ inf_in, size_t i,
                                           const typename F::elem& rinv, typename F::elem& a, typename F::elem& x, typename F::elem& y,
                                           bool& inf, unsigned* __restrict__ flag) {
    const size_t ci = ncurves == 1 ? 0 : i;
    a = point_to_plain<F>(A[ci], rinv);
    const typename F::elem b = point_to_plain<F>(B[ci], rinv);
    inf = inf_in && inf_in[i] != 0;
    x = point_to_plain<F>(P[2 * i], rinv);
    y = point_to_plain<F>(P[2 * i + 1], rinv);
    unsigned bad = 0;
    if (ecpoint::singular<F>(a, b)) bad |= POINT_FLAG_SINGULAR;
    if (!inf && !ecpoint::on_curve<F>(x, y, a, b)) bad |= POINT_FLAG_OFF_CURVE;
    if (bad) atomicOr(flag, bad);
    return bad == 0;
}

// out[i] = [k_i] P_i: double-and-add from bit nbits - 1 (the longest scalar's) down, so every lane of a wave doubles at every
// step and takes the mixed addition where its own bit is set; one inversion per row at the end.
template <class F>
__global__ __launch_bounds__(kPointBlock) void k_point_mul(const typename F::elem* __restrict__ A, const typename F::elem* __restrict__ B,
                                                           uint32_t ncurves, const typename F::elem* __restrict__ P,
                                                           const uint8_t* __restrict__ inf_in, const uint8_t* __restrict__ k,
                                                           uint32_t nscalars, uint32_t nbytes, uint32_t nbits,
                                                           typename F::elem* __restrict__ out, uint8_t* __restrict__ inf_out, size_t count,
                                                           const typename F::elem rinv, unsigned* __restrict__ flag) {
    using E = typename F::elem;
    const size_t i = (size_t)blockIdx.x * kPointBlock + threadIdx.x;
    if (i >= count) return;
    E a, x, y;
    bool inf;
    E ox = F::zero(), oy = F::zero();
    bool finite = false;
    if (point_load<F>(A, B, ncurves, P, inf_in, i, rinv, a, x, y, inf, flag) && !inf) {
        const ecpoint::Jac<F> r = ecpoint::jac_mul<F>(x, y, k + (nscalars == 1 ? 0 : i) * (size_t)nbytes, nbytes, nbits, a);
        finite = ecpoint::jac_to_affine<F>(r, &ox, &oy);
    }
    out[2 * i] = F::to_mont(ox);
    out[2 * i + 1] = F::to_mont(oy);
    inf_out[i] = finite ? 0 : 1;
}

// out[i] = the smallest j <= cap with 2^j P_i = O, -1 when there is none: the doubling of the kernel above, nothing inverted
template <class F>
__global__ __launch_bounds__(kPointBlock) void k_point_two_adicity(const typename F::elem* __restrict__ A, const typename F::elem* __restrict__ B,
                                                                   uint32_t ncurves, const typename F::elem* __restrict__ P,
                                                                   const uint8_t* __restrict__ inf_in, uint32_t cap, int32_t* __restrict__ out,
                                                                   size_t count, const typename F::elem rinv, unsigned* __restrict__ flag) {
    using E = typename F::elem;
    const size_t i = (size_t)blockIdx.x * kPointBlock + threadIdx.x;
    if (i >= count) return;
    E a, x, y;
    bool inf;
    int32_t r = -1;
    if (point_load<F>(A, B, ncurves, P, inf_in, i, rinv, a, x, y, inf, flag))
        r = inf ? 0 : ecpoint::jac_two_adicity<F>(ecpoint::Jac<F>{x, y, F::one()}, cap, a);
    out[i] = r;
}

// One batch of ecfft_curve_find_generator: thread i takes the candidate x = x0 + i on the curve (a, b) (plain).  Where
// x^3 + a x + b is a non-zero square, R = (x, its canonical root), and
//   want_gen: G = [m] R (the shared scalar m = order / 2^v); two-adicity of G exactly v -> best_gen <- min(i); 2^v G not the
//             identity -> the order is not the curve's, flagged
//   want_off: 2^(v + 1) R not the identity -> best_off <- min(i)
template <class F>
__global__ __launch_bounds__(kPointBlock) void k_find_generator(const typename F::elem a, const typename F::elem b, uint64_t x0, uint32_t count,
                                                                const uint8_t* __restrict__ m, uint32_t mbytes, uint32_t mbits, uint32_t v,
                                                                int want_gen, int want_off, unsigned* __restrict__ best_gen,
                                                                unsigned* __restrict__ best_off, unsigned* __restrict__ flag) {
    using E = typename F::elem;
    const uint32_t i = blockIdx.x * kPointBlock + threadIdx.x;
    if (i >= count) return;
    const uint64_t xi = x0 + i;
    E x = F::from_u32((uint32_t)xi);
    if constexpr (sizeof(E) == 32) x.l[1] = (uint32_t)(xi >> 32);
    const E f = ecpoint::rhs<F>(x, a, b);
    if (F::is_zero(f)) return;
    const E y = F::sqrt_canon(f);
    if (!F::eq(F::sqr(y), f)) return;
    if (want_gen) {
        const ecpoint::Jac<F> g = ecpoint::jac_mul<F>(x, y, m, mbytes, mbits, a);
        const int t = ecpoint::jac_two_adicity<F>(g, v, a);
        if (t < 0) atomicOr(flag, (unsigned)POINT_FLAG_BAD_ORDER);
        else if ((uint32_t)t == v) atomicMin(best_gen, i);
    }
    if (want_off) {
        ecpoint::Jac<F> d{x, y, F::one()};
#pragma unroll 1
        for (uint32_t j = 0; j <= v && !F::is_zero(d.Z); ++j) d = ecpoint::jac_double<F>(d, a);
        if (!F::is_zero(d.Z)) atomicMin(best_off, i);
    }
}

// ---------------------------------------------------------------------------------------------
// ecfft_seq_min_poly / ecfft_seq_nth_term (no reference counterpart): linear recurrences.  The minimal polynomial
// of a row of N terms is read off the row (r, ., t) of the remainder sequence of (x^N, h), h = sum s_i x^i, that is the first
// below degree floor(N / 2) (MCA Alg. 12.9); the terms at an index K are x^K mod C against the initial terms (Fiduccia).
// ---------------------------------------------------------------------------------------------
// The verdict and the minimal polynomial from a row of the sequence, T = c t for some scalar c != 0, deg T = dt >= 0, and dr =
// deg r: d = max(dr + 1, dt); the row is determined iff T[0] != 0 and 2 d <= n.  Then C = x^d t(1/x) / t(0): coefficient j is
// T[d - j] / T[0], which takes the scale c out, and the one inversion of the row is R / T[0] (r1 = R), so that plain products of
// stored numbers stay in crate form.  Returns the order d, or -1 for an undetermined row.
__device__ __forceinline__ int seq_minpoly_order(bool t0_nonzero, int dr, int dt, uint32_t n) {
    const int d = dr + 1 > dt ? dr + 1 : dt;
    return t0_nonzero && 2 * (uint32_t)d <= n ? d : -1;
}
// ecfft_seq_min_poly, small regime (n <= G - 1 terms): one row per workgroup of G threads, everything in LDS, thread t owning
// coefficient t of every row.  R0 = x^n is built here (the crate's 1 at index n: any non-zero scalar would do), R1 = the row, and
// gcd_remainder_loop runs with bound = floor(n / 2) and its S rows aliased to the T rows, as in rs_gao_finish: the cofactor of x^n
// is never needed, and both get the same values.  When the loop ends R1 = c r and T1 = c t for the wanted row.  seq: row p at
// seq + p n; min_poly: row p of n / 2 + 1 coefficients, C with its leading 1 at index L and zero above, a zero row where the row is
// undetermined; orders[p] = L or -1.  Every thread takes the same path: the verdict comes from LDS behind a barrier.
template <class F, int G>
__global__ __launch_bounds__(G) void k_seq_minpoly_small(const typename F::elem* __restrict__ seq, uint32_t n,
                                                         typename F::elem* __restrict__ min_poly, long long* __restrict__ orders,
                                                         typename F::elem r1) {
    using E = typename F::elem;
    __shared__ E buf[4 * G];
    __shared__ E snorm;
    __shared__ int sdeg[2];
    const uint32_t t = threadIdx.x;
    const size_t p = blockIdx.x;
    E *R0 = buf, *R1 = buf + G, *T0 = buf + 2 * G, *T1 = buf + 3 * G;
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    {
        E va = F::zero(), vb = F::zero(), one = F::zero();
        if (t == n) va = r1;
        if (t < n) vb = F::canon(seq[p * n + t]);
        if (t == 0) one = r1;
        R0[t] = va; R1[t] = vb;
        if (!F::is_zero(vb)) atomicMax(&sdeg[1], (int)t);
        T0[t] = F::zero(); T1[t] = one;
    }
    __syncthreads();
    int d0 = (int)n, d1 = sdeg[1], c0 = 1, c1 = 1;
    __syncthreads();
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    E *S0 = T0, *S1 = T1;
    gcd_remainder_loop<F>(R0, R1, d0, d1, S0, S1, T0, T1, c0, c1, 1u, (int)(n / 2), sdeg, t);
    __syncthreads();
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    if (!F::is_zero(T1[t])) atomicMax(&sdeg[0], (int)t);     // written whole at the start and zero above its length
    __syncthreads();
    const int order = seq_minpoly_order(!F::is_zero(T1[0]), d1, sdeg[0], n);
    if (t == 0) {
        E c = F::zero();
        if (order >= 0) c = F::canon(F::mul(F::inv(T1[0]), r1));
        snorm = c;
        orders[p] = order;
    }
    __syncthreads();
    const uint32_t nh = n / 2 + 1;
    if (t < nh) {
        E v = F::zero();
        if ((int)t <= order) v = F::canon(F::mul(T1[order - (int)t], snorm));
        min_poly[p * nh + t] = v;
    }
}
// ecfft_seq_min_poly, large regime: k_seq_minpoly_small's epilogue in global memory, after gcd_partial_pair has left the row's r
// and t (n + 1 coefficients each, zero-padded, fully reduced).  One workgroup: the two degrees by a strided scan, the verdict, the
// one inversion, the reversed write of min_poly (n / 2 + 1 coefficients) and *order.
template <class F>
__global__ __launch_bounds__(kBlock) void k_seq_minpoly_finish(const typename F::elem* __restrict__ r, const typename F::elem* __restrict__ tt,
                                                               uint32_t n, typename F::elem* __restrict__ min_poly,
                                                               long long* __restrict__ order_out, typename F::elem r1) {
    using E = typename F::elem;
    __shared__ E snorm;
    __shared__ int sdeg[2];
    const uint32_t t = threadIdx.x;
    if (t < 2) sdeg[t] = -1;
    __syncthreads();
    int dr = -1, dt = -1;
    for (uint32_t j = t; j <= n; j += kBlock) {
        if (!F::is_zero(F::canon(r[j]))) dr = (int)j;
        if (!F::is_zero(F::canon(tt[j]))) dt = (int)j;
    }
    if (dr >= 0) atomicMax(&sdeg[0], dr);
    if (dt >= 0) atomicMax(&sdeg[1], dt);
    __syncthreads();
    const E t0 = F::canon(tt[0]);
    const int order = seq_minpoly_order(!F::is_zero(t0), sdeg[0], sdeg[1], n);
    if (t == 0) {
        E c = F::zero();
        if (order >= 0) c = F::canon(F::mul(F::inv(t0), r1));
        snorm = c;
        *order_out = order;
    }
    __syncthreads();
    const uint32_t nh = n / 2 + 1;
    for (uint32_t j = t; j < nh; j += kBlock) {
        E v = F::zero();
        if ((int)j <= order) v = F::canon(F::mul(tt[order - (int)j], snorm));
        min_poly[j] = v;
    }
}
// sres <- x sres mod (x^e + smod) for a residue of e >= 1 crate-form coefficients and the PLAIN low coefficients smod of the monic
// modulus: a shift and one elimination step, as roots_pow_scan multiplies by its base.  Two barriers.
template <class F>
__device__ __forceinline__ void seq_shift(typename F::elem* sres, const typename F::elem* smod, uint32_t e, uint32_t t) {
    using E = typename F::elem;
    E v = F::zero();
    if (t < e) {
        const E top = sres[e - 1];
        if (t) v = sres[t - 1];
        v = F::canon(F::sub(v, F::canon(F::mul(top, smod[t]))));
    }
    __syncthreads();
    if (t < e) sres[t] = v;
    __syncthreads();
}
// ecfft_seq_nth_term, small regime (L = nc - 1 <= K): one row per workgroup of K threads.  u = x^index mod C by k_powmod_small's
// scan on the product modmul_* with the base x (a set bit is seq_shift; the scan starts from 1, so L = 1 and index = 0 need no case
// of their own), C made monic as k_powmod_small makes its modulus (a zero leading coefficient raises *flag).  Then nout rounds of
// {out = sum_j u_j init_j by a tree reduction in LDS, u <- x u mod C}.  u and init are both crate form, so the plain sum carries
// R^2 and one table multiply by R^-1 per term restores crate form (M31: R = 1).  char_poly: row b at char_poly + b (L + 1); init:
// row b at init + b L; index: nbits bits, little-endian bytes, bit nbits - 1 set (nbits == 0: index 0); out: count x nout.
template <class F, int K>
__global__ __launch_bounds__(K) void k_seq_terms_small(typename F::elem* __restrict__ out, uint32_t nout,
                                                       const typename F::elem* __restrict__ char_poly, uint32_t L,
                                                       const typename F::elem* __restrict__ init, const uint8_t* __restrict__ index,
                                                       uint32_t nbits, typename F::telem rinv, typename F::elem r1, int* __restrict__ flag) {
    using E = typename F::elem;
    __shared__ E sres[K], sinit[K], smod[K], sx[K], sprod[2 * K];
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    modmul_monic<F>(smod, sx, char_poly + b * ((size_t)L + 1), L, flag, t);
    {
        E v = F::zero(), one = F::zero();
        if (t < L) v = F::canon(init[b * L + t]);
        if (t == 0) one = r1;
        sinit[t] = v;
        sres[t] = one;
    }
    __syncthreads();
    for (uint32_t i = nbits; i-- > 0;) {
        if (i + 1 < nbits) {                                 // the top bit meets the residue 1: no squaring
            modmul_plain<F>(sx, sres, rinv, t);
            modmul_reduce<F>(sprod, sx, sres, smod, L, t);
            if (t < L) sres[t] = sprod[t];
            __syncthreads();
        }
        if ((index[i >> 3] >> (i & 7)) & 1) seq_shift<F>(sres, smod, L, t);
    }
    for (uint32_t o = 0; o < nout; ++o) {
        E v = F::zero();
        if (t < L) v = F::canon(F::mul(sres[t], sinit[t]));
        sprod[t] = v;
        __syncthreads();
        for (uint32_t h = K / 2; h > 0; h >>= 1) {
            if (t < h) sprod[t] = F::canon(F::add(sprod[t], sprod[t + h]));
            __syncthreads();
        }
        if (t == 0) {
            E sum = sprod[0];
            if constexpr (sizeof(E) == 32) sum = F::tmul(rinv, sum);
            out[b * nout + o] = F::canon(sum);
        }
        if (o + 1 < nout) seq_shift<F>(sres, smod, L, t);
    }
}
// ecfft_seq_nth_term, large regime, behind the power u = x^index mod C of every row (u: count x L, crate form): a workgroup per
// row, each thread striding over L, one block reduction per term, and between two terms the shift u' = x u mod C,
// u'_j = u_{j-1} - (u_{L-1} / c_L) c_j, from one global row into the other (u and alt, each count x L; alt is not touched for
// nout == 1).  The quotient u_{L-1} / c_L is a PLAIN number (the stored inverse of c_L times the stored u_{L-1}), so its products
// with the crate-form c_j stay crate.  A zero c_L was flagged by the power; its row computes on inv(0) = 0 and is not used.
template <class F>
__global__ __launch_bounds__(kBlock) void k_seq_terms(typename F::elem* __restrict__ out, uint32_t nout, typename F::elem* __restrict__ u,
                                                      typename F::elem* __restrict__ alt, const typename F::elem* __restrict__ char_poly,
                                                      uint32_t L, const typename F::elem* __restrict__ init, typename F::telem rinv) {
    using E = typename F::elem;
    __shared__ E sred[kBlock];
    __shared__ E slinv;
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    const E* c = char_poly + b * ((size_t)L + 1);
    const E* s0 = init + b * (size_t)L;
    E* cur = u + b * (size_t)L;
    E* nxt = alt ? alt + b * (size_t)L : nullptr;
    if (t == 0) slinv = F::canon(F::inv(F::canon(c[L])));
    for (uint32_t o = 0; o < nout; ++o) {
        E acc = F::zero();
        for (uint32_t j = t; j < L; j += kBlock) acc = F::canon(F::mul_add(cur[j], F::canon(s0[j]), acc));
        sred[t] = acc;
        __syncthreads();
        for (uint32_t h = kBlock / 2; h > 0; h >>= 1) {
            if (t < h) sred[t] = F::canon(F::add(sred[t], sred[t + h]));
            __syncthreads();
        }
        if (t == 0) {
            E sum = sred[0];
            if constexpr (sizeof(E) == 32) sum = F::tmul(rinv, sum);
            out[b * nout + o] = F::canon(sum);
        }
        if (o + 1 == nout) break;
        const E w = F::canon(F::mul(F::canon(cur[L - 1]), slinv));
        for (uint32_t j = t; j < L; j += kBlock) {
            E v = F::zero();
            if (j) v = F::canon(cur[j - 1]);
            nxt[j] = F::canon(F::sub(v, F::canon(F::mul(w, F::canon(c[j])))));
        }
        __syncthreads();                                     // the row just written is the next term's operand
        { E* x = cur; cur = nxt; nxt = x; }
    }
}

// ---------------------------------------------------------------------------------------------
// generic element-wise helper for tree construction: functor(i) for i < n
// ---------------------------------------------------------------------------------------------
template <class Fn>
__global__ __launch_bounds__(kBlock) void k_foreach(Fn fn, size_t n) {
    size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g < n) fn(g);
}

}  // namespace ecfft
