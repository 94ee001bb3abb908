// C-ABI of the MI355X ECFFT hot path — implements include/ecfft_hip.h.
#include <hip/hip_runtime.h>
#include <cstring>
#include <memory>
#include <new>
#include "device_tree.h"
#include "wire_parse.h"
#include "seq_host.h"
#include "../../include/ecfft_hip.h"
#ifdef ECFFT_TEST_HOOKS
#include "../../include/ecfft_hip_hooks.h"    // test / measurement entry points: never in the shipped library
#endif

using namespace ecfft;

struct ecfft_ctx {
    int field;
    int device;
    std::unique_ptr<DeviceChain<Secp256k1>> secp;
    std::unique_ptr<DeviceChain<M31>> m31;
    void* stage = nullptr;       // device staging for host-pointer calls (in + out), lazily sized
    size_t stage_bytes = 0;
    hipEvent_t last_op = nullptr;   // completion of the previous transform on this context: calls on other streams wait for
                                    // it before touching the shared scratch buffers (contexts serialise, see ecfft_hip.h)
    ~ecfft_ctx() { if (stage) (void)hipFree(stage); if (last_op) (void)hipEventDestroy(last_op); }
};

namespace {

inline bool is_pow2(size_t n) { return n && (n & (n - 1)) == 0; }

// ---- field dispatch ------------------------------------------------------------------------------------------------
inline bool known_field(int field) { return field == ECFFT_FIELD_SECP256K1 || field == ECFFT_FIELD_M31; }
template <class F> struct FieldTag { using type = F; };
// fn(FieldTag<F>{}) for the field with id `field`; ECFFT_ERR_BAD_ARG for an unknown id
template <class Fn>
int with_field(int field, Fn&& fn) {
    if (field == ECFFT_FIELD_SECP256K1) return fn(FieldTag<Secp256k1>{});
    if (field == ECFFT_FIELD_M31) return fn(FieldTag<M31>{});
    return ECFFT_ERR_BAD_ARG;
}
// fn(chain) with the context's chain
template <class Fn>
decltype(auto) with_chain(const ecfft_ctx* c, Fn&& fn) {
    if (c->field == ECFFT_FIELD_SECP256K1) return fn(*c->secp);
    return fn(*c->m31);
}
template <class F>
std::unique_ptr<DeviceChain<F>>& slot_of(ecfft_ctx& c) {
    if constexpr (std::is_same<F, Secp256k1>::value) return c.secp;
    else return c.m31;
}
// the largest tree of each field: src/lib.rs:62-64, src/ec.rs:510-515
template <class F> constexpr unsigned kMaxLogN = std::is_same<F, Secp256k1>::value ? 35 : 28;

// the crate's in-memory representation <-> plain residues on host buffers: Montgomery for secp256k1, the identity for M31
template <class F>
void to_crate_host(typename F::elem* v, size_t n) {
    if constexpr (std::is_same<F, Secp256k1>::value)
        for (size_t i = 0; i < n; ++i) v[i] = Secp256k1::to_mont(v[i]);
}
template <class F>
void from_crate_host(typename F::elem* v, size_t n) {
    if constexpr (std::is_same<F, Secp256k1>::value) {     // x*2^256 -> x : multiply by 2^-256 = (2^32+977)^-1
        Fe256 r = Secp256k1::zero(); r.l[0] = 977; r.l[1] = 1;
        const Fe256 rinv = Secp256k1::inv(r);
        for (size_t i = 0; i < n; ++i) v[i] = Secp256k1::mul(v[i], rinv);
    }
}
// ecfft_elems_to_standard (to_standard) / ecfft_elems_from_standard
int convert_elems(int field, const void* in, void* out, size_t n, bool to_standard) {
    if (!in || !out) return ECFFT_ERR_BAD_ARG;
    return with_field(field, [&](auto tag) -> int {
        using E = typename decltype(tag)::type::elem;
        if (in != out) memmove(out, in, n * sizeof(E));
        if (to_standard) from_crate_host<typename decltype(tag)::type>((E*)out, n);
        else to_crate_host<typename decltype(tag)::type>((E*)out, n);
        return ECFFT_OK;
    });
}
// rational maps -> the caller's arrays of 3 numerator / denominator coefficients per map, in the crate's representation
template <class F>
void maps_out(const std::vector<RatMap<F>>& maps, void* num3, void* den3) {
    using E = typename F::elem;
    for (size_t k = 0; k < maps.size(); ++k) {
        RatMap<F> m = maps[k];
        to_crate_host<F>(m.num, 3); to_crate_host<F>(m.den, 3);
        if (num3) memcpy((E*)num3 + 3 * k, m.num, sizeof(m.num));
        if (den3) memcpy((E*)den3 + 3 * k, m.den, sizeof(m.den));
    }
}

bool have_device(int device) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0 || device < 0 || device >= cnt) {
        fprintf(stderr, "ecfft: no usable HIP device %d (count=%d) — this library has no CPU fallback\n", device, cnt);
        return false;
    }
    return true;
}

// Every entry point that touches the device selects the context's device and puts the caller's current device back on
// the way out, whatever path it leaves by.
struct DeviceGuard {
    int prev = -1; bool ok = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// a hipMalloc'd temporary, freed on every exit path
struct DeviceBuffer {
    void* p = nullptr; bool ok;
    explicit DeviceBuffer(size_t bytes) : ok(hipMalloc(&p, bytes) == hipSuccess) {}
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    template <class T> T* as() const { return (T*)p; }
};

// no C++ exception (allocation failure inside the chain) crosses the C ABI
template <class Fn>
int guarded(Fn fn) {
    try { return fn(); }
    catch (const std::bad_alloc&) { return ECFFT_ERR_HIP; }
    catch (...) { return ECFFT_ERR_HIP; }
}

// ---- building a context --------------------------------------------------------------------------------------------
// A new context of `field` on `device`: its chain is made and built by `build(chain)` with the device selected, under guarded.
// The context is handed out only when that returns ECFFT_OK.
template <class F, class Build>
int new_ctx(int field, int device, ecfft_ctx** out, Build&& build) {
    std::unique_ptr<ecfft_ctx> c(new (std::nothrow) ecfft_ctx());
    if (!c) return ECFFT_ERR_HIP;
    c->field = field; c->device = device;
    std::unique_ptr<DeviceChain<F>>& slot = slot_of<F>(*c);
    const int rc = guarded([&]() -> int {
        slot.reset(new (std::nothrow) DeviceChain<F>());
        if (!slot) return ECFFT_ERR_HIP;
        DeviceGuard dev(device);
        if (!dev.ok) return ECFFT_ERR_HIP;
        return build(*slot);
    });
    if (rc == ECFFT_OK) *out = c.release();
    return rc;
}
// FFTree::new on a host tree
template <class F>
int build_chain(DeviceChain<F>& ch, HostTree<F>&& ht, int device) {
    if (ch.build(std::move(ht), device)) return ECFFT_OK;
    return ch.bad_points() ? ECFFT_ERR_BAD_ARG : ECFFT_ERR_HIP;       // a leaf that is a pole of its isogeny map is a caller error
}
// ecfft_build_fftree and the shard builders after their own checks: the size limit of the field (it needs no device), the device,
// the maps of the 2^log_n-leaf tree on the host (its leaves and layers are computed on the GPU: points_on_device), then
// build(chain, host tree) on a new context
template <class Build>
int new_tree_ctx(int field, unsigned log_n, int device, ecfft_ctx** out, Build&& build) {
    return with_field(field, [&](auto tag) -> int {
        using F = typename decltype(tag)::type;
        if (log_n > kMaxLogN<F>) return ECFFT_ERR_TREE_TOO_LARGE;
        if (!have_device(device)) return ECFFT_ERR_HIP;
        HostTree<F> ht;
        const int r = build_host_tree<F>(log_n, ht, /*points=*/false);
        if (r) return r == 1 ? ECFFT_ERR_TREE_TOO_LARGE : ECFFT_ERR_BAD_ARG;
        return new_ctx<F>(field, device, out, [&](DeviceChain<F>& ch) -> int { return build(ch, std::move(ht)); });
    });
}

// ---- one call on a context -----------------------------------------------------------------------------------------
bool ensure_stage(ecfft_ctx* c, size_t bytes) {
    if (c->stage_bytes >= bytes) return true;
    if (c->stage) (void)hipFree(c->stage);
    c->stage = nullptr; c->stage_bytes = 0;
    if (hipMalloc(&c->stage, bytes) != hipSuccess) return false;
    c->stage_bytes = bytes;
    return true;
}

// Device work on a context: selects its device, takes the chain lock, and orders the call after the previous one on the same
// context, whatever streams they use.  Its completion is recorded in `last_op` on EVERY exit path after a successful begin — an
// early error return must not leave `last_op` pointing before work that was enqueued.
struct CallScope {
    ecfft_ctx* c; hipStream_t s; DeviceGuard dev; std::unique_lock<std::mutex> lock; bool ok = false;
    CallScope(ecfft_ctx* c_, std::mutex& m, hipStream_t s_) : c(c_), s(s_), dev(c_->device) {
        if (!dev.ok) return;
        lock = std::unique_lock<std::mutex>(m);
        ok = c->last_op ? hipStreamWaitEvent(s, c->last_op, 0) == hipSuccess
                        : hipEventCreateWithFlags(&c->last_op, hipEventDisableTiming) == hipSuccess;
    }
    ~CallScope() { if (ok) (void)hipEventRecord(c->last_op, s); }
};

struct In { const void* ptr; size_t bytes; };
struct Out { void* ptr; size_t bytes; bool in_place = false; };   // in_place: the input with the same pointer, in its slot

// A call in device memory (the pointers go to `body` as they are; asynchronous on `s`) or in host memory, staged through the
// context's one grow-only device buffer: the inputs are uploaded in order, `body` runs on the staged copies and only if it returns
// ECFFT_OK are the outputs downloaded and `s` drained.  A null pointer is an absent slot.  An input with the same pointer and size
// as an earlier one is staged once: both get the same device pointer (a host-memory poly_mul(a, a) stays a squaring).
template <class Chain, size_t NI, size_t NO, class Body>
int staged(ecfft_ctx* c, Chain& ch, int mem, void* stream, const In (&in)[NI], const Out (&out)[NO], Body&& body) {
    if (mem != ECFFT_MEM_HOST && mem != ECFFT_MEM_DEVICE) return ECFFT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    CallScope scope(c, ch.lock(), s);
    if (!scope.ok) return ECFFT_ERR_HIP;
    const void* din[NI]; void* dout[NO];
    for (size_t i = 0; i < NI; ++i) din[i] = in[i].ptr;
    for (size_t o = 0; o < NO; ++o) dout[o] = out[o].ptr;
    if (mem == ECFFT_MEM_HOST) {
        size_t off[NI + NO], total = 0;
        auto same = [&](size_t i) { for (size_t j = 0; j < i; ++j) if (in[j].ptr == in[i].ptr && in[j].bytes == in[i].bytes) return j; return i; };
        for (size_t i = 0; i < NI; ++i)
            if (in[i].ptr && same(i) == i) { off[i] = total; total += (in[i].bytes + 31) & ~(size_t)31; }   // a byte mask keeps the next slot aligned
        for (size_t o = 0; o < NO; ++o)
            if (out[o].ptr && !out[o].in_place) { off[NI + o] = total; total += (out[o].bytes + 31) & ~(size_t)31; }
        if (!ensure_stage(c, total)) return ECFFT_ERR_HIP;
        char* st = (char*)c->stage;
        for (size_t i = 0; i < NI; ++i) {
            if (!in[i].ptr) continue;
            if (same(i) != i) { din[i] = din[same(i)]; continue; }
            din[i] = st + off[i];
            if (hipMemcpyAsync((void*)din[i], in[i].ptr, in[i].bytes, hipMemcpyHostToDevice, s) != hipSuccess) return ECFFT_ERR_HIP;
        }
        for (size_t o = 0; o < NO; ++o) {
            if (!out[o].ptr) continue;
            dout[o] = st + off[NI + o];
            for (size_t i = 0; i < NI && out[o].in_place; ++i) if (in[i].ptr == out[o].ptr) dout[o] = (void*)din[i];
        }
    }
    const int rc = body(din, dout);
    if (rc != ECFFT_OK || mem != ECFFT_MEM_HOST) return rc;
    for (size_t o = 0; o < NO; ++o)
        if (out[o].ptr && out[o].bytes && hipMemcpyAsync(out[o].ptr, dout[o], out[o].bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return ECFFT_ERR_HIP;
    return hipStreamSynchronize(s) == hipSuccess ? ECFFT_OK : ECFFT_ERR_HIP;
}

enum Op { OP_ENTER, OP_EXIT, OP_EXTEND };

// a context made by ecfft_build_extend_shard / ecfft_build_enter_shard / ecfft_build_exit_shard holds one rank's share of the tables of ONE split transform
// and nothing else: only that transform (ecfft_extend_sharded[_layout] / ecfft_enter_sharded / ecfft_exit_sharded with the same size, world and rank;
// run_sharded checks) plus ecfft_tree_size, ecfft_field, ecfft_ctx_device_bytes, ecfft_profile_* and ecfft_ctx_destroy accept it
inline bool shard_only(const ecfft_ctx* c) { return with_chain(c, [](auto& ch) { return ch.shard_mode(); }); }
// a context-bound call: run(chain) under guarded, on a context that holds a full tree unless `shards` (the split transforms)
template <class Run>
int on_chain(ecfft_ctx* ctx, Run&& run, bool shards = false) {
    if (!ctx || (!shards && shard_only(ctx))) return ECFFT_ERR_BAD_ARG;
    return guarded([&] { return with_chain(ctx, run); });
}

template <class F>
int run_op(ecfft_ctx* c, DeviceChain<F>& ch, Op op, const void* in, void* out, size_t len, size_t count, int moiety,
           int mem, void* stream) {
    using E = typename F::elem;
    if (!in || !out) return ECFFT_ERR_BAD_ARG;
    if (!is_pow2(len)) return ECFFT_ERR_NOT_POW2;
    if (count == 0) return ECFFT_ERR_BAD_ARG;
    size_t need_tree = (op == OP_EXTEND) ? len * 2 : len;
    if (need_tree > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;          // "FFTree is too small"
    if (op == OP_EXTEND && moiety != ECFFT_S0 && moiety != ECFFT_S1) return ECFFT_ERR_BAD_ARG;
    const size_t bytes = len * count * sizeof(E);
    return staged(c, ch, mem, stream, {{in, bytes}}, {{out, bytes}}, [&](auto d, auto o) -> int {
        const E* din = (const E*)d[0]; E* dout = (E*)o[0];
        hipStream_t s = (hipStream_t)stream;
        bool ok = true;
        switch (op) {
            case OP_ENTER: ok = ch.enter(din, dout, len, count, s); break;
            case OP_EXIT: ok = ch.exit(din, dout, len, count, s); break;
            case OP_EXTEND: ok = ch.extend_api(din, dout, len, count, moiety, s); break;
        }
        return !ok || hipGetLastError() != hipSuccess ? ECFFT_ERR_HIP : ECFFT_OK;
    });
}

// ecfft_poly_mul: inputs of na and nb and an output of na + nb - 1 elements per pair
template <class F>
int run_poly_mul(ecfft_ctx* c, DeviceChain<F>& ch, const void* a, size_t na, const void* b, size_t nb, void* out, size_t count,
                 int mem, void* stream) {
    using E = typename F::elem;
    if (!a || !b || !out) return ECFFT_ERR_BAD_ARG;
    if (na > ch.size() || nb > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t nc = na + nb - 1, N = DeviceChain<F>::mul_leaves(na, nb);
    if (N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;                   // "FFTree is too small"
    if (count > SIZE_MAX / (8 * N * sizeof(E))) return ECFFT_ERR_BAD_ARG;  // byte counts of the temporaries must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{a, na * eb}, {b, nb * eb}}, {{out, nc * eb}}, [&](auto d, auto o) -> int {
        return ch.poly_mul((const E*)d[0], na, (const E*)d[1], nb, (E*)o[0], count, (hipStream_t)stream) ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}

// ecfft_poly_divrem / ecfft_poly_inv_series: synchronous (the chain reads back the device flag of a zero divisor leading
// coefficient / f[0], reported as ECFFT_ERR_BAD_ARG)
template <class F>
int run_poly_divrem(ecfft_ctx* c, DeviceChain<F>& ch, const void* a, size_t na, const void* b, size_t nb, void* q, void* r, size_t count,
                    int mem, void* stream) {
    using E = typename F::elem;
    if (!a || !b || (!q && !r)) return ECFFT_ERR_BAD_ARG;
    const size_t lim = SIZE_MAX / (64 * sizeof(E));
    if (na > lim || nb > lim) return ECFFT_ERR_BAD_ARG;
    const size_t nq = na >= nb ? na - nb + 1 : 0, nr = nb - 1;
    const size_t N = DeviceChain<F>::divrem_leaves(na, nb);                 // 1 for nb == 1 (scaling) and na < nb (copy): no transform
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t per = N > na + nb ? N : na + nb;
    if (count > SIZE_MAX / (8 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG; // byte counts of the temporaries must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{a, na * eb}, {b, nb * eb}}, {{q, nq * eb}, {r, nr * eb}}, [&](auto d, auto o) -> int {
        bool singular = false;
        if (!ch.poly_divrem((const E*)d[0], na, (const E*)d[1], nb, (E*)o[0], (E*)o[1], count, &singular, (hipStream_t)stream)) return ECFFT_ERR_HIP;
        return singular ? ECFFT_ERR_BAD_ARG : ECFFT_OK;                     // a zero leading coefficient of b in some pair
    });
}

template <class F>
int run_inv_series(ecfft_ctx* c, DeviceChain<F>& ch, const void* f, size_t nf, void* out, size_t k, size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!f || !out) return ECFFT_ERR_BAD_ARG;
    const size_t lim = SIZE_MAX / (64 * sizeof(E));
    if (nf > lim || k > lim) return ECFFT_ERR_BAD_ARG;
    const size_t N = DeviceChain<F>::inv_series_leaves(k);
    if (N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;                     // k = 1: N = 1, any tree
    const size_t per = N > nf + k ? N : nf + k;
    if (count > SIZE_MAX / (8 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG;
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{f, nf * eb}}, {{out, k * eb}}, [&](auto d, auto o) -> int {
        bool singular = false;
        if (!ch.inv_series((const E*)d[0], nf, (E*)o[0], k, count, &singular, (hipStream_t)stream)) return ECFFT_ERR_HIP;
        return singular ? ECFFT_ERR_BAD_ARG : ECFFT_OK;                     // f[0] == 0 in some pair: no power-series inverse
    });
}

// ecfft_poly_eval_points: asynchronous on `stream` in device memory (nothing is data dependent)
template <class F>
int run_poly_eval_points(ecfft_ctx* c, DeviceChain<F>& ch, const void* f, size_t nf, const void* points, size_t m, void* out, size_t count,
                         int mem, void* stream) {
    using E = typename F::elem;
    if (!f || !points || !out) return ECFFT_ERR_BAD_ARG;
    const size_t lim = SIZE_MAX / (64 * sizeof(E));
    if (nf > lim || m > lim) return ECFFT_ERR_BAD_ARG;
    const size_t G = DeviceChain<F>::eval_group(nf), P = (m + G - 1) / G * G;
    if (G > DeviceChain<F>::kEvalLeaf && G > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;    // nf <= 64: Horner only, any tree
    if (P > SIZE_MAX / (8 * 64 * sizeof(E))) return ECFFT_ERR_BAD_ARG;     // node data: 4 P elements per level, < 64 levels
    const size_t per = P > nf ? P : nf;
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG; // byte counts of the temporaries must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{f, nf * eb}, {points, m * sizeof(E)}}, {{out, m * eb}}, [&](auto d, auto o) -> int {
        return ch.poly_eval_points((const E*)d[0], nf, (const E*)d[1], m, (E*)o[0], count, (hipStream_t)stream) ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}

// ecfft_poly_interpolate: synchronous (the chain reads back the device flag of a zero weight denominator, i.e. two equal points,
// reported as ECFFT_ERR_BAD_ARG)
template <class F>
int run_poly_interpolate(ecfft_ctx* c, DeviceChain<F>& ch, const void* points, size_t m, const void* values, void* out, size_t count,
                         int mem, void* stream) {
    using E = typename F::elem;
    if (!points || !values || !out) return ECFFT_ERR_BAD_ARG;
    if (m > SIZE_MAX / (64 * sizeof(E))) return ECFFT_ERR_BAD_ARG;
    const size_t P = DeviceChain<F>::eval_group(m);
    if (P > DeviceChain<F>::kEvalLeaf && P > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;    // m <= 64: no transform, any tree
    if (P > SIZE_MAX / (8 * 64 * sizeof(E))) return ECFFT_ERR_BAD_ARG;     // node data: 4 P elements per level, < 64 levels
    if (count > SIZE_MAX / (16 * P * sizeof(E))) return ECFFT_ERR_BAD_ARG; // byte counts of the temporaries must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{points, m * sizeof(E)}, {values, m * eb}}, {{out, m * eb}}, [&](auto d, auto o) -> int {
        bool repeated = false;
        if (!ch.poly_interpolate((const E*)d[0], m, (const E*)d[1], (E*)o[0], count, &repeated, (hipStream_t)stream)) return ECFFT_ERR_HIP;
        return repeated ? ECFFT_ERR_BAD_ARG : ECFFT_OK;                     // two equal points: no interpolant
    });
}

// ecfft_poly_pow_mod / ecfft_poly_mul_mod: synchronous (the chain reads back the device flag of a zero leading coefficient of the
// modulus, reported as ECFFT_ERR_BAD_ARG)
template <class F>
int run_poly_pow_mod(ecfft_ctx* c, DeviceChain<F>& ch, const void* a, size_t na, const void* exp, size_t exp_bytes, const void* modulus,
                     size_t nm, void* out, size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!a || !modulus || !out || (!exp && exp_bytes)) return ECFFT_ERR_BAD_ARG;
    const size_t lim = SIZE_MAX / (64 * sizeof(E));
    if (na > lim || nm > lim) return ECFFT_ERR_BAD_ARG;
    const size_t d = nm - 1;
    const size_t N = DeviceChain<F>::powmod_leaves(nm);                      // 1 for d <= kPowSmall: no transform for the power itself
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t Nd = DeviceChain<F>::divrem_leaves(na, nm);
    if (Nd > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    size_t per = N > Nd ? N : Nd;
    if (per < na + nm) per = na + nm;
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG; // byte counts of the temporaries must not wrap
    const uint8_t* e = (const uint8_t*)exp;                                  // high zero bytes do not count
    while (exp_bytes && e[exp_bytes - 1] == 0) --exp_bytes;
    size_t nbits = 0;
    if (exp_bytes) {
        if (exp_bytes > UINT32_MAX / 8) return ECFFT_ERR_BAD_ARG;
        nbits = 8 * exp_bytes;
        while (!((e[(nbits - 1) >> 3] >> ((nbits - 1) & 7)) & 1)) --nbits;
    }
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{a, na * eb}, {modulus, nm * eb}}, {{out, d * eb}}, [&](auto dv, auto o) -> int {
        bool singular = false;
        if (!ch.poly_pow_mod((const E*)dv[0], na, e, nbits, (const E*)dv[1], nm, (E*)o[0], count, &singular, (hipStream_t)stream)) return ECFFT_ERR_HIP;
        return singular ? ECFFT_ERR_BAD_ARG : ECFFT_OK;                      // a zero leading coefficient of the modulus in some pair
    });
}

template <class F>
int run_poly_mul_mod(ecfft_ctx* c, DeviceChain<F>& ch, const void* a, size_t na, const void* b, size_t nb, const void* modulus, size_t nm,
                     void* out, size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!a || !b || !modulus || !out) return ECFFT_ERR_BAD_ARG;
    const size_t lim = SIZE_MAX / (64 * sizeof(E));
    if (na > lim || nb > lim || nm > lim) return ECFFT_ERR_BAD_ARG;
    const size_t nc = na + nb - 1, d = nm - 1, N = DeviceChain<F>::mul_leaves(na, nb);
    if (N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t Nd = DeviceChain<F>::divrem_leaves(nc, nm);
    if (Nd > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    size_t per = N > Nd ? N : Nd;
    if (per < nc + nm) per = nc + nm;
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG; // byte counts of the temporaries must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{a, na * eb}, {b, nb * eb}, {modulus, nm * eb}}, {{out, d * eb}}, [&](auto dv, auto o) -> int {
        bool singular = false;
        if (!ch.poly_mul_mod((const E*)dv[0], na, (const E*)dv[1], nb, (const E*)dv[2], nm, (E*)o[0], count, &singular, (hipStream_t)stream))
            return ECFFT_ERR_HIP;
        return singular ? ECFFT_ERR_BAD_ARG : ECFFT_OK;
    });
}

// ecfft_poly_compose_mod: synchronous like ecfft_poly_pow_mod, whose tree rule it shares (independent of nf)
template <class F>
int run_poly_compose_mod(ecfft_ctx* c, DeviceChain<F>& ch, const void* f, size_t nf, const void* g, size_t ng, const void* modulus, size_t nm,
                         void* out, size_t count, int mem, void* stream) {
    using E = typename F::elem;
    const size_t lim = SIZE_MAX / (64 * sizeof(E));
    if (nf > lim || ng > lim || nm > lim) return ECFFT_ERR_BAD_ARG;
    static_assert(DeviceChain<F>::kComposeSmall + 1 == ECFFT_COMPOSE_SMALL_MAX, "the header states the small regime's bound");
    const size_t d = nm - 1;
    const size_t N = DeviceChain<F>::powmod_leaves(nm);                      // 1 for d <= kComposeSmall: Horner in one workgroup
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t Nd = DeviceChain<F>::divrem_leaves(ng, nm);
    if (Nd > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t k = DeviceChain<F>::compose_chunk(nf), kp = (nf + k - 1) / k;
    size_t per = N > Nd ? N : Nd;
    if (per < ng + nm) per = ng + nm;
    if (per < nf) per = nf;
    if (N > 1) {                                                             // the baby-step table and the chunk sums
        if (k + 1 + kp > SIZE_MAX / (16 * sizeof(E)) / d) return ECFFT_ERR_BAD_ARG;
        if (per < (k + 1 + kp) * d) per = (k + 1 + kp) * d;
    }
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG; // byte counts of the temporaries must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{f, nf * eb}, {g, ng * eb}, {modulus, nm * eb}}, {{out, d * eb}}, [&](auto dv, auto o) -> int {
        bool singular = false;
        if (!ch.poly_compose_mod((const E*)dv[0], nf, (const E*)dv[1], ng, (const E*)dv[2], nm, (E*)o[0], count, &singular, (hipStream_t)stream))
            return ECFFT_ERR_HIP;
        return singular ? ECFFT_ERR_BAD_ARG : ECFFT_OK;                      // a zero leading coefficient of the modulus in some triple
    });
}

// ecfft_poly_gcd / ecfft_poly_xgcd: synchronous (the half-GCD reads degrees back at every node, and `degrees` is a host array
// whatever `mem` is).  Nothing fails on the data.
template <class F>
int run_poly_gcd(ecfft_ctx* c, DeviceChain<F>& ch, const void* a, size_t na, const void* b, size_t nb, void* so, void* to, void* g,
                 int64_t* degrees, size_t count, bool want_cof, int mem, void* stream) {
    using E = typename F::elem;
    if (!a || !b || !g) return ECFFT_ERR_BAD_ARG;
    const size_t lim = SIZE_MAX / (64 * sizeof(E));
    if (na > lim || nb > lim) return ECFFT_ERR_BAD_ARG;
    const size_t ng = na > nb ? na : nb, ns = nb > 1 ? nb - 1 : 1, nt = na > 1 ? na - 1 : 1;
    const size_t N = DeviceChain<F>::gcd_leaves(ng);
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t per = N > 4 * ng ? N : 4 * ng;
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG;  // byte counts of the rows and temporaries must not wrap
    static_assert(sizeof(long long) == sizeof(int64_t), "degrees are read back as long long");
    static_assert(DeviceChain<F>::kGcdSmall == ECFFT_GCD_SMALL_MAX, "the header states the small regime's bound");
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{a, na * eb}, {b, nb * eb}}, {{so, ns * eb}, {to, nt * eb}, {g, ng * eb}}, [&](auto d, auto o) -> int {
        return ch.poly_gcd((const E*)d[0], na, (const E*)d[1], nb, (E*)o[0], (E*)o[1], (E*)o[2], (long long*)degrees, count, want_cof, (hipStream_t)stream)
                   ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}

// ecfft_poly_xgcd_partial: ecfft_poly_xgcd's checks and tree rule; three degrees per pair
template <class F>
int run_poly_xgcd_partial(ecfft_ctx* c, DeviceChain<F>& ch, const void* a, size_t na, const void* b, size_t nb, size_t stop, void* r, void* so,
                          void* to, int64_t* degrees, size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!a || !b || !r || !to) return ECFFT_ERR_BAD_ARG;
    const size_t lim = SIZE_MAX / (64 * sizeof(E));
    if (na > lim || nb > lim) return ECFFT_ERR_BAD_ARG;
    const size_t ng = na > nb ? na : nb;
    const size_t N = DeviceChain<F>::gcd_leaves(ng);
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t per = N > 4 * ng ? N : 4 * ng;
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG;  // byte counts of the rows and temporaries must not wrap
    static_assert(DeviceChain<F>::kGcdSmall == ECFFT_XGCD_PARTIAL_SMALL_MAX, "the header states the small regime's bound");
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{a, na * eb}, {b, nb * eb}}, {{r, ng * eb}, {so, nb * eb}, {to, na * eb}}, [&](auto d, auto o) -> int {
        return ch.poly_xgcd_partial((const E*)d[0], na, (const E*)d[1], nb, stop, (E*)o[0], (E*)o[1], (E*)o[2], (long long*)degrees, count,
                                    (hipStream_t)stream) ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}

// What the three Reed-Solomon calls check alike, after their own pointers: the first failing code or ECFFT_OK.  N: the call's
// tree rule (rs_leaves, rs_encode_leaves), which covers its interpolations, evaluations and the partial xgcd of (m + 1, m).
template <class F>
int rs_call_checks(const DeviceChain<F>& ch, size_t m, size_t k, size_t N, size_t count) {
    using E = typename F::elem;
    if (k > m || m > SIZE_MAX / (64 * sizeof(E)) / 4) return ECFFT_ERR_BAD_ARG;
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t per = N > 4 * (m + 1) ? N : 4 * (m + 1);
    if (N > SIZE_MAX / (8 * 64 * sizeof(E))) return ECFFT_ERR_BAD_ARG;       // node data of the interpolations
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG;  // byte counts of the rows and temporaries must not wrap
    return ECFFT_OK;
}

// ecfft_rs_decode: synchronous (the verdicts are returned to the host, and two equal points raise a device flag, reported as
// ECFFT_ERR_BAD_ARG)
template <class F>
int run_rs_decode(ecfft_ctx* c, DeviceChain<F>& ch, const void* points, size_t m, const void* values, size_t k, void* message,
                  int64_t* n_errors, size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!points || !values || !message || !n_errors) return ECFFT_ERR_BAD_ARG;
    static_assert(DeviceChain<F>::kRsSmall == ECFFT_RS_SMALL_MAX, "the header states the small regime's bound");
    static_assert(sizeof(long long) == sizeof(int64_t), "verdicts are read back as long long");
    if (const int rc = rs_call_checks(ch, m, k, DeviceChain<F>::rs_leaves(m), count)) return rc;
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{points, m * sizeof(E)}, {values, m * eb}}, {{message, k * eb}}, [&](auto d, auto o) -> int {
        bool repeated = false;
        if (!ch.rs_decode((const E*)d[0], m, (const E*)d[1], k, (E*)o[0], (long long*)n_errors, count, &repeated, (hipStream_t)stream))
            return ECFFT_ERR_HIP;
        return repeated ? ECFFT_ERR_BAD_ARG : ECFFT_OK;                      // two equal points: no code
    });
}

// ecfft_rs_encode: synchronous like ecfft_rs_decode (two equal points among all m are reported as ECFFT_ERR_BAD_ARG)
template <class F>
int run_rs_encode(ecfft_ctx* c, DeviceChain<F>& ch, const void* points, size_t m, const void* data, size_t k, void* codeword, size_t count,
                  int mem, void* stream) {
    using E = typename F::elem;
    if (!points || !data || !codeword) return ECFFT_ERR_BAD_ARG;
    if (const int rc = rs_call_checks(ch, m, k, DeviceChain<F>::rs_encode_leaves(m, k), count)) return rc;
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{points, m * sizeof(E)}, {data, k * eb}}, {{codeword, m * eb}}, [&](auto d, auto o) -> int {
        bool repeated = false;
        if (!ch.rs_encode((const E*)d[0], m, (const E*)d[1], k, (E*)o[0], count, &repeated, (hipStream_t)stream)) return ECFFT_ERR_HIP;
        return repeated ? ECFFT_ERR_BAD_ARG : ECFFT_OK;
    });
}

// ecfft_rs_decode_erasures: ecfft_rs_decode's checks and tree rule; the mask travels with the values
template <class F>
int run_rs_decode_erasures(ecfft_ctx* c, DeviceChain<F>& ch, const void* points, size_t m, const void* values, const uint8_t* erased, size_t k,
                           void* out, int out_form, int64_t* n_errors, size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!points || !values || !out || !n_errors) return ECFFT_ERR_BAD_ARG;
    if (out_form != ECFFT_RS_OUT_COEFFS && out_form != ECFFT_RS_OUT_CODEWORD) return ECFFT_ERR_BAD_ARG;
    if (const int rc = rs_call_checks(ch, m, k, DeviceChain<F>::rs_leaves(m), count)) return rc;
    const size_t eb = count * sizeof(E), no = out_form == ECFFT_RS_OUT_CODEWORD ? m : k;
    return staged(c, ch, mem, stream, {{points, m * sizeof(E)}, {values, m * eb}, {erased, erased ? m * count : 0}}, {{out, no * eb}},
                  [&](auto d, auto o) -> int {
        bool repeated = false;
        if (!ch.rs_decode_erasures((const E*)d[0], m, (const E*)d[1], (const uint8_t*)d[2], k, (E*)o[0], out_form == ECFFT_RS_OUT_CODEWORD,
                                   (long long*)n_errors, count, &repeated, (hipStream_t)stream))
            return ECFFT_ERR_HIP;
        return repeated ? ECFFT_ERR_BAD_ARG : ECFFT_OK;                      // two equal points, erased or not: no code
    });
}

// ecfft_seq_min_poly: synchronous (the verdicts are returned to the host).  Nothing fails on the data.
template <class F>
int run_seq_min_poly(ecfft_ctx* c, DeviceChain<F>& ch, const void* seq, size_t n, void* min_poly, int64_t* orders, size_t count, int mem,
                     void* stream) {
    using E = typename F::elem;
    if (!seq || !min_poly || !orders) return ECFFT_ERR_BAD_ARG;
    static_assert(DeviceChain<F>::kSeqSmall == ECFFT_SEQ_SMALL_MAX, "the header states the small regime's bound");
    static_assert(sizeof(long long) == sizeof(int64_t), "orders are read back as long long");
    if (n > SIZE_MAX / (64 * sizeof(E)) / 4) return ECFFT_ERR_BAD_ARG;
    const size_t N = DeviceChain<F>::seq_leaves(n);
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    if (!seq_min_poly_fits(n, count, N, sizeof(E))) return ECFFT_ERR_BAD_ARG;    // byte counts of the rows and temporaries must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{seq, n * eb}}, {{min_poly, (n / 2 + 1) * eb}}, [&](auto d, auto o) -> int {
        return ch.seq_min_poly((const E*)d[0], n, (E*)o[0], (long long*)orders, count, (hipStream_t)stream) ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}

// ecfft_seq_nth_term: synchronous like ecfft_poly_pow_mod, whose tree rule and device check of the leading coefficient it shares
template <class F>
int run_seq_nth_term(ecfft_ctx* c, DeviceChain<F>& ch, const void* char_poly, size_t nc, const void* init, const void* index,
                     size_t index_bytes, void* out, size_t nout, size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!char_poly || !init || !out || (!index && index_bytes)) return ECFFT_ERR_BAD_ARG;
    static_assert(DeviceChain<F>::kSeqTermSmall + 1 == ECFFT_SEQ_TERM_SMALL_MAX, "the header states the small regime's bound");
    if (nc > SIZE_MAX / (64 * sizeof(E))) return ECFFT_ERR_BAD_ARG;
    const size_t N = DeviceChain<F>::powmod_leaves(nc), L = nc - 1;            // 1 for L <= kSeqTermSmall
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    if (!seq_nth_term_fits(nc, nout, count, N, sizeof(E))) return ECFFT_ERR_BAD_ARG;
    size_t nbits = 0;
    if (!seq_index_bits((const uint8_t*)index, index_bytes, &nbits)) return ECFFT_ERR_BAD_ARG;
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{char_poly, nc * eb}, {init, L * eb}}, {{out, nout * eb}}, [&](auto dv, auto o) -> int {
        bool singular = false;
        if (!ch.seq_nth_term((const E*)dv[0], nc, (const E*)dv[1], (const uint8_t*)index, nbits, (E*)o[0], nout, count, &singular,
                             (hipStream_t)stream))
            return ECFFT_ERR_HIP;
        return singular ? ECFFT_ERR_BAD_ARG : ECFFT_OK;                          // a zero leading coefficient of some C_b
    });
}

// ecfft_poly_find_roots: synchronous (degrees are read back between the rounds, and `n_roots` is a host array whatever `mem` is).
// Nothing fails on the data; ECFFT_ERR_HIP also reports a factor that exhausted the attempt cap.
template <class F>
int run_poly_find_roots(ecfft_ctx* c, DeviceChain<F>& ch, const void* f, size_t nf, void* roots, int64_t* n_roots, size_t count, int mem,
                        void* stream) {
    using E = typename F::elem;
    if (!f || !n_roots || (!roots && nf > 1)) return ECFFT_ERR_BAD_ARG;
    if (nf > SIZE_MAX / (64 * sizeof(E))) return ECFFT_ERR_BAD_ARG;
    static_assert(DeviceChain<F>::kRootsSmall + 1 == ECFFT_ROOTS_SMALL_MAX, "the header states the small regime's bound");
    static_assert(sizeof(long long) == sizeof(int64_t), "root counts are read back as long long");
    const size_t N = DeviceChain<F>::roots_leaves(nf);                        // checked on the row length, before anything runs
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t per = N > 4 * nf ? N : 4 * nf;
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG;  // byte counts of the rows and temporaries must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{f, nf * eb}}, {{nf > 1 ? roots : nullptr, (nf - 1) * eb}}, [&](auto d, auto o) -> int {
        bool capped = false;
        if (!ch.poly_find_roots((const E*)d[0], nf, (E*)o[0], (long long*)n_roots, count, &capped, (hipStream_t)stream)) return ECFFT_ERR_HIP;
        return capped ? ECFFT_ERR_HIP : ECFFT_OK;
    });
}

// ecfft_poly_squarefree / ecfft_poly_distinct_degree: synchronous (degrees are read back between the steps, and `degrees` is a
// host array whatever `mem` is).  Nothing fails on the data.  Both share the tree rule of ecfft_poly_find_roots.
template <class F>
int ddf_check(DeviceChain<F>& ch, size_t nf, size_t count) {
    using E = typename F::elem;
    // square_free_factors (src/utils.rs:46-50) divides by gcd(f, f') and is right only while f' = 0 means "constant": the degree must
    // stay below p.  No tree holds more than 2^kMaxLogN coefficients and both fields have p > 2^kMaxLogN, so there is no p-th-power case.
    static_assert(kMaxLogN<F> < (sizeof(E) == 4 ? 31 : 255), "p exceeds the degree of every polynomial a tree holds");
    static_assert(DeviceChain<F>::kDdfSmall + 1 == ECFFT_DDF_SMALL_MAX, "the header states the small regime's bound");
    static_assert(sizeof(long long) == sizeof(int64_t), "degrees are read back as long long");
    if (nf > SIZE_MAX / (64 * sizeof(E))) return ECFFT_ERR_BAD_ARG;
    const size_t N = DeviceChain<F>::ddf_leaves(nf);                          // checked on the row length, before anything runs
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t per = N > 4 * nf ? N : 4 * nf;
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG;  // byte counts of the rows and temporaries must not wrap
    return ECFFT_OK;
}
template <class F>
int run_poly_squarefree(ecfft_ctx* c, DeviceChain<F>& ch, const void* f, size_t nf, void* out, int64_t* degrees, size_t count, int mem,
                        void* stream) {
    using E = typename F::elem;
    if (!f || !out || !degrees) return ECFFT_ERR_BAD_ARG;
    if (const int rc = ddf_check(ch, nf, count); rc != ECFFT_OK) return rc;
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{f, nf * eb}}, {{out, nf * eb}}, [&](auto d, auto o) -> int {
        return ch.poly_squarefree((const E*)d[0], nf, (E*)o[0], (long long*)degrees, count, (hipStream_t)stream) ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}
template <class F>
int run_poly_distinct_degree(ecfft_ctx* c, DeviceChain<F>& ch, const void* f, size_t nf, void* factors, int64_t* degrees, size_t count,
                             int mem, void* stream) {
    using E = typename F::elem;
    if (!f || !factors || !degrees) return ECFFT_ERR_BAD_ARG;
    if (const int rc = ddf_check(ch, nf, count); rc != ECFFT_OK) return rc;
    const size_t eb = count * sizeof(E), nd = nf > 1 ? nf - 1 : 1;
    return staged(c, ch, mem, stream, {{f, nf * eb}}, {{factors, nd * eb}}, [&](auto d, auto o) -> int {
        return ch.poly_distinct_degree((const E*)d[0], nf, (E*)o[0], (long long*)degrees, count, (hipStream_t)stream) ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}

// ecfft_poly_equal_degree: synchronous (degrees are read back between the rounds, and `n_factors` is a host array whatever `mem`
// is).  Nothing fails on the data; ECFFT_ERR_HIP also reports a factor that exhausted the attempt cap.
template <class F>
int run_poly_equal_degree(ecfft_ctx* c, DeviceChain<F>& ch, const void* g, size_t ng, size_t d, void* factors, int64_t* n_factors,
                          size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!g || !factors || !n_factors) return ECFFT_ERR_BAD_ARG;
    if (ng > SIZE_MAX / (64 * sizeof(E))) return ECFFT_ERR_BAD_ARG;
    static_assert(DeviceChain<F>::kEdfSmall + 1 == ECFFT_EDF_SMALL_MAX, "the header states the small regime's bound");
    static_assert(sizeof(long long) == sizeof(int64_t), "factor counts are read back as long long");
    const size_t N = DeviceChain<F>::edf_leaves(ng);                          // checked on the row length, before anything runs
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    size_t per = N > 4 * ng ? N : 4 * ng;
    const size_t dm = d < ng ? d : ng;                                        // a d above every degree the row can hold divides none: ng stands for it
    if (dm > SIZE_MAX / (64 * sizeof(E)) / ng) return ECFFT_ERR_BAD_ARG;
    if (per < dm * ng) per = dm * ng;
    if (count > SIZE_MAX / (16 * per * sizeof(E))) return ECFFT_ERR_BAD_ARG;  // byte counts of the rows and temporaries must not wrap
    const size_t eb = count * sizeof(E), nd = ng > 1 ? ng - 1 : 1;
    return staged(c, ch, mem, stream, {{g, ng * eb}}, {{factors, nd * eb}}, [&](auto dv, auto o) -> int {
        bool capped = false;
        if (!ch.poly_equal_degree((const E*)dv[0], ng, dm, (E*)o[0], (long long*)n_factors, count, &capped, (hipStream_t)stream)) return ECFFT_ERR_HIP;
        return capped ? ECFFT_ERR_HIP : ECFFT_OK;
    });
}

// ecfft_poly_squarefree_decompose / ecfft_poly_factor: synchronous (degrees are read back between the steps, and the int64 arrays are
// host arrays whatever `mem` is).  Both share ddf_check: the tree rule of ecfft_poly_find_roots and the byte counts.  Nothing fails
// on the data; ECFFT_ERR_HIP also reports a factor that exhausted the attempt cap.
template <class F>
int run_poly_squarefree_decompose(ecfft_ctx* c, DeviceChain<F>& ch, const void* f, size_t nf, void* parts, int64_t* degrees, void* lead,
                                  size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!f || !parts || !degrees) return ECFFT_ERR_BAD_ARG;
    static_assert(DeviceChain<F>::kFactorSmall + 1 == ECFFT_FACTOR_SMALL_MAX, "the header states the small regime's bound");
    if (const int rc = ddf_check(ch, nf, count); rc != ECFFT_OK) return rc;
    const size_t eb = count * sizeof(E), nd = nf > 1 ? nf - 1 : 1;
    return staged(c, ch, mem, stream, {{f, nf * eb}}, {{parts, nd * eb}, {lead, eb}}, [&](auto d, auto o) -> int {
        return ch.poly_squarefree_decompose((const E*)d[0], nf, (E*)o[0], (long long*)degrees, (E*)o[1], count, (hipStream_t)stream) ? ECFFT_OK
                                                                                                                                      : ECFFT_ERR_HIP;
    });
}
template <class F>
int run_poly_factor(ecfft_ctx* c, DeviceChain<F>& ch, const void* f, size_t nf, void* factors, int64_t* fdeg, int64_t* fmult, int64_t* n_factors,
                    void* lead, size_t count, int mem, void* stream) {
    using E = typename F::elem;
    if (!f || !factors || !fdeg || !fmult || !n_factors) return ECFFT_ERR_BAD_ARG;
    if (const int rc = ddf_check(ch, nf, count); rc != ECFFT_OK) return rc;
    const size_t eb = count * sizeof(E), nd = nf > 1 ? nf - 1 : 1;
    return staged(c, ch, mem, stream, {{f, nf * eb}}, {{factors, nd * eb}, {lead, eb}}, [&](auto d, auto o) -> int {
        bool capped = false;
        if (!ch.poly_factor((const E*)d[0], nf, (E*)o[0], (long long*)fdeg, (long long*)fmult, (long long*)n_factors, (E*)o[1], count, &capped,
                            (hipStream_t)stream))
            return ECFFT_ERR_HIP;
        return capped ? ECFFT_ERR_HIP : ECFFT_OK;
    });
}

// ecfft_division_polynomial: inputs of one element per curve and an output of L(n) elements per curve; asynchronous like ecfft_poly_mul
template <class F>
int run_division_polynomial(ecfft_ctx* c, DeviceChain<F>& ch, const void* A, const void* B, size_t n, void* out, size_t count, int mem,
                            void* stream) {
    using E = typename F::elem;
    if (!A || !B || !out) return ECFFT_ERR_BAD_ARG;
    static_assert(DeviceChain<F>::kDivpolyMaxN == ECFFT_SCHOOF_MAX_L, "the header states the largest index");
    if (n > ECFFT_SCHOOF_MAX_L) return ECFFT_ERR_BAD_ARG;
    const size_t N = DeviceChain<F>::divpoly_leaves(n), len = DeviceChain<F>::divpoly_len(n);
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;              // checked before anything runs
    if (count > SIZE_MAX / (64 * (N > 32 ? N : 32) * sizeof(E))) return ECFFT_ERR_BAD_ARG;   // byte counts of the temporaries must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{A, eb}, {B, eb}}, {{out, len * eb}}, [&](auto d, auto o) -> int {
        return ch.division_polynomial((const E*)d[0], (const E*)d[1], n, (E*)o[0], count, (hipStream_t)stream) ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}

// ecfft_curve_trace_mod: synchronous (`t_out` is a host array whatever `mem` is).  Nothing fails on the data; ECFFT_ERR_HIP also
// reports a sum the group law excludes.
template <class F>
int run_curve_trace_mod(ecfft_ctx* c, DeviceChain<F>& ch, const void* A, const void* B, size_t l, int64_t* t_out, size_t count, int mem,
                        void* stream) {
    using E = typename F::elem;
    if (!A || !B || !t_out) return ECFFT_ERR_BAD_ARG;
    static_assert(DeviceChain<F>::kSchoofSmall + 1 == ECFFT_SCHOOF_SMALL_MAX, "the header states the small regime's bound");
    static_assert(DeviceChain<F>::kSchoofMaxL == ECFFT_SCHOOF_MAX_L, "the header states the largest l");
    static_assert(sizeof(long long) == sizeof(int64_t), "residues are read back as long long");
    if (l > ECFFT_SCHOOF_MAX_L || !DeviceChain<F>::schoof_valid_l((uint32_t)l)) return ECFFT_ERR_BAD_ARG;
    const size_t N = DeviceChain<F>::schoof_leaves((uint32_t)l);
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;              // checked before anything runs
    if (count > SIZE_MAX / (16 * sizeof(E))) return ECFFT_ERR_BAD_ARG;        // byte counts must not wrap
    const size_t eb = count * sizeof(E);
    return staged(c, ch, mem, stream, {{A, eb}, {B, eb}}, {{nullptr, 0}}, [&](auto dv, auto) -> int {
        bool defect = false;
        if (!ch.curve_trace_mod((const E*)dv[0], (const E*)dv[1], (uint32_t)l, (long long*)t_out, count, &defect, (hipStream_t)stream)) return ECFFT_ERR_HIP;
        return defect ? ECFFT_ERR_HIP : ECFFT_OK;
    });
}

// Unsigned integers of 384 bits for the CRT of ecfft_curve_cardinality (the modulus stays below 2^140, its square below 2^280)
struct U384 { uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; };
inline void u_mul_small(U384& a, uint32_t m) { uint64_t c = 0; for (int i = 0; i < 12; ++i) { c += (uint64_t)a.w[i] * m; a.w[i] = (uint32_t)c; c >>= 32; } }
inline uint32_t u_mod_small(const U384& a, uint32_t m) { uint64_t r = 0; for (int i = 11; i >= 0; --i) r = ((r << 32) | a.w[i]) % m; return (uint32_t)r; }
inline void u_add(U384& a, const U384& b) { uint64_t c = 0; for (int i = 0; i < 12; ++i) { c += (uint64_t)a.w[i] + b.w[i]; a.w[i] = (uint32_t)c; c >>= 32; } }
inline void u_sub(U384& a, const U384& b) { int64_t c = 0; for (int i = 0; i < 12; ++i) { c += (int64_t)a.w[i] - b.w[i]; a.w[i] = (uint32_t)c; c >>= 32; } }   // a >= b
inline int u_cmp(const U384& a, const U384& b) { for (int i = 11; i >= 0; --i) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1; return 0; }
inline U384 u_mul(const U384& a, const U384& b) {
    U384 r;
    for (int i = 0; i < 12; ++i) { uint64_t c = 0; for (int j = 0; i + j < 12; ++j) { c += (uint64_t)a.w[i] * b.w[j] + r.w[i + j]; r.w[i + j] = (uint32_t)c; c >>= 32; } }
    return r;
}
// the field's p
template <class F>
U384 field_modulus() {
    uint8_t ep[32];
    DeviceChain<F>::modulus_bytes(ep);
    U384 p;
    for (int i = 0; i < 32; ++i) p.w[i / 4] |= (uint32_t)ep[i] << (8 * (i % 4));
    return p;
}
// l = 2, 3, 5, ... until the product exceeds 4 sqrt(p), i.e. its square exceeds 16 p (schoofs.rs:32-37)
template <class F>
std::vector<uint32_t> schoof_primes() {
    U384 p16 = field_modulus<F>(), m;
    u_mul_small(p16, 16);
    m.w[0] = 1;
    std::vector<uint32_t> out;
    for (uint32_t l = 2; u_cmp(u_mul(m, m), p16) <= 0 && l <= ECFFT_SCHOOF_MAX_L; ++l)
        if (DeviceChain<F>::schoof_valid_l(l)) { out.push_back(l); u_mul_small(m, l); }
    return out;
}
// ecfft_curve_cardinality: the residues of ecfft_curve_trace_mod for every prime of the rule, then the incremental CRT of
// schoofs.rs:52-70 on the host with the representative in (-m/2, m/2].  Synchronous.
template <class F>
int run_curve_cardinality(ecfft_ctx* c, DeviceChain<F>& ch, const void* A, const void* B, void* order, int64_t* traces, size_t count, int mem,
                          void* stream) {
    using E = typename F::elem;
    if (!A || !B || !order) return ECFFT_ERR_BAD_ARG;
    if (count > SIZE_MAX / (64 * sizeof(E))) return ECFFT_ERR_BAD_ARG;        // byte counts must not wrap
    const std::vector<uint32_t> primes = schoof_primes<F>();
    const size_t np = primes.size();
    const size_t N = DeviceChain<F>::schoof_leaves(primes.back());            // the rule of the largest l covers the others
    if (N > 1 && N > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    const size_t eb = count * sizeof(E);
    std::vector<long long> tr(np * count);
    const int rc = staged(c, ch, mem, stream, {{A, eb}, {B, eb}}, {{nullptr, 0}}, [&](auto dv, auto) -> int {
        for (size_t i = 0; i < np; ++i) {
            bool defect = false;
            if (!ch.curve_trace_mod((const E*)dv[0], (const E*)dv[1], primes[i], tr.data() + i * count, count, &defect, (hipStream_t)stream)) return ECFFT_ERR_HIP;
            if (defect) return ECFFT_ERR_HIP;
        }
        return ECFFT_OK;
    });
    if (rc != ECFFT_OK) return rc;
    const U384 p = field_modulus<F>();
    uint8_t* ob = (uint8_t*)order;
    for (size_t b = 0; b < count; ++b) {
        U384 t, m, n = p, one;
        m.w[0] = 1; one.w[0] = 1;
        bool singular = false;
        for (size_t i = 0; i < np; ++i) {
            const long long r = tr[i * count + b];
            if (traces) traces[b * np + i] = r;
            if (r < 0) { singular = true; continue; }
            const uint32_t l = primes[i], tm = u_mod_small(t, l), mm = u_mod_small(m, l);
            uint32_t inv = 1;
            while ((uint64_t)inv * mm % l != 1) ++inv;
            const uint32_t k = (uint32_t)((uint64_t)(((uint32_t)r + l - tm) % l) * inv % l);
            U384 step = m;
            u_mul_small(step, k);
            u_add(t, step);
            u_mul_small(m, l);
        }
        U384 twice = t;
        u_add(twice, t);
        u_add(n, one);
        if (u_cmp(twice, m) > 0) { U384 neg = m; u_sub(neg, t); u_add(n, neg); }      // t - m < 0: #E = p + 1 + (m - t)
        else u_sub(n, t);
        if (singular) n = U384();
        for (int i = 0; i < ECFFT_ORDER_BYTES; ++i) ob[b * ECFFT_ORDER_BYTES + i] = (uint8_t)(n.w[i / 4] >> (8 * (i % 4)));
    }
    return ECFFT_OK;
}

// standard = true: plain standard-form residues (the FFTree wire format) instead of the crate's in-memory representation
template <class F>
int table_of(DeviceChain<F>& ch, size_t m, int which, void* host_out, size_t cap, size_t* count, bool standard = false) {
    using E = typename F::elem;
    if (!is_pow2(m)) return ECFFT_ERR_NOT_POW2;
    if (m > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    unsigned l = ilog2(m);
    const typename DeviceChain<F>::Tree& T = ch.tree(l);
    const E* src = nullptr; size_t cnt = 0;
    switch (which) {
        case ECFFT_TBL_XNN_S: src = T.xnn; cnt = m; break;
        case ECFFT_TBL_XNN_S_INV: src = T.xnn_inv; cnt = m; break;
        case ECFFT_TBL_Z0_S1: src = T.z0_s1; cnt = m / 2; break;
        case ECFFT_TBL_Z1_S0: src = T.z1_s0; cnt = m / 2; break;
        case ECFFT_TBL_Z0_INV_S1: src = T.z0_inv_s1; cnt = m / 2; break;
        case ECFFT_TBL_Z1_INV_S0: src = T.z1_inv_s0; cnt = m / 2; break;
        case ECFFT_TBL_Z0Z0_REM_XNN_S: src = T.z0z0; cnt = m < 2 ? 0 : m; break;   // empty for the 1-leaf tree (src/fftree.rs:459)
        case ECFFT_TBL_Z1Z1_REM_XNN_S: src = T.z1z1; cnt = m < 2 ? 0 : m; break;
        case ECFFT_TBL_F: cnt = 2 * m; break;
        case ECFFT_TBL_RECOMBINE: case ECFFT_TBL_DECOMPOSE: cnt = 4 * m; break;
        default: return ECFFT_ERR_BAD_ARG;
    }
    if (count) *count = cnt;
    if (!host_out) return ECFFT_OK;
    if (cap < cnt) return ECFFT_ERR_BAD_ARG;
    E* o = (E*)host_out;
    if (which == ECFFT_TBL_RECOMBINE || which == ECFFT_TBL_DECOMPOSE || which == ECFFT_TBL_F) {
        // the matrices, and f of T_m: every (N/m)-th element of each layer of the top tree (src/fftree.rs:471-478), gathered on the
        // device — only the entries asked for cross the bus
        std::lock_guard<std::mutex> guard(ch.lock());
        DeviceBuffer d(cnt * sizeof(E));
        if (!d.ok) return ECFFT_ERR_HIP;
        const bool ok = which == ECFFT_TBL_F ? ch.gather_f(l, d.as<E>(), nullptr)
                                             : ch.export_matrices(l, which == ECFFT_TBL_DECOMPOSE, d.as<E>(), nullptr, standard);
        if (!ok || hipMemcpy(o, d.p, cnt * sizeof(E), hipMemcpyDeviceToHost) != hipSuccess) return ECFFT_ERR_HIP;
        if (which != ECFFT_TBL_F) return ECFFT_OK;      // the matrices are already in the crate representation
    } else if (cnt) {
        if (!src) return ECFFT_ERR_BAD_ARG;
        if (hipMemcpy(o, src, cnt * sizeof(E), hipMemcpyDeviceToHost) != hipSuccess) return ECFFT_ERR_HIP;
    }
    if (!standard) to_crate_host<F>(o, cnt);
    return ECFFT_OK;
}

template <class F>
int run_shard(ecfft_ctx* c, DeviceChain<F>& ch, void* buf, size_t e, int moiety, unsigned log_p, unsigned rank, int which, int mem, void* stream) {
    using E = typename F::elem;
    if (!buf) return ECFFT_ERR_BAD_ARG;
    if (!is_pow2(e)) return ECFFT_ERR_NOT_POW2;
    if (2 * e > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    if (moiety != ECFFT_S0 && moiety != ECFFT_S1) return ECFFT_ERR_BAD_ARG;
    if (((size_t)2 << log_p) > e || rank >= (1u << log_p)) return ECFFT_ERR_BAD_ARG;   // need >= 2 elements per rank
    const size_t bytes = (e >> log_p) * sizeof(E);
    return staged(c, ch, mem, stream, {{buf, bytes}}, {{buf, bytes, /*in_place=*/true}}, [&](auto, auto o) -> int {
        E* d = (E*)o[0];
        hipStream_t s = (hipStream_t)stream;
        if (which == 2) ch.extend_local_block(d, e, moiety, log_p, s);
        else ch.extend_top_cyclic(d, e, moiety, log_p, rank, which == 1, s);
        return hipGetLastError() != hipSuccess ? ECFFT_ERR_HIP : ECFFT_OK;
    });
}

}  // namespace

// ---- remaining algorithms: up to 3 inputs and 1 output
enum Alg { ALG_MEXTEND, ALG_REDC, ALG_MOD, ALG_VANISH, ALG_DEGREE };
template <class F>
int run_alg(ecfft_ctx* c, DeviceChain<F>& ch, Alg alg, const void* in0, const void* in1, const void* in2, void* out, size_t len,
            size_t count, int moiety, int mem, void* stream, size_t* degree) {
    using E = typename F::elem;
    if (!in0 || (alg != ALG_DEGREE && !out)) return ECFFT_ERR_BAD_ARG;
    if ((alg == ALG_REDC || alg == ALG_MOD) && !in1) return ECFFT_ERR_BAD_ARG;
    if (alg == ALG_MOD && !in2) return ECFFT_ERR_BAD_ARG;
    if (alg == ALG_DEGREE && !degree) return ECFFT_ERR_BAD_ARG;
    if (!is_pow2(len)) return ECFFT_ERR_NOT_POW2;
    if (count == 0) return ECFFT_ERR_BAD_ARG;
    size_t need = (alg == ALG_MEXTEND || alg == ALG_VANISH) ? 2 * len : len;
    if (need > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    if ((alg == ALG_MEXTEND || alg == ALG_REDC) && moiety != ECFFT_S0 && moiety != ECFFT_S1) return ECFFT_ERR_BAD_ARG;
    if ((alg == ALG_REDC || alg == ALG_MOD) && len < 2) {   // size-1 tree has no moieties: the reference would index out of bounds
        return ECFFT_ERR_BAD_ARG;
    }
    const size_t n_in = len * count, n_out = (alg == ALG_VANISH ? 2 * len : len) * count;
    return staged(c, ch, mem, stream, {{in0, n_in * sizeof(E)}, {in1, len * sizeof(E)}, {in2, len * sizeof(E)}},
                  {{alg != ALG_DEGREE ? out : nullptr, n_out * sizeof(E)}}, [&](auto d, auto o) -> int {
        const E *d0 = (const E*)d[0], *d1 = (const E*)d[1], *d2 = (const E*)d[2]; E* dout = (E*)o[0];
        hipStream_t s = (hipStream_t)stream;
        bool ok = true;
        switch (alg) {
            case ALG_MEXTEND: ok = ch.api_mextend(d0, dout, len, count, moiety, s); break;
            case ALG_REDC: ok = ch.api_redc(d0, d1, dout, len, moiety, s); break;
            case ALG_MOD: ok = ch.api_modular_reduce(d0, d1, d2, dout, len, s); break;
            case ALG_VANISH: ok = ch.api_vanish(d0, dout, len, s); break;
            case ALG_DEGREE: ok = ch.api_degree(d0, len, s, degree); break;
        }
        return ok ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}

namespace {
template <class F>
int run_table_fma(ecfft_ctx* c, DeviceChain<F>& ch, void* out, const void* x, const void* y, size_t cnt, size_t m, int which, size_t t_off,
                  size_t t_stride, int mode, int mem, void* stream) {
    using E = typename F::elem;
    if (!out || !x) return ECFFT_ERR_BAD_ARG;
    if (!is_pow2(m)) return ECFFT_ERR_NOT_POW2;
    if (m > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    if (cnt == 0) return ECFFT_OK;
    const size_t bytes = cnt * sizeof(E);
    return staged(c, ch, mem, stream, {{x, bytes}, {y, bytes}}, {{out, bytes}}, [&](auto d, auto o) -> int {
        return ch.table_fma((E*)o[0], (const E*)d[0], (const E*)d[1], cnt, ilog2(m), which, t_off, t_stride, mode, (hipStream_t)stream)
                   ? ECFFT_OK : ECFFT_ERR_BAD_ARG;
    });
}

#ifdef ECFFT_TEST_HOOKS
// the matrix-core selftests: the matrix (tn elements) and x uploaded, then launch(matrix, x, its expanded form of `ab` bytes,
// a scratch of `scratch` bytes) on the null stream, then x downloaded into out
template <class Launch>
int run_blk_selftest(const void* matrix, size_t tn, const void* x, void* out, size_t n, size_t ab, size_t scratch, int device, Launch&& launch) {
    if (!have_device(device)) return ECFFT_ERR_HIP;
    DeviceGuard dev(device);
    if (!dev.ok) return ECFFT_ERR_HIP;
    DeviceBuffer dT(tn * sizeof(Fe256)), dx(n * sizeof(Fe256)), dA(ab), dS(scratch);
    bool ok = dT.ok && dx.ok && dA.ok && dS.ok;
    ok = ok && hipMemcpy(dT.p, matrix, tn * sizeof(Fe256), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dx.p, x, n * sizeof(Fe256), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch(dT.as<Fe256>(), dx.as<Fe256>(), dA.as<uint8_t>(), dS.as<Fe256>());
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dx.p, n * sizeof(Fe256), hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? ECFFT_OK : ECFFT_ERR_HIP;
}
#endif  // ECFFT_TEST_HOOKS
}  // namespace

#ifdef ECFFT_TEST_HOOKS
template <class F>
int run_selftest(int op, const void* a, const void* b, const void* c, void* out, size_t n, int device) {
    using E = typename F::elem;
    if (!a || !b || !out || ((op == 0 || op == 4) && !c) || op < 0 || op > 6) return ECFFT_ERR_BAD_ARG;
    if (!have_device(device)) return ECFFT_ERR_HIP;
    DeviceGuard dev(device);
    if (!dev.ok) return ECFFT_ERR_HIP;
    const size_t bytes = n * sizeof(E);
    DeviceBuffer da(bytes), db(bytes), dc(bytes), dout(bytes);
    bool ok = da.ok && db.ok && dc.ok && dout.ok;
    ok = ok && hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && c) ok = hipMemcpy(dc.p, c, bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        const E *pa = da.as<E>(), *pb = db.as<E>(), *pc = dc.as<E>(); E* po = dout.as<E>();
        foreach_n(nullptr, n, [=] __device__(size_t i) {
            E r;
            if (op == 0) r = F::mul_add(pa[i], pb[i], pc[i]);
            else if (op == 1) r = F::mul(pa[i], pb[i]);
            else if (op == 2) r = F::sub(pa[i], pb[i]);
            else if (op == 3) r = F::add(pa[i], pb[i]);
            else if (op == 4) r = F::tmul_add(F::to_table(pa[i]), pb[i], pc[i]);
            else if (op == 5) r = F::tmul(F::to_table(pa[i]), pb[i]);
            else r = F::half(pa[i]);
            po[i] = r;
        });
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? ECFFT_OK : ECFFT_ERR_HIP;
}

#endif  // ECFFT_TEST_HOOKS
// dependent chain x <- T*x + c per lane: the table multiply of the butterfly kernels with nothing else around it
template <class F>
__global__ __launch_bounds__(256) void k_mul_chain(const typename F::elem* t, typename F::elem* x, int iters) {
    size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    typename F::telem tv = F::to_table(t[g]);
    typename F::elem xv = x[g], cv = t[g];
#pragma unroll 1
    for (int i = 0; i < iters; ++i) xv = F::tmul_add(tv, xv, cv);
    x[g] = F::canon(xv);
}

// the same chain with shader-clock (s_memtime) and constant 100 MHz (wall_clock64) stamps around it: effective shader clock
// of the chip while every SIMD runs the kernels' multiply — what DVFS really grants under this instruction mix
struct ClockStamp { unsigned long long cyc, wall; };
template <class F>
__global__ __launch_bounds__(256) void k_clock_probe(const typename F::elem* t, typename F::elem* x, ClockStamp* st, int iters) {
    size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    typename F::telem tv = F::to_table(t[g]);
    typename F::elem xv = x[g], cv = t[g];
    unsigned long long c0 = __builtin_amdgcn_s_memtime(), w0 = wall_clock64();
#pragma unroll 1
    for (int i = 0; i < iters; ++i) xv = F::tmul_add(tv, xv, cv);
    unsigned long long c1 = __builtin_amdgcn_s_memtime(), w1 = wall_clock64();
    x[g] = F::canon(xv);
    if (threadIdx.x == 0) { st[blockIdx.x].cyc = c1 - c0; st[blockIdx.x].wall = w1 - w0; }
}
template <class F>
int run_shader_clock(int device, double* mhz) {
    using E = typename F::elem;
    if (!mhz) return ECFFT_ERR_BAD_ARG;
    if (!have_device(device)) return ECFFT_ERR_HIP;
    DeviceGuard dev(device);
    hipDeviceProp_t p;
    if (!dev.ok || hipGetDeviceProperties(&p, device) != hipSuccess) return ECFFT_ERR_HIP;
    const int blocks = p.multiProcessorCount * 4, iters = sizeof(E) == 32 ? 2048 : 65536;    // a few ms at 4 waves per SIMD
    const size_t n = (size_t)blocks * 256;
    std::vector<E> h(n);
    memset(h.data(), 0x35, n * sizeof(E));
    std::vector<ClockStamp> hs(blocks);
    DeviceBuffer dt(n * sizeof(E)), dx(n * sizeof(E)), ds(blocks * sizeof(ClockStamp));
    bool ok = dt.ok && dx.ok && ds.ok &&
              hipMemcpy(dt.p, h.data(), n * sizeof(E), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dx.p, h.data(), n * sizeof(E), hipMemcpyHostToDevice) == hipSuccess;
    for (int r = 0; ok && r < 2; ++r) {
        hipLaunchKernelGGL(k_clock_probe<F>, dim3(blocks), dim3(256), 0, nullptr, dt.as<const E>(), dx.as<E>(), ds.as<ClockStamp>(), iters);
        ok = hipDeviceSynchronize() == hipSuccess;
    }
    ok = ok && hipMemcpy(hs.data(), ds.p, blocks * sizeof(ClockStamp), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return ECFFT_ERR_HIP;
    double cyc = 0, wall = 0;
    for (const ClockStamp& c : hs) { cyc += (double)c.cyc; wall += (double)c.wall; }
    *mhz = wall > 0 ? cyc / wall * 100.0 : 0.0;
    return ECFFT_OK;
}

template <class F>
int run_mul_ceiling(int device, int waves_per_simd, double* mul_per_s) {
    using E = typename F::elem;
    if (!mul_per_s || waves_per_simd < 1 || waves_per_simd > 8) return ECFFT_ERR_BAD_ARG;
    hipDeviceProp_t p;
    if (!have_device(device)) return ECFFT_ERR_HIP;
    DeviceGuard dev(device);
    if (!dev.ok || hipGetDeviceProperties(&p, device) != hipSuccess) return ECFFT_ERR_HIP;
    const int blocks = p.multiProcessorCount * waves_per_simd, iters = sizeof(E) == 32 ? 512 : 8192;   // one 256-thread block = one wave per SIMD
    const size_t n = (size_t)blocks * 256;
    std::vector<E> h(n);
    uint64_t sd = 88172645463325252ull;
    for (size_t i = 0; i < n; ++i) {
        unsigned char* b = reinterpret_cast<unsigned char*>(&h[i]);
        for (size_t k = 0; k < sizeof(E); ++k) { sd ^= sd << 13; sd ^= sd >> 7; sd ^= sd << 17; b[k] = (unsigned char)(sd >> 24); }
        b[sizeof(E) - 1] &= 0x3F;                                                    // < p for both fields
    }
    DeviceBuffer dt(n * sizeof(E)), dx(n * sizeof(E));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok = dt.ok && dx.ok &&
              hipMemcpy(dt.p, h.data(), n * sizeof(E), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dx.p, h.data(), n * sizeof(E), hipMemcpyHostToDevice) == hipSuccess &&
              hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    float best = 1e30f;
    for (int r = 0; ok && r < 4; ++r) {
        ok = hipEventRecord(e0, nullptr) == hipSuccess;
        hipLaunchKernelGGL(k_mul_chain<F>, dim3(blocks), dim3(256), 0, nullptr, dt.as<const E>(), dx.as<E>(), iters);
        ok = ok && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
        float ms = 0; ok = ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        if (ok && r > 0 && ms < best) best = ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (!ok) return ECFFT_ERR_HIP;
    *mul_per_s = (double)n * iters / (best * 1e-3);
    return ECFFT_OK;
}

namespace {
template <class F>
int run_sharded(ecfft_ctx* c, DeviceChain<F>& ch, ecfft_comm* comm, Op op, const void* in, void* out, size_t len, int moiety, void* stream,
                int in_layout = ECFFT_LAYOUT_BLOCK, int out_layout = ECFFT_LAYOUT_BLOCK) {
    using E = typename F::elem;
    if (!in || !out || !comm || !comm->t) return ECFFT_ERR_BAD_ARG;
    if (!is_pow2(len)) return ECFFT_ERR_NOT_POW2;
    Transport& tr = *comm->t;
    const size_t P = (size_t)tr.world;
    if (!is_pow2(P) || P > 64) return ECFFT_ERR_BAD_ARG;
    size_t need_tree = (op == OP_EXTEND) ? len * 2 : len;
    if (need_tree > ch.size()) return ECFFT_ERR_TREE_TOO_SMALL;
    if (op == OP_EXTEND && moiety != ECFFT_S0 && moiety != ECFFT_S1) return ECFFT_ERR_BAD_ARG;
    if (len / P < 2 * P) return ECFFT_ERR_BAD_ARG;                       // every rank needs at least 2P elements
    if (ch.shard_mode()) {                                               // a shard context serves exactly the split it was built for
        const bool fits = P == ((size_t)1 << ch.shard_log_p()) && (unsigned)tr.rank == ch.shard_rank() &&
                          ((ch.shard_kind() == DeviceChain<F>::kShardExtend && op == OP_EXTEND && 2 * len == ch.size()) ||
                           (ch.shard_kind() == DeviceChain<F>::kShardEnter && op == OP_ENTER && len == ch.size()) ||
                           (ch.shard_kind() == DeviceChain<F>::kShardExit && op == OP_EXIT && len == ch.size()));
        if (!fits) return ECFFT_ERR_BAD_ARG;
    }
    if ((in_layout != ECFFT_LAYOUT_BLOCK && in_layout != ECFFT_LAYOUT_CYCLIC) || (out_layout != ECFFT_LAYOUT_BLOCK && out_layout != ECFFT_LAYOUT_CYCLIC)) return ECFFT_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    CallScope scope(c, ch.lock(), s);
    if (!scope.ok) return ECFFT_ERR_HIP;
    bool ok = false;
    switch (op) {
        case OP_EXTEND: ok = ch.api_extend_split(tr, (const E*)in, (E*)out, len, moiety, s, in_layout == ECFFT_LAYOUT_CYCLIC, out_layout == ECFFT_LAYOUT_CYCLIC); break;
        case OP_ENTER: ok = ch.api_enter_split(tr, (const E*)in, (E*)out, len, s); break;
        case OP_EXIT: ok = ch.api_exit_split(tr, (const E*)in, (E*)out, len, s); break;
    }
    return ok && hipGetLastError() == hipSuccess ? ECFFT_OK : ECFFT_ERR_HIP;
}
}  // namespace

// ---- FFTree wire format (ark-serialize 0.4 conventions; hand-written impls at /root/reference/src/fftree.rs:510-660) ----------
// Vec<T> = u64 little-endian length + elements; a field element = its STANDARD-form integer, little endian (32 / 4 bytes);
// [T; N] = elements only; bool = one byte; DensePolynomial = coefficient Vec with trailing zeros trimmed.  Field order of one
// tree (:528-548): f, recombine_matrices, decompose_matrices, rational_maps, xnn_s, z0_s1, z1_s0, [xnn_s_inv, z0_inv_s1,
// z1_inv_s0 with Compress::No only], z0z0_rem_xnn_s, z1z1_rem_xnn_s, bool has_subtree, then the subtree.
// The device tables are plain residues, so every table goes to the file as it lies in HBM.
namespace {
template <class F>
size_t trimmed_len(const typename F::elem* c3) {
    size_t k = 3;
    while (k > 0 && F::is_zero(c3[k - 1])) --k;
    return k;
}
template <class F>
size_t wire_size(const DeviceChain<F>& ch, int compress) {
    const size_t eb = sizeof(typename F::elem);
    size_t total = 0;
    for (size_t m = ch.size();; m >>= 1) {
        const unsigned lm = ilog2(m); const size_t e = m / 2;
        total += 8 + 2 * m * eb + 2 * (8 + 4 * m * eb) + 8;
        for (unsigned k = 0; k < lm; ++k) total += 16 + (trimmed_len<F>(ch.host().maps[k].num) + trimmed_len<F>(ch.host().maps[k].den)) * eb;
        total += ((8 + m * eb) + 2 * (8 + e * eb)) * (compress ? 1 : 2);
        total += 2 * (8 + (m > 1 ? m : 0) * eb) + 1;
        if (m == 1) break;
    }
    return total;
}
inline void put_u64(uint8_t*& p, uint64_t v) { for (int i = 0; i < 8; ++i) *p++ = (uint8_t)(v >> (8 * i)); }
template <class F>
int wire_write(DeviceChain<F>& ch, int compress, uint8_t* buf) {
    using E = typename F::elem;
    const size_t eb = sizeof(E);
    uint8_t* p = buf;
    auto vec = [&](size_t m, int which, size_t per_entry) -> int {      // Vec of cnt / per_entry entries
        size_t cnt = 0;
        int rc = table_of(ch, m, which, nullptr, 0, &cnt, true);
        if (rc != ECFFT_OK) return rc;
        put_u64(p, cnt / per_entry);
        if (cnt) { rc = table_of(ch, m, which, p, cnt, nullptr, true); if (rc != ECFFT_OK) return rc; }
        p += cnt * eb;
        return ECFFT_OK;
    };
    for (size_t m = ch.size();; m >>= 1) {
        const unsigned lm = ilog2(m);
        int rc;
        if ((rc = vec(m, ECFFT_TBL_F, 1)) || (rc = vec(m, ECFFT_TBL_RECOMBINE, 4)) || (rc = vec(m, ECFFT_TBL_DECOMPOSE, 4))) return rc;
        put_u64(p, lm);                                                   // the subtree keeps the first log2(m) maps (split_last, :480)
        for (unsigned k = 0; k < lm; ++k) {
            const RatMap<F>& mp = ch.host().maps[k];
            const size_t ln = trimmed_len<F>(mp.num), ld = trimmed_len<F>(mp.den);
            put_u64(p, ln); memcpy(p, mp.num, ln * eb); p += ln * eb;
            put_u64(p, ld); memcpy(p, mp.den, ld * eb); p += ld * eb;
        }
        if ((rc = vec(m, ECFFT_TBL_XNN_S, 1)) || (rc = vec(m, ECFFT_TBL_Z0_S1, 1)) || (rc = vec(m, ECFFT_TBL_Z1_S0, 1))) return rc;
        if (!compress && ((rc = vec(m, ECFFT_TBL_XNN_S_INV, 1)) || (rc = vec(m, ECFFT_TBL_Z0_INV_S1, 1)) || (rc = vec(m, ECFFT_TBL_Z1_INV_S0, 1)))) return rc;
        if ((rc = vec(m, ECFFT_TBL_Z0Z0_REM_XNN_S, 1)) || (rc = vec(m, ECFFT_TBL_Z1Z1_REM_XNN_S, 1))) return rc;
        *p++ = m > 1 ? 1 : 0;
        if (m == 1) break;
    }
    return ECFFT_OK;
}

// (the bounds-checked parse itself — cursor, canonicality check, level structure — lives in wire_parse.h: pure host C++ that
// tests/cpp/wire_fuzz.cpp also drives under AddressSanitizer + UBSan without a GPU)
template <class F>
int wire_read(int field, const uint8_t* data, size_t len, int compress, int device, int verify, ecfft_ctx** out) {
    using E = typename F::elem;
    const size_t eb = sizeof(E);
    static_assert(sizeof(E) == 32 || sizeof(E) == 4, "element sizes of the two fields");
    wire::File file;
    { const int prc = wire::parse(field, data, len, compress, file); if (prc != ECFFT_OK) return prc; }
    const std::vector<wire::Level>& levels = file.levels;
    typedef wire::Level WireLevel;
    HostTree<F> ht;
    for (const wire::Map& m : file.maps) {
        RatMap<F> mp;
        for (int i = 0; i < 3; ++i) { memcpy(&mp.num[i], m.num[i], eb); memcpy(&mp.den[i], m.den[i], eb); }
        ht.maps.push_back(mp);
    }
    // FFTree::new on the file's leaves and maps: every other table is recomputed on the GPU (the reference USES the file's
    // tables; with verify != 0 each of them is compared with the recomputed one, so a file whose tables disagree with its own
    // point set is rejected instead of being silently repaired).  Compress::Yes files carry no inverse tables (:620-628).
    const size_t n = levels[0].n;
    ht.n = n; ht.f.assign(2 * n, F::zero());
    memcpy(ht.f.data() + n, levels[0].tbl[ECFFT_TBL_F] + n * eb, n * eb);
    ht.leaves_only = true;
    return new_ctx<F>(field, device, out, [&](DeviceChain<F>& ch) -> int {
        int rc = build_chain(ch, std::move(ht), device);
        if (rc != ECFFT_OK) return rc;
        // verify == 0 still checks the internal layers of every `f` (they follow from the leaves and the maps: cheap, and a file
        // whose layers disagree with its maps would otherwise load as a different tree than the reference's deserialize builds)
        std::vector<E> got;
        for (const WireLevel& lv : levels)
            for (int which = 0; which < 11; ++which) {
                if (!verify && which != ECFFT_TBL_F) continue;
                if (!lv.tbl[which] && lv.cnt[which] == 0) continue;
                got.resize(lv.cnt[which] ? lv.cnt[which] : 1);
                rc = table_of(ch, lv.n, which, got.data(), lv.cnt[which], nullptr, true);
                if (rc != ECFFT_OK) return rc;
                const size_t skip = which == ECFFT_TBL_F ? 1 : 0;           // heap index 0 is unused (src/utils.rs:228-252)
                if (verify && which == ECFFT_TBL_F && lv.cnt[which] > 0) {  // ... and zero in every tree the crate builds (src/fftree.rs:50, 471): a verified
                    bool zero0 = true;                                      // file is byte for byte what serialize writes (tests: mutated files)
                    for (size_t b = 0; b < eb; ++b) zero0 = zero0 && lv.tbl[which][b] == 0;
                    if (!zero0) { fprintf(stderr, "ecfft: entry 0 of f of the %zu-leaf subtree in the file is not zero\n", lv.n); return ECFFT_ERR_BAD_ARG; }
                }
                if (lv.cnt[which] > skip && memcmp((const uint8_t*)got.data() + skip * eb, lv.tbl[which] + skip * eb, (lv.cnt[which] - skip) * eb) != 0) {
                    fprintf(stderr, "ecfft: table %d of the %zu-leaf subtree in the file differs from the one rebuilt from its point set\n", which, lv.n);
                    return ECFFT_ERR_BAD_ARG;
                }
            }
        return ECFFT_OK;
    });
}
}  // namespace

extern "C" {

size_t ecfft_elem_size(int field) { return field == ECFFT_FIELD_SECP256K1 ? 32 : (field == ECFFT_FIELD_M31 ? 4 : 0); }

int ecfft_build_fftree(int field, size_t n, int device, ecfft_ctx** out) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (!is_pow2(n)) return ECFFT_ERR_NOT_POW2;                           // assert!(n.is_power_of_two())
    if (!known_field(field)) return ECFFT_ERR_BAD_ARG;
    return new_tree_ctx(field, ilog2(n), device, out, [&](auto& ch, auto&& ht) -> int { return build_chain(ch, std::move(ht), device); });
}

namespace {
// kind 1: EXTEND-only shard context for e = len evaluations (tree T_2e); kind 2: ENTER-only for n = len coefficients (tree T_n)
int build_shard_ctx(int kind, int field, size_t len, int device, int world, int rank, ecfft_ctx** out, ecfft_comm* comm = nullptr, int flags = 0) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (!is_pow2(len) || !is_pow2((size_t)(world > 0 ? world : 0))) return ECFFT_ERR_NOT_POW2;
    if (!known_field(field)) return ECFFT_ERR_BAD_ARG;
    if (world > 64 || rank < 0 || rank >= world || (kind >= 2 && world < 2)) return ECFFT_ERR_BAD_ARG;
    if (kind == 3 && (!comm || !comm->t)) return ECFFT_ERR_BAD_ARG;
    if (len / (size_t)world < 2 * (size_t)world) return ECFFT_ERR_BAD_ARG;   // same bound as the sharded transforms
    const unsigned log_n = ilog2(len) + (kind == 1 ? 1 : 0), log_p = ilog2((size_t)world);
    return new_tree_ctx(field, log_n, device, out, [&](auto& ch, auto&& ht) -> int {
        const bool ok = kind == 1 ? ch.build_extend_shard(std::move(ht), device, log_p, (unsigned)rank)
                      : kind == 2 ? ch.build_enter_shard(std::move(ht), device, log_p, (unsigned)rank)
                                  : ch.build_exit_shard(std::move(ht), device, *comm->t, (flags & ECFFT_EXIT_SHARD_MIN_MEMORY) != 0);
        return ok ? ECFFT_OK : ECFFT_ERR_HIP;
    });
}
}  // namespace
int ecfft_build_extend_shard(int field, size_t e, int device, int world, int rank, ecfft_ctx** out) { return build_shard_ctx(1, field, e, device, world, rank, out); }
int ecfft_build_enter_shard(int field, size_t n, int device, int world, int rank, ecfft_ctx** out) { return build_shard_ctx(2, field, n, device, world, rank, out); }
int ecfft_build_exit_shard_opts(int field, size_t n, int device, ecfft_comm* comm, int flags, ecfft_ctx** out) {
    if (!comm || !comm->t || (flags & ~ECFFT_EXIT_SHARD_MIN_MEMORY)) { if (out) *out = nullptr; return ECFFT_ERR_BAD_ARG; }
    return build_shard_ctx(3, field, n, device, comm->t->world, comm->t->rank, out, comm, flags);
}
int ecfft_build_exit_shard(int field, size_t n, int device, ecfft_comm* comm, ecfft_ctx** out) {
    return ecfft_build_exit_shard_opts(field, n, device, comm, 0, out);
}

int ecfft_fftree_new(int field, const void* leaves, size_t n, const void* map_num3, const void* map_den3, int device,
                     ecfft_ctx** out) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (!leaves || (n > 1 && (!map_num3 || !map_den3))) return ECFFT_ERR_BAD_ARG;
    if (!is_pow2(n)) return ECFFT_ERR_NOT_POW2;
    if (!known_field(field)) return ECFFT_ERR_BAD_ARG;
    if (!have_device(device)) return ECFFT_ERR_HIP;
    const unsigned log_n = ilog2(n);
    return with_field(field, [&](auto tag) -> int {
        using F = typename decltype(tag)::type;
        using E = typename F::elem;
        HostTree<F> ht; ht.n = n; ht.f.assign(2 * n, F::zero()); ht.maps.resize(log_n);
        memcpy(ht.f.data() + n, leaves, n * sizeof(E));
        from_crate_host<F>(ht.f.data() + n, n);
        for (unsigned k = 0; k < log_n; ++k) {
            RatMap<F>& m = ht.maps[k];
            memcpy(m.num, (const E*)map_num3 + 3 * k, sizeof(m.num)); memcpy(m.den, (const E*)map_den3 + 3 * k, sizeof(m.den));
            from_crate_host<F>(m.num, 3); from_crate_host<F>(m.den, 3);
            if (!F::is_zero(m.den[2])) return ECFFT_ERR_BAD_ARG;           // x-map denominators have degree 1
        }
        ht.leaves_only = true;                                         // the layers psi_k(L_k) are computed on the GPU (points_on_device)
        return new_ctx<F>(field, device, out, [&](DeviceChain<F>& ch) -> int { return build_chain(ch, std::move(ht), device); });
    });
}

int ecfft_build_points(int field, size_t n, void* f_out, void* map_num3_out, void* map_den3_out) {
    if (!f_out) return ECFFT_ERR_BAD_ARG;
    if (!is_pow2(n)) return ECFFT_ERR_NOT_POW2;
    unsigned log_n = ilog2(n);
    return with_field(field, [&](auto tag) -> int {
        using F = typename decltype(tag)::type;
        HostTree<F> ht;
        int r = build_host_tree<F>(log_n, ht);
        if (r) return r == 1 ? ECFFT_ERR_TREE_TOO_LARGE : ECFFT_ERR_BAD_ARG;
        to_crate_host<F>(ht.f.data(), 2 * n);
        memcpy(f_out, ht.f.data(), 2 * n * sizeof(typename F::elem));
        maps_out(ht.maps, map_num3_out, map_den3_out);
        return ECFFT_OK;
    });
}

void ecfft_ctx_destroy(ecfft_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard dev(ctx->device);
    delete ctx;
}

size_t ecfft_tree_size(const ecfft_ctx* ctx) {
    if (!ctx) return 0;
    return with_chain(ctx, [](auto& ch) { return ch.size(); });
}
int ecfft_field(const ecfft_ctx* ctx) { return ctx ? ctx->field : -1; }
#ifdef ECFFT_TEST_HOOKS
long ecfft_selfcheck_pointwise_z(ecfft_ctx* ctx, size_t m) {
    if (!ctx || !is_pow2(m)) return -1;
    return guarded([&] {
        return with_chain(ctx, [&](auto& ch) -> int {
            CallScope scope(ctx, ch.lock(), nullptr);                 // its pooled temporaries may still be in use by the previous asynchronous call
            if (!scope.ok) return -1;
            return (int)ch.selfcheck_pointwise_z(m);
        });
    });
}
int ecfft_test_fail_next_collective(ecfft_ctx* ctx) {
    if (!ctx) return ECFFT_ERR_BAD_ARG;
    with_chain(ctx, [](auto& ch) { ch.test_fail_next_collective(); });
    return ECFFT_OK;
}
int ecfft_test_fail_build_rank(int rank) {
    DeviceChain<Secp256k1>::test_fail_build_rank().store(rank);
    DeviceChain<M31>::test_fail_build_rank().store(rank);
    return ECFFT_OK;
}
#endif  // ECFFT_TEST_HOOKS
int ecfft_ctx_trim(ecfft_ctx* ctx) {
    if (!ctx) return ECFFT_ERR_BAD_ARG;
    DeviceGuard dev(ctx->device);
    if (!dev.ok) return ECFFT_ERR_HIP;
    // the staging buffer is used under the chain lock by every host-memory call: it is freed under that lock too
    auto free_stage = [ctx] { if (ctx->stage) { (void)hipFree(ctx->stage); ctx->stage = nullptr; ctx->stage_bytes = 0; } };
    with_chain(ctx, [&](auto& ch) { ch.trim(free_stage); });
    return ECFFT_OK;
}
size_t ecfft_ctx_device_bytes(const ecfft_ctx* ctx) {
    if (!ctx) return 0;
    return with_chain(ctx, [](auto& ch) { return ch.device_bytes(); });
}

int ecfft_enter(ecfft_ctx* ctx, const void* coeffs, void* evals, size_t n, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_op(ctx, ch, OP_ENTER, coeffs, evals, n, 1, 0, mem, stream); });
}
int ecfft_exit(ecfft_ctx* ctx, const void* evals, void* coeffs, size_t n, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_op(ctx, ch, OP_EXIT, evals, coeffs, n, 1, 0, mem, stream); });
}
int ecfft_enter_many(ecfft_ctx* ctx, const void* coeffs, void* evals, size_t n, size_t count, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_op(ctx, ch, OP_ENTER, coeffs, evals, n, count, 0, mem, stream); });
}
int ecfft_exit_many(ecfft_ctx* ctx, const void* evals, void* coeffs, size_t n, size_t count, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_op(ctx, ch, OP_EXIT, evals, coeffs, n, count, 0, mem, stream); });
}
int ecfft_extend(ecfft_ctx* ctx, const void* in, void* out, size_t e, int moiety, size_t count, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_op(ctx, ch, OP_EXTEND, in, out, e, count, moiety, mem, stream); });
}

int ecfft_poly_mul(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, void* out, size_t count, int mem, void* stream) {
    if (na == 0 || nb == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_mul(ctx, ch, a, na, b, nb, out, count, mem, stream); });
}
int ecfft_poly_inv_series(ecfft_ctx* ctx, const void* f, size_t nf, void* out, size_t k, size_t count, int mem, void* stream) {
    if (nf == 0 || k == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_inv_series(ctx, ch, f, nf, out, k, count, mem, stream); });
}
int ecfft_poly_divrem(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, void* q, void* r, size_t count, int mem, void* stream) {
    if (na == 0 || nb == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_divrem(ctx, ch, a, na, b, nb, q, r, count, mem, stream); });
}
int ecfft_poly_pow_mod(ecfft_ctx* ctx, const void* a, size_t na, const void* exp, size_t exp_bytes, const void* modulus, size_t nm,
                       void* out, size_t count, int mem, void* stream) {
    if (na == 0 || nm < 2 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_pow_mod(ctx, ch, a, na, exp, exp_bytes, modulus, nm, out, count, mem, stream); });
}
int ecfft_poly_mul_mod(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, const void* modulus, size_t nm, void* out,
                       size_t count, int mem, void* stream) {
    if (na == 0 || nb == 0 || nm < 2 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_mul_mod(ctx, ch, a, na, b, nb, modulus, nm, out, count, mem, stream); });
}
int ecfft_poly_compose_mod(ecfft_ctx* ctx, const void* f, size_t nf, const void* g, size_t ng, const void* modulus, size_t nm, void* out,
                           size_t count, int mem, void* stream) {
    if (!f || !g || !modulus || !out || nf == 0 || ng == 0 || nm < 2 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_compose_mod(ctx, ch, f, nf, g, ng, modulus, nm, out, count, mem, stream); });
}
int ecfft_poly_gcd(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, void* g, int64_t* degrees, size_t count, int mem,
                   void* stream) {
    if (na == 0 || nb == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_gcd(ctx, ch, a, na, b, nb, nullptr, nullptr, g, degrees, count, false, mem, stream); });
}
int ecfft_poly_xgcd(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, void* s, void* t, void* g, int64_t* degrees,
                    size_t count, int mem, void* stream) {
    if (na == 0 || nb == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_gcd(ctx, ch, a, na, b, nb, s, t, g, degrees, count, true, mem, stream); });
}
int ecfft_poly_xgcd_partial(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, size_t stop, void* r, void* s, void* t,
                            int64_t* degrees, size_t count, int mem, void* stream) {
    if (na == 0 || nb == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_xgcd_partial(ctx, ch, a, na, b, nb, stop, r, s, t, degrees, count, mem, stream); });
}
int ecfft_rs_decode(ecfft_ctx* ctx, const void* points, size_t m, const void* values, size_t k, void* message, int64_t* n_errors,
                    size_t count, int mem, void* stream) {
    if (m == 0 || k == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_rs_decode(ctx, ch, points, m, values, k, message, n_errors, count, mem, stream); });
}
int ecfft_rs_encode(ecfft_ctx* ctx, const void* points, size_t m, const void* data, size_t k, void* codeword, size_t count, int mem,
                    void* stream) {
    if (m == 0 || k == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_rs_encode(ctx, ch, points, m, data, k, codeword, count, mem, stream); });
}
int ecfft_rs_decode_erasures(ecfft_ctx* ctx, const void* points, size_t m, const void* values, const uint8_t* erased, size_t k, void* out,
                             int out_form, int64_t* n_errors, size_t count, int mem, void* stream) {
    if (m == 0 || k == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) {
        return run_rs_decode_erasures(ctx, ch, points, m, values, erased, k, out, out_form, n_errors, count, mem, stream);
    });
}
int ecfft_seq_min_poly(ecfft_ctx* ctx, const void* seq, size_t n_terms, void* min_poly, int64_t* orders, size_t count, int mem,
                       void* stream) {
    if (n_terms == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_seq_min_poly(ctx, ch, seq, n_terms, min_poly, orders, count, mem, stream); });
}
int ecfft_seq_nth_term(ecfft_ctx* ctx, const void* char_poly, size_t nc, const void* init, const void* index, size_t index_bytes,
                       void* out, size_t nout, size_t count, int mem, void* stream) {
    if (nc < 2 || nout == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) {
        return run_seq_nth_term(ctx, ch, char_poly, nc, init, index, index_bytes, out, nout, count, mem, stream);
    });
}
int ecfft_poly_find_roots(ecfft_ctx* ctx, const void* f, size_t nf, void* roots, int64_t* n_roots, size_t count, int mem, void* stream) {
    if (nf == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_find_roots(ctx, ch, f, nf, roots, n_roots, count, mem, stream); });
}
int ecfft_poly_squarefree(ecfft_ctx* ctx, const void* f, size_t nf, void* out, int64_t* degrees, size_t count, int mem, void* stream) {
    if (nf == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_squarefree(ctx, ch, f, nf, out, degrees, count, mem, stream); });
}
int ecfft_poly_distinct_degree(ecfft_ctx* ctx, const void* f, size_t nf, void* factors, int64_t* degrees, size_t count, int mem, void* stream) {
    if (nf == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_distinct_degree(ctx, ch, f, nf, factors, degrees, count, mem, stream); });
}
int ecfft_poly_equal_degree(ecfft_ctx* ctx, const void* g, size_t ng, size_t d, void* factors, int64_t* n_factors, size_t count, int mem,
                            void* stream) {
    if (ng == 0 || d == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_equal_degree(ctx, ch, g, ng, d, factors, n_factors, count, mem, stream); });
}
int ecfft_poly_squarefree_decompose(ecfft_ctx* ctx, const void* f, size_t nf, void* parts, int64_t* degrees, void* lead, size_t count, int mem,
                                    void* stream) {
    if (nf == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_squarefree_decompose(ctx, ch, f, nf, parts, degrees, lead, count, mem, stream); });
}
int ecfft_poly_factor(ecfft_ctx* ctx, const void* f, size_t nf, void* factors, int64_t* fdeg, int64_t* fmult, int64_t* n_factors, void* lead,
                      size_t count, int mem, void* stream) {
    if (nf == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_factor(ctx, ch, f, nf, factors, fdeg, fmult, n_factors, lead, count, mem, stream); });
}
int ecfft_division_polynomial(ecfft_ctx* ctx, const void* A, const void* B, size_t n, void* out, size_t count, int mem, void* stream) {
    if (count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_division_polynomial(ctx, ch, A, B, n, out, count, mem, stream); });
}
int ecfft_curve_trace_mod(ecfft_ctx* ctx, const void* A, const void* B, size_t l, int64_t* t_out, size_t count, int mem, void* stream) {
    if (count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_curve_trace_mod(ctx, ch, A, B, l, t_out, count, mem, stream); });
}
int ecfft_curve_cardinality(ecfft_ctx* ctx, const void* A, const void* B, void* order, int64_t* traces, size_t count, int mem, void* stream) {
    if (count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_curve_cardinality(ctx, ch, A, B, order, traces, count, mem, stream); });
}
#ifdef ECFFT_TEST_HOOKS
int ecfft_test_ddf_iterate(int mode) {
    if (mode < 0 || mode > 2) return ECFFT_ERR_BAD_ARG;
    DeviceChain<Secp256k1>::ddf_iterate_force() = mode;
    DeviceChain<M31>::ddf_iterate_force() = mode;
    return ECFFT_OK;
}
int ecfft_test_schoof_pi2(int mode) {
    if (mode < 0 || mode > 2) return ECFFT_ERR_BAD_ARG;
    DeviceChain<Secp256k1>::schoof_pi2_force() = mode;
    DeviceChain<M31>::schoof_pi2_force() = mode;
    return ECFFT_OK;
}
#endif  // ECFFT_TEST_HOOKS
int ecfft_poly_eval_points(ecfft_ctx* ctx, const void* f, size_t nf, const void* points, size_t m, void* out, size_t count, int mem,
                           void* stream) {
    if (nf == 0 || m == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_eval_points(ctx, ch, f, nf, points, m, out, count, mem, stream); });
}
int ecfft_poly_interpolate(ecfft_ctx* ctx, const void* points, size_t m, const void* values, void* out, size_t count, int mem,
                           void* stream) {
    if (m == 0 || count == 0) return ECFFT_ERR_BAD_ARG;
    return on_chain(ctx, [&](auto& ch) { return run_poly_interpolate(ctx, ch, points, m, values, out, count, mem, stream); });
}

int ecfft_extend_top_cyclic(ecfft_ctx* ctx, void* buf, size_t e, int moiety, unsigned log_p, unsigned rank, int recombine, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_shard(ctx, ch, buf, e, moiety, log_p, rank, recombine ? 1 : 0, mem, stream); });
}
int ecfft_extend_local_block(ecfft_ctx* ctx, void* buf, size_t e, int moiety, unsigned log_p, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_shard(ctx, ch, buf, e, moiety, log_p, 0, 2, mem, stream); });
}

int ecfft_mextend(ecfft_ctx* ctx, const void* in, void* out, size_t e, int moiety, size_t count, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_alg(ctx, ch, ALG_MEXTEND, in, nullptr, nullptr, out, e, count, moiety, mem, stream, nullptr); });
}
int ecfft_redc(ecfft_ctx* ctx, const void* evals, const void* a, void* out, size_t n, int moiety, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_alg(ctx, ch, ALG_REDC, evals, a, nullptr, out, n, 1, moiety, mem, stream, nullptr); });
}
int ecfft_modular_reduce(ecfft_ctx* ctx, const void* evals, const void* a, const void* c, void* out, size_t n, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_alg(ctx, ch, ALG_MOD, evals, a, c, out, n, 1, 0, mem, stream, nullptr); });
}
int ecfft_vanish(ecfft_ctx* ctx, const void* domain, void* out, size_t nd, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_alg(ctx, ch, ALG_VANISH, domain, nullptr, nullptr, out, nd, 1, 0, mem, stream, nullptr); });
}
int ecfft_degree(ecfft_ctx* ctx, const void* evals, size_t n, int mem, void* stream, size_t* degree) {
    return on_chain(ctx, [&](auto& ch) { return run_alg(ctx, ch, ALG_DEGREE, evals, nullptr, nullptr, nullptr, n, 1, 0, mem, stream, degree); });
}

// ---- one transform split over several GPUs -------------------------------------------------------------------------
int ecfft_comm_get_unique_id(void* id_out) {
    if (!id_out) return ECFFT_ERR_BAD_ARG;
    RcclApi& api = RcclApi::get();
    if (!api.ok()) return ECFFT_ERR_HIP;
    RcclApi::UniqueId id;
    if (api.GetUniqueId(&id) != 0) return ECFFT_ERR_HIP;
    memcpy(id_out, id.internal, ECFFT_COMM_ID_BYTES);
    return ECFFT_OK;
}
int ecfft_comm_set_link_striping(ecfft_comm* comm, size_t min_gain_bytes) {
    if (!comm || !comm->t) return ECFFT_ERR_BAD_ARG;
    if (comm->t->used()) return ECFFT_ERR_BAD_ARG;      // frozen once the communicator has carried an exchange: the ranks agree on it in their first vote
    comm->t->stripe_min_gain = min_gain_bytes;
    return ECFFT_OK;
}
int ecfft_comm_set_rccl_library(const char* path) {
    return RcclApi::set_library(path) ? ECFFT_OK : ECFFT_ERR_BAD_ARG;
}
int ecfft_comm_init_rank(const void* id, int world, int rank, int device, ecfft_comm** out) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (!id || world < 1 || rank < 0 || rank >= world) return ECFFT_ERR_BAD_ARG;
    if (!have_device(device)) return ECFFT_ERR_HIP;
    DeviceGuard dev(device);
    if (!dev.ok) return ECFFT_ERR_HIP;
    std::unique_ptr<RcclTransport> t(new (std::nothrow) RcclTransport());
    if (!t || !t->init(id, world, rank, device)) return ECFFT_ERR_HIP;
    ecfft_comm* c = new (std::nothrow) ecfft_comm();
    if (!c) return ECFFT_ERR_HIP;
    c->t = t.release();
    *out = c;
    return ECFFT_OK;
}
int ecfft_comm_init_callback(int world, int rank, int device, ecfft_exchange_fn fn, void* user, ecfft_comm** out) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (!fn || world < 1 || rank < 0 || rank >= world) return ECFFT_ERR_BAD_ARG;
    ecfft_comm* c = new (std::nothrow) ecfft_comm();
    if (!c) return ECFFT_ERR_HIP;
    c->t = new (std::nothrow) CallbackTransport(world, rank, device, fn, user);
    if (!c->t) { delete c; return ECFFT_ERR_HIP; }
    *out = c;
    return ECFFT_OK;
}
#ifdef ECFFT_TEST_HOOKS
int ecfft_comm_init_projection(int world, int rank, int device, double delay_us, double link_gbps, ecfft_comm** out) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world || delay_us < 0 || link_gbps < 0) return ECFFT_ERR_BAD_ARG;
    ecfft_comm* c = new (std::nothrow) ecfft_comm();
    if (!c) return ECFFT_ERR_HIP;
    c->t = new (std::nothrow) ProjectionTransport(world, rank, device, delay_us, link_gbps);
    if (!c->t) { delete c; return ECFFT_ERR_HIP; }
    *out = c;
    return ECFFT_OK;
}
#endif  // ECFFT_TEST_HOOKS
void ecfft_comm_destroy(ecfft_comm* comm) {
    if (!comm) return;
    DeviceGuard dev(comm->t ? comm->t->device : 0);
    delete comm;
}
int ecfft_comm_abort(ecfft_comm* comm) {
    if (!comm || !comm->t) return ECFFT_ERR_BAD_ARG;
    return comm->t->abort() ? ECFFT_OK : ECFFT_ERR_HIP;            // callable from another host thread than the one that is blocked
}
int ecfft_comm_rank(const ecfft_comm* comm) { return comm && comm->t ? comm->t->rank : -1; }
int ecfft_comm_world(const ecfft_comm* comm) { return comm && comm->t ? comm->t->world : 0; }
int ecfft_comm_stats_enable(ecfft_comm* comm, int on) {
    if (!comm || !comm->t) return ECFFT_ERR_BAD_ARG;
    DeviceGuard dev(comm->t->device);
    if (!dev.ok || hipDeviceSynchronize() != hipSuccess) return ECFFT_ERR_HIP;
    comm->t->stats_enable(on != 0);
    return ECFFT_OK;
}
int ecfft_comm_stats_read(ecfft_comm* comm, double* comm_ms, double* exchanges, double* bytes_sent) {
    if (!comm || !comm->t) return ECFFT_ERR_BAD_ARG;
    DeviceGuard dev(comm->t->device);
    if (!dev.ok || hipDeviceSynchronize() != hipSuccess) return ECFFT_ERR_HIP;
    comm->t->stats_read(comm_ms, exchanges, bytes_sent);
    comm->t->stats_reset();
    return ECFFT_OK;
}



int ecfft_extend_sharded(ecfft_ctx* ctx, ecfft_comm* comm, const void* in, void* out, size_t e, int moiety, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_sharded(ctx, ch, comm, OP_EXTEND, in, out, e, moiety, stream); }, true);
}
int ecfft_extend_sharded_layout(ecfft_ctx* ctx, ecfft_comm* comm, const void* in, void* out, size_t e, int moiety, int in_layout, int out_layout, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_sharded(ctx, ch, comm, OP_EXTEND, in, out, e, moiety, stream, in_layout, out_layout); }, true);
}
int ecfft_enter_sharded(ecfft_ctx* ctx, ecfft_comm* comm, const void* coeffs, void* evals, size_t n, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_sharded(ctx, ch, comm, OP_ENTER, coeffs, evals, n, 0, stream); }, true);
}
int ecfft_exit_sharded(ecfft_ctx* ctx, ecfft_comm* comm, const void* evals, void* coeffs, size_t n, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_sharded(ctx, ch, comm, OP_EXIT, evals, coeffs, n, 0, stream); }, true);
}

int ecfft_table_fma(ecfft_ctx* ctx, void* out, const void* x, const void* y, size_t cnt, size_t m, int which, size_t t_off,
                    size_t t_stride, int mode, int mem, void* stream) {
    return on_chain(ctx, [&](auto& ch) { return run_table_fma(ctx, ch, out, x, y, cnt, m, which, t_off, t_stride, mode, mem, stream); });
}

int ecfft_tree_table(ecfft_ctx* ctx, size_t m, int which, void* host_out, size_t cap, size_t* count) {
    if (!ctx || shard_only(ctx)) return ECFFT_ERR_BAD_ARG;
    DeviceGuard dev(ctx->device);
    if (!dev.ok) return ECFFT_ERR_HIP;
    // reads immutable tables only (its device temporaries are its own hipMalloc blocks, not the pool): no ordering against
    // transform calls in flight is needed
    return guarded([&] { return with_chain(ctx, [&](auto& ch) { return table_of(ch, m, which, host_out, cap, count); }); });
}

int ecfft_profile_enable(ecfft_ctx* ctx, int on) {
    if (!ctx) return ECFFT_ERR_BAD_ARG;
    Profiler& p = with_chain(ctx, [](auto& ch) -> Profiler& { return ch.profiler(); });
    DeviceGuard dev(ctx->device);
    if (!dev.ok || hipDeviceSynchronize() != hipSuccess) return ECFFT_ERR_HIP;
    p.reset(); p.on = on != 0;
    return ECFFT_OK;
}
int ecfft_profile_classes(void) { return KC_COUNT; }
int ecfft_profile_read(ecfft_ctx* ctx, int cls, char* name, size_t cap, uint64_t* launches, double* ms_total,
                       double* alg_bytes_total) {
    if (!ctx || cls < 0 || cls >= KC_COUNT) return ECFFT_ERR_BAD_ARG;
    Profiler& p = with_chain(ctx, [](auto& ch) -> Profiler& { return ch.profiler(); });
    DeviceGuard dev(ctx->device);
    if (!dev.ok || hipDeviceSynchronize() != hipSuccess) return ECFFT_ERR_HIP;
    p.collect();
    if (name && cap) snprintf(name, cap, "%s", kKernelClassName[cls]);
    if (launches) *launches = p.launches(cls);
    if (ms_total) *ms_total = p.ms(cls);
    if (alg_bytes_total) *alg_bytes_total = p.bytes(cls);
    return ECFFT_OK;
}

int ecfft_tree_rational_maps(ecfft_ctx* ctx, void* map_num3_out, void* map_den3_out) {
    if (!ctx || shard_only(ctx)) return ECFFT_ERR_BAD_ARG;
    with_chain(ctx, [&](auto& ch) { maps_out(ch.host().maps, map_num3_out, map_den3_out); });
    return ECFFT_OK;
}

int ecfft_fftree_serialize(ecfft_ctx* ctx, int compress, void* buf, size_t cap, size_t* len) {
    if (!ctx || shard_only(ctx)) return ECFFT_ERR_BAD_ARG;
    const size_t need = with_chain(ctx, [&](auto& ch) { return wire_size(ch, compress); });
    if (len) *len = need;
    if (!buf) return ECFFT_OK;
    if (cap < need) return ECFFT_ERR_BAD_ARG;
    DeviceGuard dev(ctx->device);
    if (!dev.ok) return ECFFT_ERR_HIP;
    return guarded([&] { return with_chain(ctx, [&](auto& ch) { return wire_write(ch, compress, (uint8_t*)buf); }); });
}

int ecfft_fftree_deserialize(int field, const void* bytes, size_t len, int compress, int device, int verify, ecfft_ctx** out) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (!bytes) return ECFFT_ERR_BAD_ARG;
    if (!known_field(field)) return ECFFT_ERR_BAD_ARG;
    if (!have_device(device)) return ECFFT_ERR_HIP;
    return guarded([&] {
        return with_field(field, [&](auto tag) {
            return wire_read<typename decltype(tag)::type>(field, (const uint8_t*)bytes, len, compress, device, verify, out);
        });
    });
}

int ecfft_elems_to_standard(int field, const void* in, void* out, size_t n) { return convert_elems(field, in, out, n, true); }
int ecfft_elems_from_standard(int field, const void* in, void* out, size_t n) { return convert_elems(field, in, out, n, false); }

#ifdef ECFFT_TEST_HOOKS
int ecfft_selftest_field(int field, int op, const void* a, const void* b, const void* c, void* out, size_t n, int device) {
    return with_field(field, [&](auto tag) { return run_selftest<typename decltype(tag)::type>(op, a, b, c, out, n, device); });
}

}  // extern "C"
namespace {
// mode 0: k_blk16_apply, 1..4: k_blk16_apply_n16<mode>
int run_blk16_selftest(const void* matrix256, const void* x, void* out, size_t n, int mode, int device) {
    return run_blk_selftest(matrix256, 256, x, out, n, Blk16::kABytes + Blk16::kKWords * 8, 0, device, [&](Fe256* dT, Fe256* dx, uint8_t* dA, Fe256*) {
        unsigned long long* dK = reinterpret_cast<unsigned long long*>(dA + Blk16::kABytes);
        hipLaunchKernelGGL(k_blk16_from_matrix, dim3(1), dim3(256), 0, nullptr, dT, dA, dK, false);
        if (mode == 0) hipLaunchKernelGGL(k_blk16_apply, dim3((unsigned)(n / Blk16::kSub)), dim3(512), 0, nullptr, dx, dA, dK);
        else if (mode == 1) hipLaunchKernelGGL(k_blk16_apply_n16<1>, dim3((unsigned)(n / 256)), dim3(256), 0, nullptr, dx, dA, dK);
        else if (mode == 2) hipLaunchKernelGGL(k_blk16_apply_n16<2>, dim3((unsigned)(n / 256)), dim3(128), 0, nullptr, dx, dA, dK);
        else if (mode == 3) hipLaunchKernelGGL(k_blk16_apply_n16<3>, dim3((unsigned)(n / 128)), dim3(128), 0, nullptr, dx, dA, dK);
        else hipLaunchKernelGGL(k_blk16_apply_n16<4>, dim3((unsigned)(n / 256)), dim3(256), 0, nullptr, dx, dA, dK);
    });
}
}  // namespace
extern "C" {

int ecfft_selftest_blk16(const void* matrix256, const void* x, void* out, size_t n, int device) {
    if (!matrix256 || !x || !out || !n || n % Blk16::kSub) return ECFFT_ERR_BAD_ARG;
    return run_blk16_selftest(matrix256, x, out, n, 0, device);
}
int ecfft_selftest_blk16_small(const void* matrix256, const void* x, void* out, size_t n, int mode, int device) {
    if (!matrix256 || !x || !out || !n || n % 256 || mode < 1 || mode > 4) return ECFFT_ERR_BAD_ARG;
    return run_blk16_selftest(matrix256, x, out, n, mode, device);
}

int ecfft_selftest_blk32(const void* matrix1024, const void* x, void* out, size_t n, int device) {
    if (!matrix1024 || !x || !out || !n || n % 1024) return ECFFT_ERR_BAD_ARG;
    return run_blk_selftest(matrix1024, 1024, x, out, n, Blk16::kABytes32 + Blk16::kKWords32 * 8, 1024 * sizeof(Fe256), device,
                            [&](Fe256* dT, Fe256* dx, uint8_t* dA, Fe256* dcs) {
        unsigned long long* dK = reinterpret_cast<unsigned long long*>(dA + Blk16::kABytes32);
        hipLaunchKernelGGL(k_blk32_expand, dim3(4), dim3(256), 0, nullptr, (const Fe256*)dT, dA, dcs, false);
        hipLaunchKernelGGL(k_blk32_seeds, dim3(1), dim3(32), 0, nullptr, (const Fe256*)dcs, dK);
        hipLaunchKernelGGL(k_blk32_apply, dim3((unsigned)(n / 1024)), dim3(512), 0, nullptr, dx, dA, dK);
    });
}
// which composite map the 1024-element low-level kernels of this context run for the lowest levels of ENTER (dir 0) / EXIT (dir 1):
// 32 (levels 1..5), 16 (levels 1..4) or 0 (level code)
int ecfft_ctx_low_map(const ecfft_ctx* ctx, int dir) {
    if (!ctx || dir < 0 || dir > 1 || ctx->field != ECFFT_FIELD_SECP256K1 || !ctx->secp) return 0;
    return ctx->secp->low_map(dir);
}
int ecfft_ctx_exit_cores(const ecfft_ctx* ctx) {
    if (!ctx) return 0;
    return ctx->secp ? ctx->secp->exit_cores() : ctx->m31 ? ctx->m31->exit_cores() : 0;
}
int ecfft_ctx_exit_low_cores(const ecfft_ctx* ctx) {
    if (!ctx) return 0;
    return ctx->secp ? ctx->secp->exit_low_cores() : ctx->m31 ? ctx->m31->exit_low_cores() : 0;
}
int ecfft_ctx_sym_bfly(const ecfft_ctx* ctx) {
    if (!ctx) return -1;
    return ctx->secp ? ctx->secp->sym_bfly() : ctx->m31 ? ctx->m31->sym_bfly() : -1;
}
int ecfft_ctx_low_sym(const ecfft_ctx* ctx) {
    if (!ctx) return -1;
    return ctx->secp ? ctx->secp->low_sym() : ctx->m31 ? ctx->m31->low_sym() : -1;
}
int ecfft_ctx_enter_l11(const ecfft_ctx* ctx) {
    if (!ctx) return -1;
    return ctx->secp ? ctx->secp->enter_l11() : ctx->m31 ? ctx->m31->enter_l11() : -1;
}

#endif  // ECFFT_TEST_HOOKS
int ecfft_mul_ceiling(int field, int device, int waves_per_simd, double* mul_per_s) {
    return with_field(field, [&](auto tag) { return run_mul_ceiling<typename decltype(tag)::type>(device, waves_per_simd, mul_per_s); });
}

int ecfft_device_alloc(int device, size_t bytes, void** out) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (!have_device(device)) return ECFFT_ERR_HIP;
    DeviceGuard dev(device);
    if (!dev.ok) return ECFFT_ERR_HIP;
    return hipMalloc(out, bytes ? bytes : 1) == hipSuccess ? ECFFT_OK : ECFFT_ERR_HIP;
}
int ecfft_device_free(void* ptr) { return !ptr || hipFree(ptr) == hipSuccess ? ECFFT_OK : ECFFT_ERR_HIP; }
int ecfft_device_sync(int device) {
    DeviceGuard dev(device);
    return dev.ok && hipDeviceSynchronize() == hipSuccess ? ECFFT_OK : ECFFT_ERR_HIP;
}

int ecfft_shader_clock(int field, int device, double* mhz) {
    return with_field(field, [&](auto tag) { return run_shader_clock<typename decltype(tag)::type>(device, mhz); });
}

int ecfft_device_copy(void* dst, const void* src, size_t bytes, int kind) {
    hipMemcpyKind k = kind == 0 ? hipMemcpyDeviceToHost : (kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice);
    if (!dst || !src || kind < 0 || kind > 2) return ECFFT_ERR_BAD_ARG;
    return hipMemcpy(dst, src, bytes, k) == hipSuccess ? ECFFT_OK : ECFFT_ERR_HIP;
}

int ecfft_device_info(int device, char* buf, size_t cap) {
    if (!buf || !cap) return ECFFT_ERR_BAD_ARG;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) { snprintf(buf, cap, "no HIP device"); return ECFFT_ERR_HIP; }
    snprintf(buf, cap, "%s (%s), %d CUs, %.1f GiB", p.name, p.gcnArchName, p.multiProcessorCount, p.totalGlobalMem / 1073741824.0);
    return ECFFT_OK;
}

}  // extern "C"

// ---- curve search: ecfft_find_curve_candidate / ecfft_curve_two_sylow / ecfft_find_curve / ecfft_build_fftree_on_curve ------------------
#include "curve_search.h"
#ifdef ECFFT_TEST_HOOKS
#include <chrono>
#endif

namespace {
using curve::Cand;
using curve::StageArgs;

template <class F>
typename F::elem half_of_one() { return F::inv(F::from_u32(2)); }

// candidates per batch: both queues hold a whole batch (a stage never makes candidates), 2 x 112 MiB / 2 x 384 MiB
template <class F> constexpr unsigned kSearchBatch = std::is_same<F, Secp256k1>::value ? (1u << 20) : (1u << 24);

#ifdef ECFFT_TEST_HOOKS
// entries each stage read, summed over the batches since the last ecfft_curve_search_stats: [0] bb, [1] discriminant, [2] order 4,
// [3 + r] halving round r (measurement only: tools/findcurve_time.py)
uint64_t g_stage_len[3 + 8 * 32 + 2 + 1];
double g_stage_s[3 + 8 * 32 + 2 + 1];        // host seconds around each stage's launch and the read of its queue length (which waits for it)
#endif

// The device side of one search: two queues, the length counters of every stage and the flags.
template <class F>
struct SearchWork {
    unsigned cap;
    DeviceBuffer qa, qb, lens, flags;
    explicit SearchWork(unsigned cap_) : cap(cap_), qa((size_t)cap_ * sizeof(Cand<F>)), qb((size_t)cap_ * sizeof(Cand<F>)),
                                         lens((4 + curve::kMaxRounds<F>) * sizeof(unsigned)), flags(sizeof(unsigned)) {}
    bool ok() const { return qa.ok && qb.ok && lens.ok && flags.ok; }
};

template <class F, int STAGE>
bool launch_stage(StageArgs<F>& g, unsigned* out_len_dev, unsigned* len_host) {
    g.out_len = out_len_dev;
#ifdef ECFFT_TEST_HOOKS
    const size_t slot = STAGE == curve::STAGE_HALVE ? 3 + (g.n_now - 2) : STAGE;
    g_stage_len[slot] += g.in_len;
    const auto t0 = std::chrono::steady_clock::now();
#endif
    hipLaunchKernelGGL((curve::k_stage<F, STAGE>), dim3((g.in_len + 255) / 256), dim3(256), 0, nullptr, g);
    const bool ok = hipMemcpy(len_host, out_len_dev, sizeof(unsigned), hipMemcpyDeviceToHost) == hipSuccess;   // waits for the stage
#ifdef ECFFT_TEST_HOOKS
    g_stage_s[slot] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
#endif
    return ok;
}

// `count` <= w.cap candidates through every stage.  g names the source and where results go (StageArgs); the queue fields are set here.
template <class F>
int run_search_batch(SearchWork<F>& w, StageArgs<F> g, unsigned count) {
    Cand<F>*qa = w.qa.template as<Cand<F>>(), *qb = w.qb.template as<Cand<F>>();
    unsigned* lens = w.lens.template as<unsigned>();
    if (hipMemset(lens, 0, (4 + curve::kMaxRounds<F>) * sizeof(unsigned)) != hipSuccess || hipMemset(w.flags.p, 0, sizeof(unsigned)) != hipSuccess)
        return ECFFT_ERR_HIP;
    g.flags = w.flags.template as<unsigned>(); g.cap = w.cap; g.half = half_of_one<F>();
    unsigned len = 0;
    g.in = nullptr; g.out = qa; g.in_len = count; g.n_now = 0;
    if (!launch_stage<F, curve::STAGE_BB>(g, lens + 0, &len)) return ECFFT_ERR_HIP;
    g.in = qa; g.out = qb; g.in_len = len;
    if (len && !launch_stage<F, curve::STAGE_DISC>(g, lens + 1, &len)) return ECFFT_ERR_HIP;
    g.in = qb; g.out = qa; g.in_len = len; g.n_now = 1;
    if (len && !launch_stage<F, curve::STAGE_ORDER4>(g, lens + 2, &len)) return ECFFT_ERR_HIP;
    bool bound_hit = false;
    for (unsigned r = 0; len; ++r) {                         // halving rounds: a candidate that fails round r has n = 2 + r
        if (r == curve::kMaxRounds<F>) { bound_hit = true; break; }
        g.in = (r & 1) ? qb : qa; g.out = (r & 1) ? qa : qb; g.in_len = len; g.n_now = 2 + r;
        if (!launch_stage<F, curve::STAGE_HALVE>(g, lens + 3 + r, &len)) return ECFFT_ERR_HIP;
    }
    unsigned flags = 0;
    if (hipMemcpy(&flags, w.flags.p, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess) return ECFFT_ERR_HIP;
    if (flags || bound_hit) { fprintf(stderr, "ecfft: curve search: %s\n", bound_hit ? "a candidate survived every halving round" : "a queue overflowed"); return ECFFT_ERR_HIP; }
    return ECFFT_OK;
}

// cyclic_two_sylow_subgroup of `count` curves given in PLAIN form on the host; n and x (plain) back to the host
template <class F>
int two_sylow_device(int device, const typename F::elem* a, const typename F::elem* bb, size_t count, uint32_t* n_out, typename F::elem* x_out) {
    using E = typename F::elem;
    if (!have_device(device)) return ECFFT_ERR_HIP;
    DeviceGuard dev(device);
    if (!dev.ok) return ECFFT_ERR_HIP;
    const unsigned cap = (unsigned)std::min<size_t>(count, kSearchBatch<F>);
    SearchWork<F> w(cap);
    DeviceBuffer da((size_t)cap * sizeof(E)), db((size_t)cap * sizeof(E)), dn((size_t)cap * sizeof(uint32_t)), dx((size_t)cap * sizeof(E));
    if (!w.ok() || !da.ok || !db.ok || !dn.ok || !dx.ok) return ECFFT_ERR_HIP;
    for (size_t at = 0; at < count; at += cap) {
        const unsigned cnt = (unsigned)std::min<size_t>(cap, count - at);
        if (hipMemcpy(da.p, a + at, cnt * sizeof(E), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(db.p, bb + at, cnt * sizeof(E), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(dn.p, 0, cnt * sizeof(uint32_t)) != hipSuccess || hipMemset(dx.p, 0, cnt * sizeof(E)) != hipSuccess) return ECFFT_ERR_HIP;
        StageArgs<F> g{};
        g.a_in = da.template as<const E>(); g.bb_in = db.template as<const E>(); g.base = 0;
        g.n_out = dn.template as<uint32_t>(); g.x_out = dx.template as<E>(); g.best = nullptr;
        const int rc = run_search_batch<F>(w, g, cnt);
        if (rc != ECFFT_OK) return rc;
        if (hipMemcpy(n_out + at, dn.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(x_out + at, dx.p, cnt * sizeof(E), hipMemcpyDeviceToHost) != hipSuccess) return ECFFT_ERR_HIP;
    }
    return ECFFT_OK;
}

// the smallest index in [start, start + max) of stream `seed` whose n >= k_min (UINT64_MAX: none), scanned batch by batch in order;
// the scan ends after the first batch that holds a hit
template <class F>
int scan_stream(int device, uint32_t k_min, uint64_t seed, uint64_t start, uint64_t max, uint64_t* index) {
    *index = UINT64_MAX;
    if (!have_device(device)) return ECFFT_ERR_HIP;
    DeviceGuard dev(device);
    if (!dev.ok) return ECFFT_ERR_HIP;
    const unsigned cap = (unsigned)std::min<uint64_t>(max, kSearchBatch<F>);
    SearchWork<F> w(cap);
    DeviceBuffer best(sizeof(unsigned long long));
    if (!w.ok() || !best.ok || hipMemset(best.p, 0xFF, sizeof(unsigned long long)) != hipSuccess) return ECFFT_ERR_HIP;
    for (uint64_t at = 0; at < max; at += cap) {
        const unsigned cnt = (unsigned)std::min<uint64_t>(cap, max - at);
        StageArgs<F> g{};
        g.seed = seed; g.base = start + at; g.best = best.template as<unsigned long long>(); g.k_min = k_min;
        const int rc = run_search_batch<F>(w, g, cnt);
        if (rc != ECFFT_OK) return rc;
        unsigned long long h = 0;
        if (hipMemcpy(&h, best.p, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return ECFFT_ERR_HIP;
        if (h != ~0ull) { *index = h; break; }
    }
    return ECFFT_OK;
}

template <class F>
bool on_curve(const Curve<F>& c, const Pt<F>& p) { return F::eq(F::sqr(p.y), curve::rhs<F>(p.x, c.a2, c.a4)); }
template <class F>
Pt<F> pt_double_n(const Curve<F>& c, Pt<F> p, unsigned times) { for (unsigned i = 0; i < times; ++i) p = pt_add(c, p, p); return p; }
template <class F>
Pt<F> load_point(const void* xy) {
    Pt<F> p; p.inf = false;
    memcpy(&p.x, xy, sizeof(p.x)); memcpy(&p.y, (const char*)xy + sizeof(p.x), sizeof(p.y));
    from_crate_host<F>(&p.x, 1); from_crate_host<F>(&p.y, 1);
    return p;
}
template <class F>
void store_elems(void* out, const typename F::elem* v, size_t n) {       // plain -> the crate's form, into a caller buffer that may be NULL
    if (!out) return;
    std::vector<typename F::elem> t(v, v + n);
    to_crate_host<F>(t.data(), n);
    memcpy(out, t.data(), n * sizeof(typename F::elem));
}
}  // namespace

extern "C" {

int ecfft_find_curve_candidate(int field, uint64_t seed, uint64_t index, void* a_out, void* bb_out) {
    if (!a_out || !bb_out || index >= curve::kMaxIndex) return ECFFT_ERR_BAD_ARG;
    return with_field(field, [&](auto tag) -> int {
        using F = typename decltype(tag)::type;
        const typename F::elem a = curve::stream_elem<F>(seed, 8 * index), bb = curve::stream_elem<F>(seed, 8 * index + 4);
        store_elems<F>(a_out, &a, 1); store_elems<F>(bb_out, &bb, 1);
        return ECFFT_OK;
    });
}

int ecfft_curve_two_sylow(int field, int device, const void* a, const void* bb, size_t count, uint32_t* n_out, void* x_out) {
    if (!known_field(field) || !a || !bb || !n_out || !x_out || count == 0 || count > SIZE_MAX / 64) return ECFFT_ERR_BAD_ARG;
    return guarded([&] {
        return with_field(field, [&](auto tag) -> int {
            using F = typename decltype(tag)::type;
            using E = typename F::elem;
            std::vector<E> pa((const E*)a, (const E*)a + count), pb((const E*)bb, (const E*)bb + count), px(count);
            from_crate_host<F>(pa.data(), count); from_crate_host<F>(pb.data(), count);
            const int rc = two_sylow_device<F>(device, pa.data(), pb.data(), count, n_out, px.data());
            if (rc == ECFFT_OK) store_elems<F>(x_out, px.data(), count);
            return rc;
        });
    });
}

int ecfft_find_curve(int field, int device, unsigned k, uint64_t seed, uint64_t start, uint64_t max_candidates, uint64_t* index_out,
                     uint32_t* n_out, void* a_out, void* bb_out, void* gen_xy_out, void* offset_xy_out) {
    if (!known_field(field) || !index_out || !n_out || max_candidates == 0 || start > curve::kMaxIndex ||
        max_candidates > curve::kMaxIndex - start || k > 8 * ecfft_elem_size(field)) return ECFFT_ERR_BAD_ARG;
    *index_out = UINT64_MAX; *n_out = 0;
    return guarded([&] {
        return with_field(field, [&](auto tag) -> int {
            using F = typename decltype(tag)::type;
            using E = typename F::elem;
            uint64_t idx = UINT64_MAX;
            int rc = scan_stream<F>(device, k < 2 ? 2u : k, seed, start, max_candidates, &idx);      // k.max(2), find_curve.rs:225
            if (rc != ECFFT_OK || idx == UINT64_MAX) return rc;
            const E a = curve::stream_elem<F>(seed, 8 * idx), bb = curve::stream_elem<F>(seed, 8 * idx + 4);
            uint32_t n = 0; E x;
            rc = two_sylow_device<F>(device, &a, &bb, 1, &n, &x);                                // its n and generator, from the same stages
            if (rc != ECFFT_OK) return rc;
            const Curve<F> c{a, bb, F::zero()};
            Pt<F> gen{x, F::zero(), false}, off{F::zero(), F::zero(), false};
            if (n < 2 || !curve::is_square<F>(curve::rhs<F>(x, a, bb), &gen.y)) return ECFFT_ERR_HIP;
            // coset offset: the point of smallest integer x >= 1 whose y^2 is a non-zero square and whose order does not divide 2^n
            // (none exists when the whole group is the cyclic group of order 2^n.  By the Hasse bound that is exactly n = the bit
            // length of p, M31's supersingular curves of p + 1 = 2^31 points for one: the offset is then returned as 0, 0)
            const unsigned p_bits = 8 * F::kBytes - (F::kBytes == 4 ? 1 : 0);
            bool found = n == p_bits;
            if (found) off.y = F::zero();
            for (uint32_t xi = 1; xi < (1u << 20) && !found; ++xi) {
                off.x = F::from_u32(xi);
                const E yy = curve::rhs<F>(off.x, a, bb);
                if (F::is_zero(yy) || !curve::is_square<F>(yy, &off.y)) continue;
                found = !pt_double_n<F>(c, off, n).inf;
            }
            if (!found) return ECFFT_ERR_HIP;
            *index_out = idx; *n_out = n;
            store_elems<F>(a_out, &a, 1); store_elems<F>(bb_out, &bb, 1);
            const E g2[2] = {gen.x, gen.y}, o2[2] = {off.x, off.y};
            store_elems<F>(gen_xy_out, g2, 2); store_elems<F>(offset_xy_out, o2, 2);
            return ECFFT_OK;
        });
    });
}

int ecfft_build_fftree_on_curve(int field, size_t n, const void* a, const void* bb, const void* gen_xy, unsigned gen_log_order,
                                const void* offset_xy, int device, ecfft_ctx** out) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (!a || !bb || !gen_xy || !offset_xy) return ECFFT_ERR_BAD_ARG;
    if (!is_pow2(n)) return ECFFT_ERR_NOT_POW2;
    if (!known_field(field) || gen_log_order == 0 || gen_log_order > 8 * ecfft_elem_size(field)) return ECFFT_ERR_BAD_ARG;
    if (ilog2(n) >= gen_log_order) return ECFFT_ERR_TREE_TOO_LARGE;                                  // src/lib.rs:62-64
    return guarded([&] {
        return with_field(field, [&](auto tag) -> int {
            using F = typename decltype(tag)::type;
            using E = typename F::elem;
            E ca, cbb, b;
            memcpy(&ca, a, sizeof(E)); memcpy(&cbb, bb, sizeof(E));
            from_crate_host<F>(&ca, 1); from_crate_host<F>(&cbb, 1);
            if (F::is_zero(cbb) || !F::sqrt(cbb, &b)) return ECFFT_ERR_BAD_ARG;
            const Curve<F> c{ca, cbb, F::zero()};
            const Pt<F> gen = load_point<F>(gen_xy), off = load_point<F>(offset_xy);
            if (!on_curve<F>(c, gen) || !on_curve<F>(c, off)) return ECFFT_ERR_BAD_ARG;
            const Pt<F> g2 = pt_double_n<F>(c, gen, gen_log_order - 1);                              // exact order 2^m: 2^(m-1) gen = (0, 0)
            if (g2.inf || !F::is_zero(g2.x) || !F::is_zero(g2.y)) return ECFFT_ERR_BAD_ARG;
            if (pt_double_n<F>(c, off, gen_log_order).inf) return ECFFT_ERR_BAD_ARG;                 // off + <gen> must miss the identity and pair up no +-P
            HostTree<F> ht;
            const int r = build_good_curve<F>(ca, cbb, gen, gen_log_order, off, ilog2(n), ht, /*points=*/false);
            if (r) return r == 1 ? ECFFT_ERR_TREE_TOO_LARGE : ECFFT_ERR_BAD_ARG;
            if (!have_device(device)) return ECFFT_ERR_HIP;
            return new_ctx<F>(field, device, out, [&](DeviceChain<F>& ch) -> int { return build_chain(ch, std::move(ht), device); });
        });
    });
}

}  // extern "C"

// ---- points of short-Weierstrass curves: ecfft_curve_point_mul / _point_two_adicity / _find_generator / ecfft_build_ec_fftree ----
namespace {
// 2^-256 in plain form, what takes a crate-form element of secp256k1 to plain form by one multiply (1 for M31: nothing to do)
template <class F>
typename F::elem crate_rinv() {
    if constexpr (std::is_same<F, Secp256k1>::value) { Fe256 r = Secp256k1::zero(); r.l[0] = 977; r.l[1] = 1; return Secp256k1::inv(r); }
    else return 1u;
}
template <class F>
typename F::elem elem_from_u64(uint64_t v) {
    if constexpr (std::is_same<F, Secp256k1>::value) { Fe256 r = Secp256k1::zero(); r.l[0] = (uint32_t)v; r.l[1] = (uint32_t)(v >> 32); return r; }
    else return (uint32_t)v;
}
inline bool one_or_count(size_t v, size_t count) { return v == 1 || v == count; }

// The shared front of the two per-point calls, on the selected device: curves, points and flags to the device;
// run(dA, dB, dP, dInf, dFlag) launches; then the flags are read, which waits for the kernel.
template <class F, class Run>
int point_call(const void* A, const void* B, size_t ncurves, const void* points_xy, const uint8_t* inf_in, size_t count, Run&& run) {
    using E = typename F::elem;
    DeviceBuffer dA(ncurves * sizeof(E)), dB(ncurves * sizeof(E)), dP(2 * count * sizeof(E)), dInf(count), dFlag(sizeof(unsigned));
    if (!dA.ok || !dB.ok || !dP.ok || !dInf.ok || !dFlag.ok) return ECFFT_ERR_HIP;
    if (hipMemcpy(dA.p, A, ncurves * sizeof(E), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dB.p, B, ncurves * sizeof(E), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dP.p, points_xy, 2 * count * sizeof(E), hipMemcpyHostToDevice) != hipSuccess || hipMemset(dFlag.p, 0, sizeof(unsigned)) != hipSuccess ||
        (inf_in && hipMemcpy(dInf.p, inf_in, count, hipMemcpyHostToDevice) != hipSuccess)) return ECFFT_ERR_HIP;
    const int rc = run(dA.template as<const E>(), dB.template as<const E>(), dP.template as<const E>(), inf_in ? dInf.template as<const uint8_t>() : nullptr,
                       dFlag.template as<unsigned>());
    if (rc != ECFFT_OK) return rc;
    unsigned flag = 0;
    if (hipMemcpy(&flag, dFlag.p, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess) return ECFFT_ERR_HIP;
    return flag ? ECFFT_ERR_BAD_ARG : ECFFT_OK;                    // a singular curve or a point off its curve, flagged on the device
}
inline unsigned point_blocks(size_t count) { return (unsigned)((count + kPointBlock - 1) / kPointBlock); }
}  // namespace

extern "C" {

int ecfft_curve_point_mul(int field, int device, const void* A, const void* B, size_t ncurves, const void* points_xy, const uint8_t* inf_in,
                          const void* scalars, size_t nscalars, size_t scalar_bytes, void* out_xy, uint8_t* inf_out, size_t count) {
    if (!known_field(field) || !A || !B || !points_xy || !scalars || !out_xy || !inf_out || count == 0 || count > SIZE_MAX / 128 ||
        scalar_bytes == 0 || scalar_bytes > ecpoint::kMaxScalarBytes || !one_or_count(ncurves, count) || !one_or_count(nscalars, count)) return ECFFT_ERR_BAD_ARG;
    return guarded([&] {
        return with_field(field, [&](auto tag) -> int {
            using F = typename decltype(tag)::type;
            using E = typename F::elem;
            const unsigned nbits = ecpoint::scalar_bits((const uint8_t*)scalars, nscalars, (unsigned)scalar_bytes);
            if (!have_device(device)) return ECFFT_ERR_HIP;
            DeviceGuard dev(device);
            if (!dev.ok) return ECFFT_ERR_HIP;
            DeviceBuffer dk(nscalars * scalar_bytes), d_out(2 * count * sizeof(E)), d_inf(count);
            if (!dk.ok || !d_out.ok || !d_inf.ok || hipMemcpy(dk.p, scalars, nscalars * scalar_bytes, hipMemcpyHostToDevice) != hipSuccess) return ECFFT_ERR_HIP;
            const int rc = point_call<F>(A, B, ncurves, points_xy, inf_in, count, [&](const E* dA, const E* dB, const E* dP, const uint8_t* dInf, unsigned* dFlag) -> int {
                hipLaunchKernelGGL((k_point_mul<F>), dim3(point_blocks(count)), dim3(kPointBlock), 0, nullptr, dA, dB, (uint32_t)ncurves, dP, dInf,
                                   dk.template as<const uint8_t>(), (uint32_t)nscalars, (uint32_t)scalar_bytes, nbits, d_out.template as<E>(),
                                   d_inf.template as<uint8_t>(), count, crate_rinv<F>(), dFlag);
                return ECFFT_OK;
            });
            if (rc != ECFFT_OK) return rc;
            if (hipMemcpy(out_xy, d_out.p, 2 * count * sizeof(E), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(inf_out, d_inf.p, count, hipMemcpyDeviceToHost) != hipSuccess) return ECFFT_ERR_HIP;
            return ECFFT_OK;
        });
    });
}

int ecfft_curve_point_two_adicity(int field, int device, const void* A, const void* B, size_t ncurves, const void* points_xy, const uint8_t* inf_in,
                                  unsigned cap, int32_t* out, size_t count) {
    if (!known_field(field) || !A || !B || !points_xy || !out || count == 0 || count > SIZE_MAX / 128 || !one_or_count(ncurves, count) ||
        cap > 8 * ecfft_elem_size(field) + 2) return ECFFT_ERR_BAD_ARG;
    return guarded([&] {
        return with_field(field, [&](auto tag) -> int {
            using F = typename decltype(tag)::type;
            using E = typename F::elem;
            if (!have_device(device)) return ECFFT_ERR_HIP;
            DeviceGuard dev(device);
            if (!dev.ok) return ECFFT_ERR_HIP;
            DeviceBuffer d_out(count * sizeof(int32_t));
            if (!d_out.ok) return ECFFT_ERR_HIP;
            const int rc = point_call<F>(A, B, ncurves, points_xy, inf_in, count, [&](const E* dA, const E* dB, const E* dP, const uint8_t* dInf, unsigned* dFlag) -> int {
                hipLaunchKernelGGL((k_point_two_adicity<F>), dim3(point_blocks(count)), dim3(kPointBlock), 0, nullptr, dA, dB, (uint32_t)ncurves, dP, dInf,
                                   (uint32_t)cap, d_out.template as<int32_t>(), count, crate_rinv<F>(), dFlag);
                return ECFFT_OK;
            });
            if (rc != ECFFT_OK) return rc;
            return hipMemcpy(out, d_out.p, count * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess ? ECFFT_OK : ECFFT_ERR_HIP;
        });
    });
}

int ecfft_curve_find_generator(int field, int device, const void* A, const void* B, const void* order, uint64_t start, uint64_t max_candidates,
                               unsigned* log_order_out, void* gen_xy, void* offset_xy, uint64_t* x_out) {
    if (!known_field(field) || !A || !B || !order || !log_order_out || start == 0 || max_candidates == 0 || start > curve::kMaxIndex ||
        max_candidates > curve::kMaxIndex - start) return ECFFT_ERR_BAD_ARG;
    if (field == ECFFT_FIELD_M31 && start + max_candidates > M31::P) return ECFFT_ERR_BAD_ARG;         // x runs over integers below p
    return guarded([&] {
        return with_field(field, [&](auto tag) -> int {
            using F = typename decltype(tag)::type;
            using E = typename F::elem;
            // order = 2^v m
            uint8_t m[ECFFT_ORDER_BYTES];
            memcpy(m, order, ECFFT_ORDER_BYTES);
            unsigned top = ECFFT_ORDER_BYTES;
            while (top && !m[top - 1]) --top;
            if (!top) return ECFFT_ERR_BAD_ARG;
            unsigned v = 0;
            while (!((m[v >> 3] >> (v & 7)) & 1)) ++v;
            if (v > kMaxTwoAdicity<F>) return ECFFT_ERR_BAD_ARG;
            for (unsigned i = 0; i < ECFFT_ORDER_BYTES; ++i) {          // m >>= v
                const unsigned lo = i + (v >> 3), sh = v & 7;
                const unsigned w = (lo < ECFFT_ORDER_BYTES ? m[lo] : 0u) | ((lo + 1 < ECFFT_ORDER_BYTES ? m[lo + 1] : 0u) << 8);
                m[i] = (uint8_t)(w >> sh);
            }
            const unsigned mbits = ecpoint::scalar_bits(m, 1, ECFFT_ORDER_BYTES);
            E a, b;
            memcpy(&a, A, sizeof(E)); memcpy(&b, B, sizeof(E));
            from_crate_host<F>(&a, 1); from_crate_host<F>(&b, 1);
            if (sw_singular<F>(a, b)) return ECFFT_ERR_BAD_ARG;
            *log_order_out = 0;
            if (v == 0) return ECFFT_OK;                                // an odd order: no 2-power point to find
            if (!have_device(device)) return ECFFT_ERR_HIP;
            DeviceGuard dev(device);
            if (!dev.ok) return ECFFT_ERR_HIP;
            DeviceBuffer dm(ECFFT_ORDER_BYTES), dres(3 * sizeof(unsigned));
            if (!dm.ok || !dres.ok || hipMemcpy(dm.p, m, ECFFT_ORDER_BYTES, hipMemcpyHostToDevice) != hipSuccess) return ECFFT_ERR_HIP;
            // batches in order, the first one wave wide (half of the valid candidates generate on a cyclic curve), then four times
            // the last; both answers are the smallest x of the whole window with their property, whatever the batches are
            uint64_t gen_x = 0, off_x = 0;
            uint32_t batch = kPointBlock;
            for (uint64_t at = 0; at < max_candidates && (!gen_x || !off_x); at += batch, batch = batch < (1u << 16) ? batch * 4 : batch) {
                const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch, max_candidates - at);
                const unsigned init[3] = {~0u, ~0u, 0u};
                if (hipMemcpy(dres.p, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) return ECFFT_ERR_HIP;
                unsigned* r = dres.template as<unsigned>();
                hipLaunchKernelGGL((k_find_generator<F>), dim3(point_blocks(cnt)), dim3(kPointBlock), 0, nullptr, a, b, start + at, cnt,
                                   dm.template as<const uint8_t>(), (uint32_t)ECFFT_ORDER_BYTES, mbits, v, gen_x ? 0 : 1, off_x ? 0 : 1, r, r + 1, r + 2);
                unsigned res[3];
                if (hipMemcpy(res, dres.p, sizeof(res), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess) return ECFFT_ERR_HIP;
                if (res[2]) return ECFFT_ERR_BAD_ARG;                   // [order] R != O for a point R of the curve: not its order
                if (!gen_x && res[0] != ~0u) gen_x = start + at + res[0];
                if (!off_x && res[1] != ~0u) off_x = start + at + res[1];
            }
            if (!gen_x) return ECFFT_OK;                                // no point of order 2^v in the window (a 2-Sylow subgroup that is not cyclic has none)
            // the winner's [m] R once more on the host, by the same body, made affine
            E g2[2], o2[2] = {F::zero(), F::zero()};
            const E gx = elem_from_u64<F>(gen_x), gy = F::sqrt_canon(ecpoint::rhs<F>(gx, a, b));
            if (!ecpoint::jac_to_affine<F>(ecpoint::jac_mul<F>(gx, gy, m, ECFFT_ORDER_BYTES, mbits, a), &g2[0], &g2[1])) return ECFFT_ERR_HIP;
            if (off_x) { o2[0] = elem_from_u64<F>(off_x); o2[1] = F::sqrt_canon(ecpoint::rhs<F>(o2[0], a, b)); }
            *log_order_out = v;
            if (x_out) *x_out = gen_x;
            store_elems<F>(gen_xy, g2, 2); store_elems<F>(offset_xy, o2, 2);
            return ECFFT_OK;
        });
    });
}

int ecfft_build_ec_fftree(int field, size_t n, const void* A, const void* B, const void* gen_xy, unsigned gen_log_order, const void* offset_xy,
                          int device, ecfft_ctx** out) {
    if (!out) return ECFFT_ERR_BAD_ARG;
    *out = nullptr;
    if (!A || !B || !gen_xy || !offset_xy) return ECFFT_ERR_BAD_ARG;
    if (!is_pow2(n)) return ECFFT_ERR_NOT_POW2;
    if (!known_field(field)) return ECFFT_ERR_BAD_ARG;
    if (ilog2(n) > gen_log_order) return ECFFT_ERR_TREE_TOO_LARGE;                                   // src/ec.rs:513-515: n may equal the order
    if (gen_log_order == 0 || gen_log_order > 8 * ecfft_elem_size(field)) return ECFFT_ERR_BAD_ARG;
    return guarded([&] {
        return with_field(field, [&](auto tag) -> int {
            using F = typename decltype(tag)::type;
            using E = typename F::elem;
            E a, b;
            memcpy(&a, A, sizeof(E)); memcpy(&b, B, sizeof(E));
            from_crate_host<F>(&a, 1); from_crate_host<F>(&b, 1);
            const Pt<F> gen = load_point<F>(gen_xy), off = load_point<F>(offset_xy);
            if (!check_short_weierstrass<F>(a, b, gen, gen_log_order, off)) return ECFFT_ERR_BAD_ARG;
            HostTree<F> ht;
            const int r = build_short_weierstrass<F>(a, b, gen, gen_log_order, off, ilog2(n), ht, /*points=*/false);
            if (r) return r == 1 ? ECFFT_ERR_TREE_TOO_LARGE : ECFFT_ERR_BAD_ARG;
            if (!have_device(device)) return ECFFT_ERR_HIP;
            return new_ctx<F>(field, device, out, [&](DeviceChain<F>& ch) -> int { return build_chain(ch, std::move(ht), device); });
        });
    });
}

#ifdef ECFFT_TEST_HOOKS
int ecfft_curve_search_stats(uint64_t* lens, double* seconds, size_t cap, int reset) {
    const size_t n = sizeof(g_stage_len) / sizeof(g_stage_len[0]);
    for (size_t i = 0; i < cap && i < n; ++i) { if (lens) lens[i] = g_stage_len[i]; if (seconds) seconds[i] = g_stage_s[i]; }
    if (reset) { memset(g_stage_len, 0, sizeof(g_stage_len)); memset(g_stage_s, 0, sizeof(g_stage_s)); }
    return (int)n;
}
#endif

}  // extern "C"
