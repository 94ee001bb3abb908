// ecfft_fftree.hpp — C++ host-side mirror of the reference's `FFTree<F>` / `FftreeField` surface
// (/root/reference/src/lib.rs:14-16, src/fftree.rs:17-38, 42, 123, 164, 227, 489) over the C ABI of
// ecfft_hip.h.  Header-only; link with libecfft_hip.so.  Same names, argument meaning and error
// behaviour: where the Rust code panics this throws (std::invalid_argument for non powers of two,
// std::length_error("FFTree is too small")), `build_fftree` returns std::nullopt where Rust returns None.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "ecfft_hip.h"

namespace ecfft_host {

enum class Moiety { S0 = ECFFT_S0, S1 = ECFFT_S1 };                       // src/fftree.rs:17-21

struct Secp256k1Fp { static constexpr int id = ECFFT_FIELD_SECP256K1; using Elem = std::array<uint64_t, 4>; };  // Montgomery limbs
struct M31Fp { static constexpr int id = ECFFT_FIELD_M31; using Elem = uint32_t; };

inline void check(int rc) {
    switch (rc) {
        case ECFFT_OK: return;
        case ECFFT_ERR_NOT_POW2: throw std::invalid_argument("length must be a power of two");
        case ECFFT_ERR_TREE_TOO_SMALL: throw std::length_error("FFTree is too small");
        case ECFFT_ERR_HIP: throw std::runtime_error("ecfft: HIP failure (no usable device?) - there is no CPU fallback");
        default: throw std::runtime_error("ecfft: error " + std::to_string(rc));
    }
}

inline unsigned log2_floor(size_t n) { unsigned l = 0; while (n > 1) { n >>= 1; ++l; } return l; }
inline void require(bool cond, const char* what) { if (!cond) throw std::invalid_argument(what); }

// `ecfft_comm`: inter-GPU transport of the sharded transforms, one process per GPU (RCCL underneath, ecfft_hip.h).
class Comm {
public:
    using UniqueId = std::array<unsigned char, ECFFT_COMM_ID_BYTES>;
    Comm(const Comm&) = delete;
    Comm& operator=(const Comm&) = delete;
    Comm(Comm&& o) noexcept : c_(o.c_) { o.c_ = nullptr; }
    ~Comm() { if (c_) ecfft_comm_destroy(c_); }
    // rank 0 creates the id and hands it to the other ranks by any means (MPI, a file, a socket)
    static UniqueId unique_id() { UniqueId id{}; check(ecfft_comm_get_unique_id(id.data())); return id; }
    static Comm init_rank(const UniqueId& id, int world, int rank, int device) {
        ecfft_comm* c = nullptr;
        check(ecfft_comm_init_rank(id.data(), world, rank, device, &c));
        return Comm(c);
    }
    // the RCCL library the first communicator of the process binds (ecfft_comm_set_rccl_library); "" / nullptr = the default
    static void set_rccl_library(const char* path) { check(ecfft_comm_set_rccl_library(path)); }
    // ncclCommAbort: unblocks exchanges in flight (from another host thread); later sharded calls on this communicator fail
    bool abort() { return ecfft_comm_abort(c_) == ECFFT_OK; }
    // threshold of the link striping of the big pairwise exchanges (ecfft_comm_set_link_striping); the same value on every rank
    void set_link_striping(size_t min_gain_bytes) { check(ecfft_comm_set_link_striping(c_, min_gain_bytes)); }
    int rank() const { return ecfft_comm_rank(c_); }
    int world() const { return ecfft_comm_world(c_); }
    ecfft_comm* raw() const { return c_; }
private:
    explicit Comm(ecfft_comm* c) : c_(c) {}
    ecfft_comm* c_;
};

template <class F>
class FFTree {
public:
    using Elem = typename F::Elem;
    FFTree(const FFTree&) = delete;
    FFTree& operator=(const FFTree&) = delete;
    FFTree(FFTree&& o) noexcept : ctx_(o.ctx_) { o.ctx_ = nullptr; }
    ~FFTree() { if (ctx_) ecfft_ctx_destroy(ctx_); }

    // FftreeField::build_fftree (src/lib.rs:14-16)
    static std::optional<FFTree> build_fftree(size_t n, int device = 0) {
        ecfft_ctx* c = nullptr;
        int rc = ecfft_build_fftree(F::id, n, device, &c);
        if (rc == ECFFT_ERR_TREE_TOO_LARGE) return std::nullopt;
        check(rc);
        return FFTree(c);
    }
    // sharded EXTEND-only context (ecfft_build_extend_shard): this rank's share of the tables of ONE EXTEND of e evaluations
    // over `world` GPUs; only extend_sharded works on it
    static std::optional<FFTree> build_extend_shard(size_t e, int world, int rank, int device = 0) {
        ecfft_ctx* c = nullptr;
        int rc = ecfft_build_extend_shard(F::id, e, device, world, rank, &c);
        if (rc == ECFFT_ERR_TREE_TOO_LARGE) return std::nullopt;
        check(rc);
        return FFTree(c);
    }
    // sharded ENTER-only context (ecfft_build_enter_shard): only enter_sharded works on it
    static std::optional<FFTree> build_enter_shard(size_t n, int world, int rank, int device = 0) {
        ecfft_ctx* c = nullptr;
        int rc = ecfft_build_enter_shard(F::id, n, device, world, rank, &c);
        if (rc == ECFFT_ERR_TREE_TOO_LARGE) return std::nullopt;
        check(rc);
        return FFTree(c);
    }
    // sharded EXIT-only context (ecfft_build_exit_shard), a COLLECTIVE build over `comm`: only exit_sharded works on it
    // min_memory: never keep the full tree T_2n/world for the redundant pair level (ECFFT_EXIT_SHARD_MIN_MEMORY)
    static std::optional<FFTree> build_exit_shard(size_t n, const Comm& comm, int device = 0, bool min_memory = false) {
        ecfft_ctx* c = nullptr;
        int rc = ecfft_build_exit_shard_opts(F::id, n, device, comm.raw(), min_memory ? ECFFT_EXIT_SHARD_MIN_MEMORY : 0, &c);
        if (rc == ECFFT_ERR_TREE_TOO_LARGE) return std::nullopt;
        check(rc);
        return FFTree(c);
    }
    // FFTree::new (src/fftree.rs:42-70): maps as 3 numerator + 3 denominator coefficients each
    static FFTree from_leaves(const std::vector<Elem>& leaves, const std::vector<Elem>& num3, const std::vector<Elem>& den3, int device = 0) {
        // the C ABI reads 3*log2(n) numerator and denominator coefficients: a short vector would be a host out-of-bounds read
        require(!leaves.empty() && (leaves.size() & (leaves.size() - 1)) == 0, "leaves: length must be a power of two");
        require(num3.size() == 3 * (size_t)log2_floor(leaves.size()) && den3.size() == num3.size(), "rational maps: need 3*log2(n) numerator and denominator coefficients");
        ecfft_ctx* c = nullptr;
        check(ecfft_fftree_new(F::id, leaves.data(), leaves.size(), num3.data(), den3.data(), device, &c));
        return FFTree(c);
    }
    // find_curve (src/find_curve.rs:224-246) over candidates start .. start + max_candidates - 1 of the stream `seed`
    // (ecfft_find_curve): the candidate of smallest index whose 2-Sylow subgroup is cyclic of order 2^n, n >= max(k, 2), with a
    // generator of that order and a coset offset; nullopt when the window holds none.  Synchronous.
    struct FoundCurve {
        uint64_t index; uint32_t n;
        Elem a, bb;
        std::array<Elem, 2> gen, offset;       // x, y
    };
    static std::optional<FoundCurve> find_curve(unsigned k, uint64_t seed, uint64_t start = 0, uint64_t max_candidates = uint64_t(1) << 26, int device = 0) {
        FoundCurve f{};
        check(ecfft_find_curve(F::id, device, k, seed, start, max_candidates, &f.index, &f.n, &f.a, &f.bb, f.gen.data(), f.offset.data()));
        if (f.n == 0) return std::nullopt;
        return f;
    }
    // build_fftree on a good curve of the caller's (ecfft_build_fftree_on_curve): gen of order 2^gen_log_order; nullopt when
    // log2 n >= gen_log_order.  What is no good curve, no point of it, or a generator of another order throws.
    static std::optional<FFTree> build_on_curve(size_t n, const Elem& a, const Elem& bb, const std::array<Elem, 2>& gen, unsigned gen_log_order,
                                                const std::array<Elem, 2>& offset, int device = 0) {
        ecfft_ctx* c = nullptr;
        int rc = ecfft_build_fftree_on_curve(F::id, n, &a, &bb, gen.data(), gen_log_order, offset.data(), device, &c);
        if (rc == ECFFT_ERR_TREE_TOO_LARGE) return std::nullopt;
        check(rc);
        return FFTree(c);
    }
    static std::optional<FFTree> build_on_curve(size_t n, const FoundCurve& f, int device = 0) { return build_on_curve(n, f.a, f.bb, f.gen, f.n, f.offset, device); }
    // ---- trees on short-Weierstrass curves y^2 = x^3 + A x + B (ecfft_hip.h: ecfft_curve_point_mul and what follows); synchronous ----
    using Point = std::array<Elem, 2>;         // x, y
    // out[i] = [k_i] P_i (ecfft_curve_point_mul <-> Point::mul, src/ec.rs:432-447).  A, B: one curve for all rows or one per row;
    // scalars: rows of scalar_bytes little-endian bytes, one row for all points or one per point; inf (empty: every point finite)
    // and inf_out: one byte per point, non-zero for the point at infinity.  A point off its curve or a singular curve throws.
    static std::vector<Point> curve_point_mul(const std::vector<Elem>& A, const std::vector<Elem>& B, const std::vector<Point>& points,
                                              const std::vector<uint8_t>& scalars, size_t scalar_bytes, std::vector<uint8_t>& inf_out,
                                              const std::vector<uint8_t>& inf = {}, int device = 0) {
        require(!points.empty() && A.size() == B.size() && (A.size() == 1 || A.size() == points.size()), "curve_point_mul: one curve, or one per point");
        require(scalar_bytes >= 1 && scalars.size() % scalar_bytes == 0 && (scalars.size() == scalar_bytes || scalars.size() == scalar_bytes * points.size()),
                "curve_point_mul: one scalar row, or one per point");
        require(inf.empty() || inf.size() == points.size(), "curve_point_mul: inf must hold one byte per point");
        std::vector<Point> out(points.size());
        inf_out.assign(points.size(), 0);
        check(ecfft_curve_point_mul(F::id, device, A.data(), B.data(), A.size(), points.data(), inf.empty() ? nullptr : inf.data(), scalars.data(),
                                    scalars.size() / scalar_bytes, scalar_bytes, out.data(), inf_out.data(), points.size()));
        return out;
    }
    // the smallest i <= cap with 2^i P the identity, -1 when there is none (ecfft_curve_point_two_adicity <-> two_adicity, src/utils.rs:356-365)
    static std::vector<int32_t> curve_point_two_adicity(const std::vector<Elem>& A, const std::vector<Elem>& B, const std::vector<Point>& points,
                                                        unsigned cap = 8 * sizeof(Elem) + 2, const std::vector<uint8_t>& inf = {}, int device = 0) {
        require(!points.empty() && A.size() == B.size() && (A.size() == 1 || A.size() == points.size()), "curve_point_two_adicity: one curve, or one per point");
        require(inf.empty() || inf.size() == points.size(), "curve_point_two_adicity: inf must hold one byte per point");
        std::vector<int32_t> out(points.size());
        check(ecfft_curve_point_two_adicity(F::id, device, A.data(), B.data(), A.size(), points.data(), inf.empty() ? nullptr : inf.data(), cap, out.data(), points.size()));
        return out;
    }
    // the arguments of build_ec_fftree from a curve and its number of points (ecfft_curve_find_generator; `order` as
    // curve_cardinality returns it): a generator of order 2^log_order and a coset offset (0, 0 when the window holds none), x the
    // integer x-coordinate the generator came from; nullopt when the window holds no generator.  An order that is not the curve's throws.
    struct FoundGenerator {
        unsigned log_order; uint64_t x;
        Point gen, offset;
    };
    static std::optional<FoundGenerator> curve_find_generator(const Elem& A, const Elem& B, const std::array<uint8_t, ECFFT_ORDER_BYTES>& order,
                                                              uint64_t start = 1, uint64_t max_candidates = uint64_t(1) << 12, int device = 0) {
        FoundGenerator g{};
        check(ecfft_curve_find_generator(F::id, device, &A, &B, order.data(), start, max_candidates, &g.log_order, g.gen.data(), g.offset.data(), &g.x));
        if (g.log_order == 0) return std::nullopt;
        return g;
    }
    // build_ec_fftree (src/ec.rs:498-554) on y^2 = x^3 + A x + B (ecfft_build_ec_fftree): gen of order 2^gen_log_order; nullopt
    // when log2 n > gen_log_order.  A singular curve, a point off the curve, a generator of another order or an offset whose
    // double lies in the generator's subgroup throws.
    static std::optional<FFTree> build_ec_fftree(size_t n, const Elem& A, const Elem& B, const Point& gen, unsigned gen_log_order, const Point& offset, int device = 0) {
        ecfft_ctx* c = nullptr;
        int rc = ecfft_build_ec_fftree(F::id, n, &A, &B, gen.data(), gen_log_order, offset.data(), device, &c);
        if (rc == ECFFT_ERR_TREE_TOO_LARGE) return std::nullopt;
        check(rc);
        return FFTree(c);
    }
    size_t size() const { return ecfft_tree_size(ctx_); }

    std::vector<Elem> enter(const std::vector<Elem>& coeffs) const {            // src/fftree.rs:164-167
        std::vector<Elem> out(coeffs.size());
        check(ecfft_enter(ctx_, coeffs.data(), out.data(), coeffs.size(), ECFFT_MEM_HOST, nullptr));
        return out;
    }
    std::vector<Elem> exit(const std::vector<Elem>& evals) const {              // src/fftree.rs:227-230
        std::vector<Elem> out(evals.size());
        check(ecfft_exit(ctx_, evals.data(), out.data(), evals.size(), ECFFT_MEM_HOST, nullptr));
        return out;
    }
    std::vector<Elem> extend(const std::vector<Elem>& evals, Moiety moiety) const {   // src/fftree.rs:123-126
        std::vector<Elem> out(evals.size());
        check(ecfft_extend(ctx_, evals.data(), out.data(), evals.size(), (int)moiety, 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // the remaining algorithms (src/fftree.rs:138-141, 195-198, 264-275, 286-289, 313-316)
    std::vector<Elem> mextend(const std::vector<Elem>& evals, Moiety moiety) const {
        std::vector<Elem> out(evals.size());
        check(ecfft_mextend(ctx_, evals.data(), out.data(), evals.size(), (int)moiety, 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    std::vector<Elem> redc_z0(const std::vector<Elem>& evals, const std::vector<Elem>& a) const { return redc(evals, a, Moiety::S0); }
    std::vector<Elem> redc_z1(const std::vector<Elem>& evals, const std::vector<Elem>& a) const { return redc(evals, a, Moiety::S1); }
    std::vector<Elem> modular_reduce(const std::vector<Elem>& evals, const std::vector<Elem>& a, const std::vector<Elem>& c) const {
        require(a.size() == evals.size() && c.size() == evals.size(), "modular_reduce: a and c must have evals.len() entries");
        std::vector<Elem> out(evals.size());
        check(ecfft_modular_reduce(ctx_, evals.data(), a.data(), c.data(), out.data(), evals.size(), ECFFT_MEM_HOST, nullptr));
        return out;
    }
    std::vector<Elem> vanish(const std::vector<Elem>& domain) const {
        std::vector<Elem> out(2 * domain.size());
        check(ecfft_vanish(ctx_, domain.data(), out.data(), domain.size(), ECFFT_MEM_HOST, nullptr));
        return out;
    }
    size_t degree(const std::vector<Elem>& evals) const {
        size_t d = 0;
        check(ecfft_degree(ctx_, evals.data(), evals.size(), ECFFT_MEM_HOST, nullptr, &d));
        return d;
    }
    // c = a * b in coefficient form (ecfft_poly_mul; no reference counterpart): any lengths, na + nb - 1 coefficients; the tree
    // must hold next_pow2(na + nb - 1) leaves.  mul(a, a) on the same vector is a squaring.
    std::vector<Elem> mul(const std::vector<Elem>& a, const std::vector<Elem>& b) const {
        require(!a.empty() && !b.empty(), "mul: operands must not be empty");
        std::vector<Elem> out(a.size() + b.size() - 1);
        check(ecfft_poly_mul(ctx_, a.data(), a.size(), b.data(), b.size(), out.data(), 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // a = b*q + r, deg r < deg b (ecfft_poly_divrem <-> utils::div_rem, src/utils.rs:184-193): {q, r}, q of a.size() - b.size() + 1
    // coefficients (none when a is shorter), r of b.size() - 1 (zero-padded); b.back() != 0.  Tree rule in ecfft_hip.h.  Synchronous.
    std::pair<std::vector<Elem>, std::vector<Elem>> divrem(const std::vector<Elem>& a, const std::vector<Elem>& b) const {
        require(!a.empty() && !b.empty(), "divrem: operands must not be empty");
        std::vector<Elem> q(a.size() >= b.size() ? a.size() - b.size() + 1 : 0), r(b.size() - 1);
        check(ecfft_poly_divrem(ctx_, a.data(), a.size(), b.data(), b.size(), q.empty() ? nullptr : q.data(), r.empty() ? nullptr : r.data(),
                                1, ECFFT_MEM_HOST, nullptr));
        return {std::move(q), std::move(r)};
    }
    // 1/f mod x^k (ecfft_poly_inv_series; no reference counterpart): k coefficients, f[0] != 0; the tree must hold next_pow2(2k - 1) leaves
    std::vector<Elem> inv_series(const std::vector<Elem>& f, size_t k) const {
        require(!f.empty() && k > 0, "inv_series: f must not be empty and k must be positive");
        std::vector<Elem> out(k);
        check(ecfft_poly_inv_series(ctx_, f.data(), f.size(), out.data(), k, 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // f at arbitrary points (ecfft_poly_eval_points; no reference counterpart): out[i] = f(points[i]); f.size() <= 64 on any tree,
    // otherwise the tree must hold next_pow2(f.size()) leaves
    std::vector<Elem> eval_points(const std::vector<Elem>& f, const std::vector<Elem>& points) const {
        require(!f.empty() && !points.empty(), "eval_points: f and points must not be empty");
        std::vector<Elem> out(points.size());
        check(ecfft_poly_eval_points(ctx_, f.data(), f.size(), points.data(), points.size(), out.data(), 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // the polynomial through arbitrary points (ecfft_poly_interpolate; no reference counterpart), the inverse of eval_points: the
    // coefficients of f of degree < points.size() with f(points[i]) = values[i]; the points pairwise distinct (else
    // std::runtime_error, the C ABI's ECFFT_ERR_BAD_ARG); up to 64 points on any tree, otherwise the tree must hold next_pow2(points.size()) leaves
    std::vector<Elem> interpolate(const std::vector<Elem>& points, const std::vector<Elem>& values) const {
        require(!points.empty() && points.size() == values.size(), "interpolate: as many values as points, at least one");
        std::vector<Elem> out(points.size());
        check(ecfft_poly_interpolate(ctx_, points.data(), points.size(), values.data(), out.data(), 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // a^exp mod modulus (ecfft_poly_pow_mod <-> utils::pow_mod, src/utils.rs:194-211): modulus.size() - 1 coefficients (zero-padded);
    // exp: little-endian bytes (BigUint::to_bytes_le; empty or all zero: the polynomial 1); modulus.size() >= 2, modulus.back() != 0
    // (else std::runtime_error).  Up to 65 modulus coefficients on any tree; tree rule in ecfft_hip.h.  Synchronous.
    std::vector<Elem> pow_mod(const std::vector<Elem>& a, const std::vector<uint8_t>& exp, const std::vector<Elem>& modulus) const {
        require(!a.empty() && modulus.size() >= 2, "pow_mod: a must not be empty and the modulus needs at least 2 coefficients");
        std::vector<Elem> out(modulus.size() - 1);
        check(ecfft_poly_pow_mod(ctx_, a.data(), a.size(), exp.empty() ? nullptr : exp.data(), exp.size(), modulus.data(), modulus.size(),
                                 out.data(), 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // a*b mod modulus (ecfft_poly_mul_mod <-> div_rem(&a.naive_mul(&b), modulus), the step of utils::pow_mod, src/utils.rs:205, 207)
    std::vector<Elem> mul_mod(const std::vector<Elem>& a, const std::vector<Elem>& b, const std::vector<Elem>& modulus) const {
        require(!a.empty() && !b.empty() && modulus.size() >= 2, "mul_mod: operands must not be empty and the modulus needs at least 2 coefficients");
        std::vector<Elem> out(modulus.size() - 1);
        check(ecfft_poly_mul_mod(ctx_, a.data(), a.size(), b.data(), b.size(), modulus.data(), modulus.size(), out.data(), 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // f(g) mod modulus (ecfft_poly_compose_mod; the step of distinct-degree factorisation, src/utils.rs:52-78, and the product of two
    // endomorphisms in examples/schoofs.rs:197-235): modulus.size() - 1 coefficients (zero-padded); f may be longer than the modulus;
    // modulus.size() >= 2, modulus.back() != 0 (else std::runtime_error).  Up to ECFFT_COMPOSE_SMALL_MAX modulus coefficients on any
    // tree; above that about 2 sqrt(f.size()) modular products on the tree rule of pow_mod (ecfft_hip.h).  Synchronous.
    std::vector<Elem> compose_mod(const std::vector<Elem>& f, const std::vector<Elem>& g, const std::vector<Elem>& modulus) const {
        require(!f.empty() && !g.empty() && modulus.size() >= 2, "compose_mod: operands must not be empty and the modulus needs at least 2 coefficients");
        std::vector<Elem> out(modulus.size() - 1);
        check(ecfft_poly_compose_mod(ctx_, f.data(), f.size(), g.data(), g.size(), modulus.data(), modulus.size(), out.data(), 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // the monic gcd (ecfft_poly_gcd <-> utils::gcd, src/utils.rs:132-141), trimmed to its degree (empty for a = b = 0); the operands
    // need not be trimmed and either may be zero; gcd(0, b) = b / lc(b) as utils::xgcd has it.  Up to ECFFT_GCD_SMALL_MAX coefficients
    // on any tree; tree rule in ecfft_hip.h.  Synchronous.
    std::vector<Elem> gcd(const std::vector<Elem>& a, const std::vector<Elem>& b) const {
        require(!a.empty() && !b.empty(), "gcd: operands must not be empty");
        std::vector<Elem> g(std::max(a.size(), b.size()));
        int64_t deg = -1;
        check(ecfft_poly_gcd(ctx_, a.data(), a.size(), b.data(), b.size(), g.data(), &deg, 1, ECFFT_MEM_HOST, nullptr));
        g.resize((size_t)(deg + 1));
        return g;
    }
    // {s, t, g} with a*s + b*t = g, the monic gcd (ecfft_poly_xgcd <-> utils::xgcd, src/utils.rs:147-182): the cofactors of the
    // classical extended Euclidean algorithm, all three trimmed to their degrees.  Synchronous.
    std::array<std::vector<Elem>, 3> xgcd(const std::vector<Elem>& a, const std::vector<Elem>& b) const {
        require(!a.empty() && !b.empty(), "xgcd: operands must not be empty");
        std::vector<Elem> s(std::max<size_t>(b.size() - 1, 1)), t(std::max<size_t>(a.size() - 1, 1)), g(std::max(a.size(), b.size()));
        int64_t deg = -1;
        check(ecfft_poly_xgcd(ctx_, a.data(), a.size(), b.data(), b.size(), s.data(), t.data(), g.data(), &deg, 1, ECFFT_MEM_HOST, nullptr));
        g.resize((size_t)(deg + 1));
        auto trim = [](std::vector<Elem>& v) {
            static const Elem zero{};
            while (!v.empty() && std::memcmp(&v.back(), &zero, sizeof(Elem)) == 0) v.pop_back();
        };
        trim(s); trim(t);
        return {std::move(s), std::move(t), std::move(g)};
    }
    // {r, s, t} with r = s*a + t*b: the first row of the classical remainder sequence (r_0 = a, r_1 = b) with index j >= 1 and
    // deg r < stop (deg 0 = -1), scaled so that t is monic (s where t = 0), all three trimmed to their degrees
    // (ecfft_poly_xgcd_partial; no reference counterpart).  Tree rule as xgcd.  Synchronous.
    std::array<std::vector<Elem>, 3> xgcd_partial(const std::vector<Elem>& a, const std::vector<Elem>& b, size_t stop) const {
        require(!a.empty() && !b.empty(), "xgcd_partial: operands must not be empty");
        std::vector<Elem> r(std::max(a.size(), b.size())), s(b.size()), t(a.size());
        int64_t deg[3] = {-1, -1, -1};
        check(ecfft_poly_xgcd_partial(ctx_, a.data(), a.size(), b.data(), b.size(), stop, r.data(), s.data(), t.data(), deg, 1, ECFFT_MEM_HOST, nullptr));
        r.resize((size_t)(deg[0] + 1)); s.resize((size_t)(deg[1] + 1)); t.resize((size_t)(deg[2] + 1));
        return {std::move(r), std::move(s), std::move(t)};
    }
    // Reed-Solomon decoding with errors (ecfft_rs_decode, Gao's algorithm; no reference counterpart): the k coefficients of the
    // unique f of degree < k whose codeword at the m pairwise distinct points differs from values in at most (m - k) / 2
    // positions; n_errors (may be null) receives how many did, or -1 when there is no such f (the message is then zero).  Up to
    // ECFFT_RS_SMALL_MAX points on any tree; tree rule in ecfft_hip.h.  Two equal points throw.  Synchronous.
    std::vector<Elem> rs_decode(const std::vector<Elem>& points, const std::vector<Elem>& values, size_t k, int64_t* n_errors = nullptr) const {
        require(!points.empty() && points.size() == values.size() && k >= 1 && k <= points.size(), "rs_decode: m points, m values and 1 <= k <= m");
        std::vector<Elem> message(k);
        int64_t n = -1;
        check(ecfft_rs_decode(ctx_, points.data(), points.size(), values.data(), k, message.data(), &n, 1, ECFFT_MEM_HOST, nullptr));
        if (n_errors) *n_errors = n;
        return message;
    }
    // The systematic Reed-Solomon encoder (ecfft_rs_encode; no reference counterpart): the m symbols f(x_0), ..., f(x_{m-1}) of the f
    // of degree < k with f(x_i) = data[i], i < k = data.size(): the data, then m - k parity symbols.  Up to ECFFT_RS_SMALL_MAX
    // points on any tree; tree rule in ecfft_hip.h.  Two equal points throw.  Synchronous.
    std::vector<Elem> rs_encode(const std::vector<Elem>& points, const std::vector<Elem>& data) const {
        require(!data.empty() && data.size() <= points.size(), "rs_encode: m points and 1 <= k <= m data symbols");
        std::vector<Elem> codeword(points.size());
        check(ecfft_rs_encode(ctx_, points.data(), points.size(), data.data(), data.size(), codeword.data(), 1, ECFFT_MEM_HOST, nullptr));
        return codeword;
    }
    // Reed-Solomon decoding with erasures and errors (ecfft_rs_decode_erasures): erased[i] != 0 marks a lost symbol, whose value is
    // never read (an empty vector: no erasure).  rs_decode on the kept points and values: with m' of them, the f of degree < k
    // within floor((m' - k) / 2) errors; n_errors (may be null) receives their number, or -1 when there is no such f or m' < k
    // (the result is then zero).  Returns the k coefficients of f, or with codeword = true its m symbols at all points: the erased
    // positions filled in, the first k the corrected data of rs_encode's code.  Tree rule and errors as rs_decode.  Synchronous.
    std::vector<Elem> rs_decode_erasures(const std::vector<Elem>& points, const std::vector<Elem>& values, const std::vector<uint8_t>& erased,
                                         size_t k, bool codeword = false, int64_t* n_errors = nullptr) const {
        require(!points.empty() && points.size() == values.size() && (erased.empty() || erased.size() == points.size()) && k >= 1 && k <= points.size(),
                "rs_decode_erasures: m points, m values, no or m mask bytes and 1 <= k <= m");
        std::vector<Elem> out(codeword ? points.size() : k);
        int64_t n = -1;
        check(ecfft_rs_decode_erasures(ctx_, points.data(), points.size(), values.data(), erased.empty() ? nullptr : erased.data(), k, out.data(),
                                       codeword ? ECFFT_RS_OUT_CODEWORD : ECFFT_RS_OUT_COEFFS, &n, 1, ECFFT_MEM_HOST, nullptr));
        if (n_errors) *n_errors = n;
        return out;
    }
    // The minimal polynomial of a sequence of N terms (ecfft_seq_min_poly, what Berlekamp-Massey computes; no reference
    // counterpart): the monic C = x^L + sum c_j x^j of least degree with s[i+L] + sum_j c_j s[i+j] = 0 for all 0 <= i < N - L, as
    // L + 1 coefficients ({1} for a zero sequence), where 2 L <= N makes it unique; an EMPTY vector where the sequence is too short
    // to determine it.  order (may be null) receives L or -1.  Up to ECFFT_SEQ_SMALL_MAX terms on any tree; tree rule in
    // ecfft_hip.h.  Synchronous.
    std::vector<Elem> min_poly(const std::vector<Elem>& seq, int64_t* order = nullptr) const {
        require(!seq.empty(), "min_poly: the sequence must not be empty");
        std::vector<Elem> c(seq.size() / 2 + 1);
        int64_t n = -1;
        check(ecfft_seq_min_poly(ctx_, seq.data(), seq.size(), c.data(), &n, 1, ECFFT_MEM_HOST, nullptr));
        if (order) *order = n;
        c.resize((size_t)(n + 1));
        return c;
    }
    // The terms s_K .. s_(K + nout - 1) of the linear recurrence with the characteristic polynomial char_poly (L + 1 >= 2
    // coefficients, a non-zero leading one, monic not required: sum_{j<=L} c_j s[i+j] = 0) and the L initial terms init
    // (ecfft_seq_nth_term; no reference counterpart); index is K in little-endian bytes of any length (empty: K = 0).  One power
    // x^K mod C and nout L multiply-adds.  Up to ECFFT_SEQ_TERM_SMALL_MAX coefficients on any tree; tree rule in ecfft_hip.h.  A
    // zero leading coefficient throws.  Synchronous.
    std::vector<Elem> nth_term(const std::vector<Elem>& char_poly, const std::vector<Elem>& init, const std::vector<uint8_t>& index,
                               size_t nout = 1) const {
        require(char_poly.size() >= 2 && init.size() + 1 == char_poly.size() && nout >= 1, "nth_term: L + 1 >= 2 coefficients, L initial terms, nout >= 1");
        std::vector<Elem> out(nout);
        check(ecfft_seq_nth_term(ctx_, char_poly.data(), char_poly.size(), init.data(), index.empty() ? nullptr : index.data(), index.size(),
                                 out.data(), nout, 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // ... with a 64-bit index
    std::vector<Elem> nth_term(const std::vector<Elem>& char_poly, const std::vector<Elem>& init, uint64_t index, size_t nout = 1) const {
        std::vector<uint8_t> bytes(8);
        for (int i = 0; i < 8; ++i) bytes[(size_t)i] = (uint8_t)(index >> (8 * i));
        return nth_term(char_poly, init, bytes, nout);
    }
    // the distinct roots of f in the field in ascending order of their standard form (ecfft_poly_find_roots <-> utils::find_roots,
    // src/utils.rs:25-44, whose result is sorted the same way).  f need not be trimmed; multiplicities do not matter; a non-zero
    // constant has none.  The zero polynomial, on which the reference panics, throws.  Up to ECFFT_ROOTS_SMALL_MAX coefficients on
    // any tree; tree rule in ecfft_hip.h.  Deterministic (the splitting shifts are 1, 2, 3, ...).  Synchronous.
    std::vector<Elem> find_roots(const std::vector<Elem>& f) const {
        require(!f.empty(), "find_roots: the polynomial must not be empty");
        std::vector<Elem> roots(f.size() - 1);
        int64_t n = 0;
        check(ecfft_poly_find_roots(ctx_, f.data(), f.size(), roots.empty() ? nullptr : roots.data(), &n, 1, ECFFT_MEM_HOST, nullptr));
        require(n >= 0, "find_roots: the zero polynomial (every element is a root)");
        roots.resize((size_t)n);
        return roots;
    }
    // the monic squarefree part f / gcd(f, f') (ecfft_poly_squarefree <-> utils::square_free_factors, src/utils.rs:46-50, made
    // monic), trimmed: {1} for a non-zero constant.  f need not be trimmed.  The zero polynomial throws.  Up to ECFFT_DDF_SMALL_MAX
    // coefficients on any tree; tree rule in ecfft_hip.h.  Synchronous.
    std::vector<Elem> square_free(const std::vector<Elem>& f) const {
        require(!f.empty(), "square_free: the polynomial must not be empty");
        std::vector<Elem> s(f.size());
        int64_t deg = 0;
        check(ecfft_poly_squarefree(ctx_, f.data(), f.size(), s.data(), &deg, 1, ECFFT_MEM_HOST, nullptr));
        require(deg >= 0, "square_free: the zero polynomial");
        s.resize((size_t)deg + 1);
        return s;
    }
    // degree d -> the monic product of the irreducible factors of degree d of f, with its leading 1 (ecfft_poly_distinct_degree <->
    // utils::distinct_degree_factors, src/utils.rs:52-78, which returns such a BTreeMap; this one follows the definition at every
    // degree, where the reference takes x^(p i) for x^(p^i)).  Multiplicities do not matter; a non-zero constant gives an empty map;
    // the zero polynomial throws.  Tree rule as square_free.  Synchronous.
    std::map<size_t, std::vector<Elem>> distinct_degree_factors(const std::vector<Elem>& f) const {
        require(!f.empty(), "distinct_degree_factors: the polynomial must not be empty");
        const size_t nd = f.size() > 1 ? f.size() - 1 : 1;
        std::vector<Elem> fac(nd);
        std::vector<int64_t> deg(nd);
        check(ecfft_poly_distinct_degree(ctx_, f.data(), f.size(), fac.data(), deg.data(), 1, ECFFT_MEM_HOST, nullptr));
        require(deg[0] >= 0, "distinct_degree_factors: the zero polynomial");
        Elem std_one{}, one{};
        const uint32_t u = 1;
        std::memcpy(&std_one, &u, sizeof u);                    // standard form is little-endian
        check(ecfft_elems_from_standard(F::id, &std_one, &one, 1));
        std::map<size_t, std::vector<Elem>> out;
        size_t pos = 0;
        for (size_t d = 1; d <= nd; ++d) {
            if (deg[d - 1] <= 0) continue;
            std::vector<Elem> g(fac.data() + pos, fac.data() + pos + (size_t)deg[d - 1]);
            g.push_back(one);
            out.emplace(d, std::move(g));
            pos += (size_t)deg[d - 1];
        }
        return out;
    }
    // the monic irreducible factors of degree d of g, each with its leading 1, in ascending lexicographic order of (c_0, .., c_(d-1))
    // as standard-form integers (ecfft_poly_equal_degree <-> utils::equal_degree_factorization, src/utils.rs:82-113).  g must be a
    // squarefree product of irreducibles of degree d, which is what distinct_degree_factors returns; a non-zero constant gives an
    // empty vector; the zero polynomial and a degree that d does not divide throw.  Tree rule as square_free.  Synchronous.
    std::vector<std::vector<Elem>> equal_degree_factors(const std::vector<Elem>& g, size_t d) const {
        require(!g.empty() && d > 0, "equal_degree_factors: the polynomial must not be empty and d must be positive");
        const size_t nd = g.size() > 1 ? g.size() - 1 : 1;
        std::vector<Elem> fac(nd);
        int64_t n = 0;
        check(ecfft_poly_equal_degree(ctx_, g.data(), g.size(), d, fac.data(), &n, 1, ECFFT_MEM_HOST, nullptr));
        require(n != -1, "equal_degree_factors: the zero polynomial");
        require(n >= 0, "equal_degree_factors: d does not divide the degree");
        Elem std_one{}, one{};
        const uint32_t u = 1;
        std::memcpy(&std_one, &u, sizeof u);                    // standard form is little-endian
        check(ecfft_elems_from_standard(F::id, &std_one, &one, 1));
        std::vector<std::vector<Elem>> out;
        for (size_t i = 0; i < (size_t)n; ++i) {
            std::vector<Elem> q(fac.data() + i * d, fac.data() + (i + 1) * d);
            q.push_back(one);
            out.push_back(std::move(q));
        }
        return out;
    }
    // multiplicity i -> the monic a_i of positive degree, with its leading 1, of Yun's decomposition f = lead prod_i a_i^i: the a_i
    // squarefree and pairwise coprime (ecfft_poly_squarefree_decompose; the reference's square_free_factors, src/utils.rs:46-50,
    // returns prod a_i only).  lead (may be null) receives the leading coefficient.  A non-zero constant gives an empty map; the zero
    // polynomial throws.  Up to ECFFT_FACTOR_SMALL_MAX coefficients work on any tree; tree rule as square_free.  Synchronous.
    std::map<size_t, std::vector<Elem>> square_free_decomposition(const std::vector<Elem>& f, Elem* lead = nullptr) const {
        require(!f.empty(), "square_free_decomposition: the polynomial must not be empty");
        const size_t nd = f.size() > 1 ? f.size() - 1 : 1;
        std::vector<Elem> parts(nd);
        std::vector<int64_t> deg(nd);
        check(ecfft_poly_squarefree_decompose(ctx_, f.data(), f.size(), parts.data(), deg.data(), lead, 1, ECFFT_MEM_HOST, nullptr));
        require(deg[0] >= 0, "square_free_decomposition: the zero polynomial");
        Elem std_one{}, one{};
        const uint32_t u = 1;
        std::memcpy(&std_one, &u, sizeof u);                    // standard form is little-endian
        check(ecfft_elems_from_standard(F::id, &std_one, &one, 1));
        std::map<size_t, std::vector<Elem>> out;
        size_t pos = 0;
        for (size_t i = 1; i <= nd; ++i) {
            if (deg[i - 1] <= 0) continue;
            std::vector<Elem> a(parts.data() + pos, parts.data() + pos + (size_t)deg[i - 1]);
            a.push_back(one);
            out.emplace(i, std::move(a));
            pos += (size_t)deg[i - 1];
        }
        return out;
    }
    // (q, e) for every distinct monic irreducible factor q of f = lead prod q^e, q with its leading 1, in ascending (e, deg q, then the
    // order of equal_degree_factors) (ecfft_poly_factor: the reference's three steps, src/utils.rs:25-113, for every degree and with
    // the multiplicities).  lead (may be null) receives the leading coefficient.  A non-zero constant gives an empty vector; the zero
    // polynomial throws.  Deterministic.  Up to ECFFT_FACTOR_SMALL_MAX coefficients work on any tree; tree rule as square_free.
    std::vector<std::pair<std::vector<Elem>, size_t>> factor(const std::vector<Elem>& f, Elem* lead = nullptr) const {
        require(!f.empty(), "factor: the polynomial must not be empty");
        const size_t nd = f.size() > 1 ? f.size() - 1 : 1;
        std::vector<Elem> fac(nd);
        std::vector<int64_t> fdeg(nd), fmult(nd);
        int64_t n = 0;
        check(ecfft_poly_factor(ctx_, f.data(), f.size(), fac.data(), fdeg.data(), fmult.data(), &n, lead, 1, ECFFT_MEM_HOST, nullptr));
        require(n >= 0, "factor: the zero polynomial");
        Elem std_one{}, one{};
        const uint32_t u = 1;
        std::memcpy(&std_one, &u, sizeof u);                    // standard form is little-endian
        check(ecfft_elems_from_standard(F::id, &std_one, &one, 1));
        std::vector<std::pair<std::vector<Elem>, size_t>> out;
        size_t pos = 0;
        for (size_t j = 0; j < (size_t)n; ++j) {
            std::vector<Elem> q(fac.data() + pos, fac.data() + pos + (size_t)fdeg[j]);
            q.push_back(one);
            out.emplace_back(std::move(q), (size_t)fmult[j]);
            pos += (size_t)fdeg[j];
        }
        return out;
    }
    // L(n): the coefficients of psi_n with the factor 2y of an even index removed
    static size_t division_polynomial_len(size_t n) { return n < 2 ? 1 : ((n & 1) ? (n * n - 1) / 2 + 1 : (n * n - 4) / 2 + 1); }
    // psi_n of y^2 = x^3 + A x + B, L(n) coefficients low to high, not monic (ecfft_division_polynomial <-> division_polynomial,
    // examples/schoofs.rs:368-431).  n <= 4 on any tree, otherwise next_pow2(L(n)) leaves.
    std::vector<Elem> division_polynomial(const Elem& A, const Elem& B, size_t n) const {
        std::vector<Elem> out(division_polynomial_len(n));
        check(ecfft_division_polynomial(ctx_, &A, &B, n, out.data(), 1, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    // t mod l with #E = p + 1 - t for the curves y^2 = x^3 + A[i] x + B[i], -1 for a singular curve (ecfft_curve_trace_mod <->
    // frobenius_trace_mod_l / has_even_order, examples/schoofs.rs:76-138, 345-366).  l is 2 or an odd prime up to
    // ECFFT_SCHOOF_MAX_L; l <= 11 on any tree, otherwise next_pow2(2 L(l) - 1) leaves.  Synchronous.
    std::vector<int64_t> curve_trace_mod(const std::vector<Elem>& A, const std::vector<Elem>& B, size_t l) const {
        require(!A.empty() && A.size() == B.size(), "curve_trace_mod: A and B must hold one element per curve");
        std::vector<int64_t> t(A.size());
        check(ecfft_curve_trace_mod(ctx_, A.data(), B.data(), l, t.data(), A.size(), ECFFT_MEM_HOST, nullptr));
        return t;
    }
    // #E(F_p) of y^2 = x^3 + A x + B as ECFFT_ORDER_BYTES little-endian bytes, zero for a singular curve (ecfft_curve_cardinality <->
    // cardinality, examples/schoofs.rs:30-71).  Needs the tree of the largest prime of the rule.  Synchronous.
    std::array<uint8_t, ECFFT_ORDER_BYTES> curve_cardinality(const Elem& A, const Elem& B) const {
        std::array<uint8_t, ECFFT_ORDER_BYTES> order{};
        check(ecfft_curve_cardinality(ctx_, &A, &B, order.data(), nullptr, 1, ECFFT_MEM_HOST, nullptr));
        return order;
    }
    size_t device_bytes() const { return ecfft_ctx_device_bytes(ctx_); }     // HBM held between calls: tables + scratch
    // device-resident variants (pointers into HBM, caller's stream)
    void enter_device(const Elem* coeffs, Elem* evals, size_t n, void* stream) const { check(ecfft_enter(ctx_, coeffs, evals, n, ECFFT_MEM_DEVICE, stream)); }
    void exit_device(const Elem* evals, Elem* coeffs, size_t n, void* stream) const { check(ecfft_exit(ctx_, evals, coeffs, n, ECFFT_MEM_DEVICE, stream)); }
    void extend_device(const Elem* in, Elem* out, size_t e, Moiety m, size_t count, void* stream) const { check(ecfft_extend(ctx_, in, out, e, (int)m, count, ECFFT_MEM_DEVICE, stream)); }
    // count pairs: a count x na, b count x nb, out count x (na + nb - 1)
    void mul_device(const Elem* a, size_t na, const Elem* b, size_t nb, Elem* out, size_t count, void* stream) const {
        check(ecfft_poly_mul(ctx_, a, na, b, nb, out, count, ECFFT_MEM_DEVICE, stream));
    }
    // count pairs: a count x na, b count x nb, q count x (na - nb + 1), r count x (nb - 1); q or r may be null.  Synchronous.
    void divrem_device(const Elem* a, size_t na, const Elem* b, size_t nb, Elem* q, Elem* r, size_t count, void* stream) const {
        check(ecfft_poly_divrem(ctx_, a, na, b, nb, q, r, count, ECFFT_MEM_DEVICE, stream));
    }
    // count series: f count x nf, out count x k.  Synchronous.
    void inv_series_device(const Elem* f, size_t nf, Elem* out, size_t k, size_t count, void* stream) const {
        check(ecfft_poly_inv_series(ctx_, f, nf, out, k, count, ECFFT_MEM_DEVICE, stream));
    }
    // count polynomials f count x nf at m shared points, out count x m.  Asynchronous on `stream`.
    void eval_points_device(const Elem* f, size_t nf, const Elem* points, size_t m, Elem* out, size_t count, void* stream) const {
        check(ecfft_poly_eval_points(ctx_, f, nf, points, m, out, count, ECFFT_MEM_DEVICE, stream));
    }
    // count value vectors (count x m) at m shared, pairwise distinct points, out count x m coefficients.  Synchronous.
    void interpolate_device(const Elem* points, size_t m, const Elem* values, Elem* out, size_t count, void* stream) const {
        check(ecfft_poly_interpolate(ctx_, points, m, values, out, count, ECFFT_MEM_DEVICE, stream));
    }
    // count pairs: a count x na, modulus count x nm, out count x (nm - 1); exp: HOST bytes, little-endian, shared by all pairs.  Synchronous.
    void pow_mod_device(const Elem* a, size_t na, const uint8_t* exp, size_t exp_bytes, const Elem* modulus, size_t nm, Elem* out, size_t count,
                        void* stream) const {
        check(ecfft_poly_pow_mod(ctx_, a, na, exp, exp_bytes, modulus, nm, out, count, ECFFT_MEM_DEVICE, stream));
    }
    // count triples: f count x nf, g count x ng, modulus count x nm, out count x (nm - 1).  Synchronous.
    void compose_mod_device(const Elem* f, size_t nf, const Elem* g, size_t ng, const Elem* modulus, size_t nm, Elem* out, size_t count,
                            void* stream) const {
        check(ecfft_poly_compose_mod(ctx_, f, nf, g, ng, modulus, nm, out, count, ECFFT_MEM_DEVICE, stream));
    }
    // count pairs: a count x na, b count x nb (untrimmed), g count x max(na, nb); degrees: count HOST entries or null.  Synchronous.
    void gcd_device(const Elem* a, size_t na, const Elem* b, size_t nb, Elem* g, int64_t* degrees, size_t count, void* stream) const {
        check(ecfft_poly_gcd(ctx_, a, na, b, nb, g, degrees, count, ECFFT_MEM_DEVICE, stream));
    }
    // ... with the cofactors: s count x max(nb - 1, 1), t count x max(na - 1, 1); s or t may be null.  Synchronous.
    void xgcd_device(const Elem* a, size_t na, const Elem* b, size_t nb, Elem* s, Elem* t, Elem* g, int64_t* degrees, size_t count, void* stream) const {
        check(ecfft_poly_xgcd(ctx_, a, na, b, nb, s, t, g, degrees, count, ECFFT_MEM_DEVICE, stream));
    }
    // count pairs: the first row below `stop` (ecfft_poly_xgcd_partial): r count x max(na, nb), s count x nb (may be null), t count x na;
    // degrees: count x 3 HOST entries (deg r, deg s, deg t) or null.  Synchronous.
    void xgcd_partial_device(const Elem* a, size_t na, const Elem* b, size_t nb, size_t stop, Elem* r, Elem* s, Elem* t, int64_t* degrees, size_t count, void* stream) const {
        check(ecfft_poly_xgcd_partial(ctx_, a, na, b, nb, stop, r, s, t, degrees, count, ECFFT_MEM_DEVICE, stream));
    }
    // count received words of m symbols at m shared points -> message count x k; n_errors: count HOST entries (-1: not decodable).  Synchronous.
    void rs_decode_device(const Elem* points, size_t m, const Elem* values, size_t k, Elem* message, int64_t* n_errors, size_t count, void* stream) const {
        check(ecfft_rs_decode(ctx_, points, m, values, k, message, n_errors, count, ECFFT_MEM_DEVICE, stream));
    }
    // count data rows of k symbols -> codeword count x m, the data then the parity (ecfft_rs_encode).  Synchronous.
    void rs_encode_device(const Elem* points, size_t m, const Elem* data, size_t k, Elem* codeword, size_t count, void* stream) const {
        check(ecfft_rs_encode(ctx_, points, m, data, k, codeword, count, ECFFT_MEM_DEVICE, stream));
    }
    // count received words with their masks (count x m device bytes, or null) -> out count x k coefficients, or count x m symbols
    // for out_form = ECFFT_RS_OUT_CODEWORD; n_errors: count HOST entries (-1: not decodable).  Synchronous.
    void rs_decode_erasures_device(const Elem* points, size_t m, const Elem* values, const uint8_t* erased, size_t k, Elem* out, int out_form,
                                   int64_t* n_errors, size_t count, void* stream) const {
        check(ecfft_rs_decode_erasures(ctx_, points, m, values, erased, k, out, out_form, n_errors, count, ECFFT_MEM_DEVICE, stream));
    }
    // count rows of n_terms -> min_poly count x (n_terms / 2 + 1); orders: count HOST entries (-1: undetermined, a zero row).  Synchronous.
    void min_poly_device(const Elem* seq, size_t n_terms, Elem* min_poly, int64_t* orders, size_t count, void* stream) const {
        check(ecfft_seq_min_poly(ctx_, seq, n_terms, min_poly, orders, count, ECFFT_MEM_DEVICE, stream));
    }
    // count recurrences: char_poly count x nc, init count x (nc - 1), index: index_bytes little-endian HOST bytes shared by all rows,
    // out count x nout.  Synchronous.
    void nth_term_device(const Elem* char_poly, size_t nc, const Elem* init, const void* index, size_t index_bytes, Elem* out, size_t nout,
                         size_t count, void* stream) const {
        check(ecfft_seq_nth_term(ctx_, char_poly, nc, init, index, index_bytes, out, nout, count, ECFFT_MEM_DEVICE, stream));
    }
    // count polynomials f count x nf (untrimmed), roots count x (nf - 1) sorted and zero-padded; n_roots: count HOST entries (-1: the
    // zero polynomial).  Synchronous.
    void find_roots_device(const Elem* f, size_t nf, Elem* roots, int64_t* n_roots, size_t count, void* stream) const {
        check(ecfft_poly_find_roots(ctx_, f, nf, roots, n_roots, count, ECFFT_MEM_DEVICE, stream));
    }
    // count triples: a count x na, b count x nb, modulus count x nm, out count x (nm - 1).  Synchronous.
    void mul_mod_device(const Elem* a, size_t na, const Elem* b, size_t nb, const Elem* modulus, size_t nm, Elem* out, size_t count, void* stream) const {
        check(ecfft_poly_mul_mod(ctx_, a, na, b, nb, modulus, nm, out, count, ECFFT_MEM_DEVICE, stream));
    }

    // ONE transform split over the ranks of `comm` (device pointers: this rank's block shard of len / world elements)
    void extend_sharded(const Comm& comm, const Elem* in, Elem* out, size_t e, Moiety m, void* stream) const { check(ecfft_extend_sharded(ctx_, comm.raw(), in, out, e, (int)m, stream)); }
    // the same with a CYCLIC shard (local j' = global j' * world + rank) on either side: one exchange fewer per cyclic side
    void extend_sharded_layout(const Comm& comm, const Elem* in, Elem* out, size_t e, Moiety m, bool cyclic_in, bool cyclic_out, void* stream) const {
        check(ecfft_extend_sharded_layout(ctx_, comm.raw(), in, out, e, (int)m, cyclic_in ? ECFFT_LAYOUT_CYCLIC : ECFFT_LAYOUT_BLOCK,
                                          cyclic_out ? ECFFT_LAYOUT_CYCLIC : ECFFT_LAYOUT_BLOCK, stream));
    }
    void enter_sharded(const Comm& comm, const Elem* coeffs, Elem* evals, size_t n, void* stream) const { check(ecfft_enter_sharded(ctx_, comm.raw(), coeffs, evals, n, stream)); }
    void exit_sharded(const Comm& comm, const Elem* evals, Elem* coeffs, size_t n, void* stream) const { check(ecfft_exit_sharded(ctx_, comm.raw(), evals, coeffs, n, stream)); }

    // pub tables of the subtree with m leaves (src/fftree.rs:24-38, 489-496)
    std::vector<Elem> table(int which, size_t m) const {
        size_t cnt = 0;
        check(ecfft_tree_table(ctx_, m, which, nullptr, 0, &cnt));
        std::vector<Elem> out(cnt);
        check(ecfft_tree_table(ctx_, m, which, out.data(), cnt, &cnt));
        return out;
    }
    ecfft_ctx* raw() const { return ctx_; }

private:
    std::vector<Elem> redc(const std::vector<Elem>& evals, const std::vector<Elem>& a, Moiety m) const {
        require(a.size() == evals.size(), "redc: a must have evals.len() entries");
        std::vector<Elem> out(evals.size());
        check(ecfft_redc(ctx_, evals.data(), a.data(), out.data(), evals.size(), (int)m, ECFFT_MEM_HOST, nullptr));
        return out;
    }
    explicit FFTree(ecfft_ctx* c) : ctx_(c) {}
    ecfft_ctx* ctx_;
};

}  // namespace ecfft_host
