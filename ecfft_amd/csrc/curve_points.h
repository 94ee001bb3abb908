// Point arithmetic on short-Weierstrass curves y^2 = x^3 + A x + B: the bodies of k_point_mul, k_point_two_adicity and
// k_find_generator (kernels.h), `Point::mul` (src/ec.rs:432-447) and `two_adicity` (src/utils.rs:356-365) of the reference.
//
// One body for both fields, __host__ __device__ like the steps of curve_search.h: the kernels run it one point per thread, and
// tests/cpp/ec_tree_host.cpp runs it on the CPU under the sanitizers.  Everything is in PLAIN form, like host_curve.h.
//
// Coordinates: Jacobian (X, Y, Z) with x = X / Z^2, y = Y / Z^3; Z = 0 is the point at infinity.  The base of a multiplication
// stays affine, so an addition is the mixed one.  Field multiplications (squarings counted as such):
//   doubling        10   (6 squarings + 4 products, one of them by A)
//   mixed addition  11   (3 squarings + 8 products)
// Nothing is inverted until the end of a chain; the affine result of a chain is unique, so it is bit-exact against any model of
// the group law.  The exceptional cases are exact (jac_double and jac_add_affine say why):
//   doubling:  Z = 0 or Y = 0 (a point of order 2)            -> infinity
//   addition:  accumulator at infinity                         -> the base
//              same x, same y   (accumulator = base)           -> the doubling
//              same x, other y  (accumulator = -base)          -> infinity
// The formulas run without a branch and the cases are selected limb by limb, which keeps a point in registers: the kernels use
// no scratch memory.
#pragma once
#include <stdint.h>
#include "field_secp256k1.h"
#include "field_m31.h"

namespace ecfft {
namespace ecpoint {

constexpr int kMulsPerDouble = 10, kMulsPerAdd = 11;
constexpr unsigned kMaxScalarBytes = 40;          // ECFFT_ORDER_BYTES: the width of a cardinality

template <class F>
struct Jac { typename F::elem X, Y, Z; };

template <class F>
__host__ __device__ static inline Jac<F> jac_infinity() { return Jac<F>{F::one(), F::one(), F::zero()}; }
template <class F>
__host__ __device__ static inline bool jac_is_inf(const Jac<F>& p) { return F::is_zero(p.Z); }
template <class F>
__host__ __device__ static inline typename F::elem dbl(const typename F::elem& v) { return F::add(v, v); }

// 4 A^3 + 27 B^2 = 0
template <class F>
__host__ __device__ static inline bool singular(const typename F::elem& A, const typename F::elem& B) {
    return F::is_zero(F::add(F::mul(F::from_u32(4), F::mul(F::sqr(A), A)), F::mul(F::from_u32(27), F::sqr(B))));
}
// x^3 + A x + B
template <class F>
__host__ __device__ static inline typename F::elem rhs(const typename F::elem& x, const typename F::elem& A, const typename F::elem& B) {
    return F::add(F::mul(F::add(F::sqr(x), A), x), B);
}
template <class F>
__host__ __device__ static inline bool on_curve(const typename F::elem& x, const typename F::elem& y, const typename F::elem& A, const typename F::elem& B) {
    return F::eq(F::sqr(y), rhs<F>(x, A, B));
}

// does the predicate hold in any lane of the wave?  (on the host: in this one)
__host__ __device__ static inline bool any_lane(bool c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(c) != 0;
#else
    return c;
#endif
}
// c ? a : b, limb by limb: no branch and no pointer to either operand
template <class F>
__host__ __device__ static inline typename F::elem sel(bool c, const typename F::elem& a, const typename F::elem& b) {
    if constexpr (sizeof(typename F::elem) == 4) return c ? a : b;
    else {
        typename F::elem r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r.l[i] = c ? a.l[i] : b.l[i];
        return r;
    }
}

// 2 p.  No branch: Z3 = 2 Y Z, and a field has no zero divisors, so Z3 = 0 exactly when Z = 0 (p at infinity) or Y = 0 (p of
// order 2): the formula gives infinity in both exceptional cases and in no other.
template <class F>
__host__ __device__ static inline Jac<F> jac_double(const Jac<F>& p, const typename F::elem& A) {
    using E = typename F::elem;
    const E XX = F::sqr(p.X), YY = F::sqr(p.Y), ZZ = F::sqr(p.Z);
    const E S = dbl<F>(dbl<F>(F::mul(p.X, YY)));                                  // 4 X Y^2
    const E M = F::add(F::add(dbl<F>(XX), XX), F::mul(A, F::sqr(ZZ)));            // 3 X^2 + A Z^4
    Jac<F> r;
    r.X = F::sub(F::sqr(M), dbl<F>(S));
    const E Y4 = dbl<F>(dbl<F>(dbl<F>(F::sqr(YY))));                              // 8 Y^4
    r.Z = dbl<F>(F::mul(p.Y, p.Z));
    r.Y = F::sub(F::mul(M, F::sub(S, r.X)), Y4);
    return r;
}

// p + (x2, y2), the second a finite affine point.  With H = x2 Z^2 - X and R = y2 Z^3 - Y the sum has Z3 = Z H:
//   p at infinity                     -> (x2, y2, 1), selected
//   H = 0, R = 0 (p is the base)      -> 2 p, computed instead (the chord does not exist)
//   H = 0, R != 0 (p is -base)        -> Z3 = 0: the formula gives infinity, and for finite p in no other case
template <class F>
__host__ __device__ static inline Jac<F> jac_add_affine(const Jac<F>& p, const typename F::elem& x2, const typename F::elem& y2, const typename F::elem& A) {
    using E = typename F::elem;
    const bool pinf = F::is_zero(p.Z);
    const E ZZ = F::sqr(p.Z);
    const E H = F::sub(F::mul(x2, ZZ), p.X);
    const E R = F::sub(F::mul(y2, F::mul(p.Z, ZZ)), p.Y);
    const E HH = F::sqr(H), HHH = F::mul(H, HH), V = F::mul(p.X, HH);
    Jac<F> r;
    r.X = F::sub(F::sub(F::sqr(R), HHH), dbl<F>(V));
    r.Y = F::sub(F::mul(R, F::sub(V, r.X)), F::mul(p.Y, HHH));
    r.Z = F::mul(p.Z, H);
    const bool same = !pinf && F::is_zero(H) && F::is_zero(R);
    if (any_lane(same)) {
        const Jac<F> d = jac_double<F>(p, A);
        r.X = sel<F>(same, d.X, r.X); r.Y = sel<F>(same, d.Y, r.Y); r.Z = sel<F>(same, d.Z, r.Z);
    }
    r.X = sel<F>(pinf, x2, r.X);
    r.Y = sel<F>(pinf, y2, r.Y);
    r.Z = sel<F>(pinf, F::one(), r.Z);
    return r;
}

// [k] (x, y) for the scalar of `nbytes` little-endian bytes at `k`, left to right from bit nbits - 1 (bits at and above
// 8 * nbytes read as zero): every step doubles, the addition is taken where the bit is set
template <class F>
__host__ __device__ static inline Jac<F> jac_mul(const typename F::elem& x, const typename F::elem& y, const uint8_t* k, unsigned nbytes, unsigned nbits,
                                                 const typename F::elem& A) {
    Jac<F> acc = jac_infinity<F>();
    uint32_t byte = 0;
#pragma unroll 1
    for (unsigned i = nbits; i-- > 0;) {
        if ((i & 7u) == 7u || i + 1 == nbits) byte = (i >> 3) < nbytes ? k[i >> 3] : 0u;
        acc = jac_double<F>(acc, A);
        const bool bit = (byte >> (i & 7u)) & 1u;
        if (any_lane(bit)) {
            const Jac<F> s = jac_add_affine<F>(acc, x, y, A);
            acc.X = sel<F>(bit, s.X, acc.X); acc.Y = sel<F>(bit, s.Y, acc.Y); acc.Z = sel<F>(bit, s.Z, acc.Z);
        }
    }
    return acc;
}

// the affine point: one inversion.  false: the point at infinity, (0, 0) written
template <class F>
__host__ __device__ static inline bool jac_to_affine(const Jac<F>& p, typename F::elem* x, typename F::elem* y) {
    using E = typename F::elem;
    if (F::is_zero(p.Z)) { *x = F::zero(); *y = F::zero(); return false; }
    const E zi = F::inv(p.Z), zi2 = F::sqr(zi);
    *x = F::mul(p.X, zi2);
    *y = F::mul(p.Y, F::mul(zi2, zi));
    return true;
}

// the smallest i <= cap with 2^i p = O, -1 when there is none
template <class F>
__host__ __device__ static inline int jac_two_adicity(Jac<F> p, unsigned cap, const typename F::elem& A) {
    int r = -1;
#pragma unroll 1
    for (unsigned i = 0; i <= cap; ++i) {
        if (F::is_zero(p.Z)) { r = (int)i; break; }
        if (i < cap) p = jac_double<F>(p, A);
    }
    return r;
}

// the bit length of the longest of `rows` scalars of `nbytes` little-endian bytes
static inline unsigned scalar_bits(const uint8_t* k, size_t rows, unsigned nbytes) {
    unsigned top = 0;                                   // bytes in use
    for (size_t r = 0; r < rows; ++r)
        for (unsigned b = nbytes; b-- > top;) if (k[r * nbytes + b]) { top = b + 1; break; }
    if (!top) return 0;
    uint8_t m = 0;
    for (size_t r = 0; r < rows; ++r) m |= k[r * nbytes + top - 1];
    unsigned bits = 8 * (top - 1);
    while (m) { ++bits; m >>= 1; }
    return bits;
}

}  // namespace ecpoint
}  // namespace ecfft
