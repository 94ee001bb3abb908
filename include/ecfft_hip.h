/* ecfft_hip.h — C ABI of the MI355X (gfx950) ECFFT hot path.
 *
 * Drop-in boundary for the EXTEND / ENTER / EXIT path of andrewmilson/ecfft.  The reference has no
 * FFI layer (pure generic Rust); each entry point below names the Rust item whose body a thin
 * `impl` would forward to it (see INTEGRATION.md for the binding a maintainer would add):
 *
 *   ecfft_build_fftree            <-> FftreeField::build_fftree(n) -> Option<FFTree<Self>>   src/lib.rs:14-16, 39-85, 198-215
 *   ecfft_fftree_new              <-> FFTree::new(leaves, rational_maps)                       src/fftree.rs:42-70
 *   ecfft_enter                   <-> FFTree::enter(&self, &[F]) -> Vec<F>                     src/fftree.rs:164-167
 *   ecfft_exit                    <-> FFTree::exit(&self, &[F]) -> Vec<F>                      src/fftree.rs:227-230
 *   ecfft_extend                  <-> FFTree::extend(&self, &[F], Moiety) -> Vec<F>            src/fftree.rs:123-126
 *   ecfft_tree_size / _table      <-> the pub fields of FFTree<F> / subtree_with_size          src/fftree.rs:24-38, 489-496
 *   ecfft_fftree_serialize / _deserialize <-> impl CanonicalSerialize / CanonicalDeserialize  src/fftree.rs:507-660
 *   ecfft_ctx_destroy             <-> Drop
 *
 * Element representation = the crate's in-memory one, so Rust slices pass through untouched:
 *   ECFFT_FIELD_SECP256K1: 32 bytes = [u64; 4] little-endian limbs of x * 2^256 mod p (ark-ff
 *                          Fp256<MontBackend<FqConfig, 4>>, src/lib.rs:37), fully reduced;
 *   ECFFT_FIELD_M31:       4 bytes  = u32 canonical residue (ark_ff_optimized::fp31::Fp, src/lib.rs:196).
 * Outputs are fully reduced, so equality of bytes == equality of field elements (assert_eq! in the
 * reference's tests).
 *
 * Errors: the reference panics (src/fftree.rs:40 "TODO: errors"); the ABI returns a status instead:
 *   - length not a power of two   (assert!, src/fftree.rs:490, src/lib.rs:41)  -> ECFFT_ERR_NOT_POW2
 *   - "FFTree is too small"       (panic!, src/fftree.rs:494)                   -> ECFFT_ERR_TREE_TOO_SMALL
 *   - build_fftree returning None (src/lib.rs:62-64, src/ec.rs:513-515)         -> ECFFT_ERR_TREE_TOO_LARGE, *out = NULL
 * There is no CPU fallback: without a usable HIP device every call fails with ECFFT_ERR_HIP.
 *
 * Threading: a context is immutable after creation (like &FFTree); transform calls on one context
 * serialise on its scratch buffers (a host mutex orders the enqueues, a HIP event orders the device
 * work across streams); use one context per host thread/stream for concurrency.
 * Ownership: the caller owns every buffer; `stream` is a hipStream_t passed as void* (NULL = default).
 */
#ifndef ECFFT_HIP_H
#define ECFFT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ecfft_ctx ecfft_ctx;

enum { ECFFT_FIELD_SECP256K1 = 0, ECFFT_FIELD_M31 = 1 };
enum { ECFFT_S0 = 0, ECFFT_S1 = 1 };                 /* enum Moiety, src/fftree.rs:17-21 (the TARGET moiety) */
enum { ECFFT_MEM_HOST = 0, ECFFT_MEM_DEVICE = 1 };   /* where in/out pointers live */
enum {
    ECFFT_OK = 0,
    ECFFT_ERR_NOT_POW2 = 1,
    ECFFT_ERR_TREE_TOO_SMALL = 2,
    ECFFT_ERR_TREE_TOO_LARGE = 3,
    ECFFT_ERR_HIP = 4,
    ECFFT_ERR_BAD_ARG = 5
};
/* tables of FFTree<F> exported by ecfft_tree_table (src/fftree.rs:25-37) */
enum {
    ECFFT_TBL_F = 0,              /* BinaryTree<F>, 2m entries, heap order          */
    ECFFT_TBL_RECOMBINE = 1,      /* BinaryTree<Mat2x2<F>>, m matrices = 4m elements, row-major, heap order (src/fftree.rs:26) */
    ECFFT_TBL_DECOMPOSE = 2,      /* likewise (src/fftree.rs:27); rebuilt on demand from the normalised tables */
    ECFFT_TBL_XNN_S = 3, ECFFT_TBL_XNN_S_INV = 4, ECFFT_TBL_Z0_S1 = 5, ECFFT_TBL_Z1_S0 = 6,
    ECFFT_TBL_Z0_INV_S1 = 7, ECFFT_TBL_Z1_INV_S0 = 8, ECFFT_TBL_Z0Z0_REM_XNN_S = 9, ECFFT_TBL_Z1Z1_REM_XNN_S = 10
};

/* size in bytes of one field element of `field` (32 or 4); 0 for an unknown field */
size_t ecfft_elem_size(int field);

/* FftreeField::build_fftree(n): builds the whole subtree chain T_1..T_n on `device`. */
int ecfft_build_fftree(int field, size_t n, int device, ecfft_ctx** out);

/* FFTree::new(leaves, rational_maps): n leaves and log2(n) maps, each map given as 3 numerator and
 * 3 denominator coefficients (low -> high, zero padded) — all in the element representation above. */
int ecfft_fftree_new(int field, const void* leaves, size_t n, const void* map_num3, const void* map_den3,
                     int device, ecfft_ctx** out);

void ecfft_ctx_destroy(ecfft_ctx* ctx);

size_t ecfft_tree_size(const ecfft_ctx* ctx);   /* number of leaves of the top tree */
int ecfft_field(const ecfft_ctx* ctx);
size_t ecfft_ctx_device_bytes(const ecfft_ctx* ctx);   /* HBM the context holds between calls: tables + transform scratch + pooled temporaries (+ gathered cyclic tables) */
/* The algorithm wrappers (ecfft_redc, ecfft_vanish, ecfft_degree, the sharded transforms ...) keep their temporaries in a
 * per-context pool between calls; the pool is capped (idle blocks beyond twice the transform scratch are freed at the end of a
 * call) and this call returns every idle block — except the pinned temporaries of sharded call shapes the ranks have agreed on, which
 * stay so that those calls keep running without allocation — and the host-call staging buffer to the device.  Call between transforms.
 * A full context that has served sharded EXTENDs also holds compact copies of the cyclic stages' table entries (gathered on
 * first use, counted by ecfft_ctx_device_bytes); they are returned too and gathered again when needed. */
int ecfft_ctx_trim(ecfft_ctx* ctx);

/* coefficients -> evaluations on the leaves of T_n (n = len; any power of two <= tree size) */
int ecfft_enter(ecfft_ctx* ctx, const void* coeffs, void* evals, size_t n, int mem, void* stream);
/* evaluations -> coefficients */
int ecfft_exit(ecfft_ctx* ctx, const void* evals, void* coeffs, size_t n, int mem, void* stream);
/* batched forms (no reference counterpart): `count` independent polynomials of length n, laid end to end, share every
 * kernel launch and every table read — the throughput mode for provers that transform many columns.  (An even batch of at
 * least 2^20 elements runs as two half-batches of whole polynomials on two streams, joined on `stream` before the call's work
 * is complete in stream order: same results, 4-7 % faster) */
int ecfft_enter_many(ecfft_ctx* ctx, const void* coeffs, void* evals, size_t n, size_t count, int mem, void* stream);
int ecfft_exit_many(ecfft_ctx* ctx, const void* evals, void* coeffs, size_t n, size_t count, int mem, void* stream);
/* `count` vectors of `e` evaluations on the moiety opposite to `moiety` -> evaluations on `moiety`
 * of T_{2e}; vectors are laid end to end (count = 1 is FFTree::extend).  (An even batch of >= 2^20 elements of vectors with
 * e >= 2^19 runs as two half-batches on two streams, like the batched ENTER / EXIT.) */
int ecfft_extend(ecfft_ctx* ctx, const void* in, void* out, size_t e, int moiety, size_t count, int mem, void* stream);
/* c = a * b in coefficient form; no reference counterpart (the enter -> pointwise -> exit composition of
 * src/fftree.rs:164-167, 227-230 that a user of the crate writes by hand).  a: count x na, b: count x nb,
 * out: count x (na + nb - 1) coefficients, each polynomial laid end to end.  na, nb >= 1, any length (not only powers of two).
 * Needs the context's tree to hold N = next_pow2(na + nb - 1) leaves, else ECFFT_ERR_TREE_TOO_SMALL.
 * a == b with na == nb is a squaring (one forward transform).  out must not overlap a or b.
 * An operand of at most N/2 coefficients is entered at its own size and lifted to N by EXTENDs (with its high half zero, ENTER of
 * 2m coefficients is the ENTER of m interleaved with its EXTEND onto S1), so the call costs about one ENTER_N + one EXIT_N plus
 * the pointwise product.  Memory, stream and threading as for ecfft_enter_many; temporaries are pooled (ecfft_ctx_trim). */
int ecfft_poly_mul(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, void* out, size_t count, int mem, void* stream);
/* Division with remainder on the GPU:
 *   ecfft_poly_divrem     <-> ecfft::utils::div_rem (src/utils.rs:184-193) = ark-poly DenseOrSparsePolynomial::divide_with_q_and_r
 * a = b*q + r with deg r < deg b for `count` pairs laid end to end: a: count x na, b: count x nb with b[nb-1] != 0 in every pair
 * (ark's DensePolynomial is always trimmed); q: count x nq, nq = na - nb + 1 (0 when na < nb); r: count x (nb - 1), zero-padded
 * above its true degree.  q or r may be NULL (r only = utils::div_rem), not both.  Outputs must not overlap the inputs.
 * ecfft_poly_inv_series: g = 1/f mod x^k (power-series reciprocal; no reference counterpart), f: count x nf with f[0] != 0, out: count x k.
 * Algorithm: the first 64 coefficients of 1/f by the schoolbook recurrence (one workgroup per pair), then Newton steps
 * g' = g (2 - f g), each one fused product on the leaves of T_N; q = rev(rev(a) * (1/rev(b) mod x^nq) mod x^nq) and
 * r = a - (b mod x^nr)(q mod x^nr) mod x^nr.
 * Tree: ecfft_poly_inv_series needs next_pow2(2k - 1) leaves (k = 1: any tree); ecfft_poly_divrem with na >= nb >= 2 needs
 * N = next_pow2(max(2*nq - 1, nr + min(nq, nr) - 1)) leaves, nr = nb - 1; nb == 1 (scaling) and na < nb (copy) need no transform.
 * Else ECFFT_ERR_TREE_TOO_SMALL.  ECFFT_ERR_BAD_ARG: a NULL input, both outputs NULL, a zero length or count, a context that holds
 * no full tree, a byte count that would wrap — and a zero divisor leading coefficient / zero f[0] in any pair, which is checked
 * on the device.  Because of that check both calls are SYNCHRONOUS (like ecfft_degree): they return after the work on `stream`
 * is complete.  Memory and threading as for ecfft_poly_mul; temporaries are pooled (ecfft_ctx_trim). */
int ecfft_poly_inv_series(ecfft_ctx* ctx, const void* f, size_t nf, void* out, size_t k, size_t count, int mem, void* stream);
int ecfft_poly_divrem(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, void* q, void* r, size_t count, int mem, void* stream);
/* Multipoint evaluation at arbitrary points on the GPU (no reference counterpart: the crate evaluates only on its own leaves):
 * out[b*m + i] = f_b(points[i]) for `count` polynomials laid end to end, f: count x nf coefficients, points: m field elements
 * shared by all of them, out: count x m.  Points are arbitrary (repeated, zero, leaves of the tree).  out must not overlap the inputs.
 * Algorithm: the points in groups of G = max(64, next_pow2(nf)); the subproduct tree of every group (the vanish recursion, kept as
 * evaluations on T_2d for every node of d = 64 .. G/2 points, with each node's 1/rev(M) mod x^d), a remainder tree from f down to
 * nodes of 64 points (per level two lifts, two pointwise products and two EXITs), Horner at the leaves.
 * Cost: what m' = max(m, next_pow2(nf)) points cost; the tree part is shared by the count polynomials.
 * Tree: nf <= 64 needs no transform (any tree); otherwise next_pow2(nf) leaves (as ENTER of nf coefficients), else
 * ECFFT_ERR_TREE_TOO_SMALL.  ECFFT_ERR_BAD_ARG: a NULL input or output, nf, m or count 0, a context that holds no full tree, a byte
 * count that would wrap.  Every node is monic, so nothing fails on the data: the call is asynchronous on `stream`.  Memory, stream
 * and threading as for ecfft_poly_mul; temporaries are pooled (ecfft_ctx_trim). */
int ecfft_poly_eval_points(ecfft_ctx* ctx, const void* f, size_t nf, const void* points, size_t m, void* out, size_t count, int mem,
                           void* stream);
/* Interpolation from arbitrary points on the GPU, the inverse of ecfft_poly_eval_points (no reference counterpart: the crate
 * interpolates only on its own leaves, EXIT): out: count x m coefficients; f_b of degree < m with f_b(points[i]) = values[b*m + i].
 * points: m pairwise distinct field elements shared by all `count` value vectors (any values: 0, p - 1, leaves of the tree, in any
 * order); values: count x m, laid end to end.  out must not overlap the inputs.
 * Algorithm: Lagrange form f = sum_i c_i M / (x - x_i), c_i = y_i / M'(x_i), on one group of P = max(64, next_pow2(m)) points of
 * ecfft_poly_eval_points' subproduct tree, padded with the point 0 at weight 0 (the padded sum is x^(P-m) f): M'(x_i) by one remainder
 * descent, the numerators of every 64 points in one kernel, then per level N = N_l M_r + N_r M_l on the leaves of T_2d and one EXTEND,
 * one EXIT_P per value vector at the top.
 * Cost: the subproduct tree, one descent and one product of P coefficients, shared by the count vectors; per vector log2(P/64)
 * pointwise passes and EXTENDs and one EXIT.
 * Tree: m <= 64 needs no transform (any tree); otherwise next_pow2(m) leaves (as EXIT of m evaluations rounded up), else
 * ECFFT_ERR_TREE_TOO_SMALL.  ECFFT_ERR_BAD_ARG: a NULL input or output, m or count 0, a context that holds no full tree, a byte
 * count that would wrap — and two equal points, which is checked on the device (a zero weight denominator).  Because of that check
 * the call is SYNCHRONOUS (like ecfft_poly_divrem); the context keeps working after the error.  Memory, stream and threading as
 * for ecfft_poly_mul; temporaries are pooled (ecfft_ctx_trim). */
int ecfft_poly_interpolate(ecfft_ctx* ctx, const void* points, size_t m, const void* values, void* out, size_t count, int mem,
                           void* stream);

/* Modular powers and products of polynomials.
 *   ecfft_poly_pow_mod  <-> ecfft::utils::pow_mod(a, exp, modulus)                 src/utils.rs:194-211
 *   ecfft_poly_mul_mod  <-> div_rem(&a.naive_mul(&b), modulus), pow_mod's step     src/utils.rs:205, 207
 * Layout: `count` pairs laid end to end: a is count x na, b is count x nb, modulus is count x nm coefficients with
 * modulus[nm-1] != 0 in every pair; out is count x (nm - 1) coefficients, zero-padded above the true degree, fully reduced, in the
 * crate's form.  out must not overlap the inputs.
 * Exponent: `exp` is a HOST pointer whatever `mem` is: exp_bytes little-endian bytes (the layout of BigUint::to_bytes_le), one
 * exponent shared by all pairs.  High zero bytes are ignored; exp_bytes == 0 or an all-zero exponent gives the polynomial 1.
 * Lengths: na and nb may be any value >= 1.  An operand of at least nm coefficients is reduced first (the division of
 * ecfft_poly_divrem), a shorter one is zero-padded.
 * Cost, with d = nm - 1: d <= 64 runs the whole square-and-multiply of a pair in one workgroup (one launch, no transform).
 * Above that the reciprocal of the reversed modulus is computed ONCE per call and kept, with the modulus and the base, as
 * evaluations on N = next_pow2(2d - 1) leaves (3 count N elements); every squaring or multiply of the left-to-right scan is then
 * three forward lifts, three pointwise products and three batched EXITs of N, with no Newton step.  ecfft_poly_mul_mod is one
 * ecfft_poly_mul and one division (a fresh modulus has nothing to keep).
 * Tree: d <= 64 needs no transform for the power itself; otherwise next_pow2(2d - 1) leaves.  If na >= nm, also what
 * ecfft_poly_divrem(na, nm) needs.  ecfft_poly_mul_mod needs next_pow2(na + nb - 1) leaves and what ecfft_poly_divrem(na + nb - 1,
 * nm) needs.  Else ECFFT_ERR_TREE_TOO_SMALL.
 * ECFFT_ERR_BAD_ARG: a NULL input or output, exp == NULL with exp_bytes > 0, na, nb or count 0, nm < 2 (the residue would have no
 * coefficients), a context that holds no full tree, a byte count that would wrap — and a zero leading coefficient of the modulus
 * in any pair, which is checked on the device.  Because of that check both calls are SYNCHRONOUS (like ecfft_poly_divrem); the
 * context keeps working after the error.  Memory, stream and threading as for ecfft_poly_mul; temporaries are pooled
 * (ecfft_ctx_trim) and do not grow with the number of exponent bits. */
int ecfft_poly_pow_mod(ecfft_ctx* ctx, const void* a, size_t na, const void* exp, size_t exp_bytes, const void* modulus, size_t nm,
                       void* out, size_t count, int mem, void* stream);
int ecfft_poly_mul_mod(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, const void* modulus, size_t nm, void* out,
                       size_t count, int mem, void* stream);

/* Modular composition of polynomials: out_b = f_b(g_b) mod modulus_b.
 *   ecfft_poly_compose_mod <-> the step of distinct-degree factorisation, x^(p^(i+1)) = x^(p^i) composed with x^p mod f
 *                              (src/utils.rs:52-78), and Endomorphism * Endomorphism of examples/schoofs.rs:197-235
 * Layout: `count` triples laid end to end: f is count x nf (nf >= 1, possibly longer than the modulus), g is count x ng (ng >= 1),
 * modulus is count x nm (nm >= 2) with modulus[nm-1] != 0 in every triple; out is count x (nm - 1) coefficients, zero-padded
 * above the true degree, fully reduced, in the crate's form.  out must not overlap the inputs.  g of at least nm coefficients is
 * reduced first (the division of ecfft_poly_divrem).
 * ECFFT_COMPOSE_SMALL_MAX: nm up to which one workgroup runs Horner's scheme for a triple in LDS (nf - 1 schoolbook products; one
 * launch for all triples, no transform).
 * Above it, with d = nm - 1, k = ceil(sqrt(nf)) and k' = ceil(nf / k) (Brent-Kung): the reciprocal of the reversed modulus, the
 * modulus and g are kept as evaluations on N = next_pow2(2d - 1) leaves as in ecfft_poly_pow_mod; the baby steps g^t mod modulus,
 * t = 0 .. k, take k - 1 of its modular products; the k' chunk sums C_i = sum_t f[i k + t] g^t are one dense field matrix product of
 * nf d multiply-adds; the giant steps res = res g^k + C_i take k' - 1 products against the kept evaluations of g^k.  That is
 * (k - 1) + (k' - 1) modular products where Horner on ecfft_poly_mul_mod takes nf - 1; nf <= 2 runs none.
 * Memory: (k + 1 + k') count d + 4 count N elements of pooled temporaries beyond those of one modular product.
 * Tree: the rule of ecfft_poly_pow_mod, independent of nf: nm <= ECFFT_COMPOSE_SMALL_MAX needs no transform for the composition
 * itself; otherwise next_pow2(2d - 1) leaves.  If ng >= nm, also what ecfft_poly_divrem(ng, nm) needs.  Else
 * ECFFT_ERR_TREE_TOO_SMALL, checked before anything runs.
 * ECFFT_ERR_BAD_ARG: a NULL input or output, nf, ng or count 0, nm < 2, a context that holds no full tree, a byte count that would
 * wrap — and a zero leading coefficient of the modulus in any triple, which is checked on the device.  Because of that check the
 * call is SYNCHRONOUS (like ecfft_poly_pow_mod); the context keeps working after the error.  Memory, stream and threading as for
 * ecfft_poly_mul; temporaries are pooled (ecfft_ctx_trim). */
#define ECFFT_COMPOSE_SMALL_MAX 65   /* nm up to which a row is finished in one workgroup, on any tree */
int ecfft_poly_compose_mod(ecfft_ctx* ctx, const void* f, size_t nf, const void* g, size_t ng, const void* modulus, size_t nm, void* out,
                           size_t count, int mem, void* stream);

/* Greatest common divisors of polynomials.
 *   ecfft_poly_gcd   <-> ecfft::utils::gcd(a, b)                                    src/utils.rs:132-141
 *   ecfft_poly_xgcd  <-> ecfft::utils::xgcd(a, b) -> (s, t, gcd), a s + b t = gcd    src/utils.rs:147-182
 * Layout: `count` pairs laid end to end: a is count x na, b is count x nb coefficients in the crate's form.  Unlike
 * ecfft_poly_divrem the rows NEED NOT BE TRIMMED: high zero coefficients are allowed and either operand may be the zero
 * polynomial; the true degrees are found on the device (the natural inputs, x^p - x mod f or h^k - 1 mod f, have unknown degree).
 * Outputs: g is count x max(na, nb): the MONIC gcd, zero-padded above its degree, fully reduced.  `degrees` is a HOST pointer
 * whatever `mem` is, `count` entries, and may be NULL: deg g per pair, or -1 when a = b = 0 (then g = s = t = 0).
 * Zero operands: gcd(a, 0) = a / lc(a) and gcd(0, b) = b / lc(b).  The reference's gcd(0, b) returns 0 (src/utils.rs:133-134)
 * while its own xgcd(0, b) returns monic b (test_xgcd_with_zero_polynomial); both calls here follow xgcd and the textbook.
 * ecfft_poly_xgcd: s is count x max(nb - 1, 1), t is count x max(na - 1, 1), zero-padded; either may be NULL, g may not.  They
 * are the cofactors of the classical extended Euclidean algorithm, exactly what src/utils.rs:147-182 returns: when a/g or b/g is
 * not constant, the unique pair with deg s < deg b - deg g and deg t < deg a - deg g.  The degenerate cases are the algorithm's:
 *   b = 0:            s = 1/lc(a), t = 0
 *   a = 0 or b | a:   s = 0, t = 1/lc(b)
 * ECFFT_GCD_SMALL_MAX: max(na, nb) up to which a pair runs its whole remainder sequence in one workgroup (one launch for all
 * pairs, no transform).  Above it every pair is a half-GCD (Thull-Yap form, correct for quotients of any degree) on the bodies of
 * ecfft_poly_mul and ecfft_poly_divrem, O(M(n) log n), whose nodes of at most 512 (secp256k1) or 1024 (M31) coefficients are one
 * launch of the same kernel; the pairs then run one after another, since their degree sequences differ.
 * Tree: max(na, nb) <= ECFFT_GCD_SMALL_MAX needs no transform (any tree).  Otherwise, with n = max(na, nb), next_pow2(2 n - 1)
 * leaves, which is what next_pow2(2 n) gives for every n >= 2.  The rule is checked before anything runs and true degrees are
 * only known on the device, so it is the worst case over all inputs of that shape: a second operand of low degree makes the
 * first division step a quotient of almost n coefficients, whose reciprocal and product take next_pow2(2 nq - 1) leaves as in
 * ecfft_poly_divrem.  (The half-GCD matrix times the operands needs n + floor((n - 1) / 2) coefficients, every other product
 * less.)  Else ECFFT_ERR_TREE_TOO_SMALL.
 * ECFFT_ERR_BAD_ARG: a NULL input or g, na, nb or count 0, a context that holds no full tree, a byte count that would wrap.
 * Nothing fails on the data.  Both calls are SYNCHRONOUS: the recursion reads degrees back, and `degrees` is returned to the
 * host.  Outputs must not overlap the inputs.  Memory, stream and threading as for ecfft_poly_mul; temporaries are pooled
 * (ecfft_ctx_trim) and are handed back level by level, so they grow neither with the depth nor with repeated calls. */
#define ECFFT_GCD_SMALL_MAX 256
int ecfft_poly_gcd(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, void* g, int64_t* degrees, size_t count, int mem,
                   void* stream);
int ecfft_poly_xgcd(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, void* s, void* t, void* g, int64_t* degrees,
                    size_t count, int mem, void* stream);

/* The first row of the remainder sequence below a degree: the half-GCD's own product, which rational reconstruction, Pade
 * approximation, linear-recurrence synthesis (Berlekamp-Massey) and Gao's Reed-Solomon decoder are built on.  The reference has no
 * counterpart (its xgcd, src/utils.rs:147-182, runs the sequence to its end).
 * Layout as for ecfft_poly_xgcd: `count` pairs laid end to end, rows NEED NOT BE TRIMMED, either operand may be zero.
 * Definition, per pair: the classical sequence r_0 = a, r_1 = b, r_{i+1} = r_{i-1} - q_i r_i with (s_0, t_0) = (1, 0) and
 * (s_1, t_1) = (0, 1), so that r_i = s_i a + t_i b; a first quotient of 0 when deg a < deg b is the sequence's own swap
 * (r_2 = a); the sequence ends at its first zero row.  The output is the row with the smallest j >= 1 such that
 * deg r_j < stop, where deg 0 = -1, so such a row always exists (stop = 0 selects the zero row, whose t is +-a / gcd up to scale;
 * any stop above deg b selects row 1).
 * Normalisation: the row is scaled so that t is MONIC; where t = 0 — only the row (a, 1, 0), when deg a < stop <= deg b — so
 * that s is monic.  That makes the output unique and bit-exact: b = 0 gives (0, 0, 1), a = 0 with stop <= deg b gives (0, 1, 0).
 * Sizes: r is count x max(na, nb), s is count x nb, t is count x na, zero-padded, fully reduced, in the crate's form.  s may be
 * NULL; r and t may not.  `degrees` is a HOST pointer whatever `mem` is, count x 3 entries (deg r, deg s, deg t; -1 for a zero
 * polynomial), and may be NULL.
 * ECFFT_XGCD_PARTIAL_SMALL_MAX (= ECFFT_GCD_SMALL_MAX): max(na, nb) up to which all pairs are ONE launch, a pair per workgroup in
 * LDS, on any tree.  Above it the pairs run one after another on ecfft_poly_xgcd's bodies: half-GCD steps while their half-point
 * is not below stop, then one half-GCD of the operands divided by x^k, k = 2 stop - deg, whose half-point is stop itself; a pair
 * of at most 512 (secp256k1) or 1024 (M31) coefficients is finished by the workgroup kernel.  No step passes the wanted row.
 * Tree rule, errors, synchrony, temporaries and threading are exactly those of ecfft_poly_xgcd (with r and t in the place of g). */
#define ECFFT_XGCD_PARTIAL_SMALL_MAX 256
int ecfft_poly_xgcd_partial(ecfft_ctx* ctx, const void* a, size_t na, const void* b, size_t nb, size_t stop, void* r, void* s, void* t,
                            int64_t* degrees, size_t count, int mem, void* stream);

/* Reed-Solomon decoding with errors, the headline application of the ECFFT: the encoder is ecfft_poly_eval_points (or ENTER on the
 * tree's own points) and the erasure-only decoder ecfft_poly_interpolate.  The reference has no counterpart.
 * points: m PAIRWISE DISTINCT elements shared by all rows, as in ecfft_poly_interpolate (0 and leaves of the tree are points like
 * any other, in any order).  values: count x m received symbols.  1 <= k <= m.  message: count x k coefficients, fully reduced,
 * in the crate's form: row b holds the unique f of degree < k whose codeword (f(x_0), ..., f(x_{m-1})) differs from row b of values
 * in at most floor((m - k) / 2) positions.  `n_errors` is a HOST pointer whatever `mem` is, `count` entries, required: the number
 * of corrected positions, or -1 when no such f exists; the message row is then zero.
 * Method (Gao): g0 = prod (x - x_i), g1 = the interpolant of the row, (r, s, t) = the row of ecfft_poly_xgcd_partial(g0, g1) with
 * stop = ceil((m + k) / 2), f = r / t.  Decoding succeeds iff the division leaves no remainder and deg f < k; then t is the error
 * locator up to scale and n_errors = deg t.  Only the t cofactor is computed.
 * ECFFT_RS_SMALL_MAX: m up to which a row is decoded by ONE workgroup, everything in LDS, on any tree — the shape of practical
 * codes (length <= 255, many rows): one shared launch prepares g0, the Newton basis of the points and the inverse denominators
 * of the divided differences, one launch decodes all `count` rows.  Above it g0 and all interpolants come from the body of
 * ecfft_poly_interpolate at once and the rows then run one after another through the large regime of ecfft_poly_xgcd_partial
 * and the division body of ecfft_poly_divrem.
 * Tree: m <= ECFFT_RS_SMALL_MAX needs no transform (any tree).  Otherwise next_pow2(2 m + 1) leaves, which covers the
 * interpolation (next_pow2(m)) and the partial xgcd of (m + 1, m) coefficients; else ECFFT_ERR_TREE_TOO_SMALL, checked before
 * anything runs.
 * ECFFT_ERR_BAD_ARG: a NULL pointer, m, k or count 0, k > m, a context that holds no full tree, a byte count that would wrap —
 * and two equal points, which is checked on the device.  The call is SYNCHRONOUS; the context keeps working after an error.
 * Outputs must not overlap the inputs.  Memory, stream, threading and pooled temporaries as for ecfft_poly_gcd. */
#define ECFFT_RS_SMALL_MAX 255   /* code length m up to which a row is decoded by one workgroup, on any tree */
int ecfft_rs_decode(ecfft_ctx* ctx, const void* points, size_t m, const void* values, size_t k, void* message, int64_t* n_errors,
                    size_t count, int mem, void* stream);

/* The Reed-Solomon codec: a SYSTEMATIC encoder and a decoder for erasures mixed with errors.  The reference has no counterpart.
 * ecfft_rs_encode: points as in ecfft_rs_decode; data: count x k symbols; codeword: count x m symbols, row b =
 * (f_b(x_0), ..., f_b(x_{m-1})) for the unique f_b of degree < k with f_b(x_i) = data[b][i], i < k: the first k symbols are the
 * data, fully reduced, the other m - k the parity.  1 <= k <= m; k = m copies the data.  For m <= ECFFT_RS_SMALL_MAX the parity
 * is one fixed (m - k) x k matrix (the Lagrange basis of the first k points at the others, one shared launch) applied to every
 * row in one launch; above it the body of ecfft_poly_interpolate at the first k points and the body of ecfft_poly_eval_points at
 * the other m - k, for all rows at once.
 * Tree of the encoder: m <= ECFFT_RS_SMALL_MAX, or k <= 64, needs no transform (any tree); otherwise next_pow2(k) leaves, which
 * is what the interpolation at k points and the evaluation of k coefficients need; else ECFFT_ERR_TREE_TOO_SMALL, checked before
 * anything runs.
 * ecfft_rs_decode_erasures: `erased` is count x m bytes in the same memory kind as `values`, a non-zero byte marks a LOST symbol,
 * whose stored value is never read; NULL means no erasure anywhere.  With K the kept positions of a row and m' their number,
 * the row decodes to the unique f of degree < k whose codeword differs from `values` on K in at most floor((m' - k) / 2)
 * positions, and n_errors[b] (HOST pointer, required) is the number of those positions; where there is no such f, or m' < k,
 * n_errors[b] = -1 and the output row is zero.  The result is DEFINED, beyond the radius too, as that of ecfft_rs_decode on the
 * punctured code (the points and values of K): a row without erasures is byte for byte what ecfft_rs_decode returns.
 * out_form: ECFFT_RS_OUT_COEFFS: out is count x k coefficients of f, as ecfft_rs_decode's message.  ECFFT_RS_OUT_CODEWORD: out is
 * count x m symbols, f at all m points: the erased positions are filled in and the first k symbols are the corrected data of a
 * code made by ecfft_rs_encode.
 * Method: for m <= ECFFT_RS_SMALL_MAX the shared launch of ecfft_rs_decode over ALL m points and one launch for all rows, a
 * workgroup per row: the interpolant over all points with the erased symbols read as 0 is congruent to the interpolant over K
 * modulo g0' = prod_{i in K} (x - x_i), so only the first operand of the remainder loop is the row's own.  Above it the rows
 * without erasure take the path of ecfft_rs_decode together and a row with erasures is compacted on the device and decoded as a
 * code of length m'.  Tree of the decoder: that of ecfft_rs_decode.
 * ECFFT_ERR_BAD_ARG: as ecfft_rs_decode; an unknown out_form; two equal points among ALL m, erased or not, for both calls.  Both
 * calls are SYNCHRONOUS; the context keeps working after an error.  Outputs must not overlap the inputs.  Memory, stream,
 * threading and pooled temporaries as for ecfft_rs_decode. */
#define ECFFT_RS_OUT_COEFFS   0   /* out: count x k coefficients of f, as ecfft_rs_decode's message */
#define ECFFT_RS_OUT_CODEWORD 1   /* out: count x m symbols f(x_0..x_{m-1}); the first k are the data of a systematic code */
int ecfft_rs_encode(ecfft_ctx* ctx, const void* points, size_t m, const void* data, size_t k, void* codeword, size_t count, int mem,
                    void* stream);
int ecfft_rs_decode_erasures(ecfft_ctx* ctx, const void* points, size_t m, const void* values, const uint8_t* erased, size_t k, void* out,
                             int out_form, int64_t* n_errors, size_t count, int mem, void* stream);

/* Linear recurrences: the minimal polynomial of a sequence (what Berlekamp-Massey computes) and its terms at a huge index.  The
 * reference has no counterpart.
 * A row is N elements s_0 .. s_{N-1}.  Its linear complexity L is the smallest L >= 0 with c_0 .. c_{L-1} such that
 * s_{i+L} + sum_{j<L} c_j s_{i+j} = 0 for all 0 <= i < N - L; L = 0 iff the row is zero.  Where 2 L <= N the monic
 * C(x) = x^L + sum c_j x^j is unique, the MINIMAL POLYNOMIAL; where 2 L > N it is not, and the row is reported UNDETERMINED.
 * ecfft_seq_min_poly: seq is count x N elements in the crate's form, any values.  min_poly is count x (N / 2 + 1) coefficients:
 * row b holds C_b with its leading 1 at index L_b and zero above, fully reduced; an undetermined row is zero.  `orders` is a HOST
 * pointer whatever `mem` is, `count` entries, required: L_b, or -1 for an undetermined row.  N >= 1 (N = 1: 0 for a zero term, -1
 * otherwise).  Nothing fails on the data, and the output is unique and bit-exact.
 * Method (MCA Alg. 12.9): with h = sum s_i x^i (the row as it stands) and (r, ., t) the row of ecfft_poly_xgcd_partial(x^N, h)
 * with stop = N / 2, d = max(1 + deg r, deg t): the row is determined iff t(0) != 0 and 2 d <= N, and then L = d and
 * C = x^d t(1/x) / t(0).  Only the t cofactor is computed, x^N is never staged per row, and verdict, inversion and reversal
 * happen on the device.
 * ECFFT_SEQ_SMALL_MAX: N up to which a row is ONE workgroup, everything in LDS, all rows in one launch, on any tree.  Above it
 * the rows run one after another through the large regime of ecfft_poly_xgcd_partial against one shared x^N, each finished by a
 * small kernel; the verdicts are read back once.
 * Tree: N <= ECFFT_SEQ_SMALL_MAX needs no transform (any tree).  Otherwise the rule of ecfft_poly_xgcd_partial for (N + 1, N)
 * coefficients, next_pow2(2 N + 1) leaves; else ECFFT_ERR_TREE_TOO_SMALL, checked before anything runs.
 * ecfft_seq_nth_term: char_poly is count x nc coefficients, nc >= 2, of polynomials C_b of degree L = nc - 1 whose leading
 * coefficient is non-zero (monic not required); init is count x L initial terms s_0 .. s_{L-1} of the sequences with
 * sum_{j<=L} c_j s_{i+j} = 0.  `index` is `index_bytes` little-endian HOST bytes, one K >= 0 shared by all rows (high zero bytes
 * are ignored; index may be NULL when index_bytes is 0: K = 0).  out is count x nout, nout >= 1: s_K .. s_{K+nout-1} of every row,
 * fully reduced; K < L returns initial terms themselves.
 * Method (Fiduccia): u = x^K mod C, s_K = sum_{j<L} u_j s_j, and the next term takes x u mod C: one power and nout L
 * multiply-adds per row.  ECFFT_SEQ_TERM_SMALL_MAX: nc up to which a row is ONE workgroup, all rows in one launch, on any tree.
 * Above it the kept-modulus power of ecfft_poly_pow_mod runs on the base x for all rows at once, then one launch takes the terms.
 * Tree: nc <= ECFFT_SEQ_TERM_SMALL_MAX any tree; otherwise the rule of ecfft_poly_pow_mod with nm = nc, next_pow2(2 (nc - 1) - 1)
 * leaves; else ECFFT_ERR_TREE_TOO_SMALL, checked before anything runs.
 * ECFFT_ERR_BAD_ARG, both calls: a NULL pointer (index with index_bytes > 0), N, nout or count 0, nc < 2, a context that holds no
 * full tree, a byte count that would wrap — and for ecfft_seq_nth_term a zero leading coefficient of some C_b, which is checked on
 * the device.  Both calls are SYNCHRONOUS; the context keeps working after an error.  Outputs must not overlap the inputs.
 * Memory, stream, threading and pooled temporaries as for ecfft_poly_gcd. */
#define ECFFT_SEQ_SMALL_MAX      255  /* terms N up to which a row is one workgroup, on any tree (x^N has ECFFT_GCD_SMALL_MAX coefficients) */
#define ECFFT_SEQ_TERM_SMALL_MAX  65  /* nc up to which the terms of a row are one workgroup, on any tree (= ECFFT_COMPOSE_SMALL_MAX) */
int ecfft_seq_min_poly(ecfft_ctx* ctx, const void* seq, size_t n_terms, void* min_poly, int64_t* orders, size_t count, int mem,
                       void* stream);
int ecfft_seq_nth_term(ecfft_ctx* ctx, const void* char_poly, size_t nc, const void* init, const void* index, size_t index_bytes,
                       void* out, size_t nout, size_t count, int mem, void* stream);

/* Roots of polynomials in the field.
 *   ecfft_poly_find_roots <-> ecfft::utils::find_roots(poly)                        src/utils.rs:25-44
 * Layout: f is count x nf coefficients in the crate's form; as in ecfft_poly_gcd the rows NEED NOT BE TRIMMED.  roots is
 * count x (nf - 1) elements: row b holds the n_roots[b] DISTINCT roots of f_b in the field in ascending order of their
 * standard-form integer (ark's Ord on Fp, what roots.sort() in the reference produces), fully reduced, in the crate's form, the
 * rest of the row zero.  roots may be NULL only when nf == 1 and must not overlap f.  `n_roots` is a HOST pointer whatever `mem`
 * is, `count` entries, required: a non-zero constant gives 0; the zero polynomial gives -1 and a zero row (every element is a
 * root; the reference panics there, at assert_eq!(1, factor.degree())).
 * Method (both fields have odd p, which the exponent (p - 1) / 2 below relies on):
 *   g = gcd(f, x^p - x mod f) is the product of the distinct linear factors of f WHATEVER the multiplicities are, because
 *   x^p - x is the squarefree product of all x - a.  The reference's square_free_factors and the higher degrees of its
 *   distinct_degree_factors are therefore not needed to find roots.  A monic product h of e >= 2 distinct linear factors is split
 *   by a shift c: w = (x + c)^((p-1)/2) mod h, u = gcd(h, w - 1), v = h / u, a success when 0 < deg u < e; x + a yields -a.  The
 *   shifts are the plain integers 1, 2, 3, ... from an attempt counter incremented after every attempt: no randomness, and since
 *   the set of roots does not depend on the shifts the result is deterministic and bit-exact.
 * ECFFT_ROOTS_SMALL_MAX: nf up to which a polynomial is finished by one workgroup, everything in LDS; all `count` rows are ONE
 * launch (plus the ordering).  Above it the polynomials run one after another: g on the bodies of ecfft_poly_pow_mod and
 * ecfft_poly_gcd, then rounds in which all pending factors of more than 64 roots share the launches of one modular power, until
 * every factor has at most 64 roots; those are finished by one launch of the same workgroup kernel.
 * A factor that fails 64 shifts in a row (chance below 2^-63 for distinct roots; the bound keeps a defect from spinning) ends the
 * call with ECFFT_ERR_HIP.
 * Tree: nf <= ECFFT_ROOTS_SMALL_MAX needs no transform (any tree).  Otherwise next_pow2(2 nf - 1) leaves, ecfft_poly_gcd's rule for
 * rows of nf, which covers the modular power (next_pow2(2d - 1), d <= nf - 1) and every later, smaller step; it is checked on the
 * row length before anything runs.  Else ECFFT_ERR_TREE_TOO_SMALL.
 * ECFFT_ERR_BAD_ARG: NULL f or n_roots, NULL roots with nf > 1, nf or count 0, a context that holds no full tree, a byte count
 * that would wrap.  Nothing fails on the data.  The call is SYNCHRONOUS.  Memory, stream, threading and pooled temporaries as
 * for ecfft_poly_gcd. */
#define ECFFT_ROOTS_SMALL_MAX 65     /* nf up to which a polynomial is finished in one workgroup, on any tree */
int ecfft_poly_find_roots(ecfft_ctx* ctx, const void* f, size_t nf, void* roots, int64_t* n_roots, size_t count, int mem, void* stream);

/* The squarefree part and the distinct-degree factors of polynomials over the field: the deterministic core of factorisation.
 *   ecfft_poly_squarefree      <-> ecfft::utils::square_free_factors(poly), made monic        src/utils.rs:46-50
 *   ecfft_poly_distinct_degree <-> ecfft::utils::distinct_degree_factors(poly), see below     src/utils.rs:52-78
 * Layout: f is count x nf coefficients in the crate's form; the rows NEED NOT BE TRIMMED and any non-zero leading coefficient is
 * accepted.  Outputs are fully reduced, in the crate's form, and must not overlap f.  `degrees` is a HOST pointer whatever `mem` is.
 * ecfft_poly_squarefree: out is count x nf; row b holds the monic s_b = f_b / gcd(f_b, f_b'), the product of the distinct monic
 *   irreducible factors of f_b, zero-padded.  degrees[b] = deg s_b: 0 (s = 1) for a non-zero constant, -1 for the zero polynomial
 *   (a zero row).  Both fields have p larger than any degree a tree holds, so f' = 0 only for constants: there is no p-th-power case.
 * ecfft_poly_distinct_degree (any multiplicities: it takes the squarefree part first): with nd = max(nf - 1, 1), degrees is
 *   count x nd and degrees[b][d-1] = deg g_d, where g_d is the product of all monic irreducible factors of degree d of f_b: d times
 *   their number, 0 where there are none.  The zero polynomial gives degrees[b][0] = -1 and zeros; a non-zero constant all zeros.
 *   factors is count x nd elements: row b holds the g_d with deg g_d > 0 in ascending d, laid end to end, each as its LOW deg g_d
 *   coefficients (the leading 1 is implied); they sum to deg s_b <= nf - 1, and the rest of the row is zero.
 * Method: h_1 = x^p mod s; for i = 1, 2, ...: g_i = gcd(f*, h_i - x) with every g_j, j < i, already divided out of f* (f* = s at
 *   first), and h_(i+1) = x^(p^(i+1)) mod s = h_i(h_1) mod s, a modular composition (ecfft_poly_compose_mod) or the power h_i^p,
 *   whichever takes fewer modular products.  Once deg f* < 2(i + 1), what is left is irreducible of its own degree.  There is no
 *   randomness and the outputs are defined mathematically, so they are bit-exact.  The reference computes pow_mod(x^p, i), which
 *   is x^(p i) and not x^(p^i): the two agree at i = 1 only, the one degree its own find_roots uses; this call returns the g_d of
 *   the definition above for every d.
 * ECFFT_DDF_SMALL_MAX: nf up to which a polynomial is finished by one workgroup, everything in LDS; all `count` rows are ONE
 * launch.  Above it the polynomials run one after another on the bodies of ecfft_poly_gcd, ecfft_poly_divrem, ecfft_poly_pow_mod
 * and ecfft_poly_compose_mod with the modulus s, x^p mod s and its baby steps kept for the whole row; a polynomial whose true
 * length, or whose squarefree part, fits the workgroup kernel goes there.
 * Tree: nf <= ECFFT_DDF_SMALL_MAX needs no transform (any tree).  Otherwise the rule of ecfft_poly_find_roots, next_pow2(2 nf - 1)
 * leaves, checked on the row length before anything runs.  Else ECFFT_ERR_TREE_TOO_SMALL.
 * ECFFT_ERR_BAD_ARG: a NULL pointer, nf or count 0, a context that holds no full tree, a byte count that would wrap.  Nothing
 * fails on the data.  Both calls are SYNCHRONOUS.  Memory, stream, threading and pooled temporaries as for ecfft_poly_gcd. */
#define ECFFT_DDF_SMALL_MAX 65       /* coefficients per row that one workgroup finishes, any tree */
int ecfft_poly_squarefree(ecfft_ctx* ctx, const void* f, size_t nf, void* out, int64_t* degrees, size_t count, int mem, void* stream);
int ecfft_poly_distinct_degree(ecfft_ctx* ctx, const void* f, size_t nf, void* factors, int64_t* degrees, size_t count, int mem,
                               void* stream);

/* Equal-degree splitting: the last step of factorisation over the field.
 *   ecfft_poly_equal_degree <-> ecfft::utils::equal_degree_factorization(poly, d)      src/utils.rs:82-113
 * Layout: g is count x ng coefficients in the crate's form; the rows NEED NOT BE TRIMMED and any non-zero leading coefficient is
 * accepted (the row is made monic).  d >= 1 is one degree for the whole call.  factors is count x max(ng - 1, 1) elements: row b
 * holds the n_factors[b] monic irreducible factors of degree d of g_b, each as its LOW d coefficients (the leading 1 is implied,
 * the layout of ecfft_poly_distinct_degree's g_d), laid end to end, fully reduced, in the crate's form, the rest of the row zero.
 * factors must not overlap g.
 * Order: ascending under lexicographic comparison of (c_0, c_1, ..., c_(d-1)) as standard-form integers, c_0 the most significant
 * (what Python's sorted gives on low-to-high coefficient lists).
 * `n_factors` is a HOST pointer whatever `mem` is, `count` entries: the zero polynomial gives -1 and a zero row, a non-zero
 * constant 0, a true degree that is not a multiple of d gives -2 and a zero row; nothing fails on that.
 * Precondition: g_b is squarefree and all its irreducible factors have degree d, which is what ecfft_poly_distinct_degree returns
 * once the leading 1 is appended.  On any other input the factors are unspecified, but every loop is still bounded.
 * Method (both fields have odd p): with h_i = x^(p^i) mod g, (x + c)^(p^i) = h_i + c, and (p^d - 1)/2 = (1 + p + ... + p^(d-1))
 *   (p - 1)/2; so with the norm N_c = prod_{i<d} (h_i + c) mod g the splitting element of Cantor-Zassenhaus is w =
 *   (x + c)^((p^d - 1)/2) = N_c^((p-1)/2).  Modulo each irreducible factor N_c lies in F_p, so w is 0 or +-1 there, and
 *   u = gcd(h, w - 1), v = h / u split a divisor h of g whenever two of its factors get different quadratic characters.  The h_i
 *   do not depend on c: h_1 is one power x^p and h_2 .. h_(d-1) are d - 2 Frobenius iterates, taken once per g as
 *   ecfft_poly_distinct_degree takes them.  An attempt then costs d - 1 modular products and one power with the exponent
 *   (p - 1)/2, where the reference's (x + c)^((p^d - 1)/2) has a d times longer exponent.  The shifts are the plain integers
 *   1, 2, 3, ... from an attempt counter: no randomness, and since the set of factors does not depend on the shifts and the order
 *   is fixed the result is deterministic and bit-exact.
 * ECFFT_EDF_SMALL_MAX: ng up to which a polynomial is finished by one workgroup; all `count` rows are ONE launch (plus the
 * ordering).  Above it the polynomials run one after another: the modulus g is kept once, then rounds in which all pending factors
 * of degree above 64 share one norm and the launches of one modular power, until every factor has degree d or at most 64; those
 * are finished by one launch of the same workgroup kernel.
 * Memory beyond the rows: the small regime takes (d - 1)(ng - 1) pooled elements per row of a launch (at most 65536 rows) for the
 * h_i when 2 d <= ng - 1, none otherwise; the large regime 4 N for the kept modulus, (d - 1) n for the h_i, the composition's baby
 * steps and buffers of 2 n.  An allocation that fails ends the call with ECFFT_ERR_HIP.
 * A factor that fails 64 shifts in a row (for a valid input the chance is below 2^-63; the bound keeps a defect or an input outside
 * the precondition from spinning) ends the call with ECFFT_ERR_HIP.
 * Tree: ng <= ECFFT_EDF_SMALL_MAX needs no transform (any tree).  Otherwise the rule of ecfft_poly_find_roots, next_pow2(2 ng - 1)
 * leaves, checked on the row length before anything runs.  Else ECFFT_ERR_TREE_TOO_SMALL.
 * ECFFT_ERR_BAD_ARG: a NULL pointer, ng, d or count 0, a context that holds no full tree, a byte count that would wrap.  The call is
 * SYNCHRONOUS.  Memory, stream, threading and pooled temporaries as for ecfft_poly_gcd. */
#define ECFFT_EDF_SMALL_MAX 65       /* coefficients per row that one workgroup finishes, any tree */
int ecfft_poly_equal_degree(ecfft_ctx* ctx, const void* g, size_t ng, size_t d, void* factors, int64_t* n_factors, size_t count, int mem,
                            void* stream);

/* Factorisation over the field in one call: f = lead prod_i a_i^i (squarefree decomposition) and f = lead prod_j q_j^e_j.
 *   ecfft_poly_squarefree_decompose <-> no reference item: ecfft::utils::square_free_factors (src/utils.rs:46-50) returns
 *                                       f / gcd(f, f') only; this is Yun's decomposition, which keeps the multiplicities
 *   ecfft_poly_factor               <-> square_free_factors, distinct_degree_factors and equal_degree_factorization strung
 *                                       together as find_roots strings them (src/utils.rs:25-113), for every degree and with the
 *                                       multiplicities the reference drops
 * Layout: f is count x nf coefficients in the crate's form; the rows NEED NOT BE TRIMMED and any non-zero leading coefficient is
 * accepted.  nd = max(nf - 1, 1).  `lead` may be NULL; otherwise it is `count` elements in the memory `mem` names: the leading
 * coefficient of f_b, 0 for the zero polynomial.  Element outputs are fully reduced, in the crate's form, zero-padded, and must not
 * overlap f.  The int64 outputs are HOST pointers whatever `mem` is.
 * ecfft_poly_squarefree_decompose: f_b = lead prod_i a_i^i with the a_i monic, squarefree and pairwise coprime.  degrees is
 *   count x nd and degrees[b][i-1] = deg a_i (i never exceeds deg f <= nd); the zero polynomial gives -1, 0, 0, ..., a non-zero
 *   constant all zeros.  parts is count x nd elements: row b holds the a_i of positive degree in ascending i, each as its LOW
 *   deg a_i coefficients (the leading 1 is implied: the layout of ecfft_poly_distinct_degree's g_d); sum i deg a_i = deg f_b.
 * ecfft_poly_factor: f_b = lead prod_j q_j^e_j over the distinct monic irreducible q_j.  n_factors[b] is their number: -1 for the
 *   zero polynomial, 0 for a non-zero constant.  fdeg and fmult are count x nd: entry j < n_factors[b] holds deg q_j and e_j, the
 *   rest are 0.  factors is count x nd elements: the q_j laid end to end, each as its low deg q_j coefficients.
 *   Order: ascending (e_j, deg q_j, then the lexicographic order of ecfft_poly_equal_degree).  Every group (multiplicity, degree)
 *   is one contiguous, ranked output of the equal-degree step.  Nothing in the result depends on the shifts, so it is deterministic
 *   and bit-exact.
 * Method: with f made monic, a_0 = gcd(f, f'), b = f / a_0, c = f' / a_0, d = c - b'; for i = 1, 2, ... while deg b > 0:
 *   a_i = gcd(b, d) (gcd(b, 0) = b), b <- b / a_i, c <- d / a_i, d <- c - b' (Yun).  Both fields have p larger than any degree a
 *   tree holds, so derivatives vanish for constants only and there is no p-th-power case; a squarefree f costs one iteration.
 *   ecfft_poly_factor then takes every a_i through the steps of ecfft_poly_distinct_degree and ecfft_poly_equal_degree.
 * ECFFT_FACTOR_SMALL_MAX: nf up to which everything is done by workgroup kernels, one workgroup per row or part, everything in
 *   LDS: one launch for Yun's loop over all rows, one for the distinct-degree step over all parts of all rows, one equal-degree
 *   launch per distinct degree that needs splitting (and its ordering), and one scatter; the number of launches and of read-backs
 *   does not depend on `count`.  Above it the rows run one after another on the bodies of ecfft_poly_gcd and ecfft_poly_divrem; a
 *   row whose true length fits goes to the workgroup kernels, parts of degree above 64 run the large regimes of the two calls
 *   above, and the parts of degree at most 64 of ALL rows share the launches of the small regime at the end of the call.
 * A factor that fails 64 shifts in a row (chance below 2^-63; the bound keeps a defect from spinning) ends ecfft_poly_factor with
 * ECFFT_ERR_HIP; the context keeps working.
 * Tree: nf <= ECFFT_FACTOR_SMALL_MAX needs no transform (any tree).  Otherwise the rule of ecfft_poly_find_roots, next_pow2(2 nf - 1)
 * leaves, checked on the row length before anything runs.  Else ECFFT_ERR_TREE_TOO_SMALL.
 * ECFFT_ERR_BAD_ARG: NULL f, parts / factors or host array, nf or count 0, a context that holds no full tree, a byte count that
 * would wrap.  Both calls are SYNCHRONOUS.  Memory, stream, threading and pooled temporaries as for ecfft_poly_gcd. */
#define ECFFT_FACTOR_SMALL_MAX 65   /* coefficients per row finished by workgroup kernels on any tree */
int ecfft_poly_squarefree_decompose(ecfft_ctx* ctx, const void* f, size_t nf, void* parts, int64_t* degrees, void* lead, size_t count,
                                    int mem, void* stream);
int ecfft_poly_factor(ecfft_ctx* ctx, const void* f, size_t nf, void* factors, int64_t* fdeg, int64_t* fmult, int64_t* n_factors,
                      void* lead, size_t count, int mem, void* stream);

/* Division polynomials of short Weierstrass curves y^2 = x^3 + A x + B on the GPU.
 *   ecfft_division_polynomial <-> division_polynomial(n, &curve)                          examples/schoofs.rs:368-431
 * A and B are `count` elements each in the crate's form (host or device memory per `mem`); out is count x L(n) coefficients,
 * low to high, in the crate's form, fully reduced and NOT made monic: psi_n in the reference's convention, where the factor
 * 2y of an even index is removed (psi_2 -> 1, psi_4 -> the sextic with leading coefficient 2).
 *   L(n) = (n^2 - 1)/2 + 1 for odd n; (n^2 - 4)/2 + 1 for even n >= 2; L(0) = L(1) = 1.  The leading coefficient is n for odd n
 *   and n/2 for even n; psi_0 = 0.
 * Method: a host driver on the products of ecfft_poly_mul, batched over `count`: only the O(log n) indices the recurrence
 * reaches are computed (m - 2 .. m + 2 of m = k / 2, downwards from n), each once (the reference recurses exponentially).
 * Tree: n <= 4 are closed forms and need no transform (any tree).  Otherwise next_pow2(L(n)) leaves: every product of the
 * recurrence is a factor of one term of a psi_k with k <= n, so none has more than L(n) coefficients, and the last ones have
 * exactly L(n).  Checked before anything runs, else ECFFT_ERR_TREE_TOO_SMALL.
 * ECFFT_ERR_BAD_ARG: a NULL pointer, count 0, n above ECFFT_SCHOOF_MAX_L, a context that holds no full tree, a byte count that
 * would wrap.  Nothing fails on the data (a singular curve has division polynomials too): the call is asynchronous on `stream`
 * like ecfft_poly_mul.  Memory, stream, threading and pooled temporaries as for ecfft_poly_mul. */
#define ECFFT_SCHOOF_MAX_L 199       /* the largest index and the largest prime l (the last entry of the reference's table) */
int ecfft_division_polynomial(ecfft_ctx* ctx, const void* A, const void* B, size_t n, void* out, size_t count, int mem, void* stream);

/* Schoof's algorithm, one prime at a time: the trace of Frobenius of a curve modulo a small prime.
 *   ecfft_curve_trace_mod <-> frobenius_trace_mod_l(l, curve, ring) and has_even_order(curve)      examples/schoofs.rs:76-138, 345-366
 * Curves are short Weierstrass pairs y^2 = x^3 + A x + B, `count` of them per call: A and B are `count` elements each in the
 * crate's form, in host or device memory per `mem`.  `t_out` is a HOST pointer whatever `mem` is, `count` entries: t mod l in
 * [0, l) where #E(F_p) = p + 1 - t.  A singular curve (4 A^3 + 27 B^2 = 0) gets -1 in its entry; nothing fails on it.
 * Valid l: 2, and the odd primes up to ECFFT_SCHOOF_MAX_L = 199; anything else is ECFFT_ERR_BAD_ARG.
 * Method: l = 2: t is even iff x^3 + A x + B has a root, i.e. gcd(x^p - x mod f, f) != 1.  Odd l: in the ring F_p[x]/(h), at
 *   first with h = psi_l made monic (the l-th division polynomial, (l^2 - 1)/2 + 1 coefficients, built from the closed forms of
 *   psi_3 and psi_4 and the reference's recurrence, schoofs.rs:368-431), with f = x^3 + A x + B:
 *     pi = (x^p, f^((p-1)/2) y); pi^2 either as the composition (pi_a(pi_a), pi_b(pi_a) pi_b) or as the powers (pi_a^p,
 *     pi_b^(p+1)), whichever takes fewer modular products at the degree of h (d - 1 against bits + popcount(p) - 2 per
 *     coordinate); Q = [p mod l](x, y); E = pi^2 + Q; then the j in [1, l) with j pi = E, taking j pi from (j - 1) pi by one sum.
 *     E = O, or no j, is t = 0.  The group law is the reference's Add (schoofs.rs:237-273) plus the case it lacks: a1 = a2 with
 *     b1 = -b2 is the point at infinity.  A denominator that is not invertible replaces h by the proper factor gcd(denominator,
 *     h) and the attempt starts over; with a1 = a2 and b1 != +-b2 the factor is gcd(b1 - b2, h), else gcd(b1 + b2, h).  Degrees
 *     fall strictly, so the attempts are bounded.  Every non-zero point of E[l] satisfies the same characteristic equation, so the
 *     residue is defined by the curve alone and does not depend on where the splits fall.
 *   There is NO shortcut on a modulus of degree 1 (the reference's, schoofs.rs:86-95, takes a root of psi_l for a rational point
 *   of order l; its y may lie in F_p^2, and then the eigenvalue is -1, not +1).
 * ECFFT_SCHOOF_SMALL_MAX: coefficients of a modulus up to which ONE workgroup finishes a curve (k_schoof_small).  Where psi_l fits
 * (l <= 11) all `count` curves are ONE launch, psi_l is built in the kernel, and the call needs no transform (any tree).
 * Above it (l = 13 .. 199) the curves run one after another on a host driver: psi_l from ecfft_division_polynomial's driver,
 * made monic; the modulus kept once per attempt as ecfft_poly_pow_mod keeps it; products, powers and the kept composition (one
 * set of baby steps of pi_a shared by both coordinates of pi^2) on it; inverses as the cofactor of ecfft_poly_xgcd's bodies.
 * After a split the new modulus is kept again, and a factor of at most ECFFT_SCHOOF_SMALL_MAX coefficients is handed to the
 * workgroup kernel.
 * Tree: l <= 11 none.  Otherwise next_pow2(2 L(l) - 1) leaves, ecfft_poly_gcd's rule on rows of L(l) coefficients, which covers
 * every product on the modulus and the driver of psi_l; checked before anything runs, else ECFFT_ERR_TREE_TOO_SMALL.
 * ECFFT_ERR_BAD_ARG: a NULL pointer, count 0, an l that is not valid, a context that holds no full tree, a byte count that would
 * wrap.  ECFFT_ERR_HIP also reports a sum that the group law excludes (a defect, not a property of the data).  The call is
 * SYNCHRONOUS.  Memory, stream, threading and pooled temporaries as for ecfft_poly_gcd. */
#define ECFFT_SCHOOF_SMALL_MAX 65    /* coefficients of a modulus that one workgroup finishes, any tree */
int ecfft_curve_trace_mod(ecfft_ctx* ctx, const void* A, const void* B, size_t l, int64_t* t_out, size_t count, int mem, void* stream);

/* The number of points of a curve: Schoof's algorithm.
 *   ecfft_curve_cardinality <-> cardinality(curve)                                          examples/schoofs.rs:30-71
 * A and B as for ecfft_curve_trace_mod.  `order` is a HOST pointer of count x ECFFT_ORDER_BYTES little-endian bytes: #E(F_p) of
 * curve b (it can exceed 2^256 for secp256k1); 0 for a singular curve.  `traces` (a HOST pointer, may be NULL) receives count x
 * (number of primes used) residues, row b = t mod 2, 3, 5, ... of curve b (-1 in every entry of a singular curve).
 * The primes are l = 2, 3, 5, ... until their product m exceeds 4 sqrt(p), decided exactly as m^2 > 16 p: l <= 17 (7 primes) for
 * M31, l <= 103 (27 primes) for secp256k1.  Per prime one ecfft_curve_trace_mod over all curves; then on the host the incremental
 * CRT of schoofs.rs:52-70 with the representative of t in (-m/2, m/2] and #E = p + 1 - t.
 * Tree: the rule of the largest l: 512 leaves for M31, 2^14 for secp256k1; checked before anything runs.
 * Errors and everything else as ecfft_curve_trace_mod.  SYNCHRONOUS. */
#define ECFFT_ORDER_BYTES 40
int ecfft_curve_cardinality(ecfft_ctx* ctx, const void* A, const void* B, void* order, int64_t* traces, size_t count, int mem, void* stream);

/* The remaining FFTree algorithms, composed from the same GPU kernels.  Synchronous.
 *   ecfft_mextend         <-> FFTree::mextend(&self, &[F], Moiety)      src/fftree.rs:138-141
 *   ecfft_redc            <-> FFTree::redc_z0 / redc_z1(&self, evals, a)  src/fftree.rs:264-275  (moiety S0 / S1)
 *   ecfft_modular_reduce  <-> FFTree::modular_reduce(&self, evals, a, c)  src/fftree.rs:286-289
 *   ecfft_vanish          <-> FFTree::vanish(&self, domain) -> 2*nd evals  src/fftree.rs:313-316
 *   ecfft_degree          <-> FFTree::degree(&self, evals) -> usize        src/fftree.rs:195-198 */
int ecfft_mextend(ecfft_ctx* ctx, const void* in, void* out, size_t e, int moiety, size_t count, int mem, void* stream);
int ecfft_redc(ecfft_ctx* ctx, const void* evals, const void* a, void* out, size_t n, int moiety, int mem, void* stream);
int ecfft_modular_reduce(ecfft_ctx* ctx, const void* evals, const void* a, const void* c, void* out, size_t n, int mem, void* stream);
int ecfft_vanish(ecfft_ctx* ctx, const void* domain, void* out, size_t nd, int mem, void* stream);
int ecfft_degree(ecfft_ctx* ctx, const void* evals, size_t n, int mem, void* stream, size_t* degree);

/* Building blocks of ONE EXTEND of e evaluations (tree T_{2e}) split over P = 2^log_p GPUs, for hosts that drive the
 * exchanges themselves (ecfft_extend_sharded below does the whole thing); see DESIGN.md section 8.  No reference counterpart (the reference is
 * single-process); together they compute exactly FFTree::extend (src/fftree.rs:123-126).
 *   ecfft_extend_top_cyclic : buf = the rank's CYCLIC shard (local j' <-> global j'*P + rank, e/P elements).
 *                             recombine = 0: multiply by 1/W_src, then decompose stages 0..log_p-1;
 *                             recombine = 1: recombine stages log_p-1..0, then multiply by W_target.
 *   ecfft_extend_local_block: buf = the rank's BLOCK shard (global [rank*e/P, (rank+1)*e/P)): every stage
 *                             k >= log_p, decompose then recombine, with the fused single-GPU kernels. */
int ecfft_extend_top_cyclic(ecfft_ctx* ctx, void* buf, size_t e, int moiety, unsigned log_p, unsigned rank, int recombine,
                            int mem, void* stream);
int ecfft_extend_local_block(ecfft_ctx* ctx, void* buf, size_t e, int moiety, unsigned log_p, int mem, void* stream);

/* ---- ONE transform split over several GPUs, one process per GPU (no reference counterpart: the reference is single
 * threaded; together the ranks compute exactly FFTree::extend / enter / exit, src/fftree.rs:123-126, 164-167, 227-230).
 * The loops being split are the butterfly stage loops src/fftree.rs:83-97 and 104-118: stage k pairs (i, i + e >> (k+1)), so
 * stages k >= log2 P are local when the vector is BLOCK distributed (rank r holds [r*len/P, (r+1)*len/P)) and stages
 * k < log2 P are local when it is CYCLIC (position j on rank j mod P); an all-to-all inside the group switches between the
 * two.  Data moves GPU to GPU through an `ecfft_comm`:
 *   ecfft_comm_get_unique_id + ecfft_comm_init_rank   RCCL (ncclGetUniqueId / ncclCommInitRank; librccl.so is loaded at run
 *       time): grouped ncclSend / ncclRecv over xGMI on the caller's stream.  Rank 0 creates the 128-byte id and hands it to
 *       the other ranks by any means (MPI, TCP, a file, torch.distributed); every context of the job is built for its own GPU.
 *   ecfft_comm_init_callback   the host moves the device buffers itself (tests: several ranks sharing one GPU over gloo).
 * Arguments: device pointers only; `in` / `out` = this rank's BLOCK shard (len / world elements, may alias); world = 2^k;
 * len / world >= 2 * world.  Every rank of the communicator makes the same call with the same len.  Asynchronous on `stream`.
 * Exchanges (grouped send / receive calls) per transform: EXTEND 4 (2 per cyclic side saved, ecfft_extend_sharded_layout); ENTER
 * 3 per top level + 1 (Q = 2: 1); EXIT 1 + 9 per top level above the pairs + 1 — inside a level every vector stays cyclic over its
 * group; the level of the PAIRS of ranks (blocks of 2 len / world) runs redundantly on both ranks of a pair from one exchange
 * (round 4), so EXIT takes 2 / 11 / 20 exchanges at world = 2 / 4 / 8 (before: 10 / 19 / 28).  A FULL context (tables replicated) splits an EXIT of at
 * most 2^21 (ECFFT_SPLIT_GATHER_MAX_LOG) differently: one all-gather, then every top level redundantly on the block that contains the
 * rank's chunk — ONE exchange per EXIT (the split top levels are latency bound at such sizes, tools/split_project.py). */
typedef struct ecfft_comm ecfft_comm;
#define ECFFT_COMM_ID_BYTES 128
/* n sends and n receives of device buffers that must progress together; return 0 on success */
typedef int (*ecfft_exchange_fn)(void* user, int n_send, const int* send_peer, const void* const* send_ptr, const size_t* send_bytes,
                                 int n_recv, const int* recv_peer, void* const* recv_ptr, const size_t* recv_bytes, void* stream);
int ecfft_comm_get_unique_id(void* id_out);                                                      /* ECFFT_COMM_ID_BYTES bytes */
int ecfft_comm_init_rank(const void* id, int world, int rank, int device, ecfft_comm** out);
/* The RCCL library ecfft_comm_get_unique_id / ecfft_comm_init_rank bind (dlopen, RTLD_LOCAL) instead of the copy already mapped into
 * the process or /opt/rocm/lib/librccl.so: a differently named RCCL build, or the tests' stand-in (tests/stub_rccl).  NULL or "" =
 * default.  Must precede the first communicator of the process (the binding is made once): ECFFT_ERR_BAD_ARG afterwards.  The library
 * reads no environment variable for this (or for anything else). */
int ecfft_comm_set_rccl_library(const char* path);
int ecfft_comm_init_callback(int world, int rank, int device, ecfft_exchange_fn fn, void* user, ecfft_comm** out);
void ecfft_comm_destroy(ecfft_comm* comm);
/* RCCL transports: ncclCommAbort — unblocks the exchanges in flight (a peer died or never arrived) and makes every later sharded
 * call on this communicator return ECFFT_ERR_HIP; may be called from another host thread than the blocked one.  ECFFT_ERR_HIP for a
 * callback transport (the host owns its exchanges).  The librccl that is bound: ecfft_comm_set_rccl_library. */
int ecfft_comm_abort(ecfft_comm* comm);
/* Link striping of the big pairwise exchanges of a split ENTER / EXIT (round 5): a message travels as `world` slices, slice k via
 * rank k, in two grouped exchanges, so that every link of the xGMI mesh carries 1/world of it per phase — applied to an exchange only
 * when its most loaded link gets lighter by at least `min_gain_bytes` over both phases.  OFF by default (SIZE_MAX = never; round 6:
 * bit-exact over every transport the tests have, never yet timed on xGMI — it doubles the bytes a rank injects and adds an exchange).
 * 4 MiB is the threshold the projection suggests (>= 85 us at 48 GB/s against one more exchange latency); 0 = whenever striping moves
 * fewer bytes over the most loaded link.  Every rank of the communicator must use the same value (each rank decides locally from the
 * call's message pattern): the ranks compare it in the agreement that precedes the first call of every sharded call shape, and a
 * mismatch fails that call on all of them with ECFFT_ERR_HIP.  Only BEFORE the communicator has carried its first exchange:
 * ECFFT_ERR_BAD_ARG afterwards. */
int ecfft_comm_set_link_striping(ecfft_comm* comm, size_t min_gain_bytes);
int ecfft_comm_rank(const ecfft_comm* comm);
int ecfft_comm_world(const ecfft_comm* comm);
/* communication time: while enabled every exchange is bracketed by HIP events on its stream; _read synchronises the device */
int ecfft_comm_stats_enable(ecfft_comm* comm, int on);
int ecfft_comm_stats_read(ecfft_comm* comm, double* comm_ms, double* exchanges, double* bytes_sent);
int ecfft_extend_sharded(ecfft_ctx* ctx, ecfft_comm* comm, const void* in, void* out, size_t e, int moiety, void* stream);
/* Sharded EXTEND-ONLY context: one rank's share of the tables ONE EXTEND of e evaluations over `world` GPUs reads (tree
 * T_2e of build_fftree(2e); SURVEY 8(e) "matrix tables shard the same way").  Holds 26 e/world table constants — the
 * entries i = rank (mod world) of the stage tables for the cyclic stages, the last e/world entries for the block-local stages,
 * the normalisation weights of the rank's positions — instead of the ~84 e elements of the full chain T_1 .. T_2e; no tree
 * is ever materialised on any GPU.  Accepted by ecfft_extend_sharded / ecfft_extend_sharded_layout only (same e, world and rank in the communicator, either
 * moiety), plus ecfft_tree_size / ecfft_field / ecfft_ctx_device_bytes / ecfft_profile_* / ecfft_ctx_destroy; every other call returns
 * ECFFT_ERR_BAD_ARG.  Results are bit-identical to ecfft_extend on a full context.  world = 2^k <= 64, e / world >= 2 * world;
 * ECFFT_ERR_TREE_TOO_LARGE when T_2e exceeds the curve's 2-adicity, as ecfft_build_fftree(2e). */
int ecfft_build_extend_shard(int field, size_t e, int device, int world, int rank, ecfft_ctx** out);
/* Sharded ENTER-ONLY context for ONE ENTER of n coefficients over `world` GPUs (ecfft_enter_sharded): the full chain T_1 .. T_c,
 * c = n / world, for the rank-local low levels, and for each of the log2(world) top levels only the rank's share of that tree —
 * the EXTEND tables of the split over its half-group and the c entries of xnn_s its combine step reads (src/fftree.rs:155-159).
 * All of it is pointwise in the point set: no tree above T_c is materialised on any GPU (~1/world of a full context's HBM), so
 * an ENTER can be larger than one GPU's table capacity.  Accepted by ecfft_enter_sharded only (same n, world and rank), plus
 * the informational calls listed above.  world = 2^k, 2 <= world <= 64, n / world >= 2 * world. */
int ecfft_build_enter_shard(int field, size_t n, int device, int world, int rank, ecfft_ctx** out);
/* Sharded EXIT-ONLY context for ONE EXIT of n evaluations over the ranks of `comm` (ecfft_exit_sharded) — a COLLECTIVE call: every
 * rank of the communicator makes it with the same field and n.  Holds the full chain T_1 .. T_c (c = n / world) and, for each of the
 * log2(world) top levels, only the rank's share of that tree: the EXTEND tables of the split over its group (both directions), its
 * entries of xnn_s, 1 / xnn_s, 1 / z0_s1 (pointwise in the point set) and of z0z0_rem_xnn_s — which is built distributed, level
 * by level, as the reference builds it (src/fftree.rs:418-452) but with the split EXIT's own operators and exchanges over `comm`.
 * No tree above T_c is materialised on any GPU — except T_2c for the redundant pair level, see ecfft_build_exit_shard_opts.
 * Accepted by ecfft_exit_sharded only (same n and communicator shape). */
int ecfft_build_exit_shard(int field, size_t n, int device, ecfft_comm* comm, ecfft_ctx** out);
/* ... with options.  The level of the PAIRS of ranks (blocks of 2c) has two forms: REDUNDANT — each rank also keeps the full tree
 * T_2c and both ranks of a pair run the level on the whole block from one exchange (1 exchange instead of 9, twice that level's
 * arithmetic; at world = 2 the context is then as large as a full one) — or SPLIT over the pair's shares, with no tree above T_c
 * anywhere.  Default (flags 0, = ecfft_build_exit_shard): redundant when T_2c fits the free memory of EVERY rank — the ranks agree
 * before anything is allocated — split otherwise.  ECFFT_EXIT_SHARD_MIN_MEMORY: always split (the largest n a node can reach). */
#define ECFFT_EXIT_SHARD_MIN_MEMORY 1
int ecfft_build_exit_shard_opts(int field, size_t n, int device, ecfft_comm* comm, int flags, ecfft_ctx** out);
/* ecfft_extend_sharded with a choice of distribution for the rank's shard on each side.  ECFFT_LAYOUT_CYCLIC: local element j'
 * is global position j' * world + rank.  A cyclic input saves the first of the four exchanges, a cyclic output the last one —
 * for hosts that chain split EXTENDs or that produce / consume the cyclic order anyway.  (BLOCK, BLOCK) == ecfft_extend_sharded. */
#define ECFFT_LAYOUT_BLOCK 0
#define ECFFT_LAYOUT_CYCLIC 1
int ecfft_extend_sharded_layout(ecfft_ctx* ctx, ecfft_comm* comm, const void* in, void* out, size_t e, int moiety, int in_layout,
                                int out_layout, void* stream);
/* Failure on ONE rank: the first time a context sees a sharded call of a given shape (op, size, layout, world) every rank
 * prepares its temporaries and the ranks AGREE on the outcome (one int each way, host wait) before the first exchange — if any
 * rank failed, all of them return ECFFT_ERR_HIP and none is left blocked in ncclRecv.  That first call is therefore synchronous;
 * later calls of the shape reuse the pinned temporaries, cannot fail locally and are asynchronous.  ecfft_build_exit_shard votes
 * after its local part, at every level and on its final status.  (Failure injection for the tests: ecfft_hip_hooks.h, test builds only.) */
int ecfft_enter_sharded(ecfft_ctx* ctx, ecfft_comm* comm, const void* coeffs, void* evals, size_t n, void* stream);
int ecfft_exit_sharded(ecfft_ctx* ctx, ecfft_comm* comm, const void* evals, void* coeffs, size_t n, void* stream);

/* Pointwise building block of the multi-GPU ENTER / EXIT (no reference counterpart): with T = table `which` (one of
 * ECFFT_TBL_XNN_S .. ECFFT_TBL_Z1Z1_REM_XNN_S) of the subtree with m leaves,
 *     mode 0: out[i] = x[i]*T[j]    1: x[i]*T[j] + y[i]    2: y[i] - x[i]*T[j]    3: (y[i] - x[i])*T[j],   j = t_off + i*t_stride.
 * These are the loops src/fftree.rs:155-159, 217-219, 238, 253-255, 279 restricted to an index range. */
int ecfft_table_fma(ecfft_ctx* ctx, void* out, const void* x, const void* y, size_t cnt, size_t m, int which, size_t t_off,
                    size_t t_stride, int mode, int mem, void* stream);

/* copy one table of the subtree with m leaves into host memory (element representation above);
 * returns the number of elements through *count; cap = capacity of host_out in elements. */
int ecfft_tree_table(ecfft_ctx* ctx, size_t m, int which, void* host_out, size_t cap, size_t* count);

/* FFTree wire format — impl CanonicalSerialize / CanonicalDeserialize for FFTree<F>, src/fftree.rs:507-660 (ark-serialize 0.4:
 * Vec = u64 LE length + elements, field element = standard-form integer LE, bool = 1 byte).  `compress` != 0 is
 * Compress::Yes: the three inverse tables are left out (:536-541) and regenerated on load (:620-628).
 *   ecfft_fftree_serialize   <-> FFTree::serialize_compressed / serialize_uncompressed + serialized_size (:556-590): *len receives
 *       the byte count; buf == NULL only asks for it; cap < *len is ECFFT_ERR_BAD_ARG.  Tables are copied out of HBM as they lie
 *       there (plain residues = the standard form).
 *   ecfft_fftree_deserialize <-> FFTree::deserialize_compressed / deserialize_uncompressed (:600-660): bounds-checked parse (a
 *       truncated, non-canonical or inconsistent file is ECFFT_ERR_BAD_ARG), then FFTree::new on the file's leaves and maps —
 *       every other table is recomputed on the GPU.  verify != 0 compares each table of the file with the recomputed one and
 *       rejects the file on a mismatch (the reference trusts the file: Valid::check is a no-op, :592-597).  verify == 0 still checks the
 *       internal layers of `f`; the file's OTHER tables are then neither used nor checked — a file whose tables disagree with its
 *       point set loads as the tree of its point set, where the reference would use the file's tables verbatim.  Bindings should
 *       default to verify = 1. */
int ecfft_fftree_serialize(ecfft_ctx* ctx, int compress, void* buf, size_t cap, size_t* len);
/* the pub field rational_maps (src/fftree.rs:28) of the top tree: log2(n) maps, 3 numerator + 3 denominator coefficients each
 * (low -> high, zero padded), element representation as everywhere; either output may be NULL */
int ecfft_tree_rational_maps(ecfft_ctx* ctx, void* map_num3_out, void* map_den3_out);
int ecfft_fftree_deserialize(int field, const void* bytes, size_t len, int compress, int device, int verify, ecfft_ctx** out);

/* Host-only front end of build_fftree (src/lib.rs:66-81) + the layer fill of FFTree::new
 * (src/fftree.rs:49-67): writes f (2n elements, heap order: f[n..2n) = leaves x(coset_offset + i*G))
 * and the log2(n) isogeny x-maps (3 + 3 coefficients each).  Needs no GPU; used to cross-check the
 * construction against an ark-built tree. */
int ecfft_build_points(int field, size_t n, void* f_out, void* map_num3_out, void* map_den3_out);

/* Curves of the caller's own: search for a good curve on the GPU and build a tree on it.
 *   ecfft_find_curve            <-> ecfft::find_curve::find_curve(rng, k)                 src/find_curve.rs:224-246
 *   ecfft_curve_two_sylow       <-> cyclic_two_sylow_subgroup, for many curves            src/find_curve.rs:190-218
 *   ecfft_build_fftree_on_curve <-> the body of build_fftree for a GoodCurve              src/lib.rs:39-85, src/ec.rs:38-45, 61-90
 * The curve is y^2 = x (x^2 + a x + bb).  All four calls take `field` and `device` like ecfft_mul_ceiling, need no context, take
 * HOST pointers and are SYNCHRONOUS; elements are in the crate's in-memory form, points are the pair x, y laid end to end.
 *
 * ecfft_find_curve_candidate: candidate `index` of the stream `seed`, which replaces the reference's rng so that a search can be
 * reproduced.  Host only, needs no GPU.  With mix = the splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 * z *= 0x94D049BB133111EB, z ^= z >> 31) and word number c = mix of seed + (c + 1) * 0x9E3779B97F4A7C15 mod 2^64:
 *   secp256k1: a = the 256-bit integer made of words 8 index .. 8 index + 3, low word first, mod p; bb from words 8 index + 4 .. + 7;
 *   M31:       a = the low 31 bits of word 8 index, mod p; bb from word 8 index + 4.
 * ECFFT_ERR_BAD_ARG: a NULL output, an unknown field, index >= 2^60.
 *
 * ecfft_curve_two_sylow: for `count` curves a[i], bb[i]: n_out[i] = n when the 2-Sylow subgroup of the curve's group is cyclic of
 * order 2^n and bb is a square, else 0; a zero bb or a zero discriminant a^2 - 4 bb, where the reference asserts, gives 0 too.
 * x_out[i] = the x-coordinate of a point of order 2^n, 0 when n_out[i] is 0.  Bit-exact by one convention: every square root is
 * v^((p+1)/4), accepted when its square is v (both fields have p = 3 mod 4; 0 counts as a square, as sqrt().is_some() does), and the
 * two roots of a quadratic are tried in the reference's order, (-b + s)/2 then (-b - s)/2.
 * Method: stages over device-resident queues (bb square, discriminant no square, point of order 4, then one halving round per
 * launch); each stage appends its survivors densely to the next queue, so every launch runs full waves although half the curves
 * die at each test.  A curve that survives 8 * element bytes + 2 halving rounds (impossible: the group is too small) ends the call
 * with ECFFT_ERR_HIP.  ECFFT_ERR_BAD_ARG: a NULL pointer, count 0, an unknown field.
 *
 * ecfft_find_curve: scans candidates start .. start + max_candidates - 1 of stream `seed` and returns the one with the SMALLEST
 * index whose n >= max of k and 2: the answer does not depend on how the scan is cut into batches.  It stops after the first batch
 * that holds a hit.  Outputs, when found: *index_out, *n_out, a and bb, the generator gen_xy of order 2^n (the x that
 * ecfft_curve_two_sylow gives, y = the canonical root of x (x^2 + a x + bb)), and a coset offset offset_xy: the point with the smallest
 * integer x >= 1 for which x (x^2 + a x + bb) is a non-zero square and 2^n times the point is not the identity, y canonical.  These
 * are the arguments of ecfft_build_fftree_on_curve with gen_log_order = n.  One kind of curve has no such point: when n is the bit
 * length of p the Hasse bound leaves 2^n as the only group order, the whole group is the cyclic one (M31: the supersingular curves
 * of p + 1 = 2^31 points, which a deep search meets first), and offset_xy is returned as 0, 0; a tree on such a curve takes twice the
 * generator, gen_log_order = n - 1 and the generator itself as the offset.  Nothing found: ECFFT_OK with *n_out = 0 and
 * *index_out = UINT64_MAX, the other outputs untouched.  ECFFT_ERR_BAD_ARG: NULL index_out or n_out (a_out, bb_out, gen_xy_out and
 * offset_xy_out may be NULL), max_candidates 0, start + max_candidates > 2^60, k > 8 * element bytes, an unknown field.
 *
 * ecfft_build_fftree_on_curve: ecfft_build_fftree on the good curve a, bb: leaf i = x of offset + i * 2^(gen_log_order - log2 n) gen,
 * the isogenies x -> (x - b)^2 / x.  Checked on the host before any device work, in this order:
 *   n not a power of two                                          ECFFT_ERR_NOT_POW2
 *   log2 n >= gen_log_order (the reference's rule, src/lib.rs:62-64)   ECFFT_ERR_TREE_TOO_LARGE
 *   bb zero or no square; a point not on the curve; gen not of order exactly 2^gen_log_order (2^(gen_log_order - 1) gen must be the
 *   point 0, 0); 2^gen_log_order offset the identity; a NULL pointer; gen_log_order 0 or above 8 * element bytes   ECFFT_ERR_BAD_ARG
 * With n < 2^gen_log_order the last check makes the leaves distinct and keeps every layer away from the pole of its map. */
int ecfft_find_curve_candidate(int field, uint64_t seed, uint64_t index, void* a_out, void* bb_out);
int ecfft_curve_two_sylow(int field, int device, const void* a, const void* bb, size_t count, uint32_t* n_out, void* x_out);
int ecfft_find_curve(int field, int device, unsigned k, uint64_t seed, uint64_t start, uint64_t max_candidates, uint64_t* index_out,
                     uint32_t* n_out, void* a_out, void* bb_out, void* gen_xy_out, void* offset_xy_out);
int ecfft_build_fftree_on_curve(int field, size_t n, const void* a, const void* bb, const void* gen_xy, unsigned gen_log_order,
                                const void* offset_xy, int device, ecfft_ctx** out);

/* Trees on short-Weierstrass curves y^2 = x^3 + A x + B, the (A, B) of ecfft_curve_cardinality: from a curve and its number of
 * points to a tree.
 *   ecfft_curve_point_mul          <-> Point::mul, for many points                            src/ec.rs:432-447
 *   ecfft_curve_point_two_adicity  <-> two_adicity, with an explicit cap                      src/utils.rs:356-365
 *   ecfft_curve_find_generator     <-> what a caller of build_ec_fftree does by hand: a point of order 2^v and a coset offset
 *   ecfft_build_ec_fftree          <-> build_ec_fftree(subgroup_generator, subgroup_order, coset_offset, n)   src/ec.rs:498-554
 * Like the ecfft_find_curve family the four calls take `field` and `device`, need no context, take HOST pointers and are
 * SYNCHRONOUS; elements are in the crate's in-memory form, a point is the pair x, y laid end to end.
 *
 * ecfft_curve_point_mul: out[i] = [k_i] P_i for i < count.  A and B hold `ncurves` elements each, `scalars` holds `nscalars` rows of
 * `scalar_bytes` little-endian bytes (1 <= scalar_bytes <= 40, the width of a cardinality); ncurves and nscalars are each 1 (shared by
 * every row) or count.  inf_in (may be NULL: every point finite) and inf_out hold one byte per point, non-zero for the point at
 * infinity, whose x, y are not read on the way in and written as 0, 0 on the way out.  Method: one thread per row, Jacobian
 * accumulator and affine base, left to right over the bits of the longest scalar: every lane doubles at every bit and takes the
 * addition where its bit is set; one inversion per row at the end.  The exceptional cases of the group law (accumulator at infinity,
 * equal to the base, its negative; y = 0 in a doubling; scalar 0; base at infinity) are decided exactly, and the affine result is
 * unique, so the output is bit-exact against any model.  A point that is not on its curve or a singular curve (4 A^3 + 27 B^2 = 0)
 * is flagged on the device: ECFFT_ERR_BAD_ARG, outputs untouched.  ECFFT_ERR_BAD_ARG also for a NULL pointer other than inf_in,
 * count 0, scalar_bytes 0 or above 40, ncurves or nscalars neither 1 nor count, an unknown field.
 *
 * ecfft_curve_point_two_adicity: out[i] = the smallest j >= 0 with 2^j P_i the identity, among j <= cap; -1 when there is none
 * (0 for the point at infinity).  cap <= 8 * element bytes + 2, above which no point of any curve over the field can need more.
 * Curves, points, inf_in and errors as above.
 *
 * ecfft_curve_find_generator: the arguments of ecfft_build_ec_fftree from one curve and its number of points `order`
 * (ECFFT_ORDER_BYTES little-endian bytes, as ecfft_curve_cardinality writes them).  With order = 2^v m, m odd, the candidates are
 * x = start, start + 1, ..., start + max_candidates - 1 as integers (start >= 1); those whose x^3 + A x + B is a non-zero square
 * give the point R = (x, y), y the canonical root v^((p+1)/4).  gen_xy = [m] R for the candidate of SMALLEST x whose [m] R has
 * two-adicity exactly v, and *x_out = that x; offset_xy = the candidate R of smallest x in the window for which 2^(v+1) R is not the
 * identity, 0, 0 when the window holds none (a group that is a 2-group, such as y^2 = x^3 + x over M31 with its 2^31 points, has none
 * at all; a tree on such a curve takes four times the generator, gen_log_order = v - 2 and the generator itself as the offset).  Neither answer depends on how the scan is cut into batches; the scan ends as soon as both are known.  *log_order_out = v.
 * No generator in the window (a 2-Sylow subgroup that is not cyclic has no point of order 2^v), or an odd order: ECFFT_OK with
 * *log_order_out = 0 and the other outputs untouched.  A candidate R with [order] R not the identity proves that `order` is not
 * the curve's: ECFFT_ERR_BAD_ARG.  ECFFT_ERR_BAD_ARG also for NULL A, B, order or log_order_out (gen_xy, offset_xy and x_out may be
 * NULL), an order of zero, a singular curve, start 0, max_candidates 0, start + max_candidates above 2^60 or above p, an unknown
 * field.  One batch is one launch: candidate, square test, the multiplication by the shared scalar m, two-adicity.
 *
 * ecfft_build_ec_fftree: leaf i = x of offset + i * 2^(gen_log_order - log2 n) gen.  The map of each level is chosen as the
 * reference does (src/ec.rs:526-543): the Velu 2-isogenies of the current curve from the roots of x^3 + a x + b in ascending order
 * of their standard form, the first that lowers the generator's two-adicity by exactly one.  Checked on the host before any device
 * work, in this order:
 *   n not a power of two                                                         ECFFT_ERR_NOT_POW2
 *   log2 n > gen_log_order (the reference's rule, src/ec.rs:513: n may equal the order)   ECFFT_ERR_TREE_TOO_LARGE
 *   a singular curve; a point not on the curve; gen not of order exactly 2^gen_log_order; 2^(gen_log_order + 1) offset the
 *   identity; no suitable isogeny at some level; a NULL pointer; gen_log_order 0 or above 8 * element bytes     ECFFT_ERR_BAD_ARG
 * The condition on the offset says that 2 offset is not in <gen>: then offset + P = +-(offset + Q) has no solution with P != Q in
 * <gen>, which makes the n leaves distinct, and no layer meets the pole of its map (a pole is the x of a point of order 2 of the
 * kernel, and a leaf there would put 2 offset into <gen> again). */
int ecfft_curve_point_mul(int field, int device, const void* A, const void* B, size_t ncurves, const void* points_xy, const uint8_t* inf_in,
                          const void* scalars, size_t nscalars, size_t scalar_bytes, void* out_xy, uint8_t* inf_out, size_t count);
int ecfft_curve_point_two_adicity(int field, int device, const void* A, const void* B, size_t ncurves, const void* points_xy, const uint8_t* inf_in,
                                  unsigned cap, int32_t* out, size_t count);
int ecfft_curve_find_generator(int field, int device, const void* A, const void* B, const void* order, uint64_t start, uint64_t max_candidates,
                               unsigned* log_order_out, void* gen_xy, void* offset_xy, uint64_t* x_out);
int ecfft_build_ec_fftree(int field, size_t n, const void* A, const void* B, const void* gen_xy, unsigned gen_log_order, const void* offset_xy,
                          int device, ecfft_ctx** out);

/* Per-launch timing for benchmarks (no reference counterpart): while enabled, every hot-path kernel
 * launch is bracketed by HIP events on its stream.  ecfft_profile_read synchronises the device and
 * returns, for kernel class `cls` (0 <= cls < ecfft_profile_classes()), its name, number of launches,
 * summed event time in ms and summed ALGORITHMIC bytes (stage-streaming model). */
int ecfft_profile_enable(ecfft_ctx* ctx, int on);
int ecfft_profile_classes(void);
int ecfft_profile_read(ecfft_ctx* ctx, int cls, char* name, size_t cap, uint64_t* launches, double* ms_total,
                       double* alg_bytes_total);

/* Element representation converters (host buffers, no GPU needed): the crate's in-memory form <-> the STANDARD-form
 * little-endian integer that ark-serialize writes (32 bytes for secp256k1, 4 for M31).  Used by the FFTree wire-format
 * reader/writer (ecfft_amd/serialize.py, reference: src/fftree.rs:507-660). */
int ecfft_elems_to_standard(int field, const void* in, void* out, size_t n);
int ecfft_elems_from_standard(int field, const void* in, void* out, size_t n);

/* Measurement hook: field multiplies per second of the butterfly kernels' table multiply run as a bare dependent chain
 * (x <- T*x + c per lane, `waves_per_simd` resident waves per SIMD, whole chip) — the VALU ceiling bench.py prices the hot
 * path against beside the HBM roofline. */
int ecfft_mul_ceiling(int field, int device, int waves_per_simd, double* mul_per_s);

/* Measurement hook: effective shader clock in MHz while every SIMD of the chip runs the kernels' table multiply (ratio of
 * s_memtime ticks to the constant 100 MHz wall clock inside that kernel) — the clock DVFS grants this instruction mix, needed
 * to turn rocprofv3 instruction counts into issue-cycle fractions. */
int ecfft_shader_clock(int field, int device, double* mhz);

/* Device-buffer helpers for hosts without HIP bindings (examples/sharded_extend.cpp is plain C++ over this ABI): allocate / free
 * HBM on `device`, wait for the device. */
int ecfft_device_alloc(int device, size_t bytes, void** out);
int ecfft_device_free(void* ptr);
int ecfft_device_sync(int device);

/* synchronous copy on the CURRENT device: kind 0 device -> host, 1 host -> device, 2 device -> device.  Lets a host language
 * without HIP bindings implement the exchange callback above — ecfft_amd/distributed.py does, over gloo. */
int ecfft_device_copy(void* dst, const void* src, size_t bytes, int kind);

/* library / device identification for logs: writes a NUL-terminated string */
int ecfft_device_info(int device, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
