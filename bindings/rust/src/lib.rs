//! `HipFFTree<F>`: the reference's `FFTree<F>` surface (src/fftree.rs:23-38, 123, 138, 164, 195, 227, 264-289, 313) backed by
//! the MI355X kernels through the C ABI of `include/ecfft_hip.h`.
//!
//! UNCOMPILED SOURCE — see README.md.  Element layout contract (ecfft_hip.h): `secp256k1::Fp` = `Fp256<MontBackend<_, 4>>`
//! = `[u64; 4]` Montgomery limbs, `m31::Fp` = one `u32`; both are passed as raw slices with no conversion, which is why
//! `HipField` is `unsafe` to implement.
use core::ffi::c_void;
use core::marker::PhantomData;

pub use ecfft::Moiety;

/// raw C ABI (include/ecfft_hip.h)
pub mod ffi {
    use core::ffi::c_void;
    #[repr(C)]
    pub struct EcfftCtx {
        _p: [u8; 0],
    }
    #[repr(C)]
    pub struct EcfftComm {
        _p: [u8; 0],
    }
    pub const OK: i32 = 0;
    pub const ERR_NOT_POW2: i32 = 1;
    pub const ERR_TREE_TOO_SMALL: i32 = 2;
    pub const ERR_TREE_TOO_LARGE: i32 = 3;
    pub const ERR_HIP: i32 = 4;
    pub const ERR_BAD_ARG: i32 = 5;
    pub const MEM_HOST: i32 = 0;
    pub const RS_OUT_COEFFS: i32 = 0;
    pub const RS_OUT_CODEWORD: i32 = 1;
    pub const MEM_DEVICE: i32 = 1;
    // ECFFT_TBL_*
    pub const TBL_F: i32 = 0;
    pub const TBL_RECOMBINE: i32 = 1;
    pub const TBL_DECOMPOSE: i32 = 2;
    pub const TBL_XNN_S: i32 = 3;
    pub const TBL_XNN_S_INV: i32 = 4;
    pub const TBL_Z0_S1: i32 = 5;
    pub const TBL_Z1_S0: i32 = 6;
    pub const TBL_Z0_INV_S1: i32 = 7;
    pub const TBL_Z1_INV_S0: i32 = 8;
    pub const TBL_Z0Z0_REM_XNN_S: i32 = 9;
    pub const TBL_Z1Z1_REM_XNN_S: i32 = 10;
    extern "C" {
        pub fn ecfft_elem_size(field: i32) -> usize;
        pub fn ecfft_build_fftree(field: i32, n: usize, device: i32, out: *mut *mut EcfftCtx) -> i32;
        pub fn ecfft_fftree_new(field: i32, leaves: *const c_void, n: usize, map_num3: *const c_void, map_den3: *const c_void, device: i32, out: *mut *mut EcfftCtx) -> i32;
        pub fn ecfft_ctx_destroy(ctx: *mut EcfftCtx);
        pub fn ecfft_tree_size(ctx: *const EcfftCtx) -> usize;
        pub fn ecfft_enter(ctx: *mut EcfftCtx, coeffs: *const c_void, evals: *mut c_void, n: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_exit(ctx: *mut EcfftCtx, evals: *const c_void, coeffs: *mut c_void, n: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_enter_many(ctx: *mut EcfftCtx, coeffs: *const c_void, evals: *mut c_void, n: usize, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_exit_many(ctx: *mut EcfftCtx, evals: *const c_void, coeffs: *mut c_void, n: usize, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_extend(ctx: *mut EcfftCtx, inp: *const c_void, out: *mut c_void, e: usize, moiety: i32, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_mul(ctx: *mut EcfftCtx, a: *const c_void, na: usize, b: *const c_void, nb: usize, out: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_inv_series(ctx: *mut EcfftCtx, f: *const c_void, nf: usize, out: *mut c_void, k: usize, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_divrem(ctx: *mut EcfftCtx, a: *const c_void, na: usize, b: *const c_void, nb: usize, q: *mut c_void, r: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_eval_points(ctx: *mut EcfftCtx, f: *const c_void, nf: usize, points: *const c_void, m: usize, out: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_interpolate(ctx: *mut EcfftCtx, points: *const c_void, m: usize, values: *const c_void, out: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_pow_mod(ctx: *mut EcfftCtx, a: *const c_void, na: usize, exp: *const c_void, exp_bytes: usize, modulus: *const c_void, nm: usize, out: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_mul_mod(ctx: *mut EcfftCtx, a: *const c_void, na: usize, b: *const c_void, nb: usize, modulus: *const c_void, nm: usize, out: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_compose_mod(ctx: *mut EcfftCtx, f: *const c_void, nf: usize, g: *const c_void, ng: usize, modulus: *const c_void, nm: usize, out: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_squarefree(ctx: *mut EcfftCtx, f: *const c_void, nf: usize, out: *mut c_void, degrees: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_distinct_degree(ctx: *mut EcfftCtx, f: *const c_void, nf: usize, factors: *mut c_void, degrees: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_equal_degree(ctx: *mut EcfftCtx, g: *const c_void, ng: usize, d: usize, factors: *mut c_void, n_factors: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_squarefree_decompose(ctx: *mut EcfftCtx, f: *const c_void, nf: usize, parts: *mut c_void, degrees: *mut i64, lead: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_factor(ctx: *mut EcfftCtx, f: *const c_void, nf: usize, factors: *mut c_void, fdeg: *mut i64, fmult: *mut i64, n_factors: *mut i64, lead: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_division_polynomial(ctx: *mut EcfftCtx, a: *const c_void, b: *const c_void, n: usize, out: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_curve_cardinality(ctx: *mut EcfftCtx, a: *const c_void, b: *const c_void, order: *mut c_void, traces: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_curve_trace_mod(ctx: *mut EcfftCtx, a: *const c_void, b: *const c_void, l: usize, t_out: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_find_roots(ctx: *mut EcfftCtx, f: *const c_void, nf: usize, roots: *mut c_void, n_roots: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_gcd(ctx: *mut EcfftCtx, a: *const c_void, na: usize, b: *const c_void, nb: usize, g: *mut c_void, degrees: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_xgcd(ctx: *mut EcfftCtx, a: *const c_void, na: usize, b: *const c_void, nb: usize, s: *mut c_void, t: *mut c_void, g: *mut c_void, degrees: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_poly_xgcd_partial(ctx: *mut EcfftCtx, a: *const c_void, na: usize, b: *const c_void, nb: usize, stop: usize, r: *mut c_void, s: *mut c_void, t: *mut c_void, degrees: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_rs_decode(ctx: *mut EcfftCtx, points: *const c_void, m: usize, values: *const c_void, k: usize, message: *mut c_void, n_errors: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_rs_encode(ctx: *mut EcfftCtx, points: *const c_void, m: usize, data: *const c_void, k: usize, codeword: *mut c_void, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_rs_decode_erasures(ctx: *mut EcfftCtx, points: *const c_void, m: usize, values: *const c_void, erased: *const u8, k: usize, out: *mut c_void, out_form: i32, n_errors: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_seq_min_poly(ctx: *mut EcfftCtx, seq: *const c_void, n_terms: usize, min_poly: *mut c_void, orders: *mut i64, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_seq_nth_term(ctx: *mut EcfftCtx, char_poly: *const c_void, nc: usize, init: *const c_void, index: *const c_void, index_bytes: usize, out: *mut c_void, nout: usize, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_mextend(ctx: *mut EcfftCtx, inp: *const c_void, out: *mut c_void, e: usize, moiety: i32, count: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_redc(ctx: *mut EcfftCtx, evals: *const c_void, a: *const c_void, out: *mut c_void, n: usize, moiety: i32, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_modular_reduce(ctx: *mut EcfftCtx, evals: *const c_void, a: *const c_void, c: *const c_void, out: *mut c_void, n: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_vanish(ctx: *mut EcfftCtx, domain: *const c_void, out: *mut c_void, nd: usize, mem: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_degree(ctx: *mut EcfftCtx, evals: *const c_void, n: usize, mem: i32, stream: *mut c_void, degree: *mut usize) -> i32;
        pub fn ecfft_tree_table(ctx: *mut EcfftCtx, m: usize, which: i32, host_out: *mut c_void, cap: usize, count: *mut usize) -> i32;
        pub fn ecfft_ctx_device_bytes(ctx: *const EcfftCtx) -> usize;
        pub fn ecfft_ctx_trim(ctx: *mut EcfftCtx) -> i32;
        // FFTree wire format (impl CanonicalSerialize / CanonicalDeserialize for FFTree<F>, src/fftree.rs:507-660)
        pub fn ecfft_fftree_serialize(ctx: *mut EcfftCtx, compress: i32, buf: *mut c_void, cap: usize, len: *mut usize) -> i32;
        pub fn ecfft_fftree_deserialize(field: i32, bytes: *const c_void, len: usize, compress: i32, device: i32, verify: i32, out: *mut *mut EcfftCtx) -> i32;
        pub fn ecfft_tree_rational_maps(ctx: *mut EcfftCtx, map_num3_out: *mut c_void, map_den3_out: *mut c_void) -> i32;
        // one transform split over the GPUs of a node, one process per GPU (device pointers; see ecfft_hip.h)
        pub fn ecfft_comm_get_unique_id(id_out: *mut c_void) -> i32; // ECFFT_COMM_ID_BYTES = 128
        pub fn ecfft_comm_init_rank(id: *const c_void, world: i32, rank: i32, device: i32, out: *mut *mut EcfftComm) -> i32;
        pub fn ecfft_comm_destroy(comm: *mut EcfftComm);
        pub fn ecfft_comm_rank(comm: *const EcfftComm) -> i32;
        pub fn ecfft_comm_world(comm: *const EcfftComm) -> i32;
        pub fn ecfft_build_extend_shard(field: i32, e: usize, device: i32, world: i32, rank: i32, out: *mut *mut EcfftCtx) -> i32;
        pub fn ecfft_build_enter_shard(field: i32, n: usize, device: i32, world: i32, rank: i32, out: *mut *mut EcfftCtx) -> i32;
        pub fn ecfft_build_exit_shard(field: i32, n: usize, device: i32, comm: *mut EcfftComm, out: *mut *mut EcfftCtx) -> i32; // collective
        pub fn ecfft_build_exit_shard_opts(field: i32, n: usize, device: i32, comm: *mut EcfftComm, flags: i32, out: *mut *mut EcfftCtx) -> i32; // flags: 1 = ECFFT_EXIT_SHARD_MIN_MEMORY
        pub fn ecfft_comm_set_rccl_library(path: *const std::os::raw::c_char) -> i32; // before the first communicator; NULL = default
        pub fn ecfft_comm_abort(comm: *mut EcfftComm) -> i32;
        pub fn ecfft_comm_set_link_striping(comm: *mut EcfftComm, min_gain_bytes: usize) -> i32; // usize::MAX = never (the default since round 6), 0 = whenever it helps; same value on every rank (checked in the ranks' first vote); ERR_BAD_ARG once the communicator has carried an exchange
        pub fn ecfft_extend_sharded(ctx: *mut EcfftCtx, comm: *mut EcfftComm, input: *const c_void, out: *mut c_void, e: usize, moiety: i32, stream: *mut c_void) -> i32;
        pub fn ecfft_extend_sharded_layout(ctx: *mut EcfftCtx, comm: *mut EcfftComm, input: *const c_void, out: *mut c_void, e: usize, moiety: i32, in_layout: i32, out_layout: i32, stream: *mut c_void) -> i32; // 0 block, 1 cyclic
        pub fn ecfft_enter_sharded(ctx: *mut EcfftCtx, comm: *mut EcfftComm, coeffs: *const c_void, evals: *mut c_void, n: usize, stream: *mut c_void) -> i32;
        pub fn ecfft_exit_sharded(ctx: *mut EcfftCtx, comm: *mut EcfftComm, evals: *const c_void, coeffs: *mut c_void, n: usize, stream: *mut c_void) -> i32;
        // curves of the caller's own: the search (src/find_curve.rs:190-246) and build_fftree on a good curve; host pointers, synchronous
        pub fn ecfft_find_curve_candidate(field: i32, seed: u64, index: u64, a_out: *mut c_void, bb_out: *mut c_void) -> i32;
        pub fn ecfft_curve_two_sylow(field: i32, device: i32, a: *const c_void, bb: *const c_void, count: usize, n_out: *mut u32, x_out: *mut c_void) -> i32;
        pub fn ecfft_find_curve(field: i32, device: i32, k: u32, seed: u64, start: u64, max_candidates: u64, index_out: *mut u64, n_out: *mut u32, a_out: *mut c_void, bb_out: *mut c_void, gen_xy_out: *mut c_void, offset_xy_out: *mut c_void) -> i32;
        pub fn ecfft_build_fftree_on_curve(field: i32, n: usize, a: *const c_void, bb: *const c_void, gen_xy: *const c_void, gen_log_order: u32, offset_xy: *const c_void, device: i32, out: *mut *mut EcfftCtx) -> i32;
        // trees on short-Weierstrass curves y^2 = x^3 + A x + B (src/ec.rs:432-447, 498-554; src/utils.rs:356-365); host pointers, synchronous
        pub fn ecfft_curve_point_mul(field: i32, device: i32, a: *const c_void, b: *const c_void, ncurves: usize, points_xy: *const c_void, inf_in: *const u8, scalars: *const c_void, nscalars: usize, scalar_bytes: usize, out_xy: *mut c_void, inf_out: *mut u8, count: usize) -> i32;
        pub fn ecfft_curve_point_two_adicity(field: i32, device: i32, a: *const c_void, b: *const c_void, ncurves: usize, points_xy: *const c_void, inf_in: *const u8, cap: u32, out: *mut i32, count: usize) -> i32;
        pub fn ecfft_curve_find_generator(field: i32, device: i32, a: *const c_void, b: *const c_void, order: *const c_void, start: u64, max_candidates: u64, log_order_out: *mut u32, gen_xy: *mut c_void, offset_xy: *mut c_void, x_out: *mut u64) -> i32;
        pub fn ecfft_build_ec_fftree(field: i32, n: usize, a: *const c_void, b: *const c_void, gen_xy: *const c_void, gen_log_order: u32, offset_xy: *const c_void, device: i32, out: *mut *mut EcfftCtx) -> i32;
        pub fn ecfft_device_alloc(device: i32, bytes: usize, out: *mut *mut c_void) -> i32;
        pub fn ecfft_device_free(ptr: *mut c_void) -> i32;
        pub fn ecfft_device_copy(dst: *mut c_void, src: *const c_void, bytes: usize, kind: i32) -> i32; // 0 D2H, 1 H2D, 2 D2D
        pub fn ecfft_device_sync(device: i32) -> i32;
    }
}

/// A field of the reference crate whose in-memory representation is the one `libecfft_hip.so` expects.
///
/// # Safety
/// `Self` must be exactly `ELEM_BYTES` bytes of plain data laid out as documented in `ecfft_hip.h`
/// (`[u64; 4]` Montgomery limbs for secp256k1, `u32` for M31).
pub unsafe trait HipField: ecfft::FftreeField + Copy {
    const FIELD_ID: i32;
    const ELEM_BYTES: usize;
}
unsafe impl HipField for ecfft::secp256k1::Fp {
    const FIELD_ID: i32 = 0;
    const ELEM_BYTES: usize = 32;
}
unsafe impl HipField for ecfft::m31::Fp {
    const FIELD_ID: i32 = 1;
    const ELEM_BYTES: usize = 4;
}

/// `FftreeField::build_fftree` (src/lib.rs:14-16) for the GPU tree
pub trait HipFftreeField: HipField {
    fn build_hip_fftree(n: usize) -> Option<HipFFTree<Self>> {
        HipFFTree::build_fftree(n)
    }
}
impl<F: HipField> HipFftreeField for F {}

/// Device-resident `FFTree<F>`: the whole subtree chain lives in one context (src/fftree.rs:29, 484-496).
pub struct HipFFTree<F: HipField> {
    ctx: *mut ffi::EcfftCtx,
    _f: PhantomData<F>,
}
// the context is immutable after creation; the library serialises transforms on its scratch buffers internally
unsafe impl<F: HipField> Send for HipFFTree<F> {}
unsafe impl<F: HipField> Sync for HipFFTree<F> {}

impl<F: HipField> Drop for HipFFTree<F> {
    fn drop(&mut self) {
        unsafe { ffi::ecfft_ctx_destroy(self.ctx) }
    }
}

/// What `HipFFTree::find_curve` returns: the curve y^2 = x(x^2 + a x + bb), a generator (x, y) of order 2^n and a coset offset
#[derive(Clone, Copy, Debug)]
pub struct FoundCurve<F: HipField> {
    pub index: u64,
    pub n: u32,
    pub a: F,
    pub bb: F,
    pub gen: [F; 2],
    pub offset: [F; 2],
}

/// What `HipFFTree::curve_find_generator` returns: a generator (x, y) of order 2^log_order of y^2 = x^3 + A x + B, a coset offset
/// ((0, 0) when the window holds none) and the integer x-coordinate the generator came from
#[derive(Clone, Copy, Debug)]
pub struct FoundGenerator<F: HipField> {
    pub log_order: u32,
    pub x: u64,
    pub gen: [F; 2],
    pub offset: [F; 2],
}

fn check(rc: i32) {
    match rc {
        ffi::OK => {}
        ffi::ERR_NOT_POW2 => panic!("length must be a power of two"), // assert!(n.is_power_of_two()), src/fftree.rs:490
        ffi::ERR_TREE_TOO_SMALL => panic!("FFTree is too small"),      // src/fftree.rs:494
        ffi::ERR_HIP => panic!("ecfft_hip: HIP failure (no usable MI355X?) - there is no CPU fallback"),
        e => panic!("ecfft_hip error {e}"),
    }
}

fn moiety_id(m: Moiety) -> i32 {
    match m {
        Moiety::S0 => 0,
        Moiety::S1 => 1,
    }
}

impl<F: HipField> HipFFTree<F> {
    /// `F::build_fftree(n)`: `None` when n exceeds the curve's 2-adicity (src/lib.rs:62-64, src/ec.rs:513-515)
    pub fn build_fftree(n: usize) -> Option<Self> {
        Self::build_fftree_on(n, 0)
    }
    pub fn build_fftree_on(n: usize, device: i32) -> Option<Self> {
        assert_eq!(core::mem::size_of::<F>(), F::ELEM_BYTES, "unexpected in-memory size of the field element");
        let mut ctx = core::ptr::null_mut();
        match unsafe { ffi::ecfft_build_fftree(F::FIELD_ID, n, device, &mut ctx) } {
            ffi::ERR_TREE_TOO_LARGE => None,
            rc => {
                check(rc);
                Some(Self { ctx, _f: PhantomData })
            }
        }
    }

    /// `find_curve(rng, k)` (src/find_curve.rs:224-246) on the GPU, over candidates `start .. start + max_candidates` of the
    /// reproducible stream `seed` (ecfft_hip.h): the candidate of smallest index whose 2-Sylow subgroup is cyclic of order
    /// 2^n, n >= max(k, 2).  `None` when the window holds none.
    pub fn find_curve(k: u32, seed: u64, start: u64, max_candidates: u64, device: i32) -> Option<FoundCurve<F>> {
        assert_eq!(core::mem::size_of::<F>(), F::ELEM_BYTES, "unexpected in-memory size of the field element");
        let (mut index, mut n) = (0u64, 0u32);
        let (mut a, mut bb) = (F::zero(), F::zero());
        let (mut gen, mut offset) = ([F::zero(); 2], [F::zero(); 2]);
        check(unsafe {
            ffi::ecfft_find_curve(F::FIELD_ID, device, k, seed, start, max_candidates, &mut index, &mut n, (&mut a as *mut F).cast(),
                (&mut bb as *mut F).cast(), gen.as_mut_ptr().cast(), offset.as_mut_ptr().cast())
        });
        (n != 0).then_some(FoundCurve { index, n, a, bb, gen, offset })
    }

    /// `build_fftree(n)` on a found curve (ecfft_build_fftree_on_curve): `None` when log2 n >= the generator's log order
    pub fn build_on_curve(n: usize, c: &FoundCurve<F>, device: i32) -> Option<Self> {
        let mut ctx = core::ptr::null_mut();
        match unsafe {
            ffi::ecfft_build_fftree_on_curve(F::FIELD_ID, n, (&c.a as *const F).cast(), (&c.bb as *const F).cast(), c.gen.as_ptr().cast(), c.n,
                c.offset.as_ptr().cast(), device, &mut ctx)
        } {
            ffi::ERR_TREE_TOO_LARGE => None,
            rc => {
                check(rc);
                Some(Self { ctx, _f: PhantomData })
            }
        }
    }

    /// `out[i] = [k_i] P_i` on y^2 = x^3 + a x + b (ecfft_curve_point_mul <-> `Point::mul`, src/ec.rs:432-447): one curve for all
    /// rows or one per row, `scalars` rows of `scalar_bytes` little-endian bytes (one row or one per point), `inf` empty or one byte
    /// per point.  Returns the points and their infinity flags.  Panics for a point off its curve or a singular curve.
    pub fn curve_point_mul(a: &[F], b: &[F], points: &[[F; 2]], scalars: &[u8], scalar_bytes: usize, inf: &[u8], device: i32) -> (Vec<[F; 2]>, Vec<u8>) {
        assert_eq!(core::mem::size_of::<F>(), F::ELEM_BYTES, "unexpected in-memory size of the field element");
        let count = points.len();
        assert!(count > 0 && a.len() == b.len() && (a.len() == 1 || a.len() == count), "one curve, or one per point");
        assert!(scalar_bytes >= 1 && scalars.len() % scalar_bytes == 0, "scalars: whole rows of scalar_bytes bytes");
        let nscalars = scalars.len() / scalar_bytes;
        assert!(nscalars == 1 || nscalars == count, "one scalar, or one per point");
        assert!(inf.is_empty() || inf.len() == count, "inf: one byte per point");
        let mut out = vec![[F::zero(); 2]; count];
        let mut inf_out = vec![0u8; count];
        check(unsafe {
            ffi::ecfft_curve_point_mul(F::FIELD_ID, device, a.as_ptr().cast(), b.as_ptr().cast(), a.len(), points.as_ptr().cast(),
                if inf.is_empty() { core::ptr::null() } else { inf.as_ptr() }, scalars.as_ptr().cast(), nscalars, scalar_bytes, out.as_mut_ptr().cast(),
                inf_out.as_mut_ptr(), count)
        });
        (out, inf_out)
    }

    /// the smallest i <= cap with 2^i P the identity, -1 when there is none (ecfft_curve_point_two_adicity <-> `two_adicity`,
    /// src/utils.rs:356-365)
    pub fn curve_point_two_adicity(a: &[F], b: &[F], points: &[[F; 2]], cap: u32, inf: &[u8], device: i32) -> Vec<i32> {
        assert_eq!(core::mem::size_of::<F>(), F::ELEM_BYTES, "unexpected in-memory size of the field element");
        let count = points.len();
        assert!(count > 0 && a.len() == b.len() && (a.len() == 1 || a.len() == count), "one curve, or one per point");
        assert!(inf.is_empty() || inf.len() == count, "inf: one byte per point");
        let mut out = vec![0i32; count];
        check(unsafe {
            ffi::ecfft_curve_point_two_adicity(F::FIELD_ID, device, a.as_ptr().cast(), b.as_ptr().cast(), a.len(), points.as_ptr().cast(),
                if inf.is_empty() { core::ptr::null() } else { inf.as_ptr() }, cap, out.as_mut_ptr(), count)
        });
        out
    }

    /// The arguments of `build_ec_fftree` from a curve and its number of points as `curve_cardinality` returns it
    /// (ecfft_curve_find_generator): `None` when the window `start .. start + max_candidates` holds no point of order 2^v.
    pub fn curve_find_generator(a: &F, b: &F, order: &[u8; 40], start: u64, max_candidates: u64, device: i32) -> Option<FoundGenerator<F>> {
        assert_eq!(core::mem::size_of::<F>(), F::ELEM_BYTES, "unexpected in-memory size of the field element");
        let (mut log_order, mut x) = (0u32, 0u64);
        let (mut gen, mut offset) = ([F::zero(); 2], [F::zero(); 2]);
        check(unsafe {
            ffi::ecfft_curve_find_generator(F::FIELD_ID, device, (a as *const F).cast(), (b as *const F).cast(), order.as_ptr().cast(), start, max_candidates,
                &mut log_order, gen.as_mut_ptr().cast(), offset.as_mut_ptr().cast(), &mut x)
        });
        (log_order != 0).then_some(FoundGenerator { log_order, x, gen, offset })
    }

    /// `build_ec_fftree(subgroup_generator, subgroup_order, coset_offset, n)` (src/ec.rs:498-554) on y^2 = x^3 + a x + b
    /// (ecfft_build_ec_fftree): `None` when log2 n exceeds the generator's log order
    pub fn build_ec_fftree(n: usize, a: &F, b: &F, gen: &[F; 2], gen_log_order: u32, offset: &[F; 2], device: i32) -> Option<Self> {
        assert_eq!(core::mem::size_of::<F>(), F::ELEM_BYTES, "unexpected in-memory size of the field element");
        let mut ctx = core::ptr::null_mut();
        match unsafe {
            ffi::ecfft_build_ec_fftree(F::FIELD_ID, n, (a as *const F).cast(), (b as *const F).cast(), gen.as_ptr().cast(), gen_log_order,
                offset.as_ptr().cast(), device, &mut ctx)
        } {
            ffi::ERR_TREE_TOO_LARGE => None,
            rc => {
                check(rc);
                Some(Self { ctx, _f: PhantomData })
            }
        }
    }

    /// Mirror an existing CPU tree on the device (`FFTree::new(leaves, rational_maps)`, src/fftree.rs:42-70): the point set
    /// comes from the crate, every table is recomputed on the GPU.
    pub fn from_cpu_tree(tree: &ecfft::FFTree<F>, device: i32) -> Self {
        let leaves = tree.f.leaves();
        let n = leaves.len();
        // each map as 3 numerator + 3 denominator coefficients, low -> high, zero padded (ecfft_hip.h)
        let mut num = vec![F::zero(); 3 * tree.rational_maps.len()];
        let mut den = vec![F::zero(); 3 * tree.rational_maps.len()];
        for (k, map) in tree.rational_maps.iter().enumerate() {
            for (j, c) in map.numerator.coeffs.iter().enumerate() {
                num[3 * k + j] = *c;
            }
            for (j, c) in map.denominator.coeffs.iter().enumerate() {
                den[3 * k + j] = *c;
            }
        }
        let mut ctx = core::ptr::null_mut();
        check(unsafe { ffi::ecfft_fftree_new(F::FIELD_ID, leaves.as_ptr().cast(), n, num.as_ptr().cast(), den.as_ptr().cast(), device, &mut ctx) });
        Self { ctx, _f: PhantomData }
    }

    /// number of leaves of the top tree
    pub fn size(&self) -> usize {
        unsafe { ffi::ecfft_tree_size(self.ctx) }
    }

    fn out_vec(len: usize) -> Vec<F> {
        Vec::<F>::with_capacity(len)
    }

    /// `FFTree::enter` (src/fftree.rs:164-167)
    pub fn enter(&self, coeffs: &[F]) -> Vec<F> {
        let mut out = Self::out_vec(coeffs.len());
        check(unsafe { ffi::ecfft_enter(self.ctx, coeffs.as_ptr().cast(), out.as_mut_ptr().cast(), coeffs.len(), ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(coeffs.len()) };
        out
    }

    /// `FFTree::exit` (src/fftree.rs:227-230)
    pub fn exit(&self, evals: &[F]) -> Vec<F> {
        let mut out = Self::out_vec(evals.len());
        check(unsafe { ffi::ecfft_exit(self.ctx, evals.as_ptr().cast(), out.as_mut_ptr().cast(), evals.len(), ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(evals.len()) };
        out
    }

    /// `FFTree::extend` (src/fftree.rs:123-126); `moiety` names the TARGET moiety
    pub fn extend(&self, evals: &[F], moiety: Moiety) -> Vec<F> {
        let mut out = Self::out_vec(evals.len());
        check(unsafe { ffi::ecfft_extend(self.ctx, evals.as_ptr().cast(), out.as_mut_ptr().cast(), evals.len(), moiety_id(moiety), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(evals.len()) };
        out
    }

    /// `a * b` in coefficient form (ecfft_poly_mul; no reference counterpart): `a.len() + b.len() - 1` coefficients; the tree must hold
    /// `next_pow2(a.len() + b.len() - 1)` leaves.  `mul(a, a)` is a squaring.
    pub fn mul(&self, a: &[F], b: &[F]) -> Vec<F> {
        assert!(!a.is_empty() && !b.is_empty());
        let n = a.len() + b.len() - 1;
        let mut out = Self::out_vec(n);
        check(unsafe { ffi::ecfft_poly_mul(self.ctx, a.as_ptr().cast(), a.len(), b.as_ptr().cast(), b.len(), out.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(n) };
        out
    }

    /// `ecfft::utils::div_rem` (src/utils.rs:184-193) with the quotient too: `(q, r)` with `a = b*q + r`, `deg r < deg b`; `q` has
    /// `a.len() - b.len() + 1` coefficients (none when `a` is shorter), `r` has `b.len() - 1`, zero-padded above its degree.
    /// `b`'s last coefficient must be nonzero.  Tree rule: include/ecfft_hip.h.
    pub fn div_rem(&self, a: &[F], b: &[F]) -> (Vec<F>, Vec<F>) {
        assert!(!a.is_empty() && !b.is_empty());
        let nq = if a.len() >= b.len() { a.len() - b.len() + 1 } else { 0 };
        let nr = b.len() - 1;
        let mut q = Self::out_vec(nq);
        let mut r = Self::out_vec(nr);
        let pq = if nq > 0 { q.as_mut_ptr().cast() } else { core::ptr::null_mut() };
        let pr = if nr > 0 { r.as_mut_ptr().cast() } else { core::ptr::null_mut() };
        check(unsafe { ffi::ecfft_poly_divrem(self.ctx, a.as_ptr().cast(), a.len(), b.as_ptr().cast(), b.len(), pq, pr, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe {
            q.set_len(nq);
            r.set_len(nr);
        }
        (q, r)
    }

    /// `1/f mod x^k` (ecfft_poly_inv_series; no reference counterpart): `k` coefficients, `f[0]` nonzero; the tree must hold
    /// `next_pow2(2k - 1)` leaves.
    pub fn inv_series(&self, f: &[F], k: usize) -> Vec<F> {
        assert!(!f.is_empty() && k > 0);
        let mut out = Self::out_vec(k);
        check(unsafe { ffi::ecfft_poly_inv_series(self.ctx, f.as_ptr().cast(), f.len(), out.as_mut_ptr().cast(), k, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(k) };
        out
    }

    /// `f` at arbitrary points (ecfft_poly_eval_points; no reference counterpart): `out[i] = f(points[i])`.  `f.len() <= 64` works on
    /// any tree; a longer `f` needs a tree of `next_pow2(f.len())` leaves.
    pub fn eval_points(&self, f: &[F], points: &[F]) -> Vec<F> {
        assert!(!f.is_empty() && !points.is_empty());
        let mut out = Self::out_vec(points.len());
        check(unsafe { ffi::ecfft_poly_eval_points(self.ctx, f.as_ptr().cast(), f.len(), points.as_ptr().cast(), points.len(), out.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(points.len()) };
        out
    }

    /// The polynomial through arbitrary points (ecfft_poly_interpolate; no reference counterpart), the inverse of `eval_points`:
    /// the coefficients of `f` of degree `< points.len()` with `f(points[i]) = values[i]`.  The points must be pairwise distinct
    /// (a repeated point panics like any other argument error).  Up to 64 points work on any tree; more need a tree of
    /// `next_pow2(points.len())` leaves.
    pub fn interpolate(&self, points: &[F], values: &[F]) -> Vec<F> {
        assert!(!points.is_empty() && points.len() == values.len());
        let mut out = Self::out_vec(points.len());
        check(unsafe { ffi::ecfft_poly_interpolate(self.ctx, points.as_ptr().cast(), points.len(), values.as_ptr().cast(), out.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(points.len()) };
        out
    }

    /// `ecfft::utils::pow_mod` (src/utils.rs:194-211): `a^exp mod modulus` as `modulus.len() - 1` coefficients, zero-padded above
    /// the degree.  `exp_le` holds the exponent as little-endian bytes (`BigUint::to_bytes_le`; empty or all zero gives 1).  The
    /// modulus has at least 2 coefficients, the last one nonzero.  Up to 65 modulus coefficients work on any tree; tree rule:
    /// include/ecfft_hip.h.
    pub fn pow_mod(&self, a: &[F], exp_le: &[u8], modulus: &[F]) -> Vec<F> {
        assert!(!a.is_empty() && modulus.len() >= 2);
        let n = modulus.len() - 1;
        let mut out = Self::out_vec(n);
        let pe = if exp_le.is_empty() { core::ptr::null() } else { exp_le.as_ptr().cast() };
        check(unsafe { ffi::ecfft_poly_pow_mod(self.ctx, a.as_ptr().cast(), a.len(), pe, exp_le.len(), modulus.as_ptr().cast(), modulus.len(), out.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(n) };
        out
    }

    /// `div_rem(&a.naive_mul(&b), modulus)`, the step of `ecfft::utils::pow_mod` (src/utils.rs:205, 207): `modulus.len() - 1`
    /// coefficients, zero-padded above the degree.
    pub fn mul_mod(&self, a: &[F], b: &[F], modulus: &[F]) -> Vec<F> {
        assert!(!a.is_empty() && !b.is_empty() && modulus.len() >= 2);
        let n = modulus.len() - 1;
        let mut out = Self::out_vec(n);
        check(unsafe { ffi::ecfft_poly_mul_mod(self.ctx, a.as_ptr().cast(), a.len(), b.as_ptr().cast(), b.len(), modulus.as_ptr().cast(), modulus.len(), out.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(n) };
        out
    }

    /// `f(g) mod modulus` (ecfft_poly_compose_mod): the step of distinct-degree factorisation (src/utils.rs:52-78) and the product
    /// of two endomorphisms in examples/schoofs.rs:197-235, as `modulus.len() - 1` coefficients, zero-padded above the degree.  `f`
    /// may be longer than the modulus.  Up to `ECFFT_COMPOSE_SMALL_MAX` modulus coefficients work on any tree; above that the call
    /// runs about `2 sqrt(f.len())` modular products on the tree rule of `pow_mod` (include/ecfft_hip.h).
    pub fn compose_mod(&self, f: &[F], g: &[F], modulus: &[F]) -> Vec<F> {
        assert!(!f.is_empty() && !g.is_empty() && modulus.len() >= 2);
        let n = modulus.len() - 1;
        let mut out = Self::out_vec(n);
        check(unsafe { ffi::ecfft_poly_compose_mod(self.ctx, f.as_ptr().cast(), f.len(), g.as_ptr().cast(), g.len(), modulus.as_ptr().cast(), modulus.len(), out.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(n) };
        out
    }

    /// `ecfft::utils::gcd` (src/utils.rs:132-141): the monic gcd, trimmed to its degree (empty for `a = b = 0`).  The operands need
    /// not be trimmed and either may be zero; `gcd(0, b)` is monic `b`, as `utils::xgcd` has it (`utils::gcd` returns 0 there).  Up
    /// to `ECFFT_GCD_SMALL_MAX` coefficients work on any tree; tree rule: include/ecfft_hip.h.
    pub fn gcd(&self, a: &[F], b: &[F]) -> Vec<F> {
        assert!(!a.is_empty() && !b.is_empty());
        let n = a.len().max(b.len());
        let mut g = Self::out_vec(n);
        let mut deg: i64 = -1;
        check(unsafe { ffi::ecfft_poly_gcd(self.ctx, a.as_ptr().cast(), a.len(), b.as_ptr().cast(), b.len(), g.as_mut_ptr().cast(), &mut deg, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { g.set_len((deg + 1) as usize) };
        g
    }

    /// `ecfft::utils::xgcd` (src/utils.rs:147-182): `(s, t, gcd)` with `a*s + b*t = gcd`, the cofactors of the classical extended
    /// Euclidean algorithm; all three are trimmed to their degrees like the reference's `DensePolynomial`s (a zero cofactor is
    /// empty; `F::default()` is the field's zero), `gcd` is monic.
    pub fn xgcd(&self, a: &[F], b: &[F]) -> (Vec<F>, Vec<F>, Vec<F>) {
        assert!(!a.is_empty() && !b.is_empty());
        let (ns, nt, n) = ((b.len() - 1).max(1), (a.len() - 1).max(1), a.len().max(b.len()));
        let mut s = Self::out_vec(ns);
        let mut t = Self::out_vec(nt);
        let mut g = Self::out_vec(n);
        let mut deg: i64 = -1;
        check(unsafe { ffi::ecfft_poly_xgcd(self.ctx, a.as_ptr().cast(), a.len(), b.as_ptr().cast(), b.len(), s.as_mut_ptr().cast(), t.as_mut_ptr().cast(), g.as_mut_ptr().cast(), &mut deg, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe {
            s.set_len(ns);
            t.set_len(nt);
            g.set_len((deg + 1) as usize);
        }
        // trimmed like the DensePolynomials of the reference (and like HipFFTree::xgcd in include/ecfft_fftree.hpp)
        for v in [&mut s, &mut t] {
            while v.last().map_or(false, |c| *c == F::default()) {
                v.pop();
            }
        }
        (s, t, g)
    }

    /// `ecfft_poly_xgcd_partial` (no reference counterpart): `(r, s, t)` with `r = s*a + t*b`, the first row of the classical
    /// remainder sequence (`r_0 = a`, `r_1 = b`) with index `j >= 1` and `deg r < stop` (`deg 0 = -1`), scaled so that `t` is monic
    /// (`s` where `t = 0`); all three trimmed to their degrees.  What rational reconstruction, Pade approximation and Gao's decoder
    /// are built on.  Tree rule as `xgcd`: include/ecfft_hip.h.
    pub fn xgcd_partial(&self, a: &[F], b: &[F], stop: usize) -> (Vec<F>, Vec<F>, Vec<F>) {
        assert!(!a.is_empty() && !b.is_empty());
        let n = a.len().max(b.len());
        let mut r = Self::out_vec(n);
        let mut s = Self::out_vec(b.len());
        let mut t = Self::out_vec(a.len());
        let mut deg: [i64; 3] = [-1; 3];
        check(unsafe { ffi::ecfft_poly_xgcd_partial(self.ctx, a.as_ptr().cast(), a.len(), b.as_ptr().cast(), b.len(), stop, r.as_mut_ptr().cast(), s.as_mut_ptr().cast(), t.as_mut_ptr().cast(), deg.as_mut_ptr(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe {
            r.set_len((deg[0] + 1) as usize);
            s.set_len((deg[1] + 1) as usize);
            t.set_len((deg[2] + 1) as usize);
        }
        (r, s, t)
    }

    /// `ecfft_rs_decode` (no reference counterpart): Reed-Solomon decoding with errors by Gao's algorithm.  `points`: `m` pairwise
    /// distinct elements; `values`: the `m` received symbols; `1 <= k <= m`.  `Some((message, n_errors))`: the `k` coefficients of
    /// the unique `f` of degree `< k` whose codeword differs from `values` in at most `(m - k) / 2` positions, and how many did;
    /// `None` when there is none.  Up to `ECFFT_RS_SMALL_MAX` points work on any tree; tree rule: include/ecfft_hip.h.  Panics on
    /// two equal points.
    pub fn rs_decode(&self, points: &[F], values: &[F], k: usize) -> Option<(Vec<F>, usize)> {
        assert!(!points.is_empty() && points.len() == values.len() && k >= 1 && k <= points.len());
        let mut message = Self::out_vec(k);
        let mut n_errors: i64 = -1;
        check(unsafe { ffi::ecfft_rs_decode(self.ctx, points.as_ptr().cast(), points.len(), values.as_ptr().cast(), k, message.as_mut_ptr().cast(), &mut n_errors, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { message.set_len(k) };
        if n_errors < 0 {
            None
        } else {
            Some((message, n_errors as usize))
        }
    }

    /// `ecfft_rs_encode` (no reference counterpart): the systematic Reed-Solomon encoder.  `points`: `m` pairwise distinct elements;
    /// `data`: `1 <= k <= m` symbols.  Returns the `m` symbols of the `f` of degree `< k` with `f(points[i]) = data[i]` for `i < k`
    /// at all points: the data, then `m - k` parity symbols.  Up to `ECFFT_RS_SMALL_MAX` points work on any tree; tree rule:
    /// include/ecfft_hip.h.  Panics on two equal points.
    pub fn rs_encode(&self, points: &[F], data: &[F]) -> Vec<F> {
        assert!(!data.is_empty() && data.len() <= points.len());
        let mut codeword = Self::out_vec(points.len());
        check(unsafe { ffi::ecfft_rs_encode(self.ctx, points.as_ptr().cast(), points.len(), data.as_ptr().cast(), data.len(), codeword.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { codeword.set_len(points.len()) };
        codeword
    }

    /// `ecfft_rs_decode_erasures`: Reed-Solomon decoding with erasures and errors.  `erased[i] != 0` marks a lost symbol, whose value
    /// is never read (`None`: no erasure).  The result is `rs_decode` on the kept points and values: with `m'` of them, the `f` of
    /// degree `< k` within `(m' - k) / 2` errors, `None` when there is none or `m' < k`.  `Some((out, n_errors))`: the `k`
    /// coefficients of `f`, or with `codeword` its `m` symbols at all points — the erased positions filled in, the first `k` the
    /// corrected data of `rs_encode`'s code.  Tree rule and panics as `rs_decode`.
    pub fn rs_decode_erasures(&self, points: &[F], values: &[F], erased: Option<&[u8]>, k: usize, codeword: bool) -> Option<(Vec<F>, usize)> {
        assert!(!points.is_empty() && points.len() == values.len() && k >= 1 && k <= points.len());
        assert!(erased.map_or(true, |e| e.len() == points.len()));
        let n = if codeword { points.len() } else { k };
        let mut out = Self::out_vec(n);
        let mut n_errors: i64 = -1;
        let mask = erased.map_or(core::ptr::null(), |e| e.as_ptr());
        check(unsafe { ffi::ecfft_rs_decode_erasures(self.ctx, points.as_ptr().cast(), points.len(), values.as_ptr().cast(), mask, k, out.as_mut_ptr().cast(), if codeword { ffi::RS_OUT_CODEWORD } else { ffi::RS_OUT_COEFFS }, &mut n_errors, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(n) };
        if n_errors < 0 {
            None
        } else {
            Some((out, n_errors as usize))
        }
    }

    /// `ecfft_seq_min_poly` (no reference counterpart): the minimal polynomial of the sequence `seq` of `N` terms, what
    /// Berlekamp-Massey computes.  `Some(C)`: the monic `C = x^L + sum c_j x^j` of least degree with
    /// `s[i+L] + sum_j c_j s[i+j] = 0` for all `0 <= i < N - L`, as `L + 1` coefficients (`[1]` for a zero sequence), where
    /// `2 L <= N` makes it unique; `None` where the sequence is too short to determine it.  Up to `ECFFT_SEQ_SMALL_MAX` terms work
    /// on any tree; tree rule: include/ecfft_hip.h.
    pub fn seq_min_poly(&self, seq: &[F]) -> Option<Vec<F>> {
        assert!(!seq.is_empty());
        let n = seq.len() / 2 + 1;
        let mut c = Self::out_vec(n);
        let mut order: i64 = -1;
        check(unsafe { ffi::ecfft_seq_min_poly(self.ctx, seq.as_ptr().cast(), seq.len(), c.as_mut_ptr().cast(), &mut order, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        if order < 0 {
            None
        } else {
            unsafe { c.set_len(order as usize + 1) };
            Some(c)
        }
    }

    /// `ecfft_seq_nth_term` (no reference counterpart): the terms `s_K .. s_(K + nout - 1)` of the linear recurrence with the
    /// characteristic polynomial `char_poly` (`L + 1 >= 2` coefficients, a non-zero leading one; monic not required:
    /// `sum_{j<=L} c_j s[i+j] = 0`) and the `L` initial terms `init`; `index` is `K` in little-endian bytes of any length.  One power
    /// `x^K mod C` and `nout L` multiply-adds.  Up to `ECFFT_SEQ_TERM_SMALL_MAX` coefficients work on any tree; tree rule:
    /// include/ecfft_hip.h.  Panics on a zero leading coefficient.
    pub fn seq_nth_term(&self, char_poly: &[F], init: &[F], index: &[u8], nout: usize) -> Vec<F> {
        assert!(char_poly.len() >= 2 && init.len() == char_poly.len() - 1 && nout >= 1);
        let mut out = Self::out_vec(nout);
        let idx = if index.is_empty() { core::ptr::null() } else { index.as_ptr().cast() };
        check(unsafe { ffi::ecfft_seq_nth_term(self.ctx, char_poly.as_ptr().cast(), char_poly.len(), init.as_ptr().cast(), idx, index.len(), out.as_mut_ptr().cast(), nout, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(nout) };
        out
    }

    /// `ecfft::utils::find_roots` (src/utils.rs:25-44): the distinct roots of `f` in the field, in ascending order of their
    /// standard form (the reference sorts its result the same way).  `f` need not be trimmed and multiplicities do not matter; a
    /// non-zero constant has no roots.  Panics on the zero polynomial, as the reference does.  Deterministic: the splitting shifts
    /// are 1, 2, 3, ...  Up to `ECFFT_ROOTS_SMALL_MAX` coefficients work on any tree; tree rule: include/ecfft_hip.h.
    pub fn find_roots(&self, f: &[F]) -> Vec<F> {
        assert!(!f.is_empty());
        let n = f.len() - 1;
        let mut roots = Self::out_vec(n);
        let mut count: i64 = 0;
        let p = if n == 0 { core::ptr::null_mut() } else { roots.as_mut_ptr().cast() };
        check(unsafe { ffi::ecfft_poly_find_roots(self.ctx, f.as_ptr().cast(), f.len(), p, &mut count, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        assert!(count >= 0, "find_roots: the zero polynomial");
        unsafe { roots.set_len(count as usize) };
        roots
    }

    /// `ecfft::utils::distinct_degree_factors` (src/utils.rs:52-78) by its definition: degree `d` -> the monic product of the
    /// irreducible factors of degree `d` of `f`, with its leading 1.  (The reference takes `x^(p i)` for `x^(p^i)`, so it agrees at
    /// `d = 1` only, the degree its own `find_roots` uses.)  `f` need not be trimmed or squarefree; a non-zero constant gives an empty
    /// map.  Panics on the zero polynomial.  Up to `ECFFT_DDF_SMALL_MAX` coefficients work on any tree; tree rule:
    /// include/ecfft_hip.h.
    pub fn distinct_degree_factors(&self, f: &[F]) -> std::collections::BTreeMap<usize, Vec<F>> {
        assert!(!f.is_empty());
        let nd = core::cmp::max(f.len() - 1, 1);
        let mut fac = Self::out_vec(nd);
        let mut deg = vec![0i64; nd];
        check(unsafe { ffi::ecfft_poly_distinct_degree(self.ctx, f.as_ptr().cast(), f.len(), fac.as_mut_ptr().cast(), deg.as_mut_ptr(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        assert!(deg[0] >= 0, "distinct_degree_factors: the zero polynomial");
        unsafe { fac.set_len(nd) };
        let mut out = std::collections::BTreeMap::new();
        let mut pos = 0usize;
        for (i, &n) in deg.iter().enumerate() {
            if n > 0 {
                let mut g = fac[pos..pos + n as usize].to_vec();
                g.push(F::one());
                out.insert(i + 1, g);
                pos += n as usize;
            }
        }
        out
    }

    /// `ecfft::utils::equal_degree_factorization` (src/utils.rs:82-113): the monic irreducible factors of degree `d` of `f`, each
    /// with its leading 1, in ascending lexicographic order of `(c_0, .., c_(d-1))` as standard-form integers.  `f` must be a
    /// squarefree product of irreducibles of degree `d`, which is what `distinct_degree_factors` returns; it need not be trimmed or
    /// monic.  A non-zero constant gives an empty vector.  Panics on the zero polynomial and where `d` does not divide the degree.
    /// Deterministic: the shifts are 1, 2, 3, ... where the reference draws random polynomials.  Up to `ECFFT_EDF_SMALL_MAX`
    /// coefficients work on any tree; tree rule: include/ecfft_hip.h.
    pub fn equal_degree_factorization(&self, f: &[F], d: usize) -> Vec<Vec<F>> {
        assert!(!f.is_empty() && d > 0);
        let nd = core::cmp::max(f.len() - 1, 1);
        let mut fac = Self::out_vec(nd);
        let mut n = 0i64;
        check(unsafe { ffi::ecfft_poly_equal_degree(self.ctx, f.as_ptr().cast(), f.len(), d, fac.as_mut_ptr().cast(), &mut n, 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        assert!(n != -1, "equal_degree_factorization: the zero polynomial");
        assert!(n >= 0, "equal_degree_factorization: d does not divide the degree");
        unsafe { fac.set_len(nd) };
        (0..n as usize)
            .map(|i| {
                let mut q = fac[i * d..(i + 1) * d].to_vec();
                q.push(F::one());
                q
            })
            .collect()
    }

    /// Yun's squarefree decomposition `f = lead * prod_i a_i^i` (`ecfft_poly_squarefree_decompose`; the reference's
    /// `square_free_factors`, src/utils.rs:46-50, returns `prod a_i` only): the leading coefficient and multiplicity `i` -> the monic
    /// `a_i` of positive degree with its leading 1, the `a_i` squarefree and pairwise coprime.  `f` need not be trimmed; a non-zero
    /// constant gives an empty map.  Panics on the zero polynomial.  Up to `ECFFT_FACTOR_SMALL_MAX` coefficients work on any tree;
    /// tree rule: include/ecfft_hip.h.
    pub fn square_free_decomposition(&self, f: &[F]) -> (F, std::collections::BTreeMap<usize, Vec<F>>) {
        assert!(!f.is_empty());
        let nd = core::cmp::max(f.len() - 1, 1);
        let mut parts = Self::out_vec(nd);
        let mut lead = Self::out_vec(1);
        let mut deg = vec![0i64; nd];
        check(unsafe { ffi::ecfft_poly_squarefree_decompose(self.ctx, f.as_ptr().cast(), f.len(), parts.as_mut_ptr().cast(), deg.as_mut_ptr(), lead.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        assert!(deg[0] >= 0, "square_free_decomposition: the zero polynomial");
        unsafe { parts.set_len(nd); lead.set_len(1) };
        let mut out = std::collections::BTreeMap::new();
        let mut pos = 0usize;
        for (i, &n) in deg.iter().enumerate() {
            if n > 0 {
                let mut a = parts[pos..pos + n as usize].to_vec();
                a.push(F::one());
                out.insert(i + 1, a);
                pos += n as usize;
            }
        }
        (lead[0], out)
    }

    /// The factorisation `f = lead * prod_j q_j^e_j` over the distinct monic irreducible `q_j` (`ecfft_poly_factor`: the reference's
    /// `square_free_factors`, `distinct_degree_factors` and `equal_degree_factorization`, src/utils.rs:25-113, for every degree and
    /// with the multiplicities): the leading coefficient and the `(q_j, e_j)`, `q_j` with its leading 1, in ascending
    /// `(e_j, deg q_j, the order of equal_degree_factorization)`.  Deterministic.  `f` need not be trimmed; a non-zero constant gives
    /// an empty vector.  Panics on the zero polynomial.  Up to `ECFFT_FACTOR_SMALL_MAX` coefficients work on any tree; tree rule:
    /// include/ecfft_hip.h.
    pub fn factor(&self, f: &[F]) -> (F, Vec<(Vec<F>, usize)>) {
        assert!(!f.is_empty());
        let nd = core::cmp::max(f.len() - 1, 1);
        let mut fac = Self::out_vec(nd);
        let mut lead = Self::out_vec(1);
        let (mut fdeg, mut fmult) = (vec![0i64; nd], vec![0i64; nd]);
        let mut n = 0i64;
        check(unsafe { ffi::ecfft_poly_factor(self.ctx, f.as_ptr().cast(), f.len(), fac.as_mut_ptr().cast(), fdeg.as_mut_ptr(), fmult.as_mut_ptr(), &mut n, lead.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        assert!(n >= 0, "factor: the zero polynomial");
        unsafe { fac.set_len(nd); lead.set_len(1) };
        let mut out = Vec::with_capacity(n as usize);
        let mut pos = 0usize;
        for j in 0..n as usize {
            let d = fdeg[j] as usize;
            let mut q = fac[pos..pos + d].to_vec();
            q.push(F::one());
            out.push((q, fmult[j] as usize));
            pos += d;
        }
        (lead[0], out)
    }

    /// `division_polynomial(n, &curve)` (examples/schoofs.rs:368-431) for y^2 = x^3 + a x + b: the L(n) coefficients of psi_n, low
    /// to high, not monic, the factor 2y of an even index removed.  `n <= 4` on any tree, otherwise next_pow2(L(n)) leaves.
    pub fn division_polynomial(&self, a: &F, b: &F, n: usize) -> Vec<F> {
        let len = if n < 2 { 1 } else if n & 1 == 1 { (n * n - 1) / 2 + 1 } else { (n * n - 4) / 2 + 1 };
        let mut out = Self::out_vec(len);
        check(unsafe { ffi::ecfft_division_polynomial(self.ctx, (a as *const F).cast(), (b as *const F).cast(), n, out.as_mut_ptr().cast(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(len) };
        out
    }

    /// `frobenius_trace_mod_l` / `has_even_order` (examples/schoofs.rs:76-138, 345-366): t mod l with #E = p + 1 - t for the curves
    /// y^2 = x^3 + a[i] x + b[i]; -1 for a singular curve.  `l` is 2 or an odd prime up to `ECFFT_SCHOOF_MAX_L`; `l <= 11` on
    /// any tree, otherwise next_pow2(2 L(l) - 1) leaves.
    pub fn curve_trace_mod(&self, a: &[F], b: &[F], l: usize) -> Vec<i64> {
        assert!(!a.is_empty() && a.len() == b.len());
        let mut t = vec![0i64; a.len()];
        check(unsafe { ffi::ecfft_curve_trace_mod(self.ctx, a.as_ptr().cast(), b.as_ptr().cast(), l, t.as_mut_ptr(), a.len(), ffi::MEM_HOST, core::ptr::null_mut()) });
        t
    }

    /// `cardinality(curve)` (examples/schoofs.rs:30-71): #E(F_p) of y^2 = x^3 + a x + b as 40 little-endian bytes, zero for a
    /// singular curve.  Needs the tree of the largest prime of the rule (include/ecfft_hip.h).
    pub fn curve_cardinality(&self, a: &F, b: &F) -> [u8; 40] {
        let mut order = [0u8; 40];
        check(unsafe { ffi::ecfft_curve_cardinality(self.ctx, (a as *const F).cast(), (b as *const F).cast(), order.as_mut_ptr().cast(), core::ptr::null_mut(), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        order
    }

    /// `FFTree::mextend` (src/fftree.rs:138-141)
    pub fn mextend(&self, evals: &[F], moiety: Moiety) -> Vec<F> {
        let mut out = Self::out_vec(evals.len());
        check(unsafe { ffi::ecfft_mextend(self.ctx, evals.as_ptr().cast(), out.as_mut_ptr().cast(), evals.len(), moiety_id(moiety), 1, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(evals.len()) };
        out
    }

    /// `FFTree::degree` (src/fftree.rs:195-198)
    pub fn degree(&self, evals: &[F]) -> usize {
        let mut d = 0usize;
        check(unsafe { ffi::ecfft_degree(self.ctx, evals.as_ptr().cast(), evals.len(), ffi::MEM_HOST, core::ptr::null_mut(), &mut d) });
        d
    }

    fn redc(&self, evals: &[F], a: &[F], moiety: i32) -> Vec<F> {
        assert_eq!(evals.len(), a.len());
        let mut out = Self::out_vec(evals.len());
        check(unsafe { ffi::ecfft_redc(self.ctx, evals.as_ptr().cast(), a.as_ptr().cast(), out.as_mut_ptr().cast(), evals.len(), moiety, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(evals.len()) };
        out
    }
    /// `FFTree::redc_z0` (src/fftree.rs:264-267)
    pub fn redc_z0(&self, evals: &[F], a: &[F]) -> Vec<F> {
        self.redc(evals, a, 0)
    }
    /// `FFTree::redc_z1` (src/fftree.rs:272-275)
    pub fn redc_z1(&self, evals: &[F], a: &[F]) -> Vec<F> {
        self.redc(evals, a, 1)
    }

    /// `FFTree::modular_reduce` (src/fftree.rs:286-289)
    pub fn modular_reduce(&self, evals: &[F], a: &[F], c: &[F]) -> Vec<F> {
        assert_eq!(evals.len(), a.len());
        assert_eq!(evals.len(), c.len());
        let mut out = Self::out_vec(evals.len());
        check(unsafe {
            ffi::ecfft_modular_reduce(self.ctx, evals.as_ptr().cast(), a.as_ptr().cast(), c.as_ptr().cast(), out.as_mut_ptr().cast(), evals.len(), ffi::MEM_HOST, core::ptr::null_mut())
        });
        unsafe { out.set_len(evals.len()) };
        out
    }

    /// `FFTree::vanish` (src/fftree.rs:313-316): 2 * domain.len() evaluations
    pub fn vanish(&self, domain: &[F]) -> Vec<F> {
        let mut out = Self::out_vec(2 * domain.len());
        check(unsafe { ffi::ecfft_vanish(self.ctx, domain.as_ptr().cast(), out.as_mut_ptr().cast(), domain.len(), ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(2 * domain.len()) };
        out
    }

    /// batched ENTER (no reference counterpart): `count` polynomials of length n laid end to end share every launch
    pub fn enter_many(&self, coeffs: &[F], n: usize) -> Vec<F> {
        assert!(n > 0 && coeffs.len() % n == 0);
        let mut out = Self::out_vec(coeffs.len());
        check(unsafe { ffi::ecfft_enter_many(self.ctx, coeffs.as_ptr().cast(), out.as_mut_ptr().cast(), n, coeffs.len() / n, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(coeffs.len()) };
        out
    }
    pub fn exit_many(&self, evals: &[F], n: usize) -> Vec<F> {
        assert!(n > 0 && evals.len() % n == 0);
        let mut out = Self::out_vec(evals.len());
        check(unsafe { ffi::ecfft_exit_many(self.ctx, evals.as_ptr().cast(), out.as_mut_ptr().cast(), n, evals.len() / n, ffi::MEM_HOST, core::ptr::null_mut()) });
        unsafe { out.set_len(evals.len()) };
        out
    }

    /// one of the `pub` tables of the subtree with `m` leaves (src/fftree.rs:24-38), `which` = `ffi::TBL_*`
    pub fn table(&self, m: usize, which: i32) -> Vec<F> {
        let mut cnt = 0usize;
        check(unsafe { ffi::ecfft_tree_table(self.ctx, m, which, core::ptr::null_mut(), 0, &mut cnt) });
        let mut out = Self::out_vec(cnt);
        check(unsafe { ffi::ecfft_tree_table(self.ctx, m, which, out.as_mut_ptr().cast(), cnt, &mut cnt) });
        unsafe { out.set_len(cnt) };
        out
    }
    pub fn xnn_s(&self, m: usize) -> Vec<F> {
        self.table(m, ffi::TBL_XNN_S)
    }
    pub fn z0z0_rem_xnn_s(&self, m: usize) -> Vec<F> {
        self.table(m, ffi::TBL_Z0Z0_REM_XNN_S)
    }
    /// leaves of the subtree with m leaves = `subtree_with_size(m).f.leaves()` (src/fftree.rs:471-478)
    pub fn eval_domain(&self, m: usize) -> Vec<F> {
        self.table(m, ffi::TBL_F).split_off(m)
    }

    /// `CanonicalSerialize::serialize_compressed / serialize_uncompressed` of `FFTree<F>` (src/fftree.rs:510-554): the bytes the
    /// crate itself would write for this tree (`ark_serialize::Compress::Yes` leaves the three inverse tables out, :536-541)
    pub fn serialize(&self, compress: ark_serialize::Compress) -> Vec<u8> {
        let c = matches!(compress, ark_serialize::Compress::Yes) as i32;
        let mut len = 0usize;
        check(unsafe { ffi::ecfft_fftree_serialize(self.ctx, c, core::ptr::null_mut(), 0, &mut len) });
        let mut buf = vec![0u8; len];
        check(unsafe { ffi::ecfft_fftree_serialize(self.ctx, c, buf.as_mut_ptr().cast(), len, &mut len) });
        buf
    }
    /// `CanonicalDeserialize::deserialize_compressed / deserialize_uncompressed` (src/fftree.rs:600-660): a file written by the crate
    /// (`README.md:26-41` build.rs flow) becomes a device-resident tree.  `verify`: compare every table of the file with the one
    /// recomputed from its point set and reject the file (`None`) on a mismatch; malformed input is `None` as well.
    /// Prefer [`Self::deserialize_checked`]: with `verify = false` only the layers of `f` are checked and every other table is
    /// recomputed from the point set, whereas the reference would use the file's tables verbatim.
    pub fn deserialize(bytes: &[u8], compress: ark_serialize::Compress, device: i32, verify: bool) -> Option<Self> {
        let c = matches!(compress, ark_serialize::Compress::Yes) as i32;
        let mut ctx = core::ptr::null_mut();
        match unsafe { ffi::ecfft_fftree_deserialize(F::FIELD_ID, bytes.as_ptr().cast(), bytes.len(), c, device, verify as i32, &mut ctx) } {
            ffi::ERR_BAD_ARG | ffi::ERR_NOT_POW2 => None,
            rc => {
                check(rc);
                Some(Self { ctx, _f: PhantomData })
            }
        }
    }
    /// `deserialize` with every table of the file verified against the tree rebuilt from its point set (the safe default)
    pub fn deserialize_checked(bytes: &[u8], compress: ark_serialize::Compress, device: i32) -> Option<Self> {
        Self::deserialize(bytes, compress, device, true)
    }
    /// the `pub rational_maps` field (src/fftree.rs:28) as (numerator, denominator) coefficient triples, low -> high, zero padded
    pub fn rational_maps(&self) -> Vec<([F; 3], [F; 3])> {
        let ln = self.size().trailing_zeros() as usize;
        let mut num = vec![F::zero(); 3 * ln.max(1)];
        let mut den = vec![F::zero(); 3 * ln.max(1)];
        check(unsafe { ffi::ecfft_tree_rational_maps(self.ctx, num.as_mut_ptr().cast(), den.as_mut_ptr().cast()) });
        (0..ln).map(|k| ([num[3 * k], num[3 * k + 1], num[3 * k + 2]], [den[3 * k], den[3 * k + 1], den[3 * k + 2]])).collect()
    }
    /// give the pooled temporaries of the algorithm wrappers back to the device (ecfft_ctx_trim)
    pub fn trim(&self) {
        check(unsafe { ffi::ecfft_ctx_trim(self.ctx) });
    }

    /// `FFTree::subtree_with_size` (src/fftree.rs:489-496): the chain lives in one context, so this is a size check
    pub fn subtree_with_size(&self, n: usize) -> &Self {
        assert!(n.is_power_of_two());
        if n > self.size() {
            panic!("FFTree is too small");
        }
        self
    }

    /// raw context for device-resident use (`ECFFT_MEM_DEVICE` + a HIP stream) through `ffi`
    pub fn raw(&self) -> *mut ffi::EcfftCtx {
        self.ctx
    }
}

/// What a maintainer of the reference crate would add behind a cargo feature: route the three hot methods of `FFTree<F>`
/// to the device tree, keep everything else on the CPU tree.
pub struct Accelerated<F: HipField> {
    pub cpu: ecfft::FFTree<F>,
    pub gpu: HipFFTree<F>,
}
impl<F: HipField> Accelerated<F> {
    pub fn build_fftree(n: usize) -> Option<Self> {
        let cpu = F::build_fftree(n)?;
        let gpu = HipFFTree::from_cpu_tree(&cpu, 0);
        Some(Self { cpu, gpu })
    }
    pub fn enter(&self, coeffs: &[F]) -> Vec<F> {
        self.gpu.enter(coeffs)
    }
    pub fn exit(&self, evals: &[F]) -> Vec<F> {
        self.gpu.exit(evals)
    }
    pub fn extend(&self, evals: &[F], moiety: Moiety) -> Vec<F> {
        self.gpu.extend(evals, moiety)
    }
}

#[allow(dead_code)]
fn _assert_void_ptr_is_used(_: *const c_void) {}
