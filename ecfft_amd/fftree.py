"""Host-side mirror of the reference's `FFTree<F>` / `FftreeField` surface over the C-ABI library.

Reference interface mirrored (names, argument meaning, error behaviour):
    trait FftreeField { fn build_fftree(n) -> Option<FFTree<Self>> }      /root/reference/src/lib.rs:14-16
    enum Moiety { S0, S1 }                                                 src/fftree.rs:17-21
    FFTree::{new, extend, enter, exit, subtree_with_size} + pub tables     src/fftree.rs:24-38, 42, 123, 164, 227, 489

Elements are passed in the crate's in-memory representation (secp256k1: uint64[n, 4] Montgomery limbs;
m31: uint32[n]) as numpy arrays (host) or torch CUDA tensors (device-resident, zero copy).  Where the
reference panics this raises: ValueError("FFTree is too small") / AssertionError for non powers of two.
There is no CPU fallback: if libecfft_hip.so or a HIP device is missing the call fails loudly.
"""
import ctypes
import enum
import os

import numpy as np

from . import build as _build

_DIR = os.path.dirname(os.path.abspath(__file__))

OK, ERR_NOT_POW2, ERR_TREE_TOO_SMALL, ERR_TREE_TOO_LARGE, ERR_HIP, ERR_BAD_ARG = range(6)
MEM_HOST, MEM_DEVICE = 0, 1
TBL_F, TBL_RECOMBINE, TBL_DECOMPOSE, TBL_XNN_S, TBL_XNN_S_INV, TBL_Z0_S1, TBL_Z1_S0, TBL_Z0_INV_S1, TBL_Z1_INV_S0, TBL_Z0Z0, TBL_Z1Z1 = range(11)

EXPORTS = ["ecfft_elem_size", "ecfft_build_fftree", "ecfft_fftree_new", "ecfft_ctx_destroy", "ecfft_tree_size",
           "ecfft_field", "ecfft_enter", "ecfft_exit", "ecfft_extend", "ecfft_tree_table", "ecfft_build_points",
           "ecfft_device_info", "ecfft_profile_enable", "ecfft_profile_classes", "ecfft_profile_read",
           "ecfft_extend_top_cyclic", "ecfft_extend_local_block",
           "ecfft_mul_ceiling", "ecfft_elems_to_standard", "ecfft_elems_from_standard", "ecfft_table_fma", "ecfft_enter_many", "ecfft_exit_many", "ecfft_mextend", "ecfft_redc", "ecfft_modular_reduce", "ecfft_vanish", "ecfft_degree",
           "ecfft_comm_get_unique_id", "ecfft_comm_init_rank", "ecfft_comm_init_callback", "ecfft_comm_destroy", "ecfft_comm_rank", "ecfft_comm_world",
           "ecfft_comm_stats_enable", "ecfft_comm_stats_read", "ecfft_extend_sharded", "ecfft_enter_sharded", "ecfft_exit_sharded", "ecfft_device_copy", "ecfft_shader_clock", "ecfft_device_alloc", "ecfft_device_free", "ecfft_device_sync", "ecfft_build_extend_shard", "ecfft_ctx_device_bytes", "ecfft_extend_sharded_layout", "ecfft_build_enter_shard", "ecfft_build_exit_shard", "ecfft_build_exit_shard_opts",
           "ecfft_fftree_serialize", "ecfft_fftree_deserialize", "ecfft_tree_rational_maps", "ecfft_ctx_trim", "ecfft_comm_abort", "ecfft_comm_set_rccl_library", "ecfft_comm_set_link_striping",
           "ecfft_poly_mul", "ecfft_poly_inv_series", "ecfft_poly_divrem", "ecfft_poly_eval_points", "ecfft_poly_interpolate",
           "ecfft_poly_pow_mod", "ecfft_poly_mul_mod", "ecfft_poly_gcd", "ecfft_poly_xgcd", "ecfft_poly_xgcd_partial", "ecfft_rs_decode", "ecfft_rs_encode", "ecfft_rs_decode_erasures", "ecfft_seq_min_poly", "ecfft_seq_nth_term", "ecfft_poly_find_roots",
           "ecfft_poly_compose_mod", "ecfft_poly_squarefree", "ecfft_poly_distinct_degree", "ecfft_poly_equal_degree", "ecfft_poly_squarefree_decompose", "ecfft_poly_factor", "ecfft_division_polynomial", "ecfft_curve_trace_mod", "ecfft_curve_cardinality",
           "ecfft_find_curve_candidate", "ecfft_curve_two_sylow", "ecfft_find_curve", "ecfft_build_fftree_on_curve",
           "ecfft_curve_point_mul", "ecfft_curve_point_two_adicity", "ecfft_curve_find_generator", "ecfft_build_ec_fftree"]
# include/ecfft_hip.h ECFFT_GCD_SMALL_MAX: max(na, nb) up to which a gcd runs in one workgroup per pair, on any tree
GCD_SMALL_MAX = 256
# include/ecfft_hip.h ECFFT_XGCD_PARTIAL_SMALL_MAX: max(na, nb) up to which poly_xgcd_partial runs all pairs in one launch, on any tree
XGCD_PARTIAL_SMALL_MAX = 256
# include/ecfft_hip.h ECFFT_RS_SMALL_MAX: code length m up to which rs_decode decodes a row in one workgroup, on any tree
RS_SMALL_MAX = 255
# include/ecfft_hip.h ECFFT_RS_OUT_*: what rs_decode_erasures writes, the k coefficients of f or its m re-encoded symbols
RS_OUT_COEFFS, RS_OUT_CODEWORD = 0, 1
# include/ecfft_hip.h ECFFT_SEQ_SMALL_MAX: terms N up to which seq_min_poly finds a row's minimal polynomial in one workgroup, on any tree
SEQ_SMALL_MAX = 255
# include/ecfft_hip.h ECFFT_SEQ_TERM_SMALL_MAX: nc up to which seq_nth_term takes the terms of a row in one workgroup, on any tree
SEQ_TERM_SMALL_MAX = 65
# include/ecfft_hip.h ECFFT_ROOTS_SMALL_MAX: nf up to which poly_find_roots finishes a polynomial in one workgroup, on any tree
ROOTS_SMALL_MAX = 65
# include/ecfft_hip.h ECFFT_COMPOSE_SMALL_MAX: nm up to which poly_compose_mod runs Horner for a triple in one workgroup, on any tree
COMPOSE_SMALL_MAX = 65
# include/ecfft_hip.h ECFFT_DDF_SMALL_MAX: nf up to which poly_squarefree / poly_distinct_degree finish a polynomial in one workgroup, on any tree
DDF_SMALL_MAX = 65
# include/ecfft_hip.h ECFFT_EDF_SMALL_MAX: ng up to which poly_equal_degree finishes a polynomial in one workgroup, on any tree
EDF_SMALL_MAX = 65
# include/ecfft_hip.h ECFFT_FACTOR_SMALL_MAX: nf up to which poly_squarefree_decompose / poly_factor run on workgroup kernels alone, on any tree
FACTOR_SMALL_MAX = 65
# include/ecfft_hip.h ECFFT_SCHOOF_SMALL_MAX / ECFFT_SCHOOF_MAX_L / ECFFT_ORDER_BYTES: coefficients of a modulus that one workgroup of
# curve_trace_mod finishes; the largest prime l and the largest index of division_polynomial; bytes of an order
SCHOOF_SMALL_MAX = 65
SCHOOF_MAX_L = 199
ORDER_BYTES = 40

# include/ecfft_hip_hooks.h: only in a build with -DECFFT_TEST_HOOKS (tests/hooks/libecfft_hip_hooks.so), never in the shipped library
HOOK_EXPORTS = ['ecfft_selftest_field', 'ecfft_selfcheck_pointwise_z', 'ecfft_test_fail_next_collective', 'ecfft_selftest_blk16', 'ecfft_selftest_blk16_small', 'ecfft_test_fail_build_rank', 'ecfft_comm_init_projection', 'ecfft_selftest_blk32', 'ecfft_ctx_low_map', 'ecfft_curve_search_stats', 'ecfft_test_ddf_iterate', 'ecfft_test_schoof_pi2', 'ecfft_ctx_exit_cores', 'ecfft_ctx_exit_low_cores', 'ecfft_ctx_sym_bfly', 'ecfft_ctx_low_sym', 'ecfft_ctx_enter_l11']

EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p),
                               ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p),
                               ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p)


class Moiety(enum.IntEnum):
    S0 = 0
    S1 = 1


class EcfftError(RuntimeError):
    pass


_lib = None
HOOKS_LIB = os.path.join(os.path.dirname(_DIR), "tests", "hooks", "libecfft_hip_hooks.so")


def _bind(L):
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.ecfft_elem_size.restype, L.ecfft_elem_size.argtypes = sz, [ci]
    L.ecfft_build_fftree.restype, L.ecfft_build_fftree.argtypes = ci, [ci, sz, ci, ctypes.POINTER(vp)]
    L.ecfft_fftree_new.restype, L.ecfft_fftree_new.argtypes = ci, [ci, vp, sz, vp, vp, ci, ctypes.POINTER(vp)]
    L.ecfft_ctx_destroy.restype, L.ecfft_ctx_destroy.argtypes = None, [vp]
    L.ecfft_tree_size.restype, L.ecfft_tree_size.argtypes = sz, [vp]
    L.ecfft_field.restype, L.ecfft_field.argtypes = ci, [vp]
    L.ecfft_enter.restype, L.ecfft_enter.argtypes = ci, [vp, vp, vp, sz, ci, vp]
    L.ecfft_exit.restype, L.ecfft_exit.argtypes = ci, [vp, vp, vp, sz, ci, vp]
    L.ecfft_extend.restype, L.ecfft_extend.argtypes = ci, [vp, vp, vp, sz, ci, sz, ci, vp]
    L.ecfft_poly_mul.restype, L.ecfft_poly_mul.argtypes = ci, [vp, vp, sz, vp, sz, vp, sz, ci, vp]
    L.ecfft_poly_inv_series.restype, L.ecfft_poly_inv_series.argtypes = ci, [vp, vp, sz, vp, sz, sz, ci, vp]
    L.ecfft_poly_divrem.restype, L.ecfft_poly_divrem.argtypes = ci, [vp, vp, sz, vp, sz, vp, vp, sz, ci, vp]
    L.ecfft_poly_eval_points.restype, L.ecfft_poly_eval_points.argtypes = ci, [vp, vp, sz, vp, sz, vp, sz, ci, vp]
    L.ecfft_poly_interpolate.restype, L.ecfft_poly_interpolate.argtypes = ci, [vp, vp, sz, vp, vp, sz, ci, vp]
    L.ecfft_poly_pow_mod.restype, L.ecfft_poly_pow_mod.argtypes = ci, [vp, vp, sz, vp, sz, vp, sz, vp, sz, ci, vp]
    L.ecfft_poly_mul_mod.restype, L.ecfft_poly_mul_mod.argtypes = ci, [vp, vp, sz, vp, sz, vp, sz, vp, sz, ci, vp]
    L.ecfft_poly_compose_mod.restype, L.ecfft_poly_compose_mod.argtypes = ci, [vp, vp, sz, vp, sz, vp, sz, vp, sz, ci, vp]
    L.ecfft_poly_gcd.restype, L.ecfft_poly_gcd.argtypes = ci, [vp, vp, sz, vp, sz, vp, vp, sz, ci, vp]
    L.ecfft_poly_xgcd.restype, L.ecfft_poly_xgcd.argtypes = ci, [vp, vp, sz, vp, sz, vp, vp, vp, vp, sz, ci, vp]
    L.ecfft_poly_xgcd_partial.restype, L.ecfft_poly_xgcd_partial.argtypes = ci, [vp, vp, sz, vp, sz, sz, vp, vp, vp, vp, sz, ci, vp]
    L.ecfft_rs_decode.restype, L.ecfft_rs_decode.argtypes = ci, [vp, vp, sz, vp, sz, vp, vp, sz, ci, vp]
    L.ecfft_seq_min_poly.restype, L.ecfft_seq_min_poly.argtypes = ci, [vp, vp, sz, vp, vp, sz, ci, vp]
    L.ecfft_seq_nth_term.restype, L.ecfft_seq_nth_term.argtypes = ci, [vp, vp, sz, vp, vp, sz, vp, sz, sz, ci, vp]
    L.ecfft_rs_encode.restype, L.ecfft_rs_encode.argtypes = ci, [vp, vp, sz, vp, sz, vp, sz, ci, vp]
    L.ecfft_rs_decode_erasures.restype, L.ecfft_rs_decode_erasures.argtypes = ci, [vp, vp, sz, vp, vp, sz, vp, ci, vp, sz, ci, vp]
    L.ecfft_poly_find_roots.restype, L.ecfft_poly_find_roots.argtypes = ci, [vp, vp, sz, vp, vp, sz, ci, vp]
    L.ecfft_poly_squarefree.restype, L.ecfft_poly_squarefree.argtypes = ci, [vp, vp, sz, vp, vp, sz, ci, vp]
    L.ecfft_poly_distinct_degree.restype, L.ecfft_poly_distinct_degree.argtypes = ci, [vp, vp, sz, vp, vp, sz, ci, vp]
    L.ecfft_poly_equal_degree.restype, L.ecfft_poly_equal_degree.argtypes = ci, [vp, vp, sz, sz, vp, vp, sz, ci, vp]
    L.ecfft_poly_squarefree_decompose.restype, L.ecfft_poly_squarefree_decompose.argtypes = ci, [vp, vp, sz, vp, vp, vp, sz, ci, vp]
    L.ecfft_poly_factor.restype, L.ecfft_poly_factor.argtypes = ci, [vp, vp, sz, vp, vp, vp, vp, vp, sz, ci, vp]
    L.ecfft_division_polynomial.restype, L.ecfft_division_polynomial.argtypes = ci, [vp, vp, vp, sz, vp, sz, ci, vp]
    L.ecfft_curve_cardinality.restype, L.ecfft_curve_cardinality.argtypes = ci, [vp, vp, vp, vp, vp, sz, ci, vp]
    L.ecfft_curve_trace_mod.restype, L.ecfft_curve_trace_mod.argtypes = ci, [vp, vp, vp, sz, vp, sz, ci, vp]
    L.ecfft_tree_table.restype, L.ecfft_tree_table.argtypes = ci, [vp, sz, ci, vp, sz, ctypes.POINTER(sz)]
    L.ecfft_build_points.restype, L.ecfft_build_points.argtypes = ci, [ci, sz, vp, vp, vp]
    L.ecfft_device_info.restype, L.ecfft_device_info.argtypes = ci, [ci, ctypes.c_char_p, sz]
    L.ecfft_extend_top_cyclic.restype, L.ecfft_extend_top_cyclic.argtypes = ci, [vp, vp, sz, ci, ctypes.c_uint, ctypes.c_uint, ci, ci, vp]
    L.ecfft_extend_local_block.restype, L.ecfft_extend_local_block.argtypes = ci, [vp, vp, sz, ci, ctypes.c_uint, ci, vp]
    L.ecfft_mul_ceiling.restype, L.ecfft_mul_ceiling.argtypes = ci, [ci, ci, ci, ctypes.POINTER(ctypes.c_double)]
    L.ecfft_elems_to_standard.restype, L.ecfft_elems_to_standard.argtypes = ci, [ci, vp, vp, sz]
    L.ecfft_elems_from_standard.restype, L.ecfft_elems_from_standard.argtypes = ci, [ci, vp, vp, sz]
    L.ecfft_table_fma.restype, L.ecfft_table_fma.argtypes = ci, [vp, vp, vp, vp, sz, sz, ci, sz, sz, ci, ci, vp]
    L.ecfft_enter_many.restype, L.ecfft_enter_many.argtypes = ci, [vp, vp, vp, sz, sz, ci, vp]
    L.ecfft_exit_many.restype, L.ecfft_exit_many.argtypes = ci, [vp, vp, vp, sz, sz, ci, vp]
    L.ecfft_mextend.restype, L.ecfft_mextend.argtypes = ci, [vp, vp, vp, sz, ci, sz, ci, vp]
    L.ecfft_redc.restype, L.ecfft_redc.argtypes = ci, [vp, vp, vp, vp, sz, ci, ci, vp]
    L.ecfft_modular_reduce.restype, L.ecfft_modular_reduce.argtypes = ci, [vp, vp, vp, vp, vp, sz, ci, vp]
    L.ecfft_vanish.restype, L.ecfft_vanish.argtypes = ci, [vp, vp, vp, sz, ci, vp]
    L.ecfft_degree.restype, L.ecfft_degree.argtypes = ci, [vp, vp, sz, ci, vp, ctypes.POINTER(sz)]
    L.ecfft_comm_get_unique_id.restype, L.ecfft_comm_get_unique_id.argtypes = ci, [vp]
    L.ecfft_comm_init_rank.restype, L.ecfft_comm_init_rank.argtypes = ci, [vp, ci, ci, ci, ctypes.POINTER(vp)]
    L.ecfft_comm_init_callback.restype, L.ecfft_comm_init_callback.argtypes = ci, [ci, ci, ci, EXCHANGE_FN, vp, ctypes.POINTER(vp)]
    L.ecfft_comm_destroy.restype, L.ecfft_comm_destroy.argtypes = None, [vp]
    L.ecfft_comm_rank.restype, L.ecfft_comm_rank.argtypes = ci, [vp]
    L.ecfft_comm_world.restype, L.ecfft_comm_world.argtypes = ci, [vp]
    L.ecfft_comm_stats_enable.restype, L.ecfft_comm_stats_enable.argtypes = ci, [vp, ci]
    L.ecfft_comm_stats_read.restype, L.ecfft_comm_stats_read.argtypes = ci, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.ecfft_extend_sharded.restype, L.ecfft_extend_sharded.argtypes = ci, [vp, vp, vp, vp, sz, ci, vp]
    L.ecfft_enter_sharded.restype, L.ecfft_enter_sharded.argtypes = ci, [vp, vp, vp, vp, sz, vp]
    L.ecfft_extend_sharded_layout.restype, L.ecfft_extend_sharded_layout.argtypes = ci, [vp, vp, vp, vp, sz, ci, ci, ci, vp]
    L.ecfft_build_enter_shard.restype, L.ecfft_build_enter_shard.argtypes = ci, [ci, sz, ci, ci, ci, ctypes.POINTER(vp)]
    L.ecfft_build_exit_shard.restype, L.ecfft_build_exit_shard.argtypes = ci, [ci, sz, ci, vp, ctypes.POINTER(vp)]
    L.ecfft_build_exit_shard_opts.restype, L.ecfft_build_exit_shard_opts.argtypes = ci, [ci, sz, ci, vp, ci, ctypes.POINTER(vp)]
    L.ecfft_ctx_device_bytes.restype, L.ecfft_ctx_device_bytes.argtypes = sz, [vp]
    L.ecfft_build_extend_shard.restype, L.ecfft_build_extend_shard.argtypes = ci, [ci, sz, ci, ci, ci, ctypes.POINTER(vp)]
    L.ecfft_exit_sharded.restype, L.ecfft_exit_sharded.argtypes = ci, [vp, vp, vp, vp, sz, vp]
    L.ecfft_fftree_serialize.restype, L.ecfft_fftree_serialize.argtypes = ci, [vp, ci, vp, sz, ctypes.POINTER(sz)]
    L.ecfft_fftree_deserialize.restype, L.ecfft_fftree_deserialize.argtypes = ci, [ci, vp, sz, ci, ci, ci, ctypes.POINTER(vp)]
    L.ecfft_tree_rational_maps.restype, L.ecfft_tree_rational_maps.argtypes = ci, [vp, vp, vp]
    L.ecfft_ctx_trim.restype, L.ecfft_ctx_trim.argtypes = ci, [vp]
    L.ecfft_device_copy.restype, L.ecfft_device_copy.argtypes = ci, [vp, vp, sz, ci]
    L.ecfft_shader_clock.restype, L.ecfft_shader_clock.argtypes = ci, [ci, ci, ctypes.POINTER(ctypes.c_double)]
    L.ecfft_profile_enable.restype, L.ecfft_profile_enable.argtypes = ci, [vp, ci]
    L.ecfft_profile_classes.restype, L.ecfft_profile_classes.argtypes = ci, []
    L.ecfft_profile_read.restype, L.ecfft_profile_read.argtypes = ci, [vp, ci, ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_uint64),
                                                                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    L.ecfft_find_curve_candidate.restype, L.ecfft_find_curve_candidate.argtypes = ci, [ci, u64, u64, vp, vp]
    L.ecfft_curve_two_sylow.restype, L.ecfft_curve_two_sylow.argtypes = ci, [ci, ci, vp, vp, sz, vp, vp]
    L.ecfft_find_curve.restype, L.ecfft_find_curve.argtypes = ci, [ci, ci, ctypes.c_uint, u64, u64, u64, ctypes.POINTER(u64), ctypes.POINTER(u32),
                                                                   vp, vp, vp, vp]
    L.ecfft_build_fftree_on_curve.restype, L.ecfft_build_fftree_on_curve.argtypes = ci, [ci, sz, vp, vp, vp, ctypes.c_uint, vp, ci, ctypes.POINTER(vp)]
    L.ecfft_curve_point_mul.restype, L.ecfft_curve_point_mul.argtypes = ci, [ci, ci, vp, vp, sz, vp, vp, vp, sz, sz, vp, vp, sz]
    L.ecfft_curve_point_two_adicity.restype, L.ecfft_curve_point_two_adicity.argtypes = ci, [ci, ci, vp, vp, sz, vp, vp, ctypes.c_uint, vp, sz]
    L.ecfft_curve_find_generator.restype, L.ecfft_curve_find_generator.argtypes = ci, [ci, ci, vp, vp, vp, u64, u64, ctypes.POINTER(ctypes.c_uint), vp, vp,
                                                                                       ctypes.POINTER(u64)]
    L.ecfft_build_ec_fftree.restype, L.ecfft_build_ec_fftree.argtypes = ci, [ci, sz, vp, vp, vp, ctypes.c_uint, vp, ci, ctypes.POINTER(vp)]
    L.ecfft_comm_set_rccl_library.restype, L.ecfft_comm_set_rccl_library.argtypes = ci, [ctypes.c_char_p]
    L.ecfft_comm_set_link_striping.restype, L.ecfft_comm_set_link_striping.argtypes = ci, [vp, sz]
    L.has_hooks = hasattr(L, "ecfft_selftest_field")
    if L.has_hooks:      # include/ecfft_hip_hooks.h (test builds only)
        L.ecfft_selftest_field.restype, L.ecfft_selftest_field.argtypes = ci, [ci, ci, vp, vp, vp, vp, sz, ci]
        L.ecfft_selfcheck_pointwise_z.restype, L.ecfft_selfcheck_pointwise_z.argtypes = ctypes.c_long, [vp, sz]
        L.ecfft_test_fail_next_collective.restype, L.ecfft_test_fail_next_collective.argtypes = ci, [vp]
        L.ecfft_test_fail_build_rank.restype, L.ecfft_test_fail_build_rank.argtypes = ci, [ci]
        L.ecfft_selftest_blk16.restype, L.ecfft_selftest_blk16.argtypes = ci, [vp, vp, vp, sz, ci]
        L.ecfft_selftest_blk16_small.restype, L.ecfft_selftest_blk16_small.argtypes = ci, [vp, vp, vp, sz, ci, ci]
        L.ecfft_selftest_blk32.restype, L.ecfft_selftest_blk32.argtypes = ci, [vp, vp, vp, sz, ci]
        L.ecfft_ctx_low_map.restype, L.ecfft_ctx_low_map.argtypes = ci, [vp, ci]
        L.ecfft_ctx_exit_cores.restype, L.ecfft_ctx_exit_cores.argtypes = ci, [vp]
        L.ecfft_ctx_exit_low_cores.restype, L.ecfft_ctx_exit_low_cores.argtypes = ci, [vp]
        if hasattr(L, "ecfft_ctx_sym_bfly"):
            L.ecfft_ctx_sym_bfly.restype, L.ecfft_ctx_sym_bfly.argtypes = ci, [vp]
        if hasattr(L, "ecfft_ctx_low_sym"):
            L.ecfft_ctx_low_sym.restype, L.ecfft_ctx_low_sym.argtypes = ci, [vp]
        if hasattr(L, "ecfft_ctx_enter_l11"):
            L.ecfft_ctx_enter_l11.restype, L.ecfft_ctx_enter_l11.argtypes = ci, [vp]
        L.ecfft_curve_search_stats.restype, L.ecfft_curve_search_stats.argtypes = ci, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double), sz, ci]
        L.ecfft_test_ddf_iterate.restype, L.ecfft_test_ddf_iterate.argtypes = ci, [ci]
        L.ecfft_test_schoof_pi2.restype, L.ecfft_test_schoof_pi2.argtypes = ci, [ci]
        L.ecfft_comm_init_projection.restype = ci
        L.ecfft_comm_init_projection.argtypes = [ci, ci, ci, ctypes.c_double, ctypes.c_double, ctypes.POINTER(vp)]
    return L


def _load(path):
    # PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64; load it FIRST so that this
    # library binds to the same HIP runtime instance (two runtimes in one process cannot share the
    # GPU: torch then reports "No HIP GPUs are available").  Plain C users link /opt/rocm directly.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    return _bind(ctypes.CDLL(path))


def lib():
    """Loads (building if needed) the HIP extension — the SHIPPED library unless ECFFT_LIB names another build (tuning variants;
    a variable of this Python mirror, not of the C library).  Raises if it cannot be built or loaded."""
    global _lib
    if _lib is None:
        path = os.environ.get("ECFFT_LIB") or os.path.join(_DIR, "libecfft_hip.so")
        if not os.path.exists(path):
            _build.build()
        _lib = _load(path)
    return _lib


class use_library:
    """`with use_library(path):` — every call of this module goes to that build of the library for the duration (tests and
    measurement tools: the hooks build, tests/hooks/libecfft_hip_hooks.so).  Contexts and communicators must be created AND used
    inside the same block: a handle belongs to the library instance that made it."""
    _loaded = {}

    def __init__(self, path):
        self.path = os.path.abspath(path)

    def __enter__(self):
        global _lib
        self.prev = _lib
        if self.path not in use_library._loaded:
            use_library._loaded[self.path] = _load(self.path)
        _lib = use_library._loaded[self.path]
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self.prev
        return False


def use_hooks_library():
    """the hooks build (include/ecfft_hip_hooks.h), built on demand by tests/hooks/build_hooks.py"""
    if not os.path.exists(HOOKS_LIB) or _build.stale(HOOKS_LIB):
        _build.build(out=HOOKS_LIB, defines=("ECFFT_TEST_HOOKS",))
    return use_library(HOOKS_LIB)


def _check(rc):
    if rc == OK:
        return
    if rc == ERR_NOT_POW2:
        raise AssertionError("length must be a power of two")        # assert!(n.is_power_of_two())
    if rc == ERR_TREE_TOO_SMALL:
        raise ValueError("FFTree is too small")                        # panic!("FFTree is too small")
    if rc == ERR_HIP:
        raise EcfftError("HIP failure (no usable MI355X device, or a runtime error) — there is no CPU fallback")
    raise EcfftError(f"ecfft error {rc}")


class Field:
    """One of the reference's two `FftreeField` implementors."""

    def __init__(self, name, field_id, dtype, limbs):
        self.name, self.id, self.dtype, self.limbs = name, field_id, np.dtype(dtype), limbs

    @property
    def elem_bytes(self):
        return self.dtype.itemsize * self.limbs

    def shape(self, n):
        return (n, self.limbs) if self.limbs > 1 else (n,)

    def _new_tree(self, make, device):
        """make(byref(handle)) -> rc of one of the context builders: None if the tree is too large for the curve"""
        h = ctypes.c_void_p()
        rc = make(ctypes.byref(h))
        if rc == ERR_TREE_TOO_LARGE:
            return None
        _check(rc)
        return FFTree(self, h, device)

    def build_fftree(self, n, device=0):
        """`F::build_fftree(n)`: None if n exceeds the curve's 2-adicity (src/lib.rs:62-64, src/ec.rs:513-515)."""
        return self._new_tree(lambda out: lib().ecfft_build_fftree(self.id, n, device, out), device)

    def build_extend_shard(self, e, world, rank, device=0):
        """Sharded EXTEND-only context (include/ecfft_hip.h ecfft_build_extend_shard): this rank's share of the tables of ONE
        EXTEND of e evaluations over `world` GPUs; only `extend_sharded` works on it.  None if T_2e is too large for the curve."""
        return self._new_tree(lambda out: lib().ecfft_build_extend_shard(self.id, e, device, world, rank, out), device)

    def build_enter_shard(self, n, world, rank, device=0):
        """Sharded ENTER-only context (ecfft_build_enter_shard): the chain up to n/world plus this rank's share of the top
        log2(world) trees; only `enter_sharded` works on it.  None if T_n is too large for the curve."""
        return self._new_tree(lambda out: lib().ecfft_build_enter_shard(self.id, n, device, world, rank, out), device)

    def build_exit_shard(self, n, comm, device=0, min_memory=False):
        """Sharded EXIT-only context (ecfft_build_exit_shard[_opts]) — COLLECTIVE over the ranks of `comm`: the chain up to n/world plus
        this rank's share of the top trees, z0z0_rem_xnn_s built distributed; only `exit_sharded` works on it.  min_memory: never
        keep T_2c for the redundant pair level (ECFFT_EXIT_SHARD_MIN_MEMORY)."""
        return self._new_tree(lambda out: lib().ecfft_build_exit_shard_opts(self.id, n, device, comm._h, 1 if min_memory else 0, out), device)

    def selftest(self, op, a, b, c=None, device=0):
        """device field arithmetic on raw residues (test hook): op 0 a*b+c, 1 a*b, 2 a-b, 3 a+b, 6 a/2, 4/5 the kernels' table multiply a*b+c / a*b"""
        a = np.ascontiguousarray(a, self.dtype); b = np.ascontiguousarray(b, self.dtype)
        cc = None if c is None else np.ascontiguousarray(c, self.dtype)
        out = np.empty_like(a)
        _check(lib().ecfft_selftest_field(self.id, op, a.ctypes.data, b.ctypes.data, None if cc is None else cc.ctypes.data, out.ctypes.data, a.shape[0], device))
        return out

    def mul_ceiling(self, waves_per_simd=4, device=0):
        """field multiplies per second of the kernels' table multiply as a bare dependent chain on the whole chip"""
        r = ctypes.c_double()
        _check(lib().ecfft_mul_ceiling(self.id, device, waves_per_simd, ctypes.byref(r)))
        return r.value

    def shader_clock_mhz(self, device=0):
        """effective shader clock while the whole chip runs this field's table multiply"""
        r = ctypes.c_double()
        _check(lib().ecfft_shader_clock(self.id, device, ctypes.byref(r)))
        return r.value

    def to_standard(self, a):
        """in-memory elements -> standard-form little-endian integers (same array shape)"""
        a = np.ascontiguousarray(a, self.dtype); out = np.empty_like(a)
        _check(lib().ecfft_elems_to_standard(self.id, a.ctypes.data, out.ctypes.data, a.shape[0]))
        return out

    def from_standard(self, a):
        a = np.ascontiguousarray(a, self.dtype); out = np.empty_like(a)
        _check(lib().ecfft_elems_from_standard(self.id, a.ctypes.data, out.ctypes.data, a.shape[0]))
        return out

    def build_points(self, n):
        """host-only: (f[2n], map_num[log n, 3], map_den[log n, 3]) — leaves are f[n:]."""
        ln = max(n.bit_length() - 1, 0)
        f = np.zeros(self.shape(2 * n), self.dtype)
        num = np.zeros(self.shape(3 * max(ln, 1)), self.dtype)
        den = np.zeros(self.shape(3 * max(ln, 1)), self.dtype)
        rc = lib().ecfft_build_points(self.id, n, f.ctypes.data, num.ctypes.data, den.ctypes.data)
        if rc == ERR_TREE_TOO_LARGE:
            return None
        _check(rc)
        return f, num[:3 * ln], den[:3 * ln]

    def new_fftree(self, leaves, map_num, map_den, device=0):
        """`FFTree::new(leaves, rational_maps)` (src/fftree.rs:42-70)."""
        leaves = np.ascontiguousarray(leaves, self.dtype)
        map_num = np.ascontiguousarray(map_num, self.dtype); map_den = np.ascontiguousarray(map_den, self.dtype)
        n = leaves.shape[0]
        h = ctypes.c_void_p()
        _check(lib().ecfft_fftree_new(self.id, leaves.ctypes.data, n, map_num.ctypes.data, map_den.ctypes.data, device, ctypes.byref(h)))
        return FFTree(self, h, device, maps=(map_num, map_den))

    # ---- curves of the caller's own (include/ecfft_hip.h: curve search) ----------------------------------------------
    FIND_CURVE_DEFAULT_MAX = 1 << 26

    def find_curve_candidate(self, seed, index):
        """(a, bb) of candidate `index` of the stream `seed` (ecfft_find_curve_candidate), one element each; host only"""
        a, bb = np.zeros(self.shape(1), self.dtype), np.zeros(self.shape(1), self.dtype)
        rc = lib().ecfft_find_curve_candidate(self.id, seed, index, a.ctypes.data, bb.ctypes.data)
        if rc == ERR_BAD_ARG:
            raise ValueError("find_curve_candidate: the index must be below 2^60")
        _check(rc)
        return a, bb

    def curve_two_sylow(self, a, bb, device=0):
        """(n, x) of `cyclic_two_sylow_subgroup` (src/find_curve.rs:190-218) for the curves y^2 = x(x^2 + a[i] x + bb[i]): n a numpy
        uint32 array (0: not cyclic, bb no square or a singular curve), x the x-coordinates of points of order 2^n (0 where n is 0)"""
        a = np.ascontiguousarray(a, self.dtype); bb = np.ascontiguousarray(bb, self.dtype)
        assert a.shape == bb.shape
        count = a.shape[0]
        n, x = np.zeros(count, np.uint32), np.zeros_like(a)
        rc = lib().ecfft_curve_two_sylow(self.id, device, a.ctypes.data, bb.ctypes.data, count, n.ctypes.data, x.ctypes.data)
        if rc == ERR_BAD_ARG:
            raise ValueError("curve_two_sylow: no curves")
        _check(rc)
        return n, x

    def find_curve(self, k, seed, start=0, max_candidates=None, device=0):
        """`find_curve(rng, k)` (src/find_curve.rs:224-246) over candidates start .. start + max_candidates - 1 of the stream `seed`:
        the candidate of smallest index with n >= max(k, 2), as a dict index, n, a, bb, gen (x, y of a point of order 2^n) and offset
        (x, y of a coset offset) in the crate's form, the arguments of build_fftree_on_curve; None when the window holds none."""
        if max_candidates is None:
            max_candidates = self.FIND_CURVE_DEFAULT_MAX
        idx, n = ctypes.c_uint64(), ctypes.c_uint32()
        a, bb = np.zeros(self.shape(1), self.dtype), np.zeros(self.shape(1), self.dtype)
        gen, off = np.zeros(self.shape(2), self.dtype), np.zeros(self.shape(2), self.dtype)
        rc = lib().ecfft_find_curve(self.id, device, k, seed, start, max_candidates, ctypes.byref(idx), ctypes.byref(n),
                                    a.ctypes.data, bb.ctypes.data, gen.ctypes.data, off.ctypes.data)
        if rc == ERR_BAD_ARG:
            raise ValueError("find_curve: an empty window, a window that ends above 2^60 or k above the field's bit length")
        _check(rc)
        if n.value == 0:
            return None
        return {"index": idx.value, "n": n.value, "a": a, "bb": bb, "gen": gen, "offset": off}

    MODULUS = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}

    def to_ints(self, a):
        """in-memory elements -> a list of Python ints (standard form)"""
        std = self.to_standard(a)
        return [int.from_bytes(std[i].tobytes(), "little") for i in range(std.shape[0])]

    def from_ints(self, vals):
        """Python ints (reduced modulo p) -> in-memory elements"""
        p, nb = self.MODULUS[self.name], self.dtype.itemsize * self.limbs
        raw = b"".join((int(v) % p).to_bytes(nb, "little") for v in vals)
        return self.from_standard(np.frombuffer(raw, self.dtype).reshape(self.shape(len(vals))).copy())

    def short_weierstrass(self, a, bb):
        """(A, B) of y^2 = x^3 + A x + B for the curves y^2 = x (x^2 + a[i] x + bb[i]) of find_curve, under x -> x - a/3:
        A = bb - a^2/3, B = 2 a^3/27 - a bb/3.  Same group, so curve_trace_mod counts a found curve.  Host arrays in the crate's form."""
        p = self.MODULUS[self.name]
        i3, i27 = pow(3, -1, p), pow(27, -1, p)
        av, bv = self.to_ints(a), self.to_ints(bb)
        A = [(b - x * x * i3) % p for x, b in zip(av, bv)]
        B = [(2 * x**3 * i27 - x * b * i3) % p for x, b in zip(av, bv)]
        return self.from_ints(A), self.from_ints(B)

    def build_fftree_on_curve(self, n, a, bb, gen, gen_log_order, offset, device=0):
        """`build_fftree(n)` on the good curve y^2 = x(x^2 + a x + bb) (ecfft_build_fftree_on_curve): gen = (x, y) of order
        2^gen_log_order, offset = (x, y) of a coset offset; None if log2 n >= gen_log_order.  ValueError for what is no good curve,
        no point of it, a generator of another order or an offset inside the subgroup."""
        a = np.ascontiguousarray(a, self.dtype); bb = np.ascontiguousarray(bb, self.dtype)
        gen = np.ascontiguousarray(gen, self.dtype); offset = np.ascontiguousarray(offset, self.dtype)
        assert a.size == bb.size == self.limbs and gen.size == offset.size == 2 * self.limbs

        def make(out):
            rc = lib().ecfft_build_fftree_on_curve(self.id, n, a.ctypes.data, bb.ctypes.data, gen.ctypes.data, gen_log_order, offset.ctypes.data, device, out)
            if rc == ERR_BAD_ARG:
                raise ValueError("build_fftree_on_curve: not a good curve, a point off the curve, a generator of another order or an offset inside its subgroup")
            return rc
        return self._new_tree(make, device)

    # ---- trees on short-Weierstrass curves y^2 = x^3 + A x + B (include/ecfft_hip.h: ecfft_curve_point_mul and what follows) ----
    def _curves_and_points(self, A, B, points, inf, what):
        A = np.ascontiguousarray(A, self.dtype).reshape(self.shape(-1)); B = np.ascontiguousarray(B, self.dtype).reshape(self.shape(-1))
        points = np.ascontiguousarray(points, self.dtype)
        if A.shape != B.shape or points.size == 0 or points.size % (2 * self.limbs):
            raise ValueError(f"{what}: A and B must hold one element per curve and points two elements per point")
        count = points.size // (2 * self.limbs)
        if inf is not None:
            inf = np.ascontiguousarray(inf, np.uint8)
            if inf.shape != (count,):
                raise ValueError(f"{what}: inf must hold one byte per point")
        return A, B, points, inf, count

    def curve_point_mul(self, A, B, points, scalars, scalar_bytes=None, inf=None, device=0):
        """out[i] = [k_i] P_i on y^2 = x^3 + A x + B (ecfft_curve_point_mul <-> Point::mul, src/ec.rs:432-447).  A, B: one curve for
        all rows or one per row; points: (count, 2) elements x, y in the crate's form; scalars: a list of Python ints (one for all
        rows or one per row, at most 40 bytes) or a uint8 array of rows of little-endian bytes; inf: one byte per point, non-zero for
        the point at infinity.  Returns (points, inf) of the same shapes.  ValueError for a point off its curve or a singular curve."""
        A, B, points, inf, count = self._curves_and_points(A, B, points, inf, "curve_point_mul")
        if isinstance(scalars, np.ndarray):
            k = np.ascontiguousarray(scalars, np.uint8)
            k = k.reshape(1, -1) if k.ndim == 1 else k
        else:
            scalars = [int(v) for v in scalars]
            nb = scalar_bytes or max(1, max((v.bit_length() + 7) // 8 for v in scalars))
            k = np.frombuffer(b"".join(v.to_bytes(nb, "little") for v in scalars), np.uint8).reshape(len(scalars), nb).copy()
        out, inf_out = np.zeros_like(points), np.zeros(count, np.uint8)
        rc = lib().ecfft_curve_point_mul(self.id, device, A.ctypes.data, B.ctypes.data, A.shape[0], points.ctypes.data,
                                         None if inf is None else inf.ctypes.data, k.ctypes.data, k.shape[0], k.shape[1],
                                         out.ctypes.data, inf_out.ctypes.data, count)
        if rc == ERR_BAD_ARG:
            raise ValueError("curve_point_mul: a point off its curve, a singular curve, scalars wider than 40 bytes, or curves / scalars that are neither one nor one per point")
        _check(rc)
        return out, inf_out

    def curve_point_two_adicity(self, A, B, points, cap=None, inf=None, device=0):
        """the smallest i >= 0 with 2^i P the identity for every point, among i <= cap, -1 where there is none (ecfft_curve_point_two_adicity
        <-> two_adicity, src/utils.rs:356-365); a numpy int32 array.  cap defaults to its maximum, 8 * element bytes + 2."""
        A, B, points, inf, count = self._curves_and_points(A, B, points, inf, "curve_point_two_adicity")
        cap = 8 * self.elem_bytes + 2 if cap is None else int(cap)
        out = np.zeros(count, np.int32)
        rc = lib().ecfft_curve_point_two_adicity(self.id, device, A.ctypes.data, B.ctypes.data, A.shape[0], points.ctypes.data,
                                                 None if inf is None else inf.ctypes.data, cap, out.ctypes.data, count)
        if rc == ERR_BAD_ARG:
            raise ValueError("curve_point_two_adicity: a point off its curve, a singular curve, a cap above 8 * element bytes + 2, or curves that are neither one nor one per point")
        _check(rc)
        return out

    FIND_GENERATOR_DEFAULT_MAX = 1 << 12

    def curve_find_generator(self, A, B, order, start=1, max_candidates=None, device=0):
        """The arguments of build_ec_fftree from the curve y^2 = x^3 + A x + B and its number of points `order` (a Python int, or the 40
        bytes curve_cardinality's C call writes): a dict log_order (v with order = 2^v * odd), gen (x, y of a point of order 2^v),
        offset (x, y of a coset offset; 0, 0 when the window holds none) and x (the integer x-coordinate the generator came from).
        None when the window start .. start + max_candidates - 1 holds no point of order 2^v (ecfft_curve_find_generator).
        ValueError when `order` is not the curve's."""
        A = np.ascontiguousarray(A, self.dtype); B = np.ascontiguousarray(B, self.dtype)
        assert A.size == B.size == self.limbs
        if max_candidates is None:
            max_candidates = self.FIND_GENERATOR_DEFAULT_MAX
        ob = bytes(order) if not isinstance(order, int) else order.to_bytes(ORDER_BYTES, "little")
        assert len(ob) == ORDER_BYTES
        v, x = ctypes.c_uint(), ctypes.c_uint64()
        gen, off = np.zeros(self.shape(2), self.dtype), np.zeros(self.shape(2), self.dtype)
        rc = lib().ecfft_curve_find_generator(self.id, device, A.ctypes.data, B.ctypes.data, ob, start, max_candidates, ctypes.byref(v),
                                              gen.ctypes.data, off.ctypes.data, ctypes.byref(x))
        if rc == ERR_BAD_ARG:
            raise ValueError("curve_find_generator: not the order of this curve, a singular curve, or an empty or misplaced window")
        _check(rc)
        if v.value == 0:
            return None
        return {"log_order": v.value, "gen": gen, "offset": off, "x": x.value}

    def build_ec_fftree(self, n, A, B, gen, gen_log_order, offset, device=0):
        """`build_ec_fftree(subgroup_generator, subgroup_order, coset_offset, n)` (src/ec.rs:498-554) on y^2 = x^3 + A x + B
        (ecfft_build_ec_fftree): gen = (x, y) of order 2^gen_log_order, offset = (x, y) of a coset offset; None if log2 n >
        gen_log_order.  ValueError for a singular curve, a point off the curve, a generator of another order, an offset whose
        double lies in the subgroup, or a curve without a suitable isogeny at some level."""
        A = np.ascontiguousarray(A, self.dtype); B = np.ascontiguousarray(B, self.dtype)
        gen = np.ascontiguousarray(gen, self.dtype); offset = np.ascontiguousarray(offset, self.dtype)
        assert A.size == B.size == self.limbs and gen.size == offset.size == 2 * self.limbs

        def make(out):
            rc = lib().ecfft_build_ec_fftree(self.id, n, A.ctypes.data, B.ctypes.data, gen.ctypes.data, gen_log_order, offset.ctypes.data, device, out)
            if rc == ERR_BAD_ARG:
                raise ValueError("build_ec_fftree: a singular curve, a point off the curve, a generator of another order, an offset whose double lies in its subgroup, or no suitable isogeny")
            return rc
        return self._new_tree(make, device)


def deserialize_fftree(field, data, compress, device=0, verify=True):
    """`FFTree::deserialize_compressed / deserialize_uncompressed` (src/fftree.rs:600-660) through the C ABI
    (ecfft_fftree_deserialize: bounds-checked parse, rebuild on the GPU, optional table-by-table verification)"""
    data = bytes(data)
    h = ctypes.c_void_p()
    rc = lib().ecfft_fftree_deserialize(field.id, data, len(data), int(bool(compress)), device, int(bool(verify)), ctypes.byref(h))
    if rc in (ERR_BAD_ARG, ERR_NOT_POW2):        # a file whose `f` length is not a power of two is malformed too
        raise ValueError("malformed FFTree file (or its tables disagree with its point set)")
    _check(rc)
    t = FFTree(field, h, device)
    return t


secp256k1 = Field("secp256k1", 0, np.uint64, 4)
m31 = Field("m31", 1, np.uint32, 1)
FIELDS = {"secp256k1": secp256k1, "m31": m31}


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class FFTree:
    """Device-resident `FFTree<F>` (whole subtree chain).  `&self` methods, immutable after build."""

    def __init__(self, field, handle, device, maps=None):
        self.field, self._h, self.device = field, handle, device
        # the library that created the handle serves every later call on it, __del__ included: with use_library /
        # use_hooks_library a handle can outlive the with-block it was made in, and lib() would then name another .so instance
        self._L = lib()
        self.n = self._L.ecfft_tree_size(handle)
        self._from_build = maps is None          # build_fftree: the maps are those of build_points(n)
        if maps is not None:
            self._num, self._den = maps

    @property
    def device_bytes(self):
        """HBM the context holds between calls (tables + transform scratch + pooled temporaries)"""
        return self._L.ecfft_ctx_device_bytes(self._h)

    def trim(self):
        """return the pooled temporaries of the algorithm wrappers to the device (ecfft_ctx_trim)"""
        _check(self._L.ecfft_ctx_trim(self._h))

    def __del__(self):
        try:
            if self._h:
                self._L.ecfft_ctx_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- plumbing --------------------------------------------------------------------------
    def _io(self, x, out_like=True):
        """returns (in_ptr, out_obj, out_ptr, mem, stream, count_elems)"""
        if _is_torch(x):
            import torch
            assert x.is_cuda and x.is_contiguous(), "device tensors must be contiguous CUDA tensors"
            out = torch.empty_like(x)
            stream = torch.cuda.current_stream(x.device).cuda_stream
            return x.data_ptr(), out, out.data_ptr(), MEM_DEVICE, stream, x.shape[0]
        a = np.ascontiguousarray(x, self.field.dtype)
        out = np.empty_like(a)
        return a.ctypes.data, out, out.ctypes.data, MEM_HOST, None, a.shape[0]

    # ---- the path --------------------------------------------------------------------------
    def enter(self, coeffs, count=1):
        """coefficients -> evaluations on the leaves of T_len (src/fftree.rs:164-167); count > 1: that many
        polynomials laid end to end (batched form, no reference counterpart)."""
        pin, out, pout, mem, stream, n = self._io(coeffs)
        assert n % count == 0
        _check(self._L.ecfft_enter_many(self._h, pin, pout, n // count, count, mem, stream))
        return out

    def exit(self, evals, count=1):
        """evaluations -> coefficients (src/fftree.rs:227-230)."""
        pin, out, pout, mem, stream, n = self._io(evals)
        assert n % count == 0
        _check(self._L.ecfft_exit_many(self._h, pin, pout, n // count, count, mem, stream))
        return out

    def extend(self, evals, moiety, count=1):
        """extends evaluations onto the TARGET moiety (src/fftree.rs:123-126); `count` > 1 treats the
        input as that many vectors laid end to end (batched form, no reference counterpart)."""
        pin, out, pout, mem, stream, total = self._io(evals)
        assert total % count == 0
        _check(self._L.ecfft_extend(self._h, pin, pout, total // count, int(moiety), count, mem, stream))
        return out

    def poly_mul(self, a, b, count=1):
        """c = a * b in coefficient form (ecfft_poly_mul; no reference counterpart): `count` pairs laid end to end, a of
        count * na and b of count * nb coefficients, any lengths; returns count * (na + nb - 1) coefficients.  Needs a tree of
        next_pow2(na + nb - 1) leaves.  Passing the same object as a and b is a squaring (one forward transform).  numpy arrays
        (host) or contiguous CUDA tensors (device, on the tensor's current stream), both of the same kind."""
        assert _is_torch(a) == _is_torch(b), "a and b must both be numpy arrays or both CUDA tensors"
        xs, ptrs, new, mem, stream = self._poly_io([a] if a is b else [a, b])     # a squaring converts its operand once
        (a, b), (pa, pb) = (xs * 2, ptrs * 2) if a is b else (xs, ptrs)
        assert count > 0 and a.shape[0] % count == 0 and b.shape[0] % count == 0
        na, nb = a.shape[0] // count, b.shape[0] // count
        out = new(count * max(na + nb - 1, 0))
        rc = self._L.ecfft_poly_mul(self._h, pa, na, pb, nb, self._ptr(out), count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_mul: empty operand, count = 0 or a context that holds no full tree")
        _check(rc)
        return out

    def _poly_io(self, xs):
        """numpy arrays (host) or contiguous CUDA tensors (device, all of the same kind) -> (arrays, pointers, new(rows), mem, stream)"""
        if any(_is_torch(x) for x in xs):
            import torch
            assert all(_is_torch(x) for x in xs), "operands must all be numpy arrays or all CUDA tensors"
            for x in xs:
                assert x.is_cuda and x.is_contiguous(), "device tensors must be contiguous CUDA tensors"
            x0 = xs[0]
            return (xs, [x.data_ptr() for x in xs],
                    lambda rows: torch.empty((rows,) + tuple(x0.shape[1:]), dtype=x0.dtype, device=x0.device),
                    MEM_DEVICE, torch.cuda.current_stream(x0.device).cuda_stream)
        xs = [np.ascontiguousarray(x, self.field.dtype) for x in xs]
        return xs, [x.ctypes.data for x in xs], lambda rows: np.empty(self.field.shape(rows), self.field.dtype), MEM_HOST, None

    @staticmethod
    def _ptr(x):
        return x.data_ptr() if _is_torch(x) else x.ctypes.data

    def poly_divrem(self, a, b, count=1):
        """(q, r) with a = b*q + r, deg r < deg b (ecfft_poly_divrem <-> utils::div_rem, src/utils.rs:184-193): `count` pairs laid end
        to end, a of count * na and b of count * nb coefficients, b's leading coefficient nonzero in every pair.  q has count * nq
        coefficients, nq = na - nb + 1 (none when na < nb); r has count * (nb - 1), zero-padded above its degree.  Needs a tree of
        next_pow2(max(2 nq - 1, nr + min(nq, nr) - 1)) leaves when na >= nb >= 2.  numpy arrays (host) or contiguous CUDA tensors
        (device, on the current stream), both of the same kind.  Synchronous."""
        (a, b), (pa, pb), new, mem, stream = self._poly_io([a, b])
        assert count > 0 and a.shape[0] % count == 0 and b.shape[0] % count == 0
        na, nb = a.shape[0] // count, b.shape[0] // count
        q, r = new(count * max(na - nb + 1, 0)), new(count * max(nb - 1, 0))
        pq = self._ptr(q) if q.shape[0] else None
        pr = self._ptr(r) if r.shape[0] else None
        if pq is None and pr is None:
            pr = self._ptr(r)                      # na = nb = 1 style shapes still report their errors
        rc = self._L.ecfft_poly_divrem(self._h, pa, na, pb, nb, pq, pr, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_divrem: empty operand, a zero leading coefficient of b, count = 0 or a context that holds no full tree")
        _check(rc)
        return q, r

    def poly_inv_series(self, f, k, count=1):
        """1/f mod x^k, the power-series reciprocal (ecfft_poly_inv_series; no reference counterpart): `count` series laid end to end,
        f of count * nf coefficients with f[0] nonzero in every pair; returns count * k coefficients.  Needs a tree of
        next_pow2(2k - 1) leaves.  numpy arrays or contiguous CUDA tensors (current stream).  Synchronous."""
        (f,), (pf,), new, mem, stream = self._poly_io([f])
        assert count > 0 and f.shape[0] % count == 0
        out = new(count * k)
        rc = self._L.ecfft_poly_inv_series(self._h, pf, f.shape[0] // count, self._ptr(out) if k else None, k, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_inv_series: empty f, k = 0, a zero constant coefficient, count = 0 or a context that holds no full tree")
        _check(rc)
        return out

    def poly_eval_points(self, f, points, count=1):
        """f at arbitrary points (ecfft_poly_eval_points; no reference counterpart): `count` polynomials laid end to end, f of
        count * nf coefficients, `points` of m elements shared by all of them; returns count * m values, out[b*m + i] = f_b(points[i]).
        nf <= 64 works on any tree, a longer f needs a tree of next_pow2(nf) leaves.  numpy arrays (host) or contiguous CUDA tensors
        (device, on the current stream, asynchronous), both of the same kind."""
        (f, points), (pf, pp), new, mem, stream = self._poly_io([f, points])
        assert count > 0 and f.shape[0] % count == 0
        m = points.shape[0]
        out = new(count * m)
        rc = self._L.ecfft_poly_eval_points(self._h, pf, f.shape[0] // count, pp, m, self._ptr(out) if m else None, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_eval_points: empty f or points, count = 0 or a context that holds no full tree")
        _check(rc)
        return out

    def poly_interpolate(self, points, values, count=1):
        """The polynomial through arbitrary points (ecfft_poly_interpolate; no reference counterpart), the inverse of
        poly_eval_points: `points` of m pairwise distinct elements shared by `count` value vectors laid end to end (count * m values);
        returns count * m coefficients, f_b of degree < m with f_b(points[i]) = values[b*m + i].  m <= 64 works on any tree, more
        points need a tree of next_pow2(m) leaves.  numpy arrays (host) or contiguous CUDA tensors (device, on the current stream),
        both of the same kind.  Synchronous (two equal points are detected on the device)."""
        (points, values), (pp, pv), new, mem, stream = self._poly_io([points, values])
        m = points.shape[0]
        assert count > 0 and values.shape[0] == count * m
        out = new(count * m)
        rc = self._L.ecfft_poly_interpolate(self._h, pp, m, pv, self._ptr(out) if m else None, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_interpolate: a repeated point (the points must be pairwise distinct), no points, count = 0 or a "
                             "context that holds no full tree")
        _check(rc)
        return out

    def poly_pow_mod(self, a, exp, modulus, count=1):
        """a^exp mod modulus (ecfft_poly_pow_mod <-> utils::pow_mod, src/utils.rs:194-211): `count` pairs laid end to end, a of count *
        na and modulus of count * nm coefficients, the modulus' leading coefficient nonzero in every pair; `exp` is one non-negative
        Python int shared by all pairs (0 gives the polynomial 1).  Returns count * (nm - 1) coefficients, zero-padded above the
        degree.  nm <= 65 works on any tree (the whole power runs in one workgroup per pair); a longer modulus needs a tree of
        next_pow2(2 (nm - 1) - 1) leaves, and na >= nm what poly_divrem(na, nm) needs.  numpy arrays (host) or contiguous CUDA tensors
        (device, on the current stream), both of the same kind.  Synchronous."""
        exp = int(exp)
        if exp < 0:
            raise ValueError("poly_pow_mod: the exponent must be non-negative")
        (a, modulus), (pa, pm), new, mem, stream = self._poly_io([a, modulus])
        assert count > 0 and a.shape[0] % count == 0 and modulus.shape[0] % count == 0
        na, nm = a.shape[0] // count, modulus.shape[0] // count
        eb = exp.to_bytes((exp.bit_length() + 7) // 8, "little")
        out = new(count * max(nm - 1, 0))
        rc = self._L.ecfft_poly_pow_mod(self._h, pa, na, ctypes.c_char_p(eb) if eb else None, len(eb), pm, nm,
                                        self._ptr(out) if out.shape[0] else None, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_pow_mod: empty operand, a modulus of fewer than 2 coefficients, a zero leading coefficient of the "
                             "modulus, count = 0 or a context that holds no full tree")
        _check(rc)
        return out

    def poly_mul_mod(self, a, b, modulus, count=1):
        """a * b mod modulus (ecfft_poly_mul_mod <-> div_rem(&a.naive_mul(&b), modulus), the step of utils::pow_mod, src/utils.rs:205,
        207): `count` triples laid end to end, a of count * na, b of count * nb and modulus of count * nm coefficients, the modulus'
        leading coefficient nonzero in every pair.  Returns count * (nm - 1) coefficients.  Needs a tree of next_pow2(na + nb - 1)
        leaves and what poly_divrem(na + nb - 1, nm) needs.  numpy arrays or contiguous CUDA tensors (current stream), all of the same
        kind.  Synchronous."""
        xs, ptrs, new, mem, stream = self._poly_io([a, modulus] if a is b else [a, b, modulus])
        (a, b, modulus), (pa, pb, pm) = ((xs[0], xs[0], xs[1]), (ptrs[0], ptrs[0], ptrs[1])) if a is b else (xs, ptrs)
        assert count > 0 and a.shape[0] % count == 0 and b.shape[0] % count == 0 and modulus.shape[0] % count == 0
        na, nb, nm = a.shape[0] // count, b.shape[0] // count, modulus.shape[0] // count
        out = new(count * max(nm - 1, 0))
        rc = self._L.ecfft_poly_mul_mod(self._h, pa, na, pb, nb, pm, nm, self._ptr(out) if out.shape[0] else None, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_mul_mod: empty operand, a modulus of fewer than 2 coefficients, a zero leading coefficient of the "
                             "modulus, count = 0 or a context that holds no full tree")
        _check(rc)
        return out

    def poly_compose_mod(self, f, g, modulus, count=1):
        """f(g) mod modulus (ecfft_poly_compose_mod; the step x^(p^i) -> x^(p^(i+1)) of distinct-degree factorisation, src/utils.rs:52-78,
        and the product of two endomorphisms in examples/schoofs.rs:197-235): `count` triples laid end to end, f of count * nf (it may
        be longer than the modulus), g of count * ng and modulus of count * nm coefficients, the modulus' leading coefficient nonzero
        in every triple.  Returns count * (nm - 1) coefficients, zero-padded above the degree.  nm <= COMPOSE_SMALL_MAX works on any
        tree (Horner in one workgroup per triple); a longer modulus needs a tree of next_pow2(2 (nm - 1) - 1) leaves, whatever nf is,
        and runs about 2 sqrt(nf) modular products (Brent-Kung baby and giant steps) instead of nf - 1; ng >= nm also needs what
        poly_divrem(ng, nm) needs.  numpy arrays (host) or contiguous CUDA tensors (device, on the current stream), all of the same
        kind.  Synchronous."""
        xs, ptrs, new, mem, stream = self._poly_io([f, modulus] if f is g else [f, g, modulus])
        (f, g, modulus), (pf, pg, pm) = ((xs[0], xs[0], xs[1]), (ptrs[0], ptrs[0], ptrs[1])) if f is g else (xs, ptrs)
        assert count > 0 and f.shape[0] % count == 0 and g.shape[0] % count == 0 and modulus.shape[0] % count == 0
        nf, ng, nm = f.shape[0] // count, g.shape[0] // count, modulus.shape[0] // count
        out = new(count * max(nm - 1, 0))
        rc = self._L.ecfft_poly_compose_mod(self._h, pf, nf, pg, ng, pm, nm, self._ptr(out) if out.shape[0] else None, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_compose_mod: empty operand, a modulus of fewer than 2 coefficients, a zero leading coefficient of the "
                             "modulus, count = 0 or a context that holds no full tree")
        _check(rc)
        return out

    def poly_gcd(self, a, b, count=1):
        """(g, degrees): the monic gcd (ecfft_poly_gcd <-> utils::gcd, src/utils.rs:132-141): `count` pairs laid end to end, a of
        count * na and b of count * nb coefficients; rows need not be trimmed and either operand may be zero.  g has count *
        max(na, nb) coefficients, zero-padded above its degree; degrees is a numpy int64 array of deg g per pair, -1 where a = b = 0
        (then g = 0).  gcd(a, 0) = a / lc(a), gcd(0, b) = b / lc(b).  max(na, nb) <= GCD_SMALL_MAX works on any tree; otherwise a tree
        of next_pow2(2 n - 1) leaves, n = max(na, nb) (the worst case over all degree patterns: a short b makes a long quotient).  numpy arrays (host) or contiguous
        CUDA tensors (device, on the current stream), both of the same kind.  Synchronous."""
        (a, b), (pa, pb), new, mem, stream = self._poly_io([a, b])
        assert count > 0 and a.shape[0] % count == 0 and b.shape[0] % count == 0
        na, nb = a.shape[0] // count, b.shape[0] // count
        g = new(count * max(na, nb))
        degrees = np.empty(count, np.int64)
        rc = self._L.ecfft_poly_gcd(self._h, pa, na, pb, nb, self._ptr(g) if g.shape[0] else None, degrees.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_gcd: empty operand, count = 0 or a context that holds no full tree")
        _check(rc)
        return g, degrees

    def poly_xgcd(self, a, b, count=1):
        """(s, t, g, degrees) with a*s + b*t = g, the monic gcd (ecfft_poly_xgcd <-> utils::xgcd, src/utils.rs:147-182): operands and
        g as poly_gcd; s has count * max(nb - 1, 1) and t count * max(na - 1, 1) coefficients, zero-padded: the cofactors of the
        classical extended Euclidean algorithm (deg s < deg b - deg g, deg t < deg a - deg g; b = 0: s = 1/lc(a), t = 0; a = 0 or
        b | a: s = 0, t = 1/lc(b)).  Tree, memory kinds and synchronisation as poly_gcd."""
        (a, b), (pa, pb), new, mem, stream = self._poly_io([a, b])
        assert count > 0 and a.shape[0] % count == 0 and b.shape[0] % count == 0
        na, nb = a.shape[0] // count, b.shape[0] // count
        g = new(count * max(na, nb))
        s, t = (new(count * max(nb - 1, 1)), new(count * max(na - 1, 1))) if na and nb else (new(0), new(0))
        degrees = np.empty(count, np.int64)
        rc = self._L.ecfft_poly_xgcd(self._h, pa, na, pb, nb, self._ptr(s) if s.shape[0] else None, self._ptr(t) if t.shape[0] else None,
                                     self._ptr(g) if g.shape[0] else None, degrees.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_xgcd: empty operand, count = 0 or a context that holds no full tree")
        _check(rc)
        return s, t, g, degrees

    def poly_xgcd_partial(self, a, b, stop, count=1):
        """(r, s, t, degrees): the first row r = s*a + t*b of the classical remainder sequence (r_0 = a, r_1 = b, (s_0, t_0) = (1, 0),
        (s_1, t_1) = (0, 1); deg a < deg b makes the first step a swap) with index j >= 1 and deg r < stop, where deg 0 = -1
        (ecfft_poly_xgcd_partial): what rational reconstruction, Pade approximation and Gao's Reed-Solomon decoder need.  The row is
        scaled so that t is monic (s where t = 0, the row (a, 1, 0)).  Operands as poly_gcd; r has count * max(na, nb), s count * nb
        and t count * na coefficients, zero-padded; degrees is a numpy int64 array of shape (count, 3): deg r, deg s, deg t, -1 for
        zero.  stop = 0 gives r = 0; any stop above deg b gives (b, 0, 1).  Tree, memory kinds and synchronisation as poly_gcd
        (XGCD_PARTIAL_SMALL_MAX = GCD_SMALL_MAX)."""
        (a, b), (pa, pb), new, mem, stream = self._poly_io([a, b])
        assert count > 0 and a.shape[0] % count == 0 and b.shape[0] % count == 0 and stop >= 0
        na, nb = a.shape[0] // count, b.shape[0] // count
        r, s, t = new(count * max(na, nb)), new(count * nb), new(count * na)
        degrees = np.empty((count, 3), np.int64)
        rc = self._L.ecfft_poly_xgcd_partial(self._h, pa, na, pb, nb, int(stop), self._ptr(r) if r.shape[0] else None, self._ptr(s) if s.shape[0] else None,
                                             self._ptr(t) if t.shape[0] else None, degrees.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_xgcd_partial: empty operand, count = 0 or a context that holds no full tree")
        _check(rc)
        return r, s, t, degrees

    def rs_decode(self, points, values, k, count=1):
        """(message, n_errors): Reed-Solomon decoding with errors (ecfft_rs_decode, Gao's algorithm on poly_xgcd_partial).  points: m
        pairwise distinct elements shared by all rows (the encoder is poly_eval_points at the same points); values: count * m received
        symbols; 1 <= k <= m.  message has count * k coefficients: row b is the unique f of degree < k whose codeword differs from
        row b of values in at most (m - k) // 2 positions; n_errors is a numpy int64 array of the number of corrected positions per
        row, -1 where no such f exists (the message row is then zero).  m <= RS_SMALL_MAX works on any tree (one workgroup per row,
        one launch for all rows); otherwise a tree of next_pow2(2 m + 1) leaves.  Two equal points, k = 0 or k > m raise ValueError.
        numpy arrays (host) or contiguous CUDA tensors (device, on the current stream), both of the same kind.  Synchronous."""
        (points, values), (pp, pv), new, mem, stream = self._poly_io([points, values])
        m = points.shape[0]
        assert count > 0 and m > 0 and values.shape[0] == count * m
        message = new(count * max(int(k), 0))
        n_errors = np.empty(count, np.int64)
        rc = self._L.ecfft_rs_decode(self._h, pp, m, pv, int(k), self._ptr(message) if message.shape[0] else None, n_errors.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("rs_decode: two equal points, k = 0, k > m, count = 0 or a context that holds no full tree")
        _check(rc)
        return message, n_errors

    def rs_encode(self, points, data, k, count=1):
        """codeword: the systematic Reed-Solomon encoder (ecfft_rs_encode).  points: m pairwise distinct elements shared by all rows;
        data: count * k symbols; 1 <= k <= m.  Returns count * m symbols: row b is f_b at all m points for the f_b of degree < k
        with f_b(points[i]) = data[b][i], i < k, so its first k symbols are the data (fully reduced) and the other m - k the parity.
        m <= RS_SMALL_MAX works on any tree (one fixed (m - k) x k matrix applied to every row); otherwise, for k > 64, a tree of
        next_pow2(k) leaves.  Two equal points, k = 0 or k > m raise ValueError.  numpy arrays (host) or contiguous CUDA tensors
        (device, on the current stream), both of the same kind.  Synchronous."""
        (points, data), (pp, pd), new, mem, stream = self._poly_io([points, data])
        m = points.shape[0]
        assert count > 0 and m > 0 and data.shape[0] == count * max(int(k), 0)
        codeword = new(count * m)
        rc = self._L.ecfft_rs_encode(self._h, pp, m, pd if data.shape[0] else None, int(k), self._ptr(codeword), count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("rs_encode: two equal points, k = 0, k > m, count = 0 or a context that holds no full tree")
        _check(rc)
        return codeword

    def rs_decode_erasures(self, points, values, erased, k, count=1, codeword=False):
        """(out, n_errors): Reed-Solomon decoding with erasures and errors (ecfft_rs_decode_erasures).  points, values, k as rs_decode;
        erased: count * m uint8 or bool entries of the same kind as values (numpy array or CUDA tensor), non-zero where the symbol is
        lost (its value is never read), or None for no erasure.  With m' kept symbols a row decodes to the unique f of degree < k
        that differs from the kept symbols in at most (m' - k) // 2 positions; n_errors is a numpy int64 array of their number, -1
        (and a zero row) where there is no such f or m' < k: exactly rs_decode on the kept points and values, beyond the radius
        too.  out has count * k coefficients of f, or with codeword=True count * m symbols, f at all m points: the erased positions
        filled in, the first k the corrected data of a code made by rs_encode.  Tree rule, argument errors, memory kinds and
        synchronisation as rs_decode."""
        (points, values), (pp, pv), new, mem, stream = self._poly_io([points, values])
        m = points.shape[0]
        assert count > 0 and m > 0 and values.shape[0] == count * m
        pe = None
        if erased is not None:
            if _is_torch(erased):
                import torch
                assert mem == MEM_DEVICE and erased.is_cuda and erased.is_contiguous() and erased.dtype in (torch.uint8, torch.bool)
                assert erased.numel() == count * m
                pe = erased.data_ptr()
            else:
                assert mem == MEM_HOST, "the mask is of the same kind as the values"
                erased = np.ascontiguousarray(erased)
                assert erased.dtype in (np.uint8, np.bool_) and erased.size == count * m
                pe = erased.ctypes.data
        out = new(count * (m if codeword else max(int(k), 0)))
        n_errors = np.empty(count, np.int64)
        rc = self._L.ecfft_rs_decode_erasures(self._h, pp, m, pv, pe, int(k), self._ptr(out) if out.shape[0] else None,
                                              RS_OUT_CODEWORD if codeword else RS_OUT_COEFFS, n_errors.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("rs_decode_erasures: two equal points, k = 0, k > m, count = 0 or a context that holds no full tree")
        _check(rc)
        return out, n_errors

    def seq_min_poly(self, seq, count=1):
        """(min_poly, orders): the minimal polynomials of `count` rows of N terms laid end to end (ecfft_seq_min_poly; what
        Berlekamp-Massey computes, here by the partial remainder row of (x^N, the row)).  A row's order L is the smallest L with
        s[i+L] + sum_{j<L} c_j s[i+j] = 0 for all 0 <= i < N - L; where 2 L <= N the monic C = x^L + sum c_j x^j is unique.
        min_poly has count * (N // 2 + 1) coefficients, row b holding C_b with its leading 1 at index L_b and zero above; orders is
        a numpy int64 array of the L_b, -1 where 2 L > N: the row is undetermined and its min_poly row zero.  N <= SEQ_SMALL_MAX
        works on any tree (one workgroup per row, one launch for all rows); otherwise a tree of next_pow2(2 N + 1) leaves.  numpy
        array (host) or contiguous CUDA tensor (device, on the current stream).  Synchronous."""
        (seq,), (ps,), new, mem, stream = self._poly_io([seq])
        assert count > 0 and seq.shape[0] % count == 0
        n = seq.shape[0] // count
        min_poly = new(count * (n // 2 + 1)) if n else new(0)
        orders = np.empty(count, np.int64)
        rc = self._L.ecfft_seq_min_poly(self._h, ps, n, self._ptr(min_poly) if min_poly.shape[0] else None, orders.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("seq_min_poly: an empty row, count = 0 or a context that holds no full tree")
        _check(rc)
        return min_poly, orders

    def seq_nth_term(self, char_poly, init, index, nout=1, count=1):
        """The terms s_index .. s_(index + nout - 1) of `count` linear recurrences laid end to end (ecfft_seq_nth_term, Fiduccia:
        x^index mod C against the initial terms).  char_poly: count * nc coefficients of the C_b, nc >= 2, leading coefficient
        non-zero (monic not required); init: count * (nc - 1) initial terms of the sequences with sum_{j<=L} c_j s[i+j] = 0;
        `index` is one non-negative Python int shared by all rows.  Returns count * nout terms.  nc <= SEQ_TERM_SMALL_MAX works on
        any tree (one workgroup per row); a longer recurrence needs a tree of next_pow2(2 (nc - 1) - 1) leaves.  numpy arrays
        (host) or contiguous CUDA tensors (device, on the current stream), both of the same kind.  Synchronous."""
        index = int(index)
        if index < 0:
            raise ValueError("seq_nth_term: the index must be non-negative")
        (char_poly, init), (pc, pi), new, mem, stream = self._poly_io([char_poly, init])
        assert count > 0 and char_poly.shape[0] % count == 0
        nc = char_poly.shape[0] // count
        assert init.shape[0] == count * max(nc - 1, 0)
        ib = index.to_bytes((index.bit_length() + 7) // 8, "little")
        out = new(count * max(int(nout), 0))
        rc = self._L.ecfft_seq_nth_term(self._h, pc, nc, pi if init.shape[0] else None, ctypes.c_char_p(ib) if ib else None, len(ib),
                                        self._ptr(out) if out.shape[0] else None, int(nout), count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("seq_nth_term: a characteristic polynomial of fewer than 2 coefficients, a zero leading coefficient, "
                             "nout = 0, count = 0 or a context that holds no full tree")
        _check(rc)
        return out

    def poly_find_roots(self, f, count=1):
        """(roots, n_roots): the distinct roots in the field (ecfft_poly_find_roots <-> utils::find_roots, src/utils.rs:25-44) of
        `count` polynomials laid end to end, f of count * nf coefficients; rows need not be trimmed.  roots has count * (nf - 1)
        elements: row b holds its n_roots[b] roots in ascending order of their standard form, then zeros; n_roots is a numpy int64
        array, 0 for a non-zero constant and -1 for the zero polynomial (every element is a root; the row is zero).  Multiplicities
        do not matter.  Deterministic: the splitting shifts are 1, 2, 3, ...  nf <= ROOTS_SMALL_MAX works on any tree (one launch
        for all rows); otherwise a tree of next_pow2(2 nf - 1) leaves.  numpy arrays (host) or contiguous CUDA tensors (device, on
        the current stream).  Synchronous."""
        (f,), (pf,), new, mem, stream = self._poly_io([f])
        assert count > 0 and f.shape[0] % count == 0
        nf = f.shape[0] // count
        roots = new(count * max(nf - 1, 0))
        n_roots = np.empty(count, np.int64)
        rc = self._L.ecfft_poly_find_roots(self._h, pf, nf, self._ptr(roots) if roots.shape[0] else None, n_roots.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_find_roots: empty operand, count = 0 or a context that holds no full tree")
        _check(rc)
        return roots, n_roots

    def poly_squarefree(self, f, count=1):
        """(s, degrees): the monic squarefree part s_b = f_b / gcd(f_b, f_b') (ecfft_poly_squarefree <-> utils::square_free_factors,
        src/utils.rs:46-50, made monic) of `count` polynomials laid end to end, f of count * nf coefficients; rows need not be
        trimmed.  s has count * nf coefficients, zero-padded; degrees is a numpy int64 array of deg s_b, 0 for a non-zero constant
        (s = 1) and -1 for the zero polynomial (a zero row).  nf <= DDF_SMALL_MAX works on any tree (one launch for all rows);
        otherwise a tree of next_pow2(2 nf - 1) leaves.  numpy arrays (host) or contiguous CUDA tensors (device, on the current
        stream).  Synchronous."""
        (f,), (pf,), new, mem, stream = self._poly_io([f])
        assert count > 0 and f.shape[0] % count == 0
        nf = f.shape[0] // count
        out = new(count * nf)
        degrees = np.empty(count, np.int64)
        rc = self._L.ecfft_poly_squarefree(self._h, pf, nf, self._ptr(out) if nf else None, degrees.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_squarefree: empty operand, count = 0 or a context that holds no full tree")
        _check(rc)
        return out, degrees

    def poly_distinct_degree(self, f, count=1):
        """(factors, degrees): the distinct-degree factorisation (ecfft_poly_distinct_degree <-> utils::distinct_degree_factors,
        src/utils.rs:52-78, with x^(p^i) where the reference takes x^(p i)) of `count` polynomials laid end to end, f of count * nf
        coefficients; rows need not be trimmed and multiplicities do not matter.  With nd = max(nf - 1, 1), degrees is a numpy int64
        array of shape (count, nd): degrees[b, d-1] = deg g_d, g_d the product of the monic irreducible factors of degree d of f_b (the
        zero polynomial: -1, 0, 0, ...).  factors has count * nd elements: row b holds the g_d of positive degree in ascending d, each
        as its low deg g_d coefficients (the leading 1 is implied), then zeros; ddf_unpack(row, degrees[b]) makes a dict of them.
        nf <= DDF_SMALL_MAX works on any tree (one launch for all rows); otherwise a tree of next_pow2(2 nf - 1) leaves.  numpy arrays
        (host) or contiguous CUDA tensors (device, on the current stream).  Synchronous."""
        (f,), (pf,), new, mem, stream = self._poly_io([f])
        assert count > 0 and f.shape[0] % count == 0
        nf = f.shape[0] // count
        nd = max(nf - 1, 1)
        factors = new(count * nd if nf else 0)
        degrees = np.empty((count, nd), np.int64)
        rc = self._L.ecfft_poly_distinct_degree(self._h, pf, nf, self._ptr(factors) if nf else None, degrees.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_distinct_degree: empty operand, count = 0 or a context that holds no full tree")
        _check(rc)
        return factors, degrees

    def ddf_unpack(self, row, degrees):
        """One row of poly_distinct_degree as {d: g_d}: g_d the deg g_d + 1 coefficients of the product of the irreducible factors of
        degree d, its leading 1 (in the crate's form) included.  Host arrays."""
        row = np.ascontiguousarray(row, self.field.dtype)
        std = np.zeros(self.field.shape(1), self.field.dtype)
        std.flat[0] = 1
        one = self.field.from_standard(std)
        out, pos = {}, 0
        for d, n in enumerate(np.asarray(degrees).tolist(), 1):
            if n > 0:
                out[d] = np.concatenate([row[pos:pos + n], one])
                pos += n
        return out

    def poly_equal_degree(self, g, d, count=1):
        """(factors, n_factors): the monic irreducible factors of degree d (ecfft_poly_equal_degree <->
        utils::equal_degree_factorization, src/utils.rs:82-113) of `count` polynomials laid end to end, g of count * ng coefficients;
        rows need not be trimmed.  Each g_b must be a squarefree product of irreducibles of degree d, which is what
        poly_distinct_degree returns once the leading 1 is appended (ddf_unpack); on other inputs the factors are unspecified.
        factors has count * max(ng - 1, 1) elements: row b holds its n_factors[b] factors, each as its low d coefficients (the leading
        1 is implied), in ascending lexicographic order of (c_0, .., c_(d-1)) as standard-form integers (Python's sorted on low-to-high
        coefficient lists), then zeros; edf_unpack(row, n, d) makes a list of them.  n_factors is a numpy int64 array: -1 for the
        zero polynomial, 0 for a non-zero constant, -2 where d does not divide the degree (zero rows).  Deterministic: the splitting
        shifts are 1, 2, 3, ...  ng <= EDF_SMALL_MAX works on any tree (one launch for all rows); otherwise a tree of
        next_pow2(2 ng - 1) leaves.  numpy arrays (host) or contiguous CUDA tensors (device, on the current stream).  Synchronous."""
        (g,), (pg,), new, mem, stream = self._poly_io([g])
        assert count > 0 and g.shape[0] % count == 0
        ng = g.shape[0] // count
        factors = new(count * max(ng - 1, 1) if ng else 0)
        n_factors = np.empty(count, np.int64)
        rc = self._L.ecfft_poly_equal_degree(self._h, pg, ng, int(d), self._ptr(factors) if ng else None, n_factors.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_equal_degree: empty operand, d = 0, count = 0 or a context that holds no full tree")
        _check(rc)
        return factors, n_factors

    def _crate_one(self):
        std = np.zeros(self.field.shape(1), self.field.dtype)
        std.flat[0] = 1
        return self.field.from_standard(std)

    def edf_unpack(self, row, n, d):
        """One row of poly_equal_degree as a list of its n factors, each the d + 1 coefficients with the leading 1 (in the crate's
        form) included.  Host arrays."""
        row = np.ascontiguousarray(row, self.field.dtype)
        one = self._crate_one()
        return [np.concatenate([row[i * d:(i + 1) * d], one]) for i in range(max(int(n), 0))]

    def poly_irreducible_factors(self, f):
        """{d: [factors]}: the DISTINCT monic irreducible factors of one polynomial f (host array), each with its leading 1, in the
        order of poly_equal_degree: poly_distinct_degree, then poly_equal_degree per non-empty d.  It computes no multiplicities;
        that policy stays with the caller.  The zero polynomial raises ValueError."""
        f = np.ascontiguousarray(f, self.field.dtype)
        fac, deg = self.poly_distinct_degree(f)
        if deg[0][0] < 0:
            raise ValueError("poly_irreducible_factors: the zero polynomial")
        out = {}
        for d, gd in self.ddf_unpack(fac, deg[0]).items():
            row, n = self.poly_equal_degree(np.ascontiguousarray(gd), d)
            out[d] = self.edf_unpack(row, n[0], d)
        return out

    def poly_squarefree_decompose(self, f, count=1):
        """(parts, degrees, lead): Yun's squarefree decomposition f_b = lead_b prod_i a_i^i (ecfft_poly_squarefree_decompose; the a_i
        monic, squarefree and pairwise coprime) of `count` polynomials laid end to end, f of count * nf coefficients; rows need not be
        trimmed.  With nd = max(nf - 1, 1), degrees is a numpy int64 array of shape (count, nd): degrees[b, i-1] = deg a_i (the zero
        polynomial: -1, 0, 0, ...; a non-zero constant: zeros).  parts has count * nd elements: row b holds the a_i of positive degree
        in ascending i, each as its low deg a_i coefficients (the leading 1 is implied), then zeros: the layout of
        poly_distinct_degree, so ddf_unpack(row, degrees[b]) makes the dict {i: a_i}.  lead has count elements: the leading
        coefficients, 0 for the zero polynomial.  nf <= FACTOR_SMALL_MAX works on any tree (one launch for all rows); otherwise a tree
        of next_pow2(2 nf - 1) leaves.  numpy arrays (host) or contiguous CUDA tensors (device, on the current stream).  Synchronous."""
        (f,), (pf,), new, mem, stream = self._poly_io([f])
        assert count > 0 and f.shape[0] % count == 0
        nf = f.shape[0] // count
        nd = max(nf - 1, 1)
        parts = new(count * nd if nf else 0)
        lead = new(count)
        degrees = np.empty((count, nd), np.int64)
        rc = self._L.ecfft_poly_squarefree_decompose(self._h, pf, nf, self._ptr(parts) if nf else None, degrees.ctypes.data, self._ptr(lead), count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_squarefree_decompose: empty operand, count = 0 or a context that holds no full tree")
        _check(rc)
        return parts, degrees, lead

    def poly_factor(self, f, count=1):
        """(factors, fdeg, fmult, n_factors, lead): the factorisation f_b = lead_b prod_j q_j^e_j over the distinct monic irreducible
        q_j (ecfft_poly_factor) of `count` polynomials laid end to end, f of count * nf coefficients; rows need not be trimmed.  With
        nd = max(nf - 1, 1): n_factors is a numpy int64 array, -1 for the zero polynomial and 0 for a non-zero constant; fdeg and fmult
        are int64 arrays of shape (count, nd) whose entries j < n_factors[b] hold deg q_j and e_j, the rest 0; factors has count * nd
        elements: row b holds the q_j laid end to end, each as its low deg q_j coefficients (the leading 1 is implied), in ascending
        (e_j, deg q_j, then the order of poly_equal_degree), then zeros; factor_unpack(row, fdeg[b], fmult[b], n_factors[b]) makes a
        list of them.  lead as in poly_squarefree_decompose.  Deterministic and byte-exact: nothing depends on the splitting shifts.
        nf <= FACTOR_SMALL_MAX works on any tree, with a number of launches that does not depend on count; otherwise a tree of
        next_pow2(2 nf - 1) leaves.  numpy arrays (host) or contiguous CUDA tensors (device, on the current stream).  Synchronous."""
        (f,), (pf,), new, mem, stream = self._poly_io([f])
        assert count > 0 and f.shape[0] % count == 0
        nf = f.shape[0] // count
        nd = max(nf - 1, 1)
        factors = new(count * nd if nf else 0)
        lead = new(count)
        fdeg, fmult = np.empty((count, nd), np.int64), np.empty((count, nd), np.int64)
        n_factors = np.empty(count, np.int64)
        rc = self._L.ecfft_poly_factor(self._h, pf, nf, self._ptr(factors) if nf else None, fdeg.ctypes.data, fmult.ctypes.data, n_factors.ctypes.data,
                                       self._ptr(lead), count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("poly_factor: empty operand, count = 0 or a context that holds no full tree")
        _check(rc)
        return factors, fdeg, fmult, n_factors, lead

    def factor_unpack(self, row, fdeg_row, fmult_row, n):
        """One row of poly_factor as [(q, e), ...]: q the deg q + 1 coefficients of the factor with its leading 1 (in the crate's form),
        e its multiplicity, in the call's order.  Host arrays."""
        row = np.ascontiguousarray(row, self.field.dtype)
        one = self._crate_one()
        out, pos = [], 0
        for j in range(max(int(n), 0)):
            d = int(fdeg_row[j])
            out.append((np.concatenate([row[pos:pos + d], one]), int(fmult_row[j])))
            pos += d
        return out

    @staticmethod
    def division_polynomial_len(n):
        """L(n): the number of coefficients of psi_n with the factor 2y of an even index removed"""
        n = int(n)
        return 1 if n < 2 else ((n * n - 1) // 2 + 1 if n & 1 else (n * n - 4) // 2 + 1)

    def division_polynomial(self, A, B, n):
        """psi_n of the curves y^2 = x^3 + A[b] x + B[b] (ecfft_division_polynomial <-> division_polynomial, examples/schoofs.rs:368-431):
        count * L(n) coefficients laid end to end, low to high, in the crate's form, not monic; the factor 2y of an even n is removed
        (psi_2 = 1).  A and B hold count elements each.  n <= 4 works on any tree, otherwise a tree of next_pow2(L(n)) leaves.
        numpy arrays (host) or contiguous CUDA tensors (device, on the current stream).  Asynchronous for device tensors."""
        (A, B), (pA, pB), new, mem, stream = self._poly_io([A, B])
        count = A.shape[0]
        assert count > 0 and B.shape[0] == count
        out = new(count * self.division_polynomial_len(n))
        rc = self._L.ecfft_division_polynomial(self._h, pA, pB, int(n), self._ptr(out), count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("division_polynomial: n must be at most SCHOOF_MAX_L, on a context that holds a full tree")
        _check(rc)
        return out

    def curve_trace_mod(self, A, B, l):
        """t mod l for the curves y^2 = x^3 + A[b] x + B[b] over the field, #E = p + 1 - t (ecfft_curve_trace_mod <->
        frobenius_trace_mod_l / has_even_order, examples/schoofs.rs:76-138, 345-366): a numpy int64 array with one residue in [0, l)
        per curve, -1 for a singular curve.  A and B hold count elements each in the crate's form (Field.from_standard), numpy
        arrays (host) or contiguous CUDA tensors (device, on the current stream).  l is 2 or an odd prime up to SCHOOF_MAX_L;
        anything else raises ValueError.  l <= 11: one launch for all curves, on any tree.  Above, the curves run one after
        another on a tree of next_pow2(2 L(l) - 1) leaves, L = division_polynomial_len.  Synchronous."""
        (A, B), (pA, pB), _, mem, stream = self._poly_io([A, B])
        count = A.shape[0]
        assert count > 0 and B.shape[0] == count
        t = np.empty(count, np.int64)
        rc = self._L.ecfft_curve_trace_mod(self._h, pA, pB, int(l), t.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("curve_trace_mod: l must be 2 or an odd prime up to SCHOOF_MAX_L, on a context that holds a full tree")
        _check(rc)
        return t

    def schoof_primes(self):
        """2, 3, 5, ... until the product exceeds 4 sqrt(p): the primes curve_cardinality uses"""
        p, m, out, l = self.field.MODULUS[self.field.name], 1, [], 2
        while m * m <= 16 * p:
            if l == 2 or (l % 2 and all(l % q for q in range(3, int(l ** 0.5) + 1, 2))):
                out.append(l)
                m *= l
            l += 1
        return out

    def curve_cardinality(self, A, B, traces=False):
        """#E(F_p) of the curves y^2 = x^3 + A[b] x + B[b] as a list of Python ints, 0 for a singular curve (ecfft_curve_cardinality
        <-> cardinality, examples/schoofs.rs:30-71): curve_trace_mod for every prime of schoof_primes(), then the CRT on the
        host.  traces=True also returns the residues, a numpy int64 array of count x len(schoof_primes()).  Needs the tree of the
        largest prime: 512 leaves for M31, 2^14 for secp256k1.  Synchronous."""
        (A, B), (pA, pB), _, mem, stream = self._poly_io([A, B])
        count = A.shape[0]
        assert count > 0 and B.shape[0] == count
        order = np.zeros(count * ORDER_BYTES, np.uint8)
        tr = np.empty((count, len(self.schoof_primes())), np.int64)
        rc = self._L.ecfft_curve_cardinality(self._h, pA, pB, order.ctypes.data, tr.ctypes.data, count, mem, stream)
        if rc == ERR_BAD_ARG:
            raise ValueError("curve_cardinality: no curves, or a context that holds no full tree")
        _check(rc)
        out = [int.from_bytes(order[b * ORDER_BYTES:(b + 1) * ORDER_BYTES].tobytes(), "little") for b in range(count)]
        return (out, tr) if traces else out

    # ---- the remaining FFTree algorithms (host numpy arrays; synchronous) ---------------------
    def _np(self, x):
        return np.ascontiguousarray(x, self.field.dtype)

    def mextend(self, evals, moiety):
        """src/fftree.rs:138-141"""
        a = self._np(evals); out = np.empty_like(a)
        _check(self._L.ecfft_mextend(self._h, a.ctypes.data, out.ctypes.data, a.shape[0], int(moiety), 1, MEM_HOST, None))
        return out

    def redc_z0(self, evals, a):
        """src/fftree.rs:264-267"""
        return self._redc(evals, a, Moiety.S0)

    def redc_z1(self, evals, a):
        """src/fftree.rs:272-275"""
        return self._redc(evals, a, Moiety.S1)

    def _redc(self, evals, a, moiety):
        e = self._np(evals); a = self._np(a); out = np.empty_like(e)
        assert a.shape[0] == e.shape[0]
        _check(self._L.ecfft_redc(self._h, e.ctypes.data, a.ctypes.data, out.ctypes.data, e.shape[0], int(moiety), MEM_HOST, None))
        return out

    def modular_reduce(self, evals, a, c):
        """src/fftree.rs:286-289"""
        e = self._np(evals); a = self._np(a); c = self._np(c); out = np.empty_like(e)
        assert a.shape[0] == e.shape[0] == c.shape[0]
        _check(self._L.ecfft_modular_reduce(self._h, e.ctypes.data, a.ctypes.data, c.ctypes.data, out.ctypes.data, e.shape[0], MEM_HOST, None))
        return out

    def vanish(self, domain):
        """src/fftree.rs:313-316"""
        d = self._np(domain)
        out = np.empty(self.field.shape(2 * d.shape[0]), self.field.dtype)
        _check(self._L.ecfft_vanish(self._h, d.ctypes.data, out.ctypes.data, d.shape[0], MEM_HOST, None))
        return out

    def degree(self, evals):
        """src/fftree.rs:195-198"""
        e = self._np(evals); deg = ctypes.c_size_t()
        _check(self._L.ecfft_degree(self._h, e.ctypes.data, e.shape[0], MEM_HOST, None, ctypes.byref(deg)))
        return deg.value

    def table_fma(self, x, y, m, which, t_off, t_stride, mode):
        """out[i] = f(x[i], y[i], T_m.table[which][t_off + i*t_stride]); mode 0: x*T, 1: x*T + y, 2: y - x*T, 3: (y - x)*T"""
        pin, out, pout, mem, stream, n = self._io(x)
        py, keep = None, None
        if y is not None:
            keep = y if _is_torch(y) else np.ascontiguousarray(y, self.field.dtype)     # keep the buffer alive across the call
            py = keep.data_ptr() if _is_torch(y) else keep.ctypes.data
        _check(self._L.ecfft_table_fma(self._h, pout, pin, py, n, m, which, t_off, t_stride, mode, mem, stream))
        return out

    # ---- shards of one EXTEND split over P GPUs (in place; see tests/split_model.py for the model) -----
    def _inplace(self, x):
        if _is_torch(x):
            import torch
            assert x.is_cuda and x.is_contiguous()
            return x.data_ptr(), MEM_DEVICE, torch.cuda.current_stream(x.device).cuda_stream
        assert isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"] and x.dtype == self.field.dtype
        return x.ctypes.data, MEM_HOST, None

    def extend_top_cyclic(self, shard, e, moiety, log_p, rank, recombine):
        ptr, mem, stream = self._inplace(shard)
        _check(self._L.ecfft_extend_top_cyclic(self._h, ptr, e, int(moiety), log_p, rank, int(recombine), mem, stream))

    def extend_local_block(self, shard, e, moiety, log_p):
        ptr, mem, stream = self._inplace(shard)
        _check(self._L.ecfft_extend_local_block(self._h, ptr, e, int(moiety), log_p, mem, stream))

    # ---- ONE transform split over the GPUs of a communicator (device tensors: this rank's block shard) -------------
    def _sharded(self, fn, comm, x, length, *extra):
        import torch
        assert _is_torch(x) and x.is_cuda and x.is_contiguous(), "sharded transforms take contiguous CUDA tensors"
        out = torch.empty_like(x)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(fn(self._h, comm._h, x.data_ptr(), out.data_ptr(), length, *extra, stream))
        return out

    def extend_sharded(self, comm, x_block, e, moiety, cyclic_in=False, cyclic_out=False):
        """FFTree::extend of ONE length-e vector held block-distributed over the ranks of `comm` (C++ / RCCL path);
        cyclic_in / cyclic_out: the shard on that side is cyclic (local j' = global j' * world + rank), one exchange fewer each"""
        if not (cyclic_in or cyclic_out):
            return self._sharded(self._L.ecfft_extend_sharded, comm, x_block, e, int(moiety))
        return self._sharded(self._L.ecfft_extend_sharded_layout, comm, x_block, e, int(moiety), int(cyclic_in), int(cyclic_out))

    def enter_sharded(self, comm, x_block, n):
        return self._sharded(self._L.ecfft_enter_sharded, comm, x_block, n)

    def exit_sharded(self, comm, y_block, n):
        return self._sharded(self._L.ecfft_exit_sharded, comm, y_block, n)

    # ---- benchmarking aid -------------------------------------------------------------------
    def low_map(self, direction):
        """32 / 16 / 0: the composite map the 1024-element low-level kernels run for the lowest ENTER (0) / EXIT (1) levels"""
        return self._L.ecfft_ctx_low_map(self._h, int(direction))

    def exit_cores(self):
        """3 / 4: EXTEND cores per EXIT level of the level driver (hooks build)"""
        return self._L.ecfft_ctx_exit_cores(self._h)

    def exit_low_cores(self):
        """3 / 4: EXTEND cores per level of the fused low-level EXIT kernel's loop (hooks build)"""
        return self._L.ecfft_ctx_exit_low_cores(self._h)

    def sym_bfly(self):
        """0 / 1 / 2: general basis, symmetric basis with one-multiply butterflies, symmetric basis under the general kernels (hooks build)"""
        return self._L.ecfft_ctx_sym_bfly(self._h)

    def low_sym(self):
        """bit 0 / bit 1: the 1024-element low-level ENTER / EXIT kernel runs one-multiply butterflies in its VALU sweeps (hooks build)"""
        return self._L.ecfft_ctx_low_sym(self._h)

    def enter_l11(self):
        """1 / 0: the EXTEND of ENTER level 11 runs on the compile-time row engine / on the run-time-tile row kernel (hooks build)"""
        return self._L.ecfft_ctx_enter_l11(self._h)

    def profile(self, on):
        _check(self._L.ecfft_profile_enable(self._h, int(on)))

    def profile_read(self):
        """[{name, launches, ms, alg_bytes}] per kernel class, from HIP events on the launch stream."""
        out = []
        for c in range(self._L.ecfft_profile_classes()):
            name = ctypes.create_string_buffer(64); n = ctypes.c_uint64(); ms = ctypes.c_double(); by = ctypes.c_double()
            _check(self._L.ecfft_profile_read(self._h, c, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(by)))
            out.append({"name": name.value.decode(), "launches": n.value, "ms": ms.value, "alg_bytes": by.value})
        return out

    # ---- pub fields ------------------------------------------------------------------------
    def table(self, which, m=None):
        m = self.n if m is None else m
        cnt = ctypes.c_size_t()
        _check(self._L.ecfft_tree_table(self._h, m, which, None, 0, ctypes.byref(cnt)))
        out = np.zeros(self.field.shape(cnt.value), self.field.dtype)
        _check(self._L.ecfft_tree_table(self._h, m, which, out.ctypes.data, cnt.value, ctypes.byref(cnt)))
        return out

    def leaves(self, m=None):
        m = self.n if m is None else m
        return self.table(TBL_F, m)[m:]

    def serialize(self, compress):
        """`FFTree::serialize_compressed` (compress=True) / `serialize_uncompressed` (src/fftree.rs:510-554) through the C ABI"""
        ln = ctypes.c_size_t()
        _check(self._L.ecfft_fftree_serialize(self._h, int(bool(compress)), None, 0, ctypes.byref(ln)))
        buf = ctypes.create_string_buffer(ln.value)
        _check(self._L.ecfft_fftree_serialize(self._h, int(bool(compress)), buf, ln.value, ctypes.byref(ln)))
        return buf.raw[:ln.value]

    def rational_map(self, k):
        """rational_maps[k] (src/fftree.rs:28) as (numerator[3], denominator[3]) coefficients, low -> high, zero padded"""
        if not hasattr(self, "_maps"):
            ln = max(self.n.bit_length() - 1, 1)
            num = np.zeros(self.field.shape(3 * ln), self.field.dtype); den = np.zeros(self.field.shape(3 * ln), self.field.dtype)
            _check(self._L.ecfft_tree_rational_maps(self._h, num.ctypes.data, den.ctypes.data))
            self._maps = (num, den)
        num, den = self._maps
        return num[3 * k:3 * k + 3], den[3 * k:3 * k + 3]

    def subtree_with_size(self, n):
        """src/fftree.rs:489-496 — the chain lives in one context, so this is a size check + view."""
        assert n > 0 and n & (n - 1) == 0
        if n > self.n:
            raise ValueError("FFTree is too small")
        return _SubtreeView(self, n)


class _SubtreeView:
    def __init__(self, tree, n):
        self.tree, self.n = tree, n

    def leaves(self):
        return self.tree.leaves(self.n)

    def table(self, which):
        return self.tree.table(which, self.n)

    def enter(self, c):
        if len(c) > self.n:
            raise ValueError("FFTree is too small")
        return self.tree.enter(c)

    def exit(self, e):
        if len(e) > self.n:
            raise ValueError("FFTree is too small")
        return self.tree.exit(e)


def device_info(device=0):
    buf = ctypes.create_string_buffer(256)
    lib().ecfft_device_info(device, buf, 256)
    return buf.value.decode()
