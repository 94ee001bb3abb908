"""CPU-only checks of ecfft_poly_eval_points' argument handling: the errors that need no device are reported without one, and the
entry point is exported and bound."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def prod():
    import ecfft_amd
    ecfft_amd.build.build()
    return ecfft_amd


def test_poly_eval_points_argument_errors_without_gpu(prod):
    L, F = prod.lib(), prod.fftree
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ecfft_poly_eval_points(None, p, 4, p, 4, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG        # no context
    assert L.ecfft_poly_eval_points(None, p, 4, p, 4, p, 2, F.MEM_DEVICE, None) == F.ERR_BAD_ARG
    assert L.ecfft_poly_eval_points(None, p, 0, p, 4, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG        # nf = 0
    assert L.ecfft_poly_eval_points(None, p, 4, p, 0, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG        # m = 0
    assert L.ecfft_poly_eval_points(None, p, 4, p, 4, p, 0, F.MEM_HOST, None) == F.ERR_BAD_ARG        # count = 0
    assert L.ecfft_poly_eval_points(None, None, 4, None, 4, None, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG
    assert "ecfft_poly_eval_points" in F.EXPORTS
    assert L.ecfft_poly_eval_points.argtypes is not None and len(L.ecfft_poly_eval_points.argtypes) == 9


def test_python_mirror_passes_host_arguments(prod):
    """FFTree.poly_eval_points hands numpy inputs to the C ABI as host memory, in the header's parameter order (ctypes accepts extra
    trailing arguments silently, so a shifted list would turn host pointers into device pointers)"""
    import numpy as np
    F = prod.fftree
    calls = []

    class Rec:
        def ecfft_poly_eval_points(self, *args):
            calls.append(args)
            return F.OK

    t = object.__new__(F.FFTree)
    t._L, t._h, t.field = Rec(), 1234, prod.FIELDS["m31"]
    f, x = np.arange(2 * 7, dtype=np.uint32), np.arange(5, dtype=np.uint32)
    out = t.poly_eval_points(f, x, count=2)
    assert out.shape[0] == 10
    (h, pf, nf, px, m, po, count, mem, stream), = calls
    assert (h, nf, m, count, mem, stream) == (1234, 7, 5, 2, F.MEM_HOST, None)
    assert po == out.ctypes.data
