"""CPU-only checks of ecfft_poly_divrem's and ecfft_poly_inv_series' argument handling: the errors that need no device are reported
without one."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def prod():
    import ecfft_amd
    ecfft_amd.build.build()
    return ecfft_amd


def test_poly_divrem_argument_errors_without_gpu(prod):
    L, F = prod.lib(), prod.fftree
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ecfft_poly_divrem(None, p, 4, p, 2, p, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG            # no context
    assert L.ecfft_poly_divrem(None, p, 4, p, 2, p, None, 2, F.MEM_DEVICE, None) == F.ERR_BAD_ARG
    assert L.ecfft_poly_divrem(None, p, 0, p, 2, p, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG            # empty operands
    assert L.ecfft_poly_divrem(None, p, 4, p, 0, p, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG
    assert L.ecfft_poly_divrem(None, p, 4, p, 2, p, p, 0, F.MEM_HOST, None) == F.ERR_BAD_ARG            # count = 0
    assert L.ecfft_poly_divrem(None, p, 4, p, 2, None, None, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG      # no output
    assert "ecfft_poly_divrem" in F.EXPORTS


def test_poly_inv_series_argument_errors_without_gpu(prod):
    L, F = prod.lib(), prod.fftree
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ecfft_poly_inv_series(None, p, 4, p, 4, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG              # no context
    assert L.ecfft_poly_inv_series(None, p, 0, p, 4, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG              # nf = 0
    assert L.ecfft_poly_inv_series(None, p, 4, p, 0, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG              # k = 0
    assert L.ecfft_poly_inv_series(None, p, 4, p, 4, 0, F.MEM_HOST, None) == F.ERR_BAD_ARG              # count = 0
    assert "ecfft_poly_inv_series" in F.EXPORTS
