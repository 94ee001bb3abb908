"""CPU-only checks of ecfft_poly_mul's argument handling: the errors that need no device are reported without one."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def prod():
    import ecfft_amd
    ecfft_amd.build.build()
    return ecfft_amd


def test_poly_mul_argument_errors_without_gpu(prod):
    L, F = prod.lib(), prod.fftree
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ecfft_poly_mul(None, p, 1, p, 1, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG        # no context
    assert L.ecfft_poly_mul(None, p, 4, p, 3, p, 2, F.MEM_DEVICE, None) == F.ERR_BAD_ARG
    assert L.ecfft_poly_mul(None, p, 0, p, 1, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG        # empty operand
    assert L.ecfft_poly_mul(None, p, 1, p, 0, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG
    assert L.ecfft_poly_mul(None, p, 1, p, 1, p, 0, F.MEM_HOST, None) == F.ERR_BAD_ARG        # count = 0
    assert "ecfft_poly_mul" in F.EXPORTS

