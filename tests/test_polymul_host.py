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



def test_python_mirror_passes_one_pointer_for_a_squaring(prod):
    """FFTree.poly_mul(a, a) hands the library ONE pointer for both operands, also when a needs a conversion (a list, a
    non-contiguous array): the library squares only when both operands are the same buffer.  Two equal operands stay two
    buffers.  The arguments come in the header's order with host memory."""
    import numpy as np
    F = prod.fftree
    calls = []

    class Rec:
        def ecfft_poly_mul(self, *args):
            calls.append(args)
            return F.OK

    t = object.__new__(F.FFTree)
    t._L, t._h, t.field = Rec(), 1234, prod.FIELDS["m31"]
    a = np.arange(1, 11, dtype=np.uint32)
    for x in (a, list(a), np.arange(1, 21, dtype=np.uint32)[::2]):
        calls.clear()
        out = t.poly_mul(x, x, count=2)
        assert out.shape[0] == 2 * 9
        (h, pa, na, pb, nb, po, count, mem, stream), = calls
        assert (h, na, nb, count, mem, stream) == (1234, 5, 5, 2, F.MEM_HOST, None)
        assert pa == pb and po == out.ctypes.data
    calls.clear()
    b = a.copy()
    t.poly_mul(a, b, count=2)
    (h, pa, na, pb, nb, po, count, mem, stream), = calls
    assert (h, na, nb, count, mem, stream) == (1234, 5, 5, 2, F.MEM_HOST, None)
    assert pa == a.ctypes.data and pb == b.ctypes.data and pa != pb
