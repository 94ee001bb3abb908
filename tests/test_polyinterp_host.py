"""CPU-only checks of ecfft_poly_interpolate: the errors that need no device are reported without one, the entry point is exported
and bound, the Python mirror passes its arguments in the header's order, and a small-prime model of the algorithm pins the padding
algebra (a group padded with the REPEATED point 0 at weight 0 interpolates x^k f)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def prod():
    import ecfft_amd
    ecfft_amd.build.build()
    return ecfft_amd


def test_poly_interpolate_argument_errors_without_gpu(prod):
    L, F = prod.lib(), prod.fftree
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ecfft_poly_interpolate(None, p, 4, p, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG        # no context
    assert L.ecfft_poly_interpolate(None, p, 4, p, p, 2, F.MEM_DEVICE, None) == F.ERR_BAD_ARG
    assert L.ecfft_poly_interpolate(None, p, 0, p, p, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG        # m = 0
    assert L.ecfft_poly_interpolate(None, p, 4, p, p, 0, F.MEM_HOST, None) == F.ERR_BAD_ARG        # count = 0
    assert L.ecfft_poly_interpolate(None, None, 4, None, None, 1, F.MEM_HOST, None) == F.ERR_BAD_ARG
    assert "ecfft_poly_interpolate" in F.EXPORTS
    assert L.ecfft_poly_interpolate.argtypes is not None and len(L.ecfft_poly_interpolate.argtypes) == 8


def test_python_mirror_passes_host_arguments(prod):
    """FFTree.poly_interpolate hands numpy inputs to the C ABI as host memory, in the header's parameter order (ctypes accepts extra
    trailing arguments silently, so a shifted list would turn host pointers into device pointers)"""
    import numpy as np
    F = prod.fftree
    calls = []

    class Rec:
        def ecfft_poly_interpolate(self, *args):
            calls.append(args)
            return F.OK

    t = object.__new__(F.FFTree)
    t._L, t._h, t.field = Rec(), 1234, prod.FIELDS["m31"]
    x, y = np.arange(5, dtype=np.uint32), np.arange(2 * 5, dtype=np.uint32)
    out = t.poly_interpolate(x, y, count=2)
    assert out.shape[0] == 10
    (h, px, m, py, po, count, mem, stream), = calls
    assert (h, m, count, mem, stream) == (1234, 5, 2, F.MEM_HOST, None)
    assert (px, py) == (x.ctypes.data, y.ctypes.data)                           # points first, then values
    assert po == out.ctypes.data

    class Bad(Rec):
        def ecfft_poly_interpolate(self, *args):
            return F.ERR_BAD_ARG

    t._L = Bad()
    with pytest.raises(ValueError, match="repeated point"):
        t.poly_interpolate(x, y, count=2)


# ---- the algorithm on lists mod a small prime ------------------------------------------------------------------------------------
PRIME = 2**31 - 1


def add(a, b):
    n = max(len(a), len(b))
    a, b = a + [0] * (n - len(a)), b + [0] * (n - len(b))
    return [(u + v) % PRIME for u, v in zip(a, b)]


def mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, u in enumerate(a):
        if u:
            for j, v in enumerate(b):
                out[i + j] = (out[i + j] + u * v) % PRIME
    return out


def ev(f, x):
    acc = 0
    for c in reversed(f):
        acc = (acc * x + c) % PRIME
    return acc


def leaf_numerator(xs, cs):
    """what k_interp_leaves computes for one block: one coefficient per lane, len(xs) steps keeping (M_t, N_t)"""
    B = len(xs)
    M, N = [1] + [0] * (B - 1), [0] * B
    for xt, ct in zip(xs, cs):
        Ms, Ns = [0] + M[:-1], [0] + N[:-1]                  # the neighbour coefficient
        N = [(Ns[j] - xt * N[j] + ct * M[j]) % PRIME for j in range(B)]
        M = [(Ms[j] - xt * M[j]) % PRIME for j in range(B)]
    return N


def interpolate_model(xs, ys, leaf):
    """steps 1-4 of DESIGN.md 5.5 with leaf blocks of `leaf` points; returns the m coefficients"""
    m = len(xs)
    P = leaf
    while P < m:
        P *= 2
    k = P - m
    pts = xs + [0] * k
    if P == leaf:                                            # no transform: weights formed directly over the real points
        den = [1] * m
        for i in range(m):
            for j in range(m):
                if j != i:
                    den[i] = den[i] * (xs[i] - xs[j]) % PRIME
        c = [y * pow(d, PRIME - 2, PRIME) % PRIME for y, d in zip(ys, den)] + [0] * k
        top = leaf_numerator(pts, c)
    else:
        lv = [[[(-x) % PRIME, 1] for x in pts]]
        while len(lv[-1]) > 2:
            lv.append([mul(lv[-1][2 * i], lv[-1][2 * i + 1]) for i in range(len(lv[-1]) // 2)])
        A, B, d = lv[-1][0][:-1], lv[-1][1][:-1], P // 2     # M_l = x^d + A, M_r = x^d + B
        low = add(mul(A, B), [0] * d + add(A, B))
        Mp = (low + [0] * P)[:P] + [1]
        assert not any(Mp[:k])                               # Mp = x^k M
        M = Mp[k:]
        dM = [(j + 1) * M[j + 1] % PRIME for j in range(m)]
        den = [ev(dM, x) for x in xs]
        assert all(den)                                      # distinct points
        c = [y * pow(dv, PRIME - 2, PRIME) % PRIME for y, dv in zip(ys, den)] + [0] * k
        N = [leaf_numerator(pts[i:i + leaf], c[i:i + leaf]) for i in range(0, P, leaf)]
        for L in lv:
            if len(L[0]) - 1 < leaf:
                continue                                     # the levels below the leaf blocks are the leaf kernel's
            N = [add(mul(N[2 * i], L[2 * i + 1]), mul(N[2 * i + 1], L[2 * i])) for i in range(len(N) // 2)]
        assert len(N) == 1
        top = (N[0] + [0] * P)[:P]
        assert not any(N[0][P:])
    assert not any(top[:k])                                  # the padded sum is x^k f
    return top[k:k + m]


@pytest.mark.parametrize("leaf", [1, 4, 64])
@pytest.mark.parametrize("m", [1, 5, 8, 9, 13, 64, 65, 100])
def test_padding_algebra_model(m, leaf):
    """the group padded with k = P - m copies of the point 0 at weight 0, with 0 also among the real points"""
    import random
    rnd = random.Random(m * 31 + leaf)
    xs = [0] + rnd.sample(range(1, PRIME), m - 1)
    rnd.shuffle(xs)
    ys = [rnd.randrange(PRIME) for _ in range(m)]
    f = interpolate_model(xs, ys, leaf)
    assert len(f) == m and [ev(f, x) for x in xs] == ys
    g = [rnd.randrange(PRIME) for _ in range(m)]
    assert interpolate_model(xs, [ev(g, x) for x in xs], leaf) == g


def test_model_sees_a_repeated_point():
    """M'(x_i) = 0 exactly at a repeated point: what the device flag reports"""
    xs = [3, 0, 7, 11, 0, 5, 9, 2, 6]
    with pytest.raises(AssertionError):
        interpolate_model(xs, list(range(9)), 4)
