"""CPU tests of the curve search (include/ecfft_hip.h: ecfft_find_curve_candidate, ecfft_curve_two_sylow, ecfft_find_curve,
ecfft_build_fftree_on_curve): the Python model tests/curve_ref.py against brute-force group orders and the crate's curve, the
candidate stream of the library against the model's, every argument error that is decided before a device is touched, and the host
instantiation of the Sylow computation (tests/cpp/curve_host.cpp, under AddressSanitizer + UBSan) against the model."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import curve_ref as R
import poly_ref
from conftest import ROOT

FIELDS = ["secp256k1", "m31"]


@pytest.fixture(scope="module")
def prod():
    import ecfft_amd
    ecfft_amd.build.build()
    return ecfft_amd


def crate_form(prod, field, ints):
    return prod.FIELDS[field].from_standard(poly_ref.from_ints(field, ints))


def v2(n):
    return (n & -n).bit_length() - 1


@pytest.mark.parametrize("p,cyclic", [(103, 2601), (107, 2809), (131, 4225)])
def test_model_gives_the_two_adicity_of_the_group_order(p, cyclic):
    """every curve with bb != 0 and a non-zero discriminant: n > 0 exactly on the curves with bb a square and the discriminant none
    (one point of order 2: the 2-Sylow subgroup is cyclic), and there 2^n is the full power of two in the number of points"""
    squares = {x * x % p for x in range(1, p)}
    called = 0
    for a in range(p):
        for bb in range(1, p):
            disc = (a * a - 4 * bb) % p
            if disc == 0:
                continue
            n, x = R.two_sylow(a, bb, p)
            if bb in squares and disc not in squares:
                called += 1
                assert n == v2(R.group_order(a, bb, p)) and n >= 2, (a, bb, n)
                y = R.sqrt_canon(R.rhs(x, a, bb, p), p)
                assert y is not None and R.pt_double_n((x, y), n - 1, a, bb, p) == (0, 0)
            else:
                assert (n, x) == (0, 0), (a, bb, n)
    assert called == cyclic


def test_model_on_the_crates_curve_and_singular_curves():
    p = R.P["secp256k1"]
    n, x = R.two_sylow_field("secp256k1", R.CRATE["a"], R.CRATE["bb"])
    assert n == 36
    assert R.pt_double_n((x, R.sqrt_canon(R.rhs(x, R.CRATE["a"], R.CRATE["bb"], p), p)), 35, R.CRATE["a"], R.CRATE["bb"], p) == (0, 0)
    assert R.pt_double_n(R.CRATE["gen"], 35, R.CRATE["a"], R.CRATE["bb"], p) == (0, 0)
    assert R.pt_double_n(R.CRATE["offset"], 36, R.CRATE["a"], R.CRATE["bb"], p) is not None
    for f in FIELDS:
        assert R.two_sylow_field(f, 5, 0) == (0, 0) and R.two_sylow_field(f, 2, 1) == (0, 0)


@pytest.mark.parametrize("key", sorted(R.FIRST_HITS))
def test_model_first_hits(key):
    field, seed, k = key
    assert R.find_curve(field, k, seed)[:2] == R.FIRST_HITS[key]


@pytest.mark.parametrize("field", FIELDS)
def test_candidate_stream_matches_the_model(prod, field):
    F = prod.FIELDS[field]
    for seed in (0, 1, 2**64 - 1):
        for index in (0, 1, 2631, 2**60 - 1):
            a, bb = F.find_curve_candidate(seed, index)
            assert (poly_ref.to_ints(field, F.to_standard(a))[0], poly_ref.to_ints(field, F.to_standard(bb))[0]) == R.candidate(field, seed, index)
    with pytest.raises(ValueError):
        F.find_curve_candidate(1, 2**60)


def test_argument_errors_before_any_device(prod):
    L, FT = prod.lib(), prod.fftree
    buf = (C.c_uint64 * 16)()
    p = C.addressof(buf)
    n32, i64, h = C.c_uint32(7), C.c_uint64(7), C.c_void_p()
    # ecfft_find_curve_candidate
    assert L.ecfft_find_curve_candidate(0, 1, 0, None, p) == FT.ERR_BAD_ARG
    assert L.ecfft_find_curve_candidate(0, 1, 0, p, None) == FT.ERR_BAD_ARG
    assert L.ecfft_find_curve_candidate(7, 1, 0, p, p) == FT.ERR_BAD_ARG
    assert L.ecfft_find_curve_candidate(1, 1, 2**60, p, p) == FT.ERR_BAD_ARG
    assert L.ecfft_find_curve_candidate(1, 1, 2**60 - 1, p, p) == FT.OK
    # ecfft_curve_two_sylow
    for args in ((0, 0, None, p, 1, p, p), (0, 0, p, None, 1, p, p), (0, 0, p, p, 1, None, p), (0, 0, p, p, 1, p, None), (0, 0, p, p, 0, p, p),
                 (7, 0, p, p, 1, p, p)):
        assert L.ecfft_curve_two_sylow(*args) == FT.ERR_BAD_ARG, args
    # ecfft_find_curve
    bi, bn = C.byref(i64), C.byref(n32)
    for field, eb in ((0, 32), (1, 4)):
        assert L.ecfft_find_curve(field, 0, 6, 1, 0, 16, None, bn, p, p, p, p) == FT.ERR_BAD_ARG
        assert L.ecfft_find_curve(field, 0, 6, 1, 0, 16, bi, None, p, p, p, p) == FT.ERR_BAD_ARG
        assert L.ecfft_find_curve(field, 0, 6, 1, 0, 0, bi, bn, p, p, p, p) == FT.ERR_BAD_ARG
        assert L.ecfft_find_curve(field, 0, 6, 1, 2**60 - 15, 16, bi, bn, p, p, p, p) == FT.ERR_BAD_ARG
        assert L.ecfft_find_curve(field, 0, 6, 1, 2**64 - 1, 2, bi, bn, p, p, p, p) == FT.ERR_BAD_ARG
        assert L.ecfft_find_curve(field, 0, 8 * eb + 1, 1, 0, 16, bi, bn, p, p, p, p) == FT.ERR_BAD_ARG
    assert L.ecfft_find_curve(7, 0, 6, 1, 0, 16, bi, bn, p, p, p, p) == FT.ERR_BAD_ARG
    assert (i64.value, n32.value) == (7, 7)                      # rejected calls write nothing


def test_build_fftree_on_curve_checks_the_curve_on_the_host(prod):
    """the crate's curve with one thing wrong at a time; every row is decided before a device is looked for"""
    import torch
    F, FT, L = prod.secp256k1, prod.fftree, prod.lib()
    cr, p = R.CRATE, R.P["secp256k1"]
    one = lambda v: crate_form(prod, "secp256k1", [v])
    pt = lambda xy: crate_form(prod, "secp256k1", list(xy))

    def call(n=256, a=cr["a"], bb=cr["bb"], gen=cr["gen"], m=cr["log_order"], off=cr["offset"], out=True):
        h = C.c_void_p()
        aa, b, g, o = one(a), one(bb), pt(gen), pt(off)
        rc = L.ecfft_build_fftree_on_curve(0, n, aa.ctypes.data, b.ctypes.data, g.ctypes.data, m, o.ctypes.data, 0, C.byref(h) if out else None)
        if h.value:
            L.ecfft_ctx_destroy(h)
        return rc

    assert call(n=48) == FT.ERR_NOT_POW2
    assert call(n=1 << 36) == FT.ERR_TREE_TOO_LARGE and call(n=1 << 40) == FT.ERR_TREE_TOO_LARGE
    assert call(n=1 << 8, m=8, gen=R.pt_double_n(cr["gen"], 28, cr["a"], cr["bb"], p)) == FT.ERR_TREE_TOO_LARGE
    assert F.build_fftree_on_curve(1 << 36, one(cr["a"]), one(cr["bb"]), pt(cr["gen"]), 36, pt(cr["offset"])) is None
    non_square = next(v for v in range(2, 50) if R.sqrt_canon(v, p) is None)
    bad = {
        "bb zero": dict(bb=0),
        "bb no square": dict(bb=non_square),
        "a changed": dict(a=cr["a"] + 1),
        "bb changed": dict(bb=cr["bb"] + 1),
        "generator x changed": dict(gen=(cr["gen"][0] + 1, cr["gen"][1])),
        "generator y changed": dict(gen=(cr["gen"][0], cr["gen"][1] + 1)),
        "offset x changed": dict(off=(cr["offset"][0] + 1, cr["offset"][1])),
        "offset y changed": dict(off=(cr["offset"][0], cr["offset"][1] + 1)),
        "generator doubled once": dict(gen=R.pt_double(cr["gen"], cr["a"], cr["bb"], p)),
        "order claimed too small": dict(m=35),
        "order claimed too large": dict(m=37),
        "order zero": dict(m=0, n=1),
        "order above the field": dict(m=257),
        "offset in the subgroup": dict(off=cr["gen"]),
        "no handle": dict(out=False),
    }
    for what, kw in bad.items():
        assert call(**kw) == FT.ERR_BAD_ARG, what
    with pytest.raises(ValueError):
        F.build_fftree_on_curve(256, one(cr["a"] + 1), one(cr["bb"]), pt(cr["gen"]), 36, pt(cr["offset"]))
    for null in range(4):
        h = C.c_void_p()
        ptrs = [x.ctypes.data for x in (one(cr["a"]), one(cr["bb"]), pt(cr["gen"]), pt(cr["offset"]))]
        ptrs[null] = None
        assert L.ecfft_build_fftree_on_curve(0, 256, ptrs[0], ptrs[1], ptrs[2], 36, ptrs[3], 0, C.byref(h)) == FT.ERR_BAD_ARG
    assert L.ecfft_build_fftree_on_curve(7, 256, *[x.ctypes.data for x in (one(1), one(1), pt((1, 1)))], 36, pt((1, 1)).ctypes.data, 0, C.byref(C.c_void_p())) == FT.ERR_BAD_ARG
    if not torch.cuda.is_available():
        assert call() == FT.ERR_HIP                                   # a good call gets as far as the device: no CPU fallback


@functools.lru_cache(maxsize=None)
def model_rows(field, seed, count):
    return [R.two_sylow_field(field, *R.candidate(field, seed, i)) for i in range(count)]


def test_host_instantiation_matches_the_model_under_sanitizers(tmp_path):
    exe = str(tmp_path / "curve_host")
    src = os.path.join(ROOT, "tests", "cpp", "curve_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src,
                    "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")     # (libamdhip64 is linked for its symbols, never called)
    r = subprocess.run([exe, "1", "4096"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and r.stdout.endswith("CURVE_HOST_OK\n"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = {f: [] for f in FIELDS}
    for line in r.stdout.splitlines()[:-1]:
        f, i, n, x = line.split()
        assert int(i) == len(got[f])
        got[f].append((int(n), int(x, 16)))
    for f in FIELDS:
        assert got[f] == model_rows(f, 1, 4096)
        assert max(n for n, _ in got[f]) >= 10
