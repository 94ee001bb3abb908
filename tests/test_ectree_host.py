"""CPU tests of the short-Weierstrass front end on the product (include/ecfft_hip.h: ecfft_curve_point_mul,
ecfft_curve_point_two_adicity, ecfft_curve_find_generator, ecfft_build_ec_fftree): every argument error that is decided before a device
is touched, the crate's M31 tree through the generic builder against the model, and the host instantiation of the builder, its checks
and the point kernels' group law (tests/cpp/ec_tree_host.cpp, under AddressSanitizer + UBSan) against the model tests/ec_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ec_ref as E
from conftest import ROOT


@pytest.fixture(scope="module")
def prod():
    import ecfft_amd
    ecfft_amd.build.build()
    return ecfft_amd


def curve(field, A, B):
    return next(c for c in E.fixture() if (c["field"], c["A"], c["B"]) == (field, A, B))


def secp_10():
    """secp256k1 (1, 0): generator, offset and v from the model"""
    p = E.P["secp256k1"]
    v, gen, off, x = E.find_generator(1, 0, curve("secp256k1", 1, 0)["order"], p)
    return p, v, gen, off


def test_point_calls_reject_bad_shapes_before_any_device(prod):
    L, FT = prod.lib(), prod.fftree
    buf = (C.c_uint64 * 64)()
    p = C.addressof(buf)
    for field in (0, 1):
        ok = dict(A=p, B=p, nc=1, P=p, inf=None, k=p, nk=1, kb=4, out=p, io=p, count=3)

        def mul(**kw):
            a = dict(ok, **kw)
            return L.ecfft_curve_point_mul(field, 0, a["A"], a["B"], a["nc"], a["P"], a["inf"], a["k"], a["nk"], a["kb"], a["out"], a["io"], a["count"])
        for bad in (dict(A=None), dict(B=None), dict(P=None), dict(k=None), dict(out=None), dict(io=None), dict(count=0), dict(kb=0), dict(kb=41),
                    dict(nc=2), dict(nc=0), dict(nk=2), dict(nk=0), dict(nk=4)):
            assert mul(**bad) == FT.ERR_BAD_ARG, bad

        def adic(**kw):
            a = dict(dict(ok, cap=8), **kw)
            return L.ecfft_curve_point_two_adicity(field, 0, a["A"], a["B"], a["nc"], a["P"], a["inf"], a["cap"], a["out"], a["count"])
        eb = 32 if field == 0 else 4
        for bad in (dict(A=None), dict(B=None), dict(P=None), dict(out=None), dict(count=0), dict(nc=2), dict(cap=8 * eb + 3)):
            assert adic(**bad) == FT.ERR_BAD_ARG, bad
    assert L.ecfft_curve_point_mul(7, 0, p, p, 1, p, None, p, 1, 4, p, p, 3) == FT.ERR_BAD_ARG
    assert L.ecfft_curve_point_two_adicity(7, 0, p, p, 1, p, None, 8, p, 3) == FT.ERR_BAD_ARG


def test_find_generator_rejects_bad_arguments_before_any_device(prod):
    L, FT = prod.lib(), prod.fftree
    v, x = C.c_uint(7), C.c_uint64(7)
    for field, name in ((0, "secp256k1"), (1, "m31")):
        F = prod.FIELDS[name]
        A, B = F.from_ints([1]), F.from_ints([6])
        order = (12).to_bytes(40, "little")
        gen = np.zeros(F.shape(2), F.dtype)
        call = lambda a=A.ctypes.data, b=B.ctypes.data, o=order, start=1, mx=16, vo=C.byref(v): L.ecfft_curve_find_generator(
            field, 0, a, b, o, start, mx, vo, gen.ctypes.data, gen.ctypes.data, C.byref(x))
        assert call(a=None) == FT.ERR_BAD_ARG and call(b=None) == FT.ERR_BAD_ARG and call(o=None) == FT.ERR_BAD_ARG and call(vo=None) == FT.ERR_BAD_ARG
        assert call(start=0) == FT.ERR_BAD_ARG and call(mx=0) == FT.ERR_BAD_ARG
        assert call(start=2**60, mx=2) == FT.ERR_BAD_ARG and call(start=2**64 - 1, mx=2) == FT.ERR_BAD_ARG
        assert call(o=bytes(40)) == FT.ERR_BAD_ARG                                   # an order of zero
        z = F.from_ints([0])
        assert call(a=z.ctypes.data, b=z.ctypes.data) == FT.ERR_BAD_ARG              # a singular curve
        assert (v.value, x.value) == (7, 7)                                          # rejected calls write nothing
        assert call(o=(15).to_bytes(40, "little")) == FT.OK and v.value == 0         # an odd order: nothing to find, and no device needed
        v.value = 7
    assert L.ecfft_curve_find_generator(1, 0, A.ctypes.data, B.ctypes.data, order, 2**31 - 10, 16, C.byref(v), None, None, None) == FT.ERR_BAD_ARG   # x must stay below p
    assert L.ecfft_curve_find_generator(7, 0, A.ctypes.data, B.ctypes.data, order, 1, 16, C.byref(v), None, None, None) == FT.ERR_BAD_ARG


def test_build_ec_fftree_checks_curve_and_points_on_the_host(prod):
    """every row of the header's table with one thing wrong at a time; each is decided before a device is looked for"""
    import torch
    FT, L = prod.fftree, prod.lib()
    p, v, gen, off = secp_10()
    assert v == 4
    F = prod.secp256k1
    one = lambda val: F.from_ints([val])
    pt = lambda xy: F.from_ints(list(xy))

    def call(n=16, A=1, B=0, g=gen, m=v, o=off, out=True, field=0):
        h = C.c_void_p()
        a, b, gg, oo = one(A), one(B), pt(g), pt(o)
        rc = L.ecfft_build_ec_fftree(field, n, a.ctypes.data, b.ctypes.data, gg.ctypes.data, m, oo.ctypes.data, 0, C.byref(h) if out else None)
        if h.value:
            L.ecfft_ctx_destroy(h)
        return rc

    assert call(n=12) == FT.ERR_NOT_POW2
    assert call(n=32) == FT.ERR_TREE_TOO_LARGE and call(n=1 << 40) == FT.ERR_TREE_TOO_LARGE
    assert F.build_ec_fftree(32, one(1), one(0), pt(gen), v, pt(off)) is None
    g2 = E.add(gen, gen, 1, p)
    two_torsion = (0, 0)                                                 # the point of order 2 of y^2 = x^3 + x
    bad = {
        "singular curve": dict(A=0, B=0),
        "singular curve with the points on it": dict(A=p - 3, B=2, g=(1, 0), o=(1, 0), m=1, n=2),
        "generator x changed": dict(g=(gen[0] + 1, gen[1])),
        "generator y changed": dict(g=(gen[0], gen[1] + 1)),
        "offset x changed": dict(o=(off[0] + 1, off[1])),
        "offset y changed": dict(o=(off[0], off[1] + 1)),
        "B changed": dict(B=1),
        "generator doubled once": dict(g=g2),
        "order claimed too small": dict(m=v - 1, n=8),
        "order claimed too large": dict(m=v + 1),
        "offset in the subgroup": dict(o=gen),
        "offset whose double is in the subgroup": dict(g=g2, m=v - 1, o=gen, n=8),
        "offset of order 2": dict(o=two_torsion),
        "order zero": dict(m=0, n=1),
        "order above the field": dict(m=257),
        "no handle": dict(out=False),
        "unknown field": dict(field=7),
    }
    for what, kw in bad.items():
        assert call(**kw) == FT.ERR_BAD_ARG, what
    with pytest.raises(ValueError):
        F.build_ec_fftree(16, one(1), one(1), pt(gen), v, pt(off))
    for null in range(4):
        h = C.c_void_p()
        ptrs = [x.ctypes.data for x in (one(1), one(0), pt(gen), pt(off))]
        ptrs[null] = None
        assert L.ecfft_build_ec_fftree(0, 16, ptrs[0], ptrs[1], ptrs[2], v, ptrs[3], 0, C.byref(h)) == FT.ERR_BAD_ARG
    # ("no suitable isogeny at some level" cannot be reached through this call: for a generator of order exactly 2^m the isogeny whose
    # kernel is generated by 2^(m-1) gen always qualifies.  The builder's own answer is checked in the host program below.)
    if not torch.cuda.is_available():
        assert call() == FT.ERR_HIP                                      # a good call gets as far as the device: no CPU fallback


@pytest.mark.parametrize("n", [2, 64, 4096])
def test_the_crates_m31_tree_through_the_generic_builder_is_the_models(prod, n):
    """build_m31 is build_short_weierstrass with the crate's constants: leaves, maps and layers of ecfft_build_points against the model"""
    p, cr = E.P["m31"], E.CRATE_M31
    log_n = n.bit_length() - 1
    f, num, den = prod.m31.build_points(n)
    g = E.double_n(cr["gen"], cr["log_order"] - log_n, cr["A"], p)
    maps = E.velu_chain(cr["A"], cr["B"], g, log_n, p)
    assert [tuple(int(v) for v in num[3 * k:3 * k + 3]) for k in range(log_n)] == [m[0] for m in maps]
    assert [tuple(int(v) for v in den[3 * k:3 * k + 3]) for k in range(log_n)] == [m[1] for m in maps]
    lv = E.leaves(cr["A"], cr["B"], cr["gen"], cr["log_order"], cr["offset"], n, p)
    assert [int(v) for v in f[n:]] == lv
    for k, layer in enumerate(E.layers(lv, maps, p)):
        sz = n >> k
        assert [int(v) for v in f[sz:2 * sz]] == layer[:sz]


def _commands():
    """(lines, expected output lines) for tests/cpp/ec_tree_host.cpp"""
    cmds, want = [], []
    hx = lambda v: "%x" % v
    for c in E.fixture():
        field, A, B, order = c["field"], c["A"], c["B"], c["order"]
        p = E.P[field]
        # the group law: [k] R for a valid candidate R and scalars that reach every exceptional case
        R = next(E.candidate(x, A, B, p) for x in range(1, 50) if E.candidate(x, A, B, p))
        for k in (0, 1, 2, 3, order - 1, order, order + 1, order >> E.v2(order), 2**320 - 1):
            cmds.append(f"mul {field} {A} {B} {R[0]} {R[1]} {hx(k)}")
            got = E.mul(k, R, A, p)
            want.append("mul inf" if got is None else f"mul {hx(got[0])} {hx(got[1])}")
            want.append(f"adic {E.two_adicity(got, A, p, E.MAX_TWO_ADICITY[field])}")
        fg = E.find_generator(A, B, order, p, max_candidates=200)
        if fg is None:
            continue
        v, gen, off, _ = fg
        if off == (0, 0):                          # a 2-group: the header's recipe, four times the generator and the generator as the offset
            off, gen, v = gen, E.double_n(gen, 2, A, p), v - 2
        args = f"{field} {A} {B} {gen[0]} {gen[1]} {v} {off[0]} {off[1]}"
        cmds.append(f"check {args}"); want.append("check 1")
        cmds.append(f"check {field} {A} {B} {gen[0]} {(gen[1] + 1) % p} {v} {off[0]} {off[1]}"); want.append("check 0")
        cmds.append(f"check {field} {A} {B} {gen[0]} {gen[1]} {v - 1} {off[0]} {off[1]}"); want.append("check 0")
        cmds.append(f"check {field} {A} {B} {gen[0]} {gen[1]} {v} {gen[0]} {gen[1]}"); want.append("check 0")
        log_n = min(v, 4)
        n = 1 << log_n
        cmds.append(f"tree {args} {log_n}")
        g = E.double_n(gen, v - log_n, A, p)
        maps = E.velu_chain(A, B, g, log_n, p)
        assert maps is not None
        want.append("tree 0")
        want += ["map " + " ".join(hx(x) for x in m[0] + m[1]) for m in maps]
        lv = E.leaves(A, B, gen, v, off, n, p)
        want += [f"leaf {hx(x)}" for x in lv]
        for k, layer in enumerate(E.layers(lv, maps, p)[1:], 1):
            want.append(f"layer {k} " + " ".join(hx(x) for x in layer))
        cmds.append(f"tree {args} {v + 1}"); want.append("tree 1")
        if order >> v > 1:                         # a "generator" with an odd part in its order: no isogeny lowers a two-adicity it does not have
            cmds.append(f"tree {field} {A} {B} {R[0]} {R[1]} {v} {off[0]} {off[1]} 1"); want.append("tree 2")
    return cmds, want


def test_host_instantiation_matches_the_model_under_sanitizers(tmp_path):
    exe, script = str(tmp_path / "ec_tree_host"), tmp_path / "commands.txt"
    src = os.path.join(ROOT, "tests", "cpp", "ec_tree_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src,
                    "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True, capture_output=True)
    cmds, want = _commands()
    script.write_text("\n".join(cmds) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")     # (libamdhip64 is linked for its symbols, never called)
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and r.stdout.endswith("EC_TREE_HOST_OK\n"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()[:-1]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
