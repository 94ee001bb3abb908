"""GPU tests of ecfft_poly_compose_mod, f(g) mod h: k_compose_small (residues of at most 64 coefficients, Horner in one workgroup)
and the large regime (Brent-Kung baby and giant steps on the kept-modulus products of poly_pow_mod, k_compose_rows between them).
Every comparison is an equality of bytes or ints through the standard-form converters: against the exact Horner reference of
tests/compose_ref.py up to the sizes it can afford; above them against the values f(g(r_i)) at every root of a modulus that splits
into distinct linear factors, which determine the result; and, GPU against GPU, against the Frobenius iterates x^(p^i) of
poly_pow_mod."""
import ctypes

import numpy as np
import pytest

import compose_ref as C
import poly_ref as R
import powmod_ref as W
from conftest import horner_mt, std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P

_trees = {}


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def to_std(F, x):
    x = np.ascontiguousarray(x, F.dtype)
    out = np.empty_like(x)
    if x.shape[0]:
        F._to_std(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0])
    return out


def to_mem(F, x):
    return std_to_field(F, x) if x.shape[0] else np.ascontiguousarray(x)


def rows(x, count, i):
    n = x.shape[0] // count
    return x[i * n:(i + 1) * n]


def modulus_std(field, nm, seed):
    return R.set_nonzero(field, R.rand_std(field, nm, seed), nm - 1)


def ng_of(kind, nm):
    return {"below": max(1, nm // 2), "at": nm, "above": 2 * nm + 3}[kind]


KINDS = ["below", "at", "above"]


def check_compose(F, field, t, nf, ng, nm, count, seed):
    """t.poly_compose_mod on `count` different standard-form triples == the exact reference, row by row"""
    f, g = R.rand_std(field, count * nf, seed), R.rand_std(field, count * ng, seed + 1)
    h = np.concatenate([modulus_std(field, nm, seed + 2 + i) for i in range(count)])
    got = to_std(F, t.poly_compose_mod(to_mem(F, f), to_mem(F, g), to_mem(F, h), count=count))
    assert got.shape[0] == count * (nm - 1)
    assert R.canonical(field, got).all()
    for i in range(count):
        want = C.compose_mod(field, rows(f, count, i), rows(g, count, i), rows(h, count, i))
        assert np.array_equal(rows(got, count, i), want), (i, nf, ng, nm, count)


# ---- the small regime ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("idx,d", list(enumerate([1, 2, 3, 63, 64])))
def test_small_regime_matches_reference(oracle_mod, field, idx, d):
    """one workgroup per row: ng below nm on a 4-leaf tree (no transform), ng at nm and at 2 nm + 3 on the 4096 tree (the reduction
    of g needs it); one row and three different rows"""
    F, nm = oracle_mod.field(field), d + 1
    for j, nf in enumerate([1, 2, 3, 64, 65, 130]):
        for count, kind in ((1, KINDS[(idx + j) % 3]), (3, KINDS[(idx + j + 1) % 3])):
            ng = ng_of(kind, nm)
            t = tree(field, 4 if ng < nm else 4096)
            check_compose(F, field, t, nf, ng, nm, count, 1000 * d + 10 * nf + count)


# ---- the large regime against the exact reference -----------------------------------------------------------------------------------
LARGE = [("secp256k1", d) for d in (65, 66, 127, 128, 129)] + [("m31", d) for d in (65, 66, 127, 128, 129, 200, 300)]
NFS = [1, 2, 3, 4, 5, 13, 16, 17, 100, 101, 145]          # a perfect square, one above it, a last chunk of one coefficient (101, 145)


@pytest.mark.parametrize("idx,field,d", [(i, f, d) for i, (f, d) in enumerate(LARGE)])
def test_large_regime_matches_reference(oracle_mod, idx, field, d):
    F, t, nm = oracle_mod.field(field), tree(field, 4096), d + 1
    for j, nf in enumerate(NFS):
        count = 3 if nf in (2, 4, 17, 101) else 1
        check_compose(F, field, t, nf, ng_of(KINDS[(idx + j) % 3], nm), nm, count, 7000 * d + 10 * nf)


def test_large_regime_m31_long_f(oracle_mod):
    """f longer than the modulus, up to the bound of the exact reference for M31 (d = 300, nf = 290 and one above a square)"""
    F, t = oracle_mod.field("m31"), tree("m31", 4096)
    for nf, kind in ((290, "below"), (257, "above")):
        check_compose(F, "m31", t, nf, ng_of(kind, 301), 301, 1, 31 + nf)


# ---- larger sizes: a modulus that splits -----------------------------------------------------------------------------------------------
def check_split(F, field, t, d, nf, ng, seed):
    """h = prod (x - r_i) over d distinct roots: out has fewer than d coefficients and out(r_i) = f(g(r_i)) at EVERY root, which
    determines it.  Both sides by the oracle's Horner."""
    roots = R.rand_std(field, d, seed, specials=False)
    assert len(set(R.to_ints(field, roots))) == d
    h = W.from_roots(field, roots)
    f, g = to_mem(F, R.rand_std(field, nf, seed + 1)), to_mem(F, R.rand_std(field, ng, seed + 2))
    out = t.poly_compose_mod(f, g, to_mem(F, h))
    assert out.shape[0] == d and R.canonical(field, to_std(F, out)).all()
    rm = to_mem(F, roots)
    want = horner_mt(F, f, horner_mt(F, g, rm))
    assert np.array_equal(to_std(F, horner_mt(F, out, rm)), to_std(F, want)), (d, nf, ng)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d", [257, 1030])
def test_split_modulus(oracle_mod, field, d):
    F, t = oracle_mod.field(field), tree(field, 4096)
    check_split(F, field, t, d, d, d - 1, 50 + d)
    check_split(F, field, t, d, 2 * d + 3, d + 1 if d == 257 else d // 3, 60 + d)


def test_split_modulus_m31_4097(oracle_mod):
    check_split(oracle_mod.field("m31"), "m31", tree("m31", 1 << 14), 4097, 4097, 4097, 70)


# ---- Frobenius iterates, GPU against GPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d", [65, 200])
def test_frobenius_iterates(oracle_mod, field, d):
    """w = x^p mod h has coefficients in the field, so u(x)^p = u(w) mod h for any residue u: x^(p^2) = w(w), x^(p^3) = (w(w))(w)"""
    F, t, p = oracle_mod.field(field), tree(field, 4096), P[field]
    h = to_mem(F, modulus_std(field, d + 1, 90 + d))
    x = to_mem(F, R.from_ints(field, [0, 1]))
    w = t.poly_pow_mod(x, p, h)
    w2 = t.poly_compose_mod(w, w, h)
    assert np.array_equal(w2, t.poly_pow_mod(w, p, h))
    assert np.array_equal(t.poly_compose_mod(w2, w, h), t.poly_pow_mod(w2, p, h))


# ---- batches, memory kinds, repeated use ---------------------------------------------------------------------------------------------
def mem_inputs(F, field, nf, ng, nm, count, seed):
    f, g = R.rand_std(field, count * nf, seed), R.rand_std(field, count * ng, seed + 1)
    h = np.concatenate([modulus_std(field, nm, seed + 2 + i) for i in range(count)])
    return to_mem(F, f), to_mem(F, g), to_mem(F, h)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nf,ng,nm", [(37, 9, 21), (37, 50, 21), (50, 70, 101), (26, 250, 101)])
def test_every_row_of_a_batch_equals_its_own_call(oracle_mod, field, nf, ng, nm):
    F, t = oracle_mod.field(field), tree(field, 4096)
    f, g, h = mem_inputs(F, field, nf, ng, nm, 3, nf + ng + nm)
    got = t.poly_compose_mod(f, g, h, count=3)
    for i in range(3):
        assert np.array_equal(rows(got, 3, i), t.poly_compose_mod(rows(f, 3, i), rows(g, 3, i), rows(h, 3, i))), i


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d", [40, 150])
def test_device_tensors_match_host(oracle_mod, field, d):
    import torch
    F, t = oracle_mod.field(field), tree(field, 4096)
    f, g, h = mem_inputs(F, field, 2 * d + 1, d + 9, d + 1, 3, d)
    want = t.poly_compose_mod(f, g, h, count=3)
    v = np.int64 if field != "m31" else np.int32           # torch has no unsigned 64-bit tensors: same bytes, signed view
    tf, tg, th = (torch.from_numpy(x.view(v)).cuda() for x in (f, g, h))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = t.poly_compose_mod(tf, tg, th, count=3)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy().view(want.dtype), want)
    assert np.array_equal(t.poly_compose_mod(f, g, h, count=3), want)            # a repeated call: the same bytes


@pytest.mark.parametrize("field", FIELDS)
def test_repeated_calls_do_not_grow_the_pool(oracle_mod, field):
    import ecfft_amd
    F = oracle_mod.field(field)
    t = ecfft_amd.FIELDS[field].build_fftree(4096)
    f, g, h = mem_inputs(F, field, 120, 300, 201, 2, 5)
    first = t.poly_compose_mod(f, g, h, count=2)            # the transform scratch (grow-only, not a temporary) reaches its size
    t.trim()
    before = t.device_bytes
    for _ in range(2):
        assert np.array_equal(t.poly_compose_mod(f, g, h, count=2), first)
    held = t.device_bytes
    assert held > before
    for _ in range(4):
        assert np.array_equal(t.poly_compose_mod(f, g, h, count=2), first)
    assert t.device_bytes == held                           # 2 calls and 6 calls hold the same temporaries
    t.trim()
    assert t.device_bytes == before


# ---- errors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_tree_rule(oracle_mod, field):
    """the rule of poly_pow_mod, whatever nf is: next_pow2(2d - 1) leaves above 64 coefficients, and the division's rule for ng >= nm"""
    F, t = oracle_mod.field(field), tree(field, 4096)
    big = to_mem(F, R.rand_std(field, 6000, 81, specials=False))
    t.poly_compose_mod(big[:3], big[3:100], big[100:2149])                       # d = 2048: 2d - 1 = 4095
    with pytest.raises(ValueError, match="too small"):
        t.poly_compose_mod(big[:3], big[3:100], big[100:2150])                   # d = 2049: 2d - 1 = 4097
    t.poly_compose_mod(big[:5000], big[5000:5050], big[5100:5201])               # nf = 5000 at d = 100: nf does not enter
    t.poly_compose_mod(big[:3], big[10:2060], big[3000:3003])                    # ng = 2050, nm = 3: nq = 2048, 2 nq - 1 = 4095
    with pytest.raises(ValueError, match="too small"):
        t.poly_compose_mod(big[:3], big[10:2061], big[3000:3003])
    small = tree(field, 4)
    small.poly_compose_mod(big[:200], big[200:264], big[300:365])                # nm = 65: any tree
    with pytest.raises(ValueError, match="too small"):
        small.poly_compose_mod(big[:200], big[200:264], big[300:366])


@pytest.mark.parametrize("field", FIELDS)
def test_bad_args(oracle_mod, field):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    F, t = oracle_mod.field(field), tree(field, 4096)
    L = t._L
    f, g, h = mem_inputs(F, field, 30, 150, 101, 3, 71)
    out = np.zeros_like(g)
    pf, pg, ph, po = f.ctypes.data, g.ctypes.data, h.ctypes.data, out.ctypes.data
    H, BAD = FT.MEM_HOST, FT.ERR_BAD_ARG
    cm = lambda *args: L.ecfft_poly_compose_mod(t._h, *args)
    assert cm(pf, 30, pg, 150, ph, 101, po, 3, H, None) == FT.OK
    assert cm(None, 30, pg, 150, ph, 101, po, 1, H, None) == BAD                      # NULL input or output
    assert cm(pf, 30, None, 150, ph, 101, po, 1, H, None) == BAD
    assert cm(pf, 30, pg, 150, None, 101, po, 1, H, None) == BAD
    assert cm(pf, 30, pg, 150, ph, 101, None, 1, H, None) == BAD
    assert cm(pf, 0, pg, 150, ph, 101, po, 1, H, None) == BAD                         # an empty f, an empty g
    assert cm(pf, 30, pg, 0, ph, 101, po, 1, H, None) == BAD
    assert cm(pf, 30, pg, 150, ph, 1, po, 1, H, None) == BAD                          # nm = 1: no residue
    assert cm(pf, 30, pg, 150, ph, 0, po, 1, H, None) == BAD
    assert cm(pf, 30, pg, 150, ph, 101, po, 0, H, None) == BAD
    assert cm(pf, 30, pg, 150, ph, 101, po, (1 << 64) // 3, H, None) == BAD           # bytes would wrap
    assert cm(pf, 30, pg, 150, ph, 101, po, 1, 7, None) == BAD                        # unknown memory kind
    shard = ecfft_amd.FIELDS[field].build_extend_shard(1024, 1, 0)                    # EXTEND-only context: holds no full tree
    assert L.ecfft_poly_compose_mod(shard._h, pf, 8, pg, 8, ph, 4, po, 1, H, None) == BAD
    with pytest.raises(ValueError, match="fewer than 2"):
        t.poly_compose_mod(f[:5], g[:5], h[:1])
    with pytest.raises(ValueError, match="empty operand"):
        t.poly_compose_mod(f[:0], g[:5], h[:4])
    good = t.poly_compose_mod(f, g, h, count=3)
    # a zero leading coefficient of the modulus in ONE row of three, in both regimes, ng below and above nm; the context computes
    # a correct composition after each error
    for nm in (20, 101):
        hh = np.ascontiguousarray(h.reshape((3, 101) + h.shape[1:])[:, :nm]).reshape((3 * nm,) + h.shape[1:])
        for row in (0, 2):
            zh = hh.copy()
            zh[row * nm + nm - 1] = 0
            for ng in (10, 150):
                gg = np.ascontiguousarray(g.reshape((3, 150) + g.shape[1:])[:, :ng]).reshape((3 * ng,) + g.shape[1:])
                with pytest.raises(ValueError, match="leading coefficient"):
                    t.poly_compose_mod(f, gg, zh, count=3)
                assert np.array_equal(t.poly_compose_mod(f, g, h, count=3), good)
