"""GPU tests of ecfft_poly_pow_mod / ecfft_poly_mul_mod (utils::pow_mod, src/utils.rs:194-211): k_powmod_small (residues of at most
64 coefficients, the whole square-and-multiply in one workgroup) and the large regime (the reciprocal, the modulus and the base kept
as evaluations for the call; three lifts and three EXITs per modular product).  Every comparison is an equality of bytes or ints:
against the exact Barrett reference of tests/powmod_ref.py through the oracle's standard-form converters (so the crate's Montgomery
representation of secp256k1 is exercised), between the fused step and the one-shot poly_mul_mod, and against the Frobenius identity
a^p = a mod a modulus that splits into distinct linear factors, which needs no reference and runs at full size."""
import ctypes

import numpy as np
import pytest

import poly_ref as R
import powmod_ref as W
from conftest import std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P
BIG_TREE = {"secp256k1": 1 << 20, "m31": 1 << 22}

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


def modulus_std(field, nm, seed, lead=None):
    f = R.rand_std(field, nm, seed)
    R.set_nonzero(field, f, nm - 1)
    if lead is not None:
        f[nm - 1] = R.from_ints(field, [lead % P[field]])[0]
    return f


def rand_mem(field, n, seed):
    """n elements in the in-memory form without a per-element loop (secp256k1: any value < 2^255 is a reduced residue)"""
    rng = np.random.default_rng(seed)
    if field == "m31":
        return rng.integers(1, 2**31 - 1, n, dtype=np.uint32)
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)
    a[:, 0] |= np.uint64(1)
    return a


def check_pow(F, field, t, a, e, f, count=1):
    """t.poly_pow_mod on `count` pairs of standard-form a, f == the reference, pair by pair"""
    got = to_std(F, t.poly_pow_mod(to_mem(F, a), e, to_mem(F, f), count=count))
    d = f.shape[0] // count - 1
    assert got.shape[0] == count * d
    assert R.canonical(field, got).all()
    for i in range(count):
        want = W.pow_mod(field, rows(a, count, i), e, rows(f, count, i))
        assert np.array_equal(rows(got, count, i), want), (i, d, e.bit_length())
    return got


def na_of(kind, nm):
    return {"below": max(1, nm // 2), "at": nm, "above": 2 * nm + 3}[kind]


# ---- exact against the reference: the full exponent p ------------------------------------------------------------------------------
DEGREES = [1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 200]
KINDS = ["below", "at", "above"]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("idx,d", list(enumerate(DEGREES)))
def test_full_exponent_matches_reference(oracle_mod, field, idx, d):
    """a^p mod f (the power distinct_degree_factors takes): na below, at and above nm in turn, one pair and three"""
    F, t, nm = oracle_mod.field(field), tree(field, 4096), d + 1
    for count, kind in ((1, KINDS[idx % 3]), (3, KINDS[(idx + 1) % 3]), (1, KINDS[(idx + 2) % 3])):
        na = na_of(kind, nm)
        f = np.concatenate([modulus_std(field, nm, 1000 * d + 10 * count + i) for i in range(count)])
        a = R.rand_std(field, count * na, 77 * d + count)
        check_pow(F, field, t, a, P[field], f, count)


@pytest.mark.parametrize("d", [1024, 4097])
def test_full_exponent_m31_larger(oracle_mod, d):
    F, t = oracle_mod.field("m31"), tree("m31", 1 << 14)
    for na in (d // 3, d + 1, 2 * d + 5):
        check_pow(F, "m31", t, R.rand_std("m31", na, d + na), P["m31"], modulus_std("m31", d + 1, d))


# ---- short exponents at larger sizes ---------------------------------------------------------------------------------------------
# exponents 0, 1, 2, 3, 2^k and 2^k - 1 and one mixed pattern; at 2^16 + 1 the exact reference costs 5 s (M31) and 110 s (secp256k1)
# of pure-Python products per modular product, so k is 2 / 1 there and the mixed pattern is 7 / 3
SHORT_EXPS = {1024: [0, 1, 2, 3, 1 << 9, (1 << 9) - 1, 0xB6E5], 4097: [0, 1, 2, 3, 1 << 9, (1 << 9) - 1, 0xB6E5],
              ("m31", (1 << 16) + 1): [0, 1, 2, 3, 4, 7], ("secp256k1", (1 << 16) + 1): [0, 1, 2, 3]}


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d", [1024, 4097, (1 << 16) + 1])
def test_short_exponents(oracle_mod, field, d):
    F = oracle_mod.field(field)
    t = tree(field, 1 << 18)
    f = modulus_std(field, d + 1, d + 5, lead=None if d & 1 else 12345)
    a = R.rand_std(field, d, d + 6)
    exps = SHORT_EXPS.get(d) or SHORT_EXPS[(field, d)]
    fm, am = to_mem(F, f), to_mem(F, a)
    B = W.Barrett(field, f)
    for e in exps:
        got = to_std(F, t.poly_pow_mod(am, e, fm))
        assert np.array_equal(got, W.pow_mod(field, a, e, f, B)), e
    # the same exponent with extra high zero bytes, through the C ABI
    e = exps[-1]
    want = t.poly_pow_mod(am, e, fm)
    out = np.zeros_like(want)
    eb = e.to_bytes(2, "little") + bytes(11)
    from ecfft_amd import fftree as FT
    rc = t._L.ecfft_poly_pow_mod(t._h, am.ctypes.data, d, eb, len(eb), fm.ctypes.data, d + 1, out.ctypes.data, 1, FT.MEM_HOST, None)
    assert rc == FT.OK and np.array_equal(out, want)


# ---- cross-path identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d", [64, 65, 1 << 12, 1 << 16])
def test_cross_path_identities(field, d):
    """the fused step of pow_mod against the one-shot mul_mod (poly_mul + the division): bytes equal"""
    t = tree(field, 1 << 18)
    count = 2 if d <= (1 << 12) else 1
    a, f = rand_mem(field, count * d, d + 1), rand_mem(field, count * (d + 1), d + 2)
    mm = lambda x, y: t.poly_mul_mod(x, y, f, count=count)
    pw = lambda e: t.poly_pow_mod(a, e, f, count=count)
    a2 = mm(a, a)
    assert np.array_equal(pw(1), a)
    assert np.array_equal(pw(2), a2)
    assert np.array_equal(pw(3), mm(a2, a))
    e1, e2 = 0b101101, 0b11011
    assert np.array_equal(pw(e1 + e2), mm(pw(e1), pw(e2)))
    assert np.array_equal(mm(a, a.copy()), a2)              # the squaring path of poly_mul against the two-operand one


def test_regimes_agree_around_the_switch(oracle_mod):
    """the same residue problem posed at d = 64 (one workgroup) and, padded by a factor (x - c), consistent at d = 65 (transforms):
    a^e mod f == (a^e mod f (x - c)) mod f"""
    for field in FIELDS:
        F, t = oracle_mod.field(field), tree(field, 4096)
        f = modulus_std(field, 65, 3)
        lin = R.from_ints(field, [P[field] - 9, 1])
        f2 = R.mul_exact(field, f, lin)
        a = R.rand_std(field, 64, 4)
        e = P[field] >> 3
        small = t.poly_pow_mod(to_mem(F, a), e, to_mem(F, f))
        big = t.poly_pow_mod(to_mem(F, a), e, to_mem(F, f2))
        assert np.array_equal(t.poly_divrem(big, to_mem(F, f))[1], small)


DIV_SHAPES = [(1, 2), (3, 10), (2, 2), (100, 100), (72, 10), (73, 10), (74, 10), (130, 4), (131, 4), (132, 4), (257, 3), (258, 3), (259, 3),
              (1046, 24), (1047, 24), (1048, 24), (2050, 4), (2051, 4), (364, 300), (1019, 20), (2048, 1025)]   # test_gpu_polydiv.SHAPES, nb >= 2


@pytest.mark.parametrize("field", FIELDS)
def test_mul_mod_matches_reference(oracle_mod, field):
    """a b mod f with len(a b) = na, len(f) = nb at the division shapes: against mul_exact and long division"""
    F, t, p = oracle_mod.field(field), tree(field, 4096), P[field]
    for nc, nm in DIV_SHAPES:
        na = max(1, nc // 3)
        nb = nc + 1 - na
        a, b, f = R.rand_std(field, na, nc), R.rand_std(field, nb, nc + 1), modulus_std(field, nm, nc + 2)
        got = to_std(F, t.poly_mul_mod(to_mem(F, a), to_mem(F, b), to_mem(F, f)))
        want = W.long_division_rem(R.to_ints(field, R.mul_exact(field, a, b)), R.to_ints(field, f), p)
        assert R.to_ints(field, got) == want, (nc, nm)


# ---- the Frobenius identity at full size and full exponent -------------------------------------------------------------------------
def distinct_mem(field, d, seed):
    """d pairwise distinct seeded elements in the in-memory form"""
    rng = np.random.default_rng(seed)
    if field == "m31":
        c = np.unique(rng.integers(1, 2**31 - 1, d + d // 2 + 8, dtype=np.uint32))
        assert c.shape[0] >= d
        return rng.permutation(c)[:d].copy()
    c = rand_mem(field, d, seed)
    assert np.unique(c, axis=0).shape[0] == d
    return c


def gpu_from_roots(F, t, c):
    """f = prod (x + c_i) for d = 2^k constants c_i (in-memory form), by a product tree of batched poly_mul on monic nodes kept as
    their low coefficients: (x^m + A)(x^m + B) = x^2m + x^m (A + B) + A B.  d + 1 coefficients."""
    L, d, tail = c, c.shape[0], c.shape[1:]
    m = 1
    while m < d:
        half = d // m // 2
        X = L.reshape((half, 2, m) + tail)
        A = np.ascontiguousarray(X[:, 0]).reshape((half * m,) + tail)
        B = np.ascontiguousarray(X[:, 1]).reshape((half * m,) + tail)
        new = np.zeros((half, 2 * m) + tail, dtype=L.dtype)
        new[:, :2 * m - 1] = t.poly_mul(A, B, count=half).reshape((half, 2 * m - 1) + tail)
        hi = np.ascontiguousarray(new[:, m:]).reshape((half * m,) + tail)
        new[:, m:] = F.add(hi, F.add(A, B)).reshape((half, m) + tail)
        L = new.reshape((d,) + tail)
        m *= 2
    return np.concatenate([L, F.from_ints([1])])


def check_frobenius(F, t, field, d, seed):
    f = gpu_from_roots(F, t, distinct_mem(field, d, seed))
    for na in (d // 2 + 1, d + 1 + d // 4):
        a = rand_mem(field, na, seed + na)
        if na >= d + 1:
            want = t.poly_divrem(a, f)[1]
        else:
            want = np.zeros_like(f[:d])
            want[:na] = a
        assert np.array_equal(t.poly_pow_mod(a, P[field], f), want), (d, na)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("log_d", [12, 16])
def test_frobenius(oracle_mod, field, log_d):
    """f = prod (x - r_i) with distinct r_i: a^p mod f == a mod f for any a"""
    check_frobenius(oracle_mod.field(field), tree(field, 1 << 18), field, 1 << log_d, 100 + log_d)


@pytest.mark.parametrize("field", FIELDS)
def test_from_roots_matches_reference(oracle_mod, field):
    """the GPU product tree of the Frobenius tests against powmod_ref.from_roots"""
    F, t, p = oracle_mod.field(field), tree(field, 4096), P[field]
    roots = R.rand_std(field, 256, 11, specials=False)
    assert len(set(R.to_ints(field, roots))) == 256
    negc = to_mem(F, R.from_ints(field, [(-r) % p for r in R.to_ints(field, roots)]))
    assert np.array_equal(to_std(F, gpu_from_roots(F, t, negc)), W.from_roots(field, roots))


@pytest.mark.parametrize("field,log_d", [("secp256k1", 19), ("m31", 21)])
def test_frobenius_at_the_largest_size(oracle_mod, field, log_d):
    """d = 2^19 (secp256k1, N = 2^20) / 2^21 (M31, N = 2^22) with the full exponent p: some 500 / 60 modular products"""
    F, t = oracle_mod.field(field), tree(field, BIG_TREE[field])
    d = 1 << log_d
    f = gpu_from_roots(F, t, distinct_mem(field, d, 200 + log_d))
    a = rand_mem(field, d, 300 + log_d)
    assert np.array_equal(t.poly_pow_mod(a, P[field], f), a)


# ---- non-monic and special moduli, special bases ----------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d", [5, 64, 65, 300])
def test_special_moduli_and_bases(oracle_mod, field, d):
    F, t, p = oracle_mod.field(field), tree(field, 4096), P[field]
    e = p if d <= 65 else (p >> max(p.bit_length() - 40, 0))          # 40 bits at d = 300 for secp256k1, all 31 for M31
    a = R.rand_std(field, d, d)
    x = R.from_ints(field, [0, 1])
    for lead in (1, p - 1, 0xABCDEF123457 % p):
        check_pow(F, field, t, a, e, modulus_std(field, d + 1, 20 + d, lead=lead))
    sparse = R.from_ints(field, [p - 3] + [0] * (d - 1) + [1])                       # x^d - 3
    check_pow(F, field, t, a, e, sparse)
    check_pow(F, field, t, x, e, sparse)
    f0 = modulus_std(field, d + 1, 30 + d)
    f0[0] = 0                                                                        # f(0) = 0
    check_pow(F, field, t, a, e, f0)
    f = modulus_std(field, d + 1, 40 + d)
    got = check_pow(F, field, t, x, p, f)                                            # x^p mod f, the root finder's call
    assert got.shape[0] == d
    zero, one = R.from_ints(field, [0]), R.from_ints(field, [1])
    for e2 in (0, 1, 5, e):
        check_pow(F, field, t, zero, e2, f)
        check_pow(F, field, t, one, e2, f)
        check_pow(F, field, t, np.concatenate([one, R.from_ints(field, [0] * (d + 3))]), e2, f)


# ---- device tensors, repeated use ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d", [40, 700])
def test_device_tensors_match_host(field, d):
    import torch
    t = tree(field, 4096)
    a, b, f = rand_mem(field, 3 * (d + 9), 11), rand_mem(field, 3 * d, 12), rand_mem(field, 3 * (d + 1), 13)
    e = P[field] >> 5
    wp, wm = t.poly_pow_mod(a, e, f, count=3), t.poly_mul_mod(a, b, f, count=3)
    v = np.int64 if field != "m31" else np.int32           # torch has no unsigned 64-bit tensors: same bytes, signed view
    ta, tb, tf = (torch.from_numpy(x.view(v)).cuda() for x in (a, b, f))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tp, tm = t.poly_pow_mod(ta, e, tf, count=3), t.poly_mul_mod(ta, tb, tf, count=3)
    s.synchronize()
    assert np.array_equal(tp.cpu().numpy().view(wp.dtype), wp)
    assert np.array_equal(tm.cpu().numpy().view(wm.dtype), wm)


@pytest.mark.parametrize("field", FIELDS)
def test_repeated_use_and_trim(field):
    """a 2^16 tree serves two different calls back to back, trim between them: hundreds of steps must not grow the pool"""
    import ecfft_amd
    t = ecfft_amd.FIELDS[field].build_fftree(1 << 16)
    d1, d2 = 1 << 15, 3000
    a1, f1 = rand_mem(field, d1, 21), rand_mem(field, d1 + 1, 22)
    a2, f2 = rand_mem(field, 2 * d2, 23), rand_mem(field, 2 * (d2 + 1), 24)
    e_short, e_long = 0b1011, P[field] >> 2
    t.poly_pow_mod(a1, 2, f1)                               # the transform scratch (grow-only, not a temporary) reaches its size:
    t.trim()                                                # the three kept operands are lifted as one batch of three
    before = t.device_bytes
    short = t.poly_pow_mod(a1, e_short, f1)
    held_short = t.device_bytes
    first = t.poly_pow_mod(a2, e_long, f2, count=2)
    t.trim()
    assert t.device_bytes == before
    again = t.poly_pow_mod(a1, e_short, f1)
    assert np.array_equal(again, short)
    assert t.device_bytes == held_short                     # the same call holds the same temporaries
    t.poly_pow_mod(a1, (e_short << 20) | 0xFFFFF, f1)       # six times the steps ...
    assert t.device_bytes == held_short                     # ... in the same pool
    assert np.array_equal(t.poly_pow_mod(a2, e_long, f2, count=2), first)
    a2a = a2[:d2]
    assert np.array_equal(first[:d2], t.poly_mul_mod(t.poly_pow_mod(a2a, e_long - 1, f2[:d2 + 1]), a2a, f2[:d2 + 1]))
    t.trim()
    assert t.device_bytes == before


# ---- errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_bad_args(field):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    t = tree(field, 4096)
    L = t._L
    a, b, f = rand_mem(field, 3 * 300, 71), rand_mem(field, 3 * 100, 72), rand_mem(field, 3 * 101, 73)
    out = np.zeros_like(a)
    pa, pb, pf, po = a.ctypes.data, b.ctypes.data, f.ctypes.data, out.ctypes.data
    H, BAD = FT.MEM_HOST, FT.ERR_BAD_ARG
    e = b"\x2d\x01"
    pw = lambda *args: L.ecfft_poly_pow_mod(t._h, *args)
    mm = lambda *args: L.ecfft_poly_mul_mod(t._h, *args)
    assert pw(pa, 300, e, 2, pf, 101, po, 3, H, None) == FT.OK
    assert mm(pa, 300, pb, 100, pf, 101, po, 3, H, None) == FT.OK
    assert pw(None, 300, e, 2, pf, 101, po, 1, H, None) == BAD                        # NULL input or output
    assert pw(pa, 300, e, 2, None, 101, po, 1, H, None) == BAD
    assert pw(pa, 300, e, 2, pf, 101, None, 1, H, None) == BAD
    assert pw(pa, 300, None, 2, pf, 101, po, 1, H, None) == BAD                       # exp == NULL with exp_bytes > 0
    assert pw(pa, 300, None, 0, pf, 101, po, 1, H, None) == FT.OK                     # ... without: the exponent 0
    assert pw(pa, 0, e, 2, pf, 101, po, 1, H, None) == BAD
    assert pw(pa, 300, e, 2, pf, 101, po, 0, H, None) == BAD
    assert pw(pa, 300, e, 2, pf, 1, po, 1, H, None) == BAD                            # nm < 2: no residue
    assert pw(pa, 300, e, 2, pf, 0, po, 1, H, None) == BAD
    assert pw(pa, 300, e, 2, pf, 101, po, (1 << 64) // 3, H, None) == BAD             # bytes would wrap
    assert pw(pa, 300, e, 2, pf, 101, po, 1, 7, None) == BAD                          # unknown memory kind
    assert mm(None, 300, pb, 100, pf, 101, po, 1, H, None) == BAD
    assert mm(pa, 300, None, 100, pf, 101, po, 1, H, None) == BAD
    assert mm(pa, 300, pb, 100, None, 101, po, 1, H, None) == BAD
    assert mm(pa, 300, pb, 100, pf, 101, None, 1, H, None) == BAD
    assert mm(pa, 0, pb, 100, pf, 101, po, 1, H, None) == BAD
    assert mm(pa, 300, pb, 0, pf, 101, po, 1, H, None) == BAD
    assert mm(pa, 300, pb, 100, pf, 1, po, 1, H, None) == BAD
    assert mm(pa, 300, pb, 100, pf, 101, po, 0, H, None) == BAD
    assert mm(pa, 300, pb, 100, pf, 101, po, (1 << 64) // 3, H, None) == BAD
    assert mm(pa, 300, pb, 100, pf, 101, po, 1, 7, None) == BAD
    shard = ecfft_amd.FIELDS[field].build_extend_shard(1024, 1, 0)                    # EXTEND-only context: holds no full tree
    assert L.ecfft_poly_pow_mod(shard._h, pa, 8, e, 2, pf, 4, po, 1, H, None) == BAD
    assert L.ecfft_poly_mul_mod(shard._h, pa, 8, pb, 8, pf, 4, po, 1, H, None) == BAD
    with pytest.raises(ValueError, match="non-negative"):
        t.poly_pow_mod(a, -1, f, count=3)
    good = t.poly_pow_mod(a, 301, f, count=3)
    # a zero leading coefficient of the modulus in pair 0 and in the last pair of a batch, on every path: small and large residues,
    # na below and above nm; the context computes a correct power after each error
    for nm in (20, 101):
        ff = np.ascontiguousarray(f.reshape((3, 101) + f.shape[1:])[:, :nm]).reshape((3 * nm,) + f.shape[1:])
        for pair in (0, 2):
            zf = ff.copy()
            zf[pair * nm + nm - 1] = 0
            for na in (10, 300):
                aa = np.ascontiguousarray(a.reshape((3, 300) + a.shape[1:])[:, :na]).reshape((3 * na,) + a.shape[1:])
                with pytest.raises(ValueError, match="leading coefficient"):
                    t.poly_pow_mod(aa, 301, zf, count=3)
                with pytest.raises(ValueError, match="leading coefficient"):
                    t.poly_mul_mod(aa, aa, zf, count=3)
                assert np.array_equal(t.poly_pow_mod(a, 301, f, count=3), good)


@pytest.mark.parametrize("field", FIELDS)
def test_tree_rules(oracle_mod, field):
    """d <= 64 needs no transform; otherwise next_pow2(2d - 1) leaves, plus the division's rule for an operand of at least nm
    coefficients; mul_mod needs next_pow2(na + nb - 1) and the division's rule for (na + nb - 1, nm)"""
    F, t = oracle_mod.field(field), tree(field, 4096)
    e = 0b110101
    big = rand_mem(field, 10000, 81)
    f = rand_mem(field, 10000, 82)
    assert np.array_equal(to_std(F, t.poly_pow_mod(big[:64], e, f[:65])), W.pow_mod(field, to_std(F, big[:64]), e, to_std(F, f[:65])))
    t.poly_pow_mod(big[:2048], e, f[:2049])                      # 2d - 1 = 4095
    with pytest.raises(ValueError, match="too small"):
        t.poly_pow_mod(big[:2049], e, f[:2050])                  # 2d - 1 = 4097
    t.poly_pow_mod(big[:2050], e, f[:3])                         # nq = 2048: 2 nq - 1 = 4095, the power itself in one workgroup
    with pytest.raises(ValueError, match="too small"):
        t.poly_pow_mod(big[:2051], e, f[:3])
    with pytest.raises(ValueError, match="too small"):
        t.poly_pow_mod(big[:6000], e, f[:500])
    t.poly_mul_mod(big[:2048], big[2048:4097], f[:2100])         # na + nb - 1 = 4096
    with pytest.raises(ValueError, match="too small"):
        t.poly_mul_mod(big[:2049], big[2049:4098], f[:2100])     # 4097
    with pytest.raises(ValueError, match="too small"):
        t.poly_mul_mod(big[:1500], big[1500:3000], f[:3])        # nc = 2999, nq = 2997: 2 nq - 1 > 4096
    assert np.array_equal(t.poly_pow_mod(big[:64], e, f[:65]), t.poly_pow_mod(big[:64].copy(), e, f[:65]))
