"""GPU tests of ecfft_seq_min_poly and ecfft_seq_nth_term (linear recurrences): k_seq_minpoly_small (N <= SEQ_SMALL_MAX terms, a
row per workgroup, on any tree), the large regime of min_poly (the partial xgcd driver against one shared x^N, then
k_seq_minpoly_finish per row), k_seq_terms_small (nc <= SEQ_TERM_SMALL_MAX) and the large regime of nth_term (the kept-modulus
power on the base x, then k_seq_terms).  Orders, minimal polynomials and terms are compared byte for byte, through the oracle's
standard-form converters, with the exact model of tests/seq_ref.py.

The tree rule of seq_nth_term is that of poly_pow_mod, next_pow2(2 (nc - 1) - 1) leaves: nc = 66 takes 256 leaves and fails on
128, nc = 130 takes 512 and fails on 256."""
import ctypes
import random

import numpy as np
import pytest

import gcd_ref as G
import poly_ref as R
import seq_ref as Q
from conftest import std_to_field

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


def from_ints(F, field, v):
    return std_to_field(F, G.arr(field, v, len(v)))


def recurrent(p, rng, L, n):
    """n terms of a seeded recurrence of order L (for almost every seed its linear complexity)"""
    C = [rng.randrange(p) for _ in range(L)] + [1]
    return Q.iterate(p, C, [rng.randrange(p) for _ in range(L)], n) if L else [0] * n


def beyond_half(p, rng, n):
    """a row of linear complexity n // 2 + 1, one past the determined range: a recurrence of order L' = n - n // 2 - 1 whose last
    term is wrong has complexity n - L' (a generic row of n terms only reaches ceil(n / 2))"""
    row = recurrent(p, rng, n - n // 2 - 1, n)
    row[-1] = (row[-1] + 1 + rng.randrange(p - 1)) % p
    return row


# ---- seq_min_poly ----

def min_poly_and_check(F, field, t, rows, want, device=False):
    """seq_min_poly on the rows (int lists of one length) against want = [(L or -1, C)]: orders and every byte of min_poly"""
    n, count, nh = len(rows[0]), len(rows), len(rows[0]) // 2 + 1
    seq = from_ints(F, field, [x for row in rows for x in row])
    if device:
        import torch
        mp, orders = t.seq_min_poly(torch.from_numpy(seq).cuda(), count=count)
        assert mp.is_cuda
        mp = mp.cpu().numpy()
    else:
        mp, orders = t.seq_min_poly(seq, count=count)
    assert mp.shape[0] == count * nh and orders.shape == (count,) and orders.dtype == np.int64
    mp = to_std(F, mp)
    for i, (L, C) in enumerate(want):
        assert orders[i] == L, (n, i, orders[i], L)
        assert np.array_equal(mp[i * nh:(i + 1) * nh], G.arr(field, C, nh)), (n, i)


def small_rows(p, n, rng):
    """(name, row) for one call: the shapes the kernel's epilogue has to tell apart"""
    h = n // 2
    g = 2 + rng.randrange(p - 2)
    rows = [("zero", [0] * n),
            ("geometric", [5 * pow(g, i, p) % p for i in range(n)]),
            ("order N/2", recurrent(p, rng, h, n)),
            ("order N/2 + 1", beyond_half(p, rng, n)),
            ("c_0 = 0", Q.iterate(p, [0, rng.randrange(p), rng.randrange(p), 1], [0, 0, 1], n)),
            ("spike at the end", [0] * (n - 1) + [1 + rng.randrange(p - 1)]),
            ("spike at the start", [1 + rng.randrange(p - 1)] + [0] * (n - 1)),
            # s_(i+k) = a s_i from (1, 0, .., 0): zero runs between the non-zero terms, so the remainder sequence of (x^N, h) has
            # quotients of degree k > 1
            ("zero runs", Q.iterate(p, [p - 3] + [0] * (max(n // 4, 2) - 1) + [1], [1] + [0] * (max(n // 4, 2) - 1), n)),
            ("uniform a", [rng.randrange(p) for _ in range(n)]),
            ("uniform b", [rng.randrange(p) for _ in range(n)]),
            ("uniform c", [rng.randrange(p) for _ in range(n)]),
            ("all p - 1", [p - 1] * n),
            ("p - 1 recurrence", Q.iterate(p, [p - 1, p - 1, 1], [p - 1, p - 1], n))]
    return rows


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 64, 254, 255])
def test_min_poly_small(oracle_mod, field, n):
    """13 rows of every shape in one call on a tree of four leaves, from host arrays and from device tensors"""
    p, rng = P[field], random.Random(1000 + n)
    F, t = oracle_mod.field(field), tree(field, 4)
    named = small_rows(p, n, rng)
    rows = [row for _, row in named]
    want = [Q.euclid_min_poly(p, row) for row in rows]
    byname = {name: w for (name, _), w in zip(named, want)}
    assert byname["zero"] == (0, [1])
    assert byname["order N/2 + 1"] == (-1, []) and Q.berlekamp_massey(p, rows[3])[0] == n // 2 + 1
    if n >= 2:
        assert byname["geometric"][0] == 1 and byname["order N/2"][0] == n // 2
        assert byname["spike at the end"][0] == -1 and byname["all p - 1"] == (1, [p - 1, 1])
    if n >= 8:
        assert byname["c_0 = 0"][0] == 3 and byname["c_0 = 0"][1][0] == 0 and byname["zero runs"][0] == n // 4
        for row, (L, C) in zip(rows, want):                          # the model against textbook Berlekamp-Massey, on these rows too
            Lb, Cb = Q.berlekamp_massey(p, row)
            assert (L, C) == ((Lb, Cb) if 2 * Lb <= n else (-1, [])), row
    min_poly_and_check(F, field, t, rows, want)
    min_poly_and_check(F, field, t, rows, want, device=True)


@pytest.mark.parametrize("field", FIELDS)
def test_min_poly_more_rows_than_one_wave_of_workgroups(oracle_mod, field):
    """700 rows of 12 terms in one call, every order from 0 to 7 (7: undetermined)"""
    p, n, rng = P[field], 12, random.Random(5)
    F, t = oracle_mod.field(field), tree(field, 4)
    rows = [beyond_half(p, rng, n) if i % 8 == 7 else recurrent(p, rng, i % 8, n) for i in range(700)]
    want = [Q.euclid_min_poly(p, row) for row in rows]
    assert {w[0] for w in want} == {-1, 0, 1, 2, 3, 4, 5, 6}
    min_poly_and_check(F, field, t, rows, want)


LARGE = [("secp256k1", 256), ("m31", 256), ("secp256k1", 600), ("m31", 1100)]


@pytest.mark.parametrize("field,n", LARGE)
def test_min_poly_large(oracle_mod, field, n):
    """N = 256: the first size of the regime, which the workgroup leaf alone finishes; N + 1 above the half-GCD leaf (512 / 1024
    coefficients): real half-GCD steps.  Orders N/2, N/4, N/2 + 1 (undetermined) and the zero row; Berlekamp-Massey is the model
    here (tests/test_seq_ref_host.py ties it to the definition)."""
    p, rng = P[field], random.Random(n)
    leaves = 4
    while leaves < 2 * n + 1:
        leaves <<= 1
    F, t = oracle_mod.field(field), tree(field, leaves)
    rows = [recurrent(p, rng, n // 2, n), recurrent(p, rng, n // 4, n), beyond_half(p, rng, n), [0] * n]
    want = []
    for row in rows:
        L, C = Q.berlekamp_massey(p, row)
        want.append((L, C) if 2 * L <= n else (-1, []))
    assert [w[0] for w in want] == [n // 2, n // 4, -1, 0] and Q.berlekamp_massey(p, rows[2])[0] == n // 2 + 1
    min_poly_and_check(F, field, t, rows, want)
    # one size below next_pow2(2 N + 1): refused before anything runs, the outputs untouched
    small = tree(field, leaves // 2)
    seq = from_ints(F, field, rows[0])
    mp = np.full(small.field.elem_bytes * (n // 2 + 1), 0xAB, np.uint8)
    orders = np.full(1, 77, np.int64)
    from ecfft_amd import fftree as FT
    rc = small._L.ecfft_seq_min_poly(small._h, seq.ctypes.data, n, mp.ctypes.data, orders.ctypes.data, 1, FT.MEM_HOST, None)
    assert rc == FT.ERR_TREE_TOO_SMALL and orders[0] == 77 and (mp == 0xAB).all()
    with pytest.raises(ValueError, match="too small"):
        small.seq_min_poly(seq)


# ---- seq_nth_term ----

def term_rows(p, rng, L):
    """six rows on three characteristic polynomials: a monic one (four rows, one of them with zero initial terms), a non-monic one
    and one with c_0 = 0"""
    Ca = [rng.randrange(p) for _ in range(L)] + [1]
    Cb = [rng.randrange(p) for _ in range(L)] + [2 + rng.randrange(p - 2)]
    Cc = [0] + [rng.randrange(p) for _ in range(L - 1)] + [1]
    init = lambda: [rng.randrange(p) for _ in range(L)]
    return [(Ca, init()), (Cb, init()), (Ca, [0] * L), (Cc, init()), (Ca, [p - 1] * L), (Ca, init())]


def terms_and_check(F, field, t, rows, K, nout, cache, device=False):
    p, count = P[field], len(rows)
    cp = from_ints(F, field, [c for C, _ in rows for c in C])
    init = from_ints(F, field, [x for _, s in rows for x in s])
    if device:
        import torch
        out = t.seq_nth_term(torch.from_numpy(cp).cuda(), torch.from_numpy(init).cuda(), K, nout=nout, count=count)
        assert out.is_cuda
        out = out.cpu().numpy()
    else:
        out = t.seq_nth_term(cp, init, K, nout=nout, count=count)
    assert out.shape[0] == count * nout
    want = []
    for C, s in rows:
        key = (tuple(C), K)
        if key not in cache:
            cache[key] = Q.power_of_x(p, C, K)
        want += Q.nth_terms(p, C, s, K, nout, u=cache[key])
    assert np.array_equal(to_std(F, out), G.arr(field, want, len(want))), (K, nout)


def indices(p, L, nc):
    ks = [0, 1, L - 1, L, 2 * L + 1, 10**6 + 3, 2**64 + 5]
    return ks + [p - 2] if nc <= 17 else ks


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nc", [2, 3, 17, 65])
def test_nth_term_small(oracle_mod, field, nc):
    """six rows per call on a tree of four leaves, every index with nout = 1 and 5; nout = L once (nc = 65); device tensors once"""
    p, L, rng = P[field], nc - 1, random.Random(nc)
    F, t = oracle_mod.field(field), tree(field, 4)
    rows, cache = term_rows(p, rng, L), {}
    for K in indices(p, L, nc):
        for nout in (1, 5):
            terms_and_check(F, field, t, rows, K, nout, cache)
    for (C, s) in rows[:2]:                                          # an index below L returns the initial terms themselves
        assert Q.nth_terms(p, C, s, 0, L) == [x % p for x in s]
    terms_and_check(F, field, t, rows, 3, L, cache)
    terms_and_check(F, field, t, rows, 10**6 + 3, 5, cache, device=True)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nc,leaves", [(66, 256), (130, 512)])
def test_nth_term_large(oracle_mod, field, nc, leaves):
    p, L, rng = P[field], nc - 1, random.Random(nc)
    F, t = oracle_mod.field(field), tree(field, leaves)
    rows, cache = term_rows(p, rng, L), {}
    for K in indices(p, L, nc):
        for nout in (1, 5):
            terms_and_check(F, field, t, rows, K, nout, cache)
    if nc == 66:
        terms_and_check(F, field, t, rows, 3, L, cache)
        terms_and_check(F, field, t, rows, 10**6 + 3, 5, cache, device=True)
    cp = from_ints(F, field, [c for C, _ in rows for c in C])
    init = from_ints(F, field, [x for _, s in rows for x in s])
    with pytest.raises(ValueError, match="too small"):              # one size below next_pow2(2 (nc - 1) - 1)
        tree(field, leaves // 2).seq_nth_term(cp, init, 5, count=len(rows))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nc,leaves", [(4, 4), (66, 256)])
def test_nth_term_zero_leading_coefficient(oracle_mod, field, nc, leaves):
    """found on the device, in one row of three; the context keeps working"""
    p, L, rng = P[field], nc - 1, random.Random(3)
    F, t = oracle_mod.field(field), tree(field, leaves)
    rows = term_rows(p, rng, L)[:3]
    bad = [(C, s) for C, s in rows]
    bad[1] = (bad[1][0][:L] + [0], bad[1][1])
    with pytest.raises(ValueError):
        t.seq_nth_term(from_ints(F, field, [c for C, _ in bad for c in C]), from_ints(F, field, [x for _, s in bad for x in s]), 9, count=3)
    terms_and_check(F, field, t, rows, 9, 2, {})


# ---- both together ----

@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("L,leaves", [(8, 4), (40, 4), (129, 1024)])
def test_round_trip(oracle_mod, field, L, leaves):
    """C = prod (x - a_i) over distinct non-zero a_i and s_j = sum a_i^j (every weight 1, so C is minimal): the 2 L terms from
    seq_nth_term(C, init, 0, nout = 2 L) go through seq_min_poly and come back as C.  L = 129: both large regimes."""
    import rs_ref as S
    p, rng = P[field], random.Random(L)
    F, t = oracle_mod.field(field), tree(field, leaves)
    count, n = 3, 2 * L
    Cs, inits = [], []
    for _ in range(count):
        roots = set()
        while len(roots) < L:
            roots.add(1 + rng.randrange(p - 1))
        roots = sorted(roots)
        Cs.append(S.from_roots(p, roots))
        pw, init = [1] * L, []
        for _ in range(L):
            init.append(sum(pw) % p)
            pw = [a * b % p for a, b in zip(pw, roots)]
        inits.append(init)
    cp = from_ints(F, field, [c for C in Cs for c in C])
    terms = t.seq_nth_term(cp, from_ints(F, field, [x for s in inits for x in s]), 0, nout=n, count=count)
    mp, orders = t.seq_min_poly(terms, count=count)
    assert list(orders) == [L] * count
    mp = to_std(F, mp)
    for i, C in enumerate(Cs):
        assert np.array_equal(mp[i * (L + 1):(i + 1) * (L + 1)], G.arr(field, C, L + 1)), i


def test_abi_errors(oracle_mod):
    from ecfft_amd import fftree as FT
    assert FT.SEQ_SMALL_MAX == 255 and FT.SEQ_TERM_SMALL_MAX == 65
    field = "m31"
    F, t = oracle_mod.field(field), tree(field, 4)
    L_, h, bad = t._L, t._h, FT.ERR_BAD_ARG
    seq = from_ints(F, field, [1, 2, 4, 8])
    mp, orders, out = np.zeros(3, F.dtype), np.zeros(1, np.int64), np.zeros(2, F.dtype)
    ps, pm, po, pout = seq.ctypes.data, mp.ctypes.data, orders.ctypes.data, out.ctypes.data
    assert L_.ecfft_seq_min_poly(h, ps, 4, pm, None, 1, FT.MEM_HOST, None) == bad         # orders is required
    assert L_.ecfft_seq_min_poly(h, None, 4, pm, po, 1, FT.MEM_HOST, None) == bad
    assert L_.ecfft_seq_min_poly(h, ps, 4, None, po, 1, FT.MEM_HOST, None) == bad
    assert L_.ecfft_seq_min_poly(h, ps, 0, pm, po, 1, FT.MEM_HOST, None) == bad
    assert L_.ecfft_seq_min_poly(h, ps, 4, pm, po, 0, FT.MEM_HOST, None) == bad
    assert L_.ecfft_seq_min_poly(None, ps, 4, pm, po, 1, FT.MEM_HOST, None) == bad
    cp, init, idx = from_ints(F, field, [P[field] - 2, 1]), from_ints(F, field, [1]), ctypes.c_char_p(b"\x03")
    pc, pi = cp.ctypes.data, init.ctypes.data
    assert L_.ecfft_seq_nth_term(h, pc, 1, pi, idx, 1, pout, 2, 1, FT.MEM_HOST, None) == bad    # nc = 1
    assert L_.ecfft_seq_nth_term(h, pc, 2, pi, idx, 1, pout, 2, 0, FT.MEM_HOST, None) == bad    # count = 0
    assert L_.ecfft_seq_nth_term(h, pc, 2, pi, idx, 1, pout, 0, 1, FT.MEM_HOST, None) == bad    # nout = 0
    assert L_.ecfft_seq_nth_term(h, pc, 2, pi, None, 1, pout, 2, 1, FT.MEM_HOST, None) == bad   # no index, but one byte of it
    assert L_.ecfft_seq_nth_term(h, pc, 2, None, idx, 1, pout, 2, 1, FT.MEM_HOST, None) == bad
    assert L_.ecfft_seq_nth_term(h, pc, 2, pi, idx, 1, None, 2, 1, FT.MEM_HOST, None) == bad
    with pytest.raises(ValueError):
        t.seq_nth_term(cp, init, -1)
    # after all of them the context works: 2^3, 2^4, then index NULL with no bytes (K = 0), then the order of 1, 2, 4, 8
    assert L_.ecfft_seq_nth_term(h, pc, 2, pi, idx, 1, pout, 2, 1, FT.MEM_HOST, None) == FT.OK
    assert R.to_ints(field, to_std(F, out)) == [8, 16]
    assert L_.ecfft_seq_nth_term(h, pc, 2, pi, None, 0, pout, 2, 1, FT.MEM_HOST, None) == FT.OK
    assert R.to_ints(field, to_std(F, out)) == [1, 2]
    assert L_.ecfft_seq_min_poly(h, ps, 4, pm, po, 1, FT.MEM_HOST, None) == FT.OK
    assert orders[0] == 1 and R.to_ints(field, to_std(F, mp)) == [P[field] - 2, 1, 0]
