"""GPU tests of ecfft_poly_squarefree and ecfft_poly_distinct_degree: k_ddf_small (a polynomial of at most DDF_SMALL_MAX
coefficients finished by one workgroup, all rows in one launch, on any tree) and the large regime (the squarefree part on gcd_pair
and the division body, x^p on the kept modulus, then per degree a gcd, a division and a Frobenius iterate, taken either as a kept
composition or as a fresh power; the hooks build forces each of the two).  Every comparison is an equality of bytes or ints through
the oracle's standard-form converters.  The expected outputs are known by CONSTRUCTION: f = k prod (x - r)^m prod (x^n - a)^m with
the binomials irreducible by tests/ddf_ref.binomial_irreducible, so g_d is the product of the distinct factors of degree d; where the
exact model tests/ddf_ref.ddf can afford it (small regime, factors of degree <= 9) it must agree as well.  The reference's own
distinct_degree_factors cannot serve: it takes x^(p i) for x^(p^i) (src/utils.rs:63).

Time on one MI355X: a fresh power of secp256k1 is 504 modular products, about a quarter of a second per iterate at these degrees,
so the three cases the issue sets with 40 and 62 iterates (irr81, two63, irr126) take 10 to 16 s there with both methods forced;
every other case keeps its factors at degree <= 9 and takes a few seconds at the most, the M31 cases and the small regime well
below one."""
import ctypes

import numpy as np
import pytest

import ddf_ref as D
import poly_ref as R
from conftest import std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P

_trees = {}
_binomials = {}


def small_max():
    from ecfft_amd import fftree as FT
    return FT.DDF_SMALL_MAX


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


def mem_rows(F, field, rows, nf):
    """int-list rows, each zero-padded to nf coefficients, laid end to end in the crate's form"""
    flat = []
    for r in rows:
        assert len(r) <= nf
        flat += [v % P[field] for v in r] + [0] * (nf - len(r))
    return std_to_field(F, R.from_ints(field, flat))


def ib(field, n, count):
    """the first `count` irreducible binomials x^n - a, a >= 2"""
    key = (field, n)
    if len(_binomials.get(key, [])) < count:
        _binomials[key] = D.irreducible_binomials(n, count, P[field])
    return _binomials[key][:count]


def lin(field, count, seed=0):
    """`count` distinct linear factors x - r, r spread over the field and never 0"""
    p = P[field]
    a = 0x9E3779B1 if field == "m31" else 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95
    return [[-((a * (i + 1) + 1000 * seed + 1) % p) % p, 1] for i in range(count)]


def make(field, parts, k=3):
    """(f, want): f = k prod q^m over parts = [(q, m), ...] with DISTINCT monic irreducible q; want = {d: the product of the q of degree d}"""
    p = P[field]
    f = D.product([q for q, m in parts for _ in range(m)], p)
    want = {}
    for q, m in parts:
        want.setdefault(len(q) - 1, []).append(q)
    return [v * k % p for v in f], {d: D.product(qs, p) for d, qs in want.items()}


def check(F, field, t, rows, wants, nf=None):
    """poly_distinct_degree and poly_squarefree of the rows (int lists; wants: {d: g_d}, None for a zero row) in ONE call each"""
    p, count = P[field], len(rows)
    nf = nf or max(len(r) for r in rows)
    nd = max(nf - 1, 1)
    fm = mem_rows(F, field, rows, nf)
    fac, deg = t.poly_distinct_degree(fm, count=count)
    assert fac.shape[0] == count * nd and deg.dtype == np.int64 and deg.shape == (count, nd)
    got = R.to_ints(field, to_std(F, fac))
    sq, sdeg = t.poly_squarefree(fm, count=count)
    assert sq.shape[0] == count * nf and sdeg.dtype == np.int64 and sdeg.shape == (count,)
    gsq = R.to_ints(field, to_std(F, sq))
    for b, want in enumerate(wants):
        row, degrees = D.pack(want, nd)
        assert deg[b].tolist() == degrees, (b, deg[b].tolist(), degrees)
        assert got[b * nd:(b + 1) * nd] == row, b
        s = None if want is None else D.product([want[d] for d in sorted(want)], p)
        assert sdeg[b] == (-1 if s is None else len(s) - 1), b
        assert gsq[b * nf:(b + 1) * nf] == ([] if s is None else s) + [0] * (nf - (0 if s is None else len(s))), b
    return fac, deg, sq, sdeg


def model_agrees(field, f, want):
    assert D.ddf(f, P[field]) == want


# ---- the small regime: one workgroup per polynomial, a 4-leaf tree ------------------------------------------------------------------
def mix(field, deg, seed=1):
    """degree exactly deg: linear factors with multiplicities 1, 2, 3, ..., (x^2 - a) and (x^3 - b)^2 where they fit"""
    parts, left = [], deg
    if left >= 12:
        parts += [(ib(field, 3, 1)[0], 2), (ib(field, 2, 1)[0], 1)]
        left -= 8
    ls, i = lin(field, 64, seed), 0
    while left:
        m = min(1 + i % 3, left)
        parts.append((ls[i], m))
        left -= m
        i += 1
    return make(field, parts, k=5 + seed)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("deg", [1, 2, 3, 63, 64])
def test_small_mixed_factors_alone_and_three_rows_in_one_launch(oracle_mod, field, deg):
    F, t = oracle_mod.field(field), tree(field, 4)
    f, want = mix(field, deg)
    assert len(f) == deg + 1
    one = check(F, field, t, [f], [want])
    model_agrees(field, f, want)
    f2, want2 = mix(field, max(deg - 1, 1), seed=2)
    f3, want3 = make(field, [(q, 1) for q in lin(field, deg, 3)])            # deg distinct linear factors: h_1 = x
    three = check(F, field, t, [f2, f, f3], [want2, want, want3], nf=deg + 1)
    nd = max(deg, 1)
    assert np.array_equal(three[0][nd:2 * nd], one[0]) and np.array_equal(three[1][1], one[1][0])


@pytest.mark.parametrize("field", FIELDS)
def test_small_64_distinct_linear_factors_and_the_root_zero(oracle_mod, field):
    F, t = oracle_mod.field(field), tree(field, 4)
    f, want = make(field, [(q, 1) for q in lin(field, 64)])
    check(F, field, t, [f], [want])
    x = [0, 1]
    for parts in ([(x, 1)], [(x, 3), (ib(field, 2, 1)[0], 1)], [(x, 2)] + [(q, 1) for q in lin(field, 5)] + [(ib(field, 3, 1)[0], 1)]):
        f, want = make(field, parts)
        check(F, field, t, [f], [want])
        model_agrees(field, f, want)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [2, 7, 21])
def test_small_boundary_two_factors_of_half_the_degree(oracle_mod, field, n):
    """deg f* = 2i exactly: (x^n - a1)(x^n - a2) must come out as g_n of degree 2n, not as one factor of degree 2n; alone and next
    to lower factors"""
    F, t = oracle_mod.field(field), tree(field, 4)
    a, b = ib(field, n, 2)
    f, want = make(field, [(a, 1), (b, 1)])
    assert sorted(want) == [n] and len(want[n]) == 2 * n + 1
    check(F, field, t, [f], [want])
    lower = [(lin(field, 1)[0], 2)] + ([(ib(field, 2, 3)[2], 1)] if n > 2 else [])
    g, wg = make(field, [(a, 1), (b, 2 if n <= 7 else 1)] + lower)                # at most 64 in all
    check(F, field, t, [g, f], [wg, want])
    if n <= 7:
        model_agrees(field, f, want)
        model_agrees(field, g, wg)


@pytest.mark.parametrize("field", FIELDS)
def test_small_remainder_irreducible_by_the_exit_rule_and_the_longest_loop(oracle_mod, field):
    """(x^21 - a)(x^42 - b): after g_21 the rest has degree 42 < 2 * 22 and is irreducible of its own degree; x^63 - a alone, and
    times (x - r): all 31 iterates at degree 64"""
    F, t = oracle_mod.field(field), tree(field, 4)
    f, want = make(field, [(ib(field, 21, 1)[0], 1), (ib(field, 42, 1)[0], 1)])
    assert sorted(want) == [21, 42]
    check(F, field, t, [f], [want])
    q = ib(field, 63, 1)[0]
    f, want = make(field, [(q, 1)])
    g, wg = make(field, [(q, 1), (lin(field, 1)[0], 1)])
    assert len(g) == 65 and sorted(wg) == [1, 63]
    check(F, field, t, [f], [want])
    check(F, field, t, [g, f], [wg, want])


@pytest.mark.parametrize("field", FIELDS)
def test_small_zero_constant_and_untrimmed_rows_in_one_call(oracle_mod, field):
    F, t = oracle_mod.field(field), tree(field, 4)
    f, want = mix(field, 20)
    for nf in (small_max(), 30, 22):
        check(F, field, t, [[0], [12345], f + [0]], [None, {}, want], nf=nf)
    fac, deg = t.poly_distinct_degree(mem_rows(F, field, [[0], [7], [0]], 1), count=3)      # nf = 1: one entry per row all the same
    assert deg.tolist() == [[-1], [0], [-1]] and not np.ascontiguousarray(fac).view(np.uint8).any()
    sq, sdeg = t.poly_squarefree(mem_rows(F, field, [[0], [7]], 1), count=2)
    assert sdeg.tolist() == [-1, 0] and R.to_ints(field, to_std(F, sq)) == [0, 1]


@pytest.mark.parametrize("field", FIELDS)
def test_squarefree_of_a_square_and_of_a_squarefree_input(oracle_mod, field):
    F, t, p = oracle_mod.field(field), tree(field, 4), P[field]
    g, want = make(field, [(q, 1) for q in lin(field, 9)] + [(ib(field, 7, 1)[0], 1), (ib(field, 9, 1)[0], 1)], k=1)
    assert len(g) - 1 == 25
    sq = check(F, field, t, [D.product([g, g], p), g], [want, want])[2]
    assert R.to_ints(field, to_std(F, sq))[:51] == g + [0] * 25
    assert D.squarefree_part(D.product([g, g], p), p) == g


# ---- the large regime: both iterate methods, both fields, a 4096-leaf tree --------------------------------------------------------------
def pattern(field, name):
    """(rows, wants, nf) of a large-regime case"""
    l = lambda n, seed=0: [(q, 1) for q in lin(field, n, seed)]
    b = lambda n, k=1: ib(field, n, k)
    cases = {
        # mixed factor patterns that sum exactly to d, factors of degree <= 9 (a fresh power of secp256k1 is 504 products per iterate);
        # multiplicities make the squarefree part a gcd_pair and a division; the last factor of mix65 and mix129 is what the exit
        # rule leaves
        "mix65": [l(26) + [(b(2)[0], 2), (b(3)[0], 1), (b(7)[0], 2), (b(9)[0], 1), (b(6)[0], 1), (lin(field, 1, 5)[0], 3)]],
        "mix66": [l(42) + [(b(2)[0], 1), (b(2, 2)[1], 1), (b(6)[0], 1), (b(7)[0], 1), (b(7, 2)[1], 1)]],      # ends at deg f* = 2i
        "mix128": [l(90) + [(b(3)[0], 1), (b(3, 2)[1], 1), (b(7)[0], 2), (b(9)[0], 2)]],
        "mix129": [l(100) + [(b(2)[0], 3), (b(7)[0], 1), (b(7, 2)[1], 1), (b(9)[0], 1)]],
        "mix130": [l(97) + [(b(2)[0], 3), (b(7)[0], 1), (b(7, 2)[1], 1), (b(6)[0], 1), (b(7, 3)[2], 1)]],
        "lin130": [l(130)],
        "two63": [[(b(63, 2)[0], 1), (b(63, 2)[1], 1)]],                     # 62 iterates, then g_63 of degree 126
        "irr126": [[(b(126)[0], 1)]],                                        # every gcd trivial
        "irr81": [[(b(81)[0], 1)]],
        "square": [l(35) + [(b(9)[0], 1), (b(21)[0], 1)]],                   # squared below: f = g^2, deg 130, deg s = 65
        "short": [l(4) + [(b(2)[0], 2), (b(9)[0], 1)]],                      # true length 18 inside nf = 130
        "sqshort": [l(20, 2) + [(b(3)[0], 3), (b(21)[0], 3)]],               # deg 92, deg s = 44: the workgroup kernel on s
        "two": [l(122) + [(b(2)[0], 1), (b(3)[0], 1), (b(2, 2)[1], 1)], l(100, 3) + [(b(9)[0], 2), (b(9, 2)[1], 1)]],
        "m200": [l(90) + [(b(2)[0], 1), (b(9)[0], 2), (b(27)[0], 1), (b(63)[0], 1)]],
        "m300": [l(120) + [(b(81)[0], 1), (b(42)[0], 1), (b(18)[0], 1), (b(21)[0], 1), (b(9)[0], 2)]],
    }
    rows, wants = [], []
    for parts in cases[name]:
        if name == "square":
            parts = [(q, 2) for q, m in parts]
        f, want = make(field, parts)
        rows.append(f)
        wants.append(want)
    degs = {"mix65": 65, "mix66": 66, "mix128": 128, "mix129": 129, "mix130": 130, "lin130": 130, "two63": 126, "irr126": 126,
            "irr81": 81, "square": 130, "short": 17, "sqshort": 92, "two": 129, "m200": 200, "m300": 300}
    assert len(rows[0]) - 1 == degs[name], (name, len(rows[0]) - 1)
    nf = 130 if name == "short" else max(len(r) for r in rows)
    return rows, wants, nf


LARGE = [(f, n) for f in FIELDS for n in ("mix65", "mix66", "mix128", "mix129", "mix130", "lin130", "two63", "irr126", "irr81", "square",
                                          "short", "sqshort", "two")] + [("m31", "m200"), ("m31", "m300")]


@pytest.mark.parametrize("field,name", LARGE)
def test_large_regime_with_both_iterate_methods(oracle_mod, hooks_lib, field, name):
    """the kept composition (1) and the fresh power (2), forced by ecfft_test_ddf_iterate: the constructed factors, and the same bytes"""
    import ecfft_amd
    F = oracle_mod.field(field)
    rows, wants, nf = pattern(field, name)
    t = ecfft_amd.FIELDS[field].build_fftree(4096)
    outs = []
    try:
        for mode in (1, 2):
            assert hooks_lib.ecfft_test_ddf_iterate(mode) == 0
            outs.append(check(F, field, t, rows, wants, nf=nf))
    finally:
        assert hooks_lib.ecfft_test_ddf_iterate(0) == 0
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and np.array_equal(outs[0][1], outs[1][1])
    assert hooks_lib.ecfft_test_ddf_iterate(3) != 0


@pytest.mark.parametrize("field", FIELDS)
def test_large_regime_shipped_rule_device_memory_and_gpu_against_gpu(oracle_mod, field):
    """the shipped library (the rule picks the method) on host and on device memory; the roots of g_1 are the roots of f, and the
    product of the g_d is the squarefree part"""
    import torch
    F, t, p = oracle_mod.field(field), tree(field, 4096), P[field]
    rows, wants, nf = pattern(field, "two")
    fac, deg, sq, sdeg = check(F, field, t, rows, wants, nf=nf)
    fm = mem_rows(F, field, rows, nf)
    as_int = lambda a: a.view(np.int64) if field == "secp256k1" else a.view(np.int32)
    dfac, ddeg = t.poly_distinct_degree(torch.from_numpy(as_int(fm)).cuda(), count=2)
    assert np.array_equal(ddeg, deg) and np.array_equal(dfac.cpu().numpy().view(fac.dtype).reshape(fac.shape), fac)
    dsq, dsdeg = t.poly_squarefree(torch.from_numpy(as_int(fm)).cuda(), count=2)
    assert np.array_equal(dsdeg, sdeg) and np.array_equal(dsq.cpu().numpy().view(sq.dtype).reshape(sq.shape), sq)
    nd = nf - 1
    for b in range(2):
        gs = t.ddf_unpack(fac[b * nd:(b + 1) * nd], deg[b])
        assert sorted(gs) == sorted(wants[b])
        r1, n1 = t.poly_find_roots(np.ascontiguousarray(gs[1]))
        rf, nf_ = t.poly_find_roots(np.ascontiguousarray(fm[b * nf:(b + 1) * nf]))
        assert n1[0] == nf_[0] == deg[b][0] and np.array_equal(r1[:n1[0]], rf[:n1[0]])
        prod = None
        for d in sorted(gs):
            prod = gs[d] if prod is None else t.poly_mul(np.ascontiguousarray(prod), np.ascontiguousarray(gs[d]))
        assert np.array_equal(to_std(F, prod), to_std(F, sq[b * nf:b * nf + sdeg[b] + 1]))


# ---- errors and the tree rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_errors_and_the_tree_rule(oracle_mod, field):
    from ecfft_amd import fftree as FT
    F, t = oracle_mod.field(field), tree(field, 4)
    L = FT.lib()
    f65, want = make(field, [(q, 1) for q in lin(field, 60)] + [(ib(field, 2, 1)[0], 2)])
    assert len(f65) == 65 == small_max()
    check(F, field, t, [f65], [want])                                         # nf = 65 works on the 4-leaf tree
    fm = mem_rows(F, field, [f65], 66)
    out = np.zeros_like(fm)
    deg = np.zeros(65, np.int64)
    n = np.zeros(1, np.int64)
    want_rc = L.ecfft_poly_find_roots(t._h, fm.ctypes.data, 66, out.ctypes.data, n.ctypes.data, 1, FT.MEM_HOST, None)
    assert want_rc == FT.ERR_TREE_TOO_SMALL
    for fn in (L.ecfft_poly_distinct_degree, L.ecfft_poly_squarefree):
        assert fn(t._h, fm.ctypes.data, 66, out.ctypes.data, deg.ctypes.data, 1, FT.MEM_HOST, None) == want_rc
        assert fn(t._h, fm.ctypes.data, 0, out.ctypes.data, deg.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert fn(t._h, fm.ctypes.data, 65, out.ctypes.data, deg.ctypes.data, 0, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert fn(t._h, None, 65, out.ctypes.data, deg.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert fn(t._h, fm.ctypes.data, 65, None, deg.ctypes.data, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert fn(t._h, fm.ctypes.data, 65, out.ctypes.data, None, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
        assert fn(t._h, fm.ctypes.data, 65, out.ctypes.data, deg.ctypes.data, 1, 7, None) == FT.ERR_BAD_ARG
    with pytest.raises(ValueError):
        t.poly_distinct_degree(fm)
    with pytest.raises(ValueError):
        t.poly_squarefree(fm)
