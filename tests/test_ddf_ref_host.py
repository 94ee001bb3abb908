"""CPU tests of tests/ddf_ref.py, the exact model that tests/test_gpu_polyddf.py compares ecfft_poly_squarefree and
ecfft_poly_distinct_degree with: against brute-force trial division by every monic irreducible at primes small enough to list
them, the binomial criterion against the model in both real fields, and the packing of the C ABI's two output rows."""
import itertools
import random

import pytest

import ddf_ref as D
import gcd_ref as G
import poly_ref as R

P = R.P


def monic_polys(p, deg):
    for low in itertools.product(range(p), repeat=deg):
        yield list(low) + [1]


def divides(g, f, p):
    """the monic g divides f: long division on plain lists (the primes here are tiny; independent of gcd_ref.divmod_school)"""
    r, ng = list(f), len(g)
    for i in range(len(r) - ng, -1, -1):
        c = r[i + ng - 1]
        if c:
            for j in range(ng):
                r[i + j] = (r[i + j] - c * g[j]) % p
    return not any(r[:ng - 1])


def irreducibles(p, maxdeg):
    """{d: [monic irreducibles of degree d]} by a sieve of trial divisions"""
    out = {}
    for d in range(1, maxdeg + 1):
        out[d] = [f for f in monic_polys(p, d) if not any(divides(g, f, p) for e in range(1, d // 2 + 1) for g in out[e])]
    return out


def brute(f, p, irr):
    """(squarefree part, {d: g_d}) of a non-constant f by trial division"""
    f = G.trim(f)
    sq, fac = [1], {}
    for d in sorted(irr):
        for g in irr[d]:
            if len(g) <= len(f) and divides(g, f, p):
                sq = D.product([sq, g], p)
                fac[d] = D.product([fac.get(d, [1]), g], p)
    return sq, fac


@pytest.mark.parametrize("p", [5, 7])
def test_model_against_trial_division_for_every_polynomial_of_degree_at_most_4(p):
    irr = irreducibles(p, 4)
    assert [len(irr[d]) for d in (1, 2, 3)] == [p, (p * p - p) // 2, (p ** 3 - p) // 3]
    n = 0
    for deg in range(1, 5):
        for f in monic_polys(p, deg):
            sq, fac = brute(f, p, irr)
            assert D.squarefree_part(f, p) == sq, f
            assert D.ddf(f, p) == fac, f
            n += 1
    assert n == sum(p ** d for d in range(1, 5))
    lead = [3 * v % p for v in irr[2][0]]                     # a leading coefficient other than 1, and an untrimmed row
    assert D.ddf(lead + [0, 0], p) == {2: irr[2][0]} and D.squarefree_part(lead + [0], p) == irr[2][0]


def test_model_against_trial_division_for_a_sample_of_degree_at_most_6_over_f31():
    p = 31
    irr = irreducibles(p, 3)                                  # a factor of degree 4 .. 6 of a degree-6 polynomial is what is left
    rng = random.Random(7)
    for _ in range(100):
        deg = rng.randint(1, 6)
        f = [rng.randrange(p) for _ in range(deg)] + [1]
        sq, fac = brute(f, p, irr)
        rest = G.divmod_school(D.squarefree_part(f, p), sq, p)
        assert not rest[1]
        want = dict(fac)
        if len(rest[0]) > 1:                                  # no factor of degree <= 3: degree 4, 5 or 6 means irreducible
            assert len(rest[0]) - 1 >= 4
            want[len(rest[0]) - 1] = rest[0]
        assert D.ddf(f, p) == want, f
    for parts in ([irr[1][3]] * 3 + [irr[2][5]] * 2, [irr[3][10], irr[3][11]], [irr[2][0], irr[2][1], irr[1][0], irr[1][0]]):
        f = D.product(parts, p)
        sq, fac = brute(f, p, irr)
        assert D.squarefree_part(f, p) == sq and D.ddf(f, p) == fac


def test_degenerate_inputs():
    p = 31
    assert D.squarefree_part([0, 0], p) is None and D.ddf([0], p) is None
    assert D.squarefree_part([7, 0], p) == [1] and D.ddf([7], p) == {}
    assert D.ddf([3, 2], p) == {1: [3 * pow(2, p - 2, p) % p, 1]}
    with pytest.raises(AssertionError):
        D.squarefree_part([1] + [0] * 4 + [1], 5)             # degree p: the p-th-power case the model does not have


@pytest.mark.parametrize("field", ["secp256k1", "m31"])
def test_binomial_criterion_against_the_model(field):
    """x^n - a for n <= 21 and a few a: irreducible by the criterion iff the model returns the binomial itself as g_n"""
    p = P[field]
    assert p % 4 == 3
    seen = {True: 0, False: 0}
    for n in (2, 3, 4, 5, 6, 7, 9, 12, 14, 21):
        for a in (2, 3, 5, 6):
            f = D.binomial(n, a, p)
            irr = D.binomial_irreducible(n, a, p)
            assert (D.ddf(f, p) == {n: f}) == irr, (n, a)
            seen[irr] += 1
    assert seen[True] >= 6 and seen[False] >= 6
    for n in (2, 3, 7, 9, 21):                                # the degrees the GPU tests build on exist in both fields
        assert len(D.irreducible_binomials(n, 2, p)) == 2


def test_pack_and_unpack_round_trip():
    p = 31
    f = D.product([[1, 1], [2, 1], D.irreducible_binomials(2, 1, p)[0], D.irreducible_binomials(3, 1, p)[0]], p)
    fac = D.ddf(f, p)
    assert sorted(fac) == [1, 2, 3]
    row, deg = D.pack(fac, 9)
    assert deg == [2, 2, 3, 0, 0, 0, 0, 0, 0] and len(row) == 9 and row[7:] == [0, 0]
    assert row[:2] == fac[1][:2] and row[2:4] == fac[2][:2] and row[4:7] == fac[3][:3]
    assert D.unpack(row, deg) == fac
    assert D.pack(None, 3) == ([0, 0, 0], [-1, 0, 0]) and D.unpack([0, 0, 0], [-1, 0, 0]) is None
    assert D.pack({}, 1) == ([0], [0]) and D.unpack([0], [0]) == {}
