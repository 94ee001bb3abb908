"""CPU tests of tests/schoof_ref.py, the exact model behind tests/test_gpu_schoof.py: division polynomials against their defining
property, the trace modulo l and the CRT against known orders (the reference's own TODO value among them), N P = O, the
residues of secp256k1's published order, and the recorded residues of tests/golden/schoof_residues.json with the branches the
GPU inputs must reach: a split, the point at infinity, and a restart that ends on a modulus of degree 1."""
import json
import os
import random

import pytest

import schoof_ref as S

P31 = S.P["m31"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schoof_residues.json")

# (A, B): (#E, t mod 3, 5, 7, 11, 13, 17) over M31
TABLE = {
    (8, 81): (2147489041, [1, 2, 4, 8, 2, 13]),          # the value the reference's TODO expects (schoofs.rs:29)
    (1, 1): (2147423272, [1, 1, 1, 8, 4, 9]),
    (2, 3): (2147477024, [0, 4, 2, 2, 7, 11]),
    (5, 7): (2147430114, [2, 4, 5, 8, 0, 1]),
    (0, 7): (2147444533, [1, 0, 6, 10, 11, 15]),
    (11, 19): (2147429416, [1, 2, 3, 2, 9, 2]),
    (3, 0): (2147483648, [0] * 6),                       # supersingular: p = 3 mod 4
    (1, 0): (2147483648, [0] * 6),
}


def random_point(A, B, p, rng):
    while True:
        x = rng.randrange(p)
        y = S.sqrt_mod((x**3 + A * x + B) % p, p)
        if y:
            return x, y


def test_lengths_leading_coefficients_and_indices():
    assert [S.L(n) for n in range(8)] == [1, 1, 1, 5, 7, 13, 17, 25]
    assert S.L(11) == 61 and S.L(13) == 85 and S.L(17) == 145 and S.L(199) == 19801
    for n in (3, 4, 5, 6, 7, 8, 9, 12, 17, 24):
        v = S.divpoly(n, 8, 81, P31)
        assert len(v) == S.L(n) and v[-1] == (n if n & 1 else n // 2)
    assert S.divpoly(0, 8, 81, P31) == [] and S.divpoly(1, 8, 81, P31) == [1] and S.divpoly(2, 8, 81, P31) == [1]
    assert len(S.divpoly_indices(199)) <= 4 * 8 + 5                            # O(log n) indices, not the reference's recursion
    assert S.primes_for(P31) == [2, 3, 5, 7, 11, 13, 17]
    ps = S.primes_for(S.P["secp256k1"])
    assert ps[-1] == 103 and ps[:5] == [2, 3, 5, 7, 11]


@pytest.mark.parametrize("field", ["m31", "secp256k1"])
def test_division_polynomial_gives_the_x_of_n_times_a_point(field):
    """x(n P) = x - psi_(n-1) psi_(n+1) / psi_n^2 with the full psi (the factor 2y put back on even indices), at random points"""
    p = S.P[field]
    rng = random.Random(5)
    A, B = 8, 81
    ev = lambda f, x: sum(c * pow(x, i, p) for i, c in enumerate(f)) % p
    for _ in range(3):
        x, y = random_point(A, B, p, rng)
        full = lambda n: ev(S.divpoly(n, A, B, p), x) * (2 * y if n % 2 == 0 else 1) % p
        for n in range(2, 10):
            Q = S.ec_mul(n, (x, y), A, p)
            den = full(n)
            if Q is None:
                assert den == 0
                continue
            assert Q[0] == (x - full(n - 1) * full(n + 1) * pow(den * den, -1, p)) % p


@pytest.mark.parametrize("curve", sorted(TABLE))
def test_m31_table(curve):
    A, B = curve
    N, tr = TABLE[curve]
    n, t = S.cardinality(A, B, P31)
    assert n == N and t[1:] == tr and t[0] == (P31 + 1 - N) % 2
    rng = random.Random(A * 100 + B)
    for _ in range(3):
        assert S.ec_mul(N, random_point(A, B, P31, rng), A, P31) is None        # N P = O


def test_singular_curve_and_the_crt():
    assert S.trace_mod(-3, 2, 5, P31) == -1 and S.cardinality(-3, 2, P31) == (0, [])
    primes = S.primes_for(P31)
    for t in (0, 1, -1, 92681, -92681, 5404):
        assert S.crt([t % l for l in primes], primes) == t


def test_find_curve_form_maps_to_short_weierstrass():
    """y^2 = x (x^2 + a x + bb) and its image under x -> x - a/3 have the same points"""
    rng = random.Random(9)
    a, bb = 12345, 678
    A, B = S.from_find_curve(a, bb, P31)
    i3 = pow(3, -1, P31)
    for _ in range(8):
        x = rng.randrange(P31)
        u = (x + a * i3) % P31
        assert (x * (x * x + a * x + bb)) % P31 == (u**3 + A * u + B) % P31


def test_recorded_residues_and_the_branches_the_gpu_inputs_reach():
    """every entry of the golden file recomputed; over these inputs the model splits, meets the point at infinity, and restarts
    down to a modulus of degree 1; (0, 7) over secp256k1 agrees with the published order"""
    with open(GOLDEN) as f:
        gold = json.load(f)
    total = [0, 0, 0]
    for field, rows in gold.items():
        p = S.P[field]
        assert len(rows) == 8
        for r in rows:
            for l in (2, 3, 5, 7, 11):
                st = S.new_stats()
                assert S.trace_mod(r["A"], r["B"], l, p, st) == r["t"][str(l)], (field, r["A"], r["B"], l)
                got = [st["splits"], st["infinity"], st["deg1"]]
                assert got == r["splits_infinity_deg1"][str(l)]
                assert all(d <= S.SMALL_MAX - 1 for d in st["degrees"])
                total = [a + b for a, b in zip(total, got)]
                if st["deg1"]:
                    assert st["degrees"][-1] == 1 and st["splits"] >= 1          # the restart ended on degree 1
    assert total == [13, 14, 7]                                                # pinned: splits, infinity branches, degree-1 attempts
    tr = S.P["secp256k1"] + 1 - S.SECP256K1_ORDER
    k1 = gold["secp256k1"][0]
    assert (k1["A"], k1["B"]) == (0, 7) and [k1["t"][str(l)] for l in (3, 5, 7, 11)] == [tr % l for l in (3, 5, 7, 11)] == [1, 2, 6, 5]


@pytest.mark.parametrize("field", ["m31", "secp256k1"])
def test_field_short_weierstrass_is_the_models_map(field):
    """Field.short_weierstrass (host only) against from_find_curve, through Field.from_ints / to_ints"""
    import ecfft_amd
    ecfft_amd.build.build()
    fld, p = ecfft_amd.FIELDS[field], S.P[field]
    rng = random.Random(3)
    a, bb = [rng.randrange(p) for _ in range(5)] + [0, 3], [rng.randrange(p) for _ in range(5)] + [1, 0]
    assert fld.to_ints(fld.from_ints(a)) == a
    A, B = fld.short_weierstrass(fld.from_ints(a), fld.from_ints(bb))
    assert list(zip(fld.to_ints(A), fld.to_ints(B))) == [S.from_find_curve(x, y, p) for x, y in zip(a, bb)]


def test_the_large_regime_split_the_gpu_test_uses():
    """M31, (1, 4), l = 13: psi_13 (degree 84) splits once and the restart runs on a factor of degree 6, which the small kernel
    takes; the residue is 12.  (8, 81) never splits at l = 13."""
    st = S.new_stats()
    assert S.trace_mod(1, 4, 13, P31, st) == 12 and st["splits"] == 1 and st["degrees"] == [84, 6]
    st = S.new_stats()
    assert S.trace_mod(8, 81, 13, P31, st) == 2 and st["splits"] == 0
