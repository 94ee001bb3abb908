"""CPU tests of tests/edf_ref.py, the exact model that tests/test_gpu_polyedf.py compares ecfft_poly_equal_degree with: against
trial division by every monic irreducible at primes small enough to list them, the norm identity N_c mod f_j = (-1)^d f_j(-c) in
both real fields, the condition that keeps the GPU tests' inputs away from the attempt cap, and the C ABI's surface.

At p = 5 and 7 there are only p shifts, so some pairs of irreducibles get the same character at every shift and cannot be
separated (the Weil bound says nothing at such p).  The shifts repeat with period p < 64, so the model must then run into the cap,
and only then; the test computes which inputs these are from the characters of f_j(-c) alone and asserts exactly that."""
import itertools
import os
import random

import numpy as np
import pytest

import ddf_ref as D
import edf_ref as E
import gcd_ref as G
import poly_ref as R
import roots_ref as RR

P = R.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def monic_polys(p, deg):
    for low in itertools.product(range(p), repeat=deg):
        yield list(low) + [1]


def divides(g, f, p):
    """the monic g divides f: long division on plain lists (independent of gcd_ref.divmod_school)"""
    r, ng = list(f), len(g)
    for i in range(len(r) - ng, -1, -1):
        c = r[i + ng - 1]
        if c:
            for j in range(ng):
                r[i + j] = (r[i + j] - c * g[j]) % p
    return not any(r[:ng - 1])


def irreducibles(p, maxdeg):
    out = {}
    for d in range(1, maxdeg + 1):
        out[d] = [f for f in monic_polys(p, d) if not any(divides(g, f, p) for e in range(1, d // 2 + 1) for g in out[e])]
    return out


def eval_at(f, x, p):
    v = 0
    for c in reversed(f):
        v = (v * x + c) % p
    return v


def plus_one(q, c, p):
    """the splitting element is +1 modulo q at the shift c: the norm (-1)^d q(-c) is a non-zero square"""
    d = len(q) - 1
    return pow((-1) ** d * eval_at(q, -c % p, p) % p, (p - 1) // 2, p) == 1


def separable(qs, p):
    """every pair of the factors is told apart by some shift"""
    sig = [tuple(plus_one(q, c, p) for c in range(p)) for q in qs]
    return len(set(sig)) == len(sig)


def check_subset(qs, d, p, irr_d, k=1):
    g = [v * k % p for v in D.product(qs, p)]
    want = sorted(q for q in irr_d if divides(q, g, p))               # trial division
    assert want == sorted(qs)
    if separable(qs, p):
        got, attempts, worst = E.equal_degree(g, d, p)
        assert got == want and worst < p
        return 1
    with pytest.raises(OverflowError):
        E.equal_degree(g, d, p)
    return 0


@pytest.mark.parametrize("p", [5, 7])
def test_model_against_trial_division_for_every_product_of_degree_at_most_6(p):
    """d = 1, 2, 3 and every r with r d <= 6; a product of degree 4 .. 6 with d above 3 is one irreducible and comes back as it is
    (test_degenerate_inputs_and_the_packing)"""
    irr = irreducibles(p, 3)
    done = split = 0
    for d in range(1, 4):
        for r in range(1, 6 // d + 1):
            for qs in itertools.combinations(irr[d], r):
                split += check_subset(list(qs), d, p, irr[d], k=1 + (done % (p - 1)))
                done += 1
    assert done == sum(len(list(itertools.combinations(irr[d], r))) for d in range(1, 4) for r in range(1, 6 // d + 1))
    assert split > done // 2                                          # most inputs split even at these primes


def test_model_against_trial_division_for_a_sample_of_degree_at_most_8_over_f31():
    p = 31
    irr = irreducibles(p, 3)
    rng = random.Random(11)
    n = 0
    for d, r in ((1, 8), (1, 2), (2, 4), (2, 3), (3, 2), (2, 2), (1, 5)):
        for _ in range(25):
            n += check_subset(rng.sample(irr[d], r), d, p, irr[d], k=rng.randrange(1, p))
    assert n >= 165


def test_degenerate_inputs_and_the_packing():
    p = 31
    assert E.equal_degree([0, 0], p=p, d=2) is None and E.equal_degree([7, 0], 3, p) == ([], 0, 0)
    assert E.equal_degree([1, 2, 3, 1], 2, p) == -2
    q = D.irreducible_binomials(3, 1, p)[0]
    assert E.equal_degree([5 * v % p for v in q] + [0], 3, p) == ([q], 0, 0)
    qs = sorted([[3, 1], [30, 1], [7, 1]])
    row, n = E.pack(qs, 5, 1)
    assert (row, n) == ([3, 7, 30, 0, 0], 3) and E.unpack(row, n, 1) == qs
    two = sorted([[5, 1, 1], [2, 30, 1]])
    assert E.pack(list(reversed(two)), 4, 2) == ([2, 30, 5, 1], 2) and E.unpack([2, 30, 5, 1], 2, 2) == two
    assert E.pack(None, 3, 2) == ([0, 0, 0], -1) and E.pack(-2, 3, 2) == ([0, 0, 0], -2) and E.pack([], 1, 4) == ([0], 0)
    assert E.shifted([1, 2, 3], 4, p) == [(1 + 2 * 4 + 3 * 16) % p, (2 + 3 * 8) % p, 3]


@pytest.mark.parametrize("field", ["secp256k1", "m31"])
@pytest.mark.parametrize("d", [2, 3, 7])
def test_norm_identity(field, d):
    """N_c mod f_j = (-1)^d f_j(-c), an element of F_p, for every factor of a product of three irreducibles and a few shifts"""
    p = P[field]
    g, qs = E.case(d, 3, p)
    g = RR.monic(g, p)
    hs = E.frobenius(g, d, p)
    assert hs[0] == [0, 1] and len(hs) == d
    for c in (1, 2, 17):
        nc = E.norm(hs, c, g, p)
        for q in qs:
            assert RR.rem(nc, q, p) == [(-1) ** d * eval_at(q, -c % p, p) % p]
        u, v = E.split(g, hs, g, c, p)                                # the splitting element is +1 exactly on the factors in u
        assert sorted(q for q in qs if plus_one(q, c, p)) == sorted(q for q in qs if divides(q, u, p))
        assert D.product([u, v], p) == g


# Every (field, d, r) that tests/test_gpu_polyedf.py passes to the GPU (tests/edf_ref.gpu_cases) and the model can afford here: all of
# M31, and of secp256k1 the single factors and those with d <= 9 and at most 71 coefficients.  What is left out, with the reason: secp256k1 (21, 3), (21, 4)
# and (63, 2) have d > 9 (20 to 62 Frobenius powers of 384 products each), and secp256k1 (3, 100) and (2, 160) are 301 and 321
# coefficients, where the model's schoolbook products make one Frobenius power alone some 40 times the 5 s that (3, 21) takes.
def affordable(field, d, r):
    return field == "m31" or r == 1 or (d <= 9 and d * r + 1 <= 71)      # one factor comes back as it is and costs nothing


AFFORDABLE = [(f, d, r) for f in ("m31", "secp256k1") for d, r in E.gpu_cases(f) if affordable(f, d, r)]


def test_the_affordable_cases_are_the_gpu_cases():
    assert len(E.gpu_cases("m31")) == 22 and len(E.gpu_cases("secp256k1")) == 22
    left_out = sorted(set((f, d, r) for f in ("m31", "secp256k1") for d, r in E.gpu_cases(f)) - set(AFFORDABLE))
    assert left_out == [("secp256k1", 2, 160), ("secp256k1", 3, 100), ("secp256k1", 21, 3), ("secp256k1", 21, 4), ("secp256k1", 63, 2)]


@pytest.mark.parametrize("field,d,r", AFFORDABLE)
def test_gpu_inputs_stay_away_from_the_cap(field, d, r):
    """a condition on the inputs, not a measurement: the model's longest run of consecutive failed shifts on one factor is <= 16,
    a quarter of the cap of 64"""
    p = P[field]
    g, want = E.case(d, r, p, k=5 if r == 1 else 3)
    got, attempts, worst = E.equal_degree(g, d, p)
    assert got == want and len(got) == r
    assert worst <= 16, (worst, attempts)
    if d <= 9:
        assert all(D.ddf(q, p) == {d: q} for q in want[:2])           # the shifted binomials are irreducible
    if (d, r) == E.GPU_MIXED_ROWS[3]:
        assert E.equal_degree(g, E.GPU_MIXED_ROWS[0][0], p) == -2     # the row the GPU test passes with a degree that does not divide


@pytest.mark.parametrize("field", ["secp256k1", "m31"])
def test_pipeline_inputs_stay_away_from_the_cap(field):
    """the g_d of test_pipeline_irreducible_factors: five linear factors, three x^2 - a, two x^3 - b"""
    p = P[field]
    for d, qs in ((1, E.irreducibles(1, 5, p)), (2, D.irreducible_binomials(2, 3, p)), (3, D.irreducible_binomials(3, 2, p))):
        got, attempts, worst = E.equal_degree(D.product(qs, p), d, p)
        assert got == sorted(qs) and worst <= 16


def test_symbol_is_exported_and_checks_its_arguments_without_a_gpu():
    import ecfft_amd
    from ecfft_amd import fftree as FT
    ecfft_amd.build.build()
    L = FT.lib()
    assert "ecfft_poly_equal_degree" in FT.EXPORTS and hasattr(L, "ecfft_poly_equal_degree")
    header = open(os.path.join(ROOT, "include", "ecfft_hip.h")).read()
    assert f"#define ECFFT_EDF_SMALL_MAX {FT.EDF_SMALL_MAX} " in header
    assert FT.EDF_SMALL_MAX == 65
    for name in ("poly_equal_degree", "edf_unpack", "poly_irreducible_factors"):
        assert hasattr(FT.FFTree, name)
    buf = np.zeros(8, np.uint32)
    n = np.zeros(1, np.int64)
    ptr, pn = buf.ctypes.data, n.ctypes.data
    ed = L.ecfft_poly_equal_degree
    # a NULL context; then ng, d and count of zero and NULL pointers: all decided before a device is touched
    assert ed(None, ptr, 3, 1, ptr, pn, 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    for ng, d, count in ((0, 1, 1), (3, 0, 1), (3, 1, 0)):
        assert ed(None, ptr, ng, d, ptr, pn, count, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    for args in ((None, ptr, pn), (ptr, None, pn), (ptr, ptr, None)):
        assert ed(None, args[0], 3, 1, args[1], args[2], 1, FT.MEM_HOST, None) == FT.ERR_BAD_ARG
    assert not buf.any() and not n.any()
