"""CPU tests of tests/poly_ref.py, the exact references of tests/test_gpu_poly_regimes.py: the Kronecker product, the division and
series checks against the numpy-object schoolbook, long division and recurrence of the GPU modules, at random shapes in both fields
with full-range and special values and at the slot-width edges; and every check (exact and Schwartz-Zippel) rejects a result with
one coefficient changed by +1 at the first, the middle and the last position."""
import numpy as np
import pytest

import poly_ref as R

FIELDS = ["secp256k1", "m31"]


def schoolbook(a, b, p):
    return [int(x) % p for x in np.convolve(np.array(a, dtype=object), np.array(b, dtype=object))]


def long_division(a, b, p):
    nb, nq = len(b), max(len(a) - len(b) + 1, 0)
    r = np.array(a, dtype=object)
    bb = np.array(b, dtype=object)
    q = [0] * nq
    inv = pow(b[-1], p - 2, p)
    for i in range(nq - 1, -1, -1):
        c = int(r[i + nb - 1]) * inv % p
        q[i] = c
        if c:
            r[i:i + nb] = (r[i:i + nb] - c * bb) % p
    rem = [int(x) % p for x in r[:nb - 1]] + [0] * max(nb - 1 - len(a), 0)
    return q, rem[:nb - 1]


def reciprocal(f, k, p):
    g0 = pow(f[0], p - 2, p)
    fa = np.array(f[1:k], dtype=object)
    ga = np.zeros(k, dtype=object)
    ga[0] = g0
    for j in range(1, k):
        m = min(j, len(f) - 1)
        s = int(np.dot(fa[:m], ga[j - 1::-1][:m])) if m else 0
        ga[j] = (-g0 * s) % p
    return [int(x) for x in ga]


def bump(field, x, i):
    """x with coefficient i changed by +1 mod p (standard form)"""
    v = R.to_ints(field, x)
    v[i] = (v[i] + 1) % R.P[field]
    return R.from_ints(field, v)


def positions(n):
    return sorted({0, n // 2, n - 1})


SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (31, 17), (64, 64), (100, 3), (129, 250), (300, 299)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", SHAPES)
@pytest.mark.parametrize("specials", [False, True])
def test_product_matches_schoolbook(field, na, nb, specials):
    p = R.P[field]
    a, b = R.rand_std(field, na, na * 31 + nb, specials), R.rand_std(field, nb, na * 37 + nb + 1, specials)
    c = R.mul_exact(field, a, b)
    assert R.to_ints(field, c) == schoolbook(R.to_ints(field, a), R.to_ints(field, b), p)
    assert R.check_mul(field, a, b, c) == ""
    for i in positions(c.shape[0]):
        assert R.check_mul(field, a, b, bump(field, c, i)) != "", i


def test_full_range_inputs():
    """the secp256k1 generator reaches [2^255, p) and stays below p; the specials are where asked"""
    a = R.rand_std("secp256k1", 4096, 1, specials=False)
    top = a[:, 3] >> np.uint64(63)
    assert 0.4 < top.mean() < 0.6
    assert R.canonical("secp256k1", a).all()
    vals = set(R.to_ints("secp256k1", R.rand_std("secp256k1", 512, 2)))
    assert {0, 1, R.P["secp256k1"] - 1} <= vals
    assert R.canonical("secp256k1", R.from_ints("secp256k1", [R.P["secp256k1"] - 1])).all()
    assert not R.canonical("secp256k1", R.from_ints("secp256k1", [R.P["secp256k1"], 2**256 - 1])).any()
    assert not R.canonical("m31", np.array([2**31 - 1, 2**32 - 1], dtype=np.uint32)).any()


def _widest(field, w):
    """the largest operand length whose product coefficients use slots of w bytes"""
    lo, hi = 1, 1
    while R.slot_bytes(field, hi * 2, hi * 2) <= w:
        hi *= 2
    hi *= 2
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if R.slot_bytes(field, mid, mid) <= w else (lo, mid)
    return lo


@pytest.mark.parametrize("field,widths", [("secp256k1", (64, 65)), ("m31", (8, 9))])
def test_slot_width_edge(field, widths):
    """every coefficient p - 1 at the largest length each slot width is used for, and one longer: the middle coefficient of the
    product is the largest possible sum"""
    p = R.P[field]
    for w in widths:
        n = _widest(field, w)
        assert R.slot_bytes(field, n, n) == w and R.slot_bytes(field, n + 1, n + 1) == w + 1
        for m in (n, n + 1):
            a = R.from_ints(field, [p - 1] * m)
            assert R.to_ints(field, R.mul_exact(field, a, a)) == schoolbook([p - 1] * m, [p - 1] * m, p), (w, m)


DIV_SHAPES = [(1, 1), (50, 1), (3, 10), (2, 2), (100, 100), (130, 4), (257, 3), (364, 300), (300, 120)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", DIV_SHAPES)
def test_divrem_check_matches_long_division(field, na, nb):
    p = R.P[field]
    a = R.rand_std(field, na, na * 7 + nb)
    b = R.set_nonzero(field, R.rand_std(field, nb, na * 11 + nb), nb - 1)
    q, r = long_division(R.to_ints(field, a), R.to_ints(field, b), p)
    qa = R.from_ints(field, q) if q else np.zeros(R.shape(field, 0), R.dtype(field))
    ra = R.from_ints(field, r) if r else np.zeros(R.shape(field, 0), R.dtype(field))
    assert R.check_divrem(field, a, b, qa, ra) == ""
    zs = R.sz_points(field, R.sz_count(field, na), 5)
    assert R.sz_divrem(field, a, b, qa, ra, zs) == ""
    for name, x in (("q", qa), ("r", ra)):
        for i in positions(x.shape[0]) if x.shape[0] else []:
            qb, rb = (bump(field, qa, i), ra) if name == "q" else (qa, bump(field, ra, i))
            assert R.check_divrem(field, a, b, qb, rb) != "", (name, i)
            assert R.sz_divrem(field, a, b, qb, rb, zs) != "", (name, i)
    if qa.shape[0]:                                          # lengths are asserted separately
        assert R.check_divrem(field, a, b, qa[:-1], ra) != ""
        assert R.sz_divrem(field, a, b, qa[:-1], ra, zs) != ""


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nf,k", [(1, 1), (1, 40), (5, 3), (60, 200), (300, 100), (257, 257)])
def test_series_checks_match_recurrence(field, nf, k):
    p = R.P[field]
    f = R.set_nonzero(field, R.rand_std(field, nf, nf * 13 + k), 0)
    g = R.from_ints(field, reciprocal(R.to_ints(field, f), k, p))
    zs = R.sz_points(field, R.sz_count(field, k), 7)
    assert R.check_inv_series(field, f, g) == ""
    assert R.sz_inv_series(field, f, g, zs) == ""
    for i in positions(k):
        assert R.check_inv_series(field, f, bump(field, g, i)) != "", i
        assert R.sz_inv_series(field, f, bump(field, g, i), zs) != "", i


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb", [(1, 1), (40, 3), (200, 150)])
def test_sz_mul_and_horner(field, na, nb):
    p = R.P[field]
    a, b = R.rand_std(field, na, na + 1), R.rand_std(field, nb, nb + 2)
    c = R.mul_exact(field, a, b)
    zs = R.sz_points(field, R.sz_count(field, na + nb), 3)
    ai = R.to_ints(field, a)
    assert R.horner(field, a, zs) == [sum(x * pow(z, i, p) for i, x in enumerate(ai)) % p for z in R.to_ints(field, zs)]
    assert R.sz_mul(field, a, b, c, zs) == ""
    for i in positions(c.shape[0]):
        assert R.sz_mul(field, a, b, bump(field, c, i), zs) != "", i


def test_sz_count():
    assert R.sz_count("secp256k1", 1 << 24) == 2
    for D in (2, 1 << 13, 1 << 17, 1 << 21, 1 << 24):
        t = R.sz_count("m31", D)
        assert (D / R.P["m31"]) ** t <= 2.0 ** -64, D


def test_noncanonical_output_is_rejected():
    """a coefficient equal to p is congruent to 0 but not canonical"""
    p = R.P["m31"]
    a = np.array([3, 5], dtype=np.uint32)
    c = R.mul_exact("m31", a, a)
    assert R.check_mul("m31", a, a, c) == ""
    z = np.array([0, 1], dtype=np.uint32)
    zc = R.mul_exact("m31", z, z)
    assert zc[0] == 0
    zc[0] = p
    assert R.check_mul("m31", z, z, zc) != ""
    assert R.sz_mul("m31", z, z, zc, R.sz_points("m31", 3, 1)) != ""


# ---- the witness identity of a modular product ----------------------------------------------------------------------------------------
MULMOD_SHAPES = [(30, 25, 20), (20, 20, 21), (7, 5, 11), (40, 3, 2), (5, 4, 30), (64, 64, 65)]      # (nx, ny, nm): long, one and no quotient


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nx,ny,nm", MULMOD_SHAPES)
def test_sz_mul_mod_accepts_the_remainder_and_rejects_one_changed_coefficient(field, nx, ny, nm):
    p = R.P[field]
    x, y = R.rand_std(field, nx, nx + 3 * ny), R.rand_std(field, ny, ny + 5 * nm)
    f = R.set_nonzero(field, R.rand_std(field, nm, nm + 7 * nx), nm - 1)
    qi, ri = long_division(schoolbook(R.to_ints(field, x), R.to_ints(field, y), p), R.to_ints(field, f), p)
    q, r = R.from_ints(field, qi), R.from_ints(field, ri)
    assert q.shape[0] == max(nx + ny - nm, 0) and r.shape[0] == nm - 1
    zs = R.sz_points(field, R.sz_count(field, nx + ny), 5)
    assert R.sz_mul_mod(field, x, y, f, q, r, zs) == ""
    for i in positions(r.shape[0]):
        assert R.sz_mul_mod(field, x, y, f, q, bump(field, r, i), zs) != "", i
    for i in positions(q.shape[0]) if q.shape[0] else []:
        assert R.sz_mul_mod(field, x, y, f, bump(field, q, i), r, zs) != "", i
    # shapes and canonical form are part of the check: a remainder one coefficient short or long, a zero leading coefficient of f
    assert "lengths" in R.sz_mul_mod(field, x, y, f, q, r[:-1], zs)
    assert "lengths" in R.sz_mul_mod(field, x, y, f, q[:-1] if q.shape[0] else R.from_ints(field, [0]), r, zs)
    z = f.copy()
    z[nm - 1] = 0
    assert "leading" in R.sz_mul_mod(field, x, y, z, q, r, zs)
    bad = r.copy()
    bad[0] = R.from_ints(field, [p])[0]
    assert "canonical" in R.sz_mul_mod(field, x, y, f, q, bad, zs)


@pytest.mark.parametrize("field", FIELDS)
def test_sz_mul_mod_with_a_passed_horner(field):
    """the horner_fn interface (standard form in, Python ints out), as the GPU module passes the oracle's"""
    p = R.P[field]
    calls = []

    def h(c, zs):
        calls.append(c.shape[0])
        return R.horner(field, c, zs)

    x, y = R.rand_std(field, 50, 1), R.rand_std(field, 50, 2)
    f = R.set_nonzero(field, R.rand_std(field, 41, 3), 40)
    qi, ri = long_division(schoolbook(R.to_ints(field, x), R.to_ints(field, y), p), R.to_ints(field, f), p)
    zs = R.sz_points(field, 3, 9)
    assert R.sz_mul_mod(field, x, y, f, R.from_ints(field, qi), R.from_ints(field, ri), zs, h) == ""
    assert sorted(calls) == [40, 41, 50, 50, 59]
