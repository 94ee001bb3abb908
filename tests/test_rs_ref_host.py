"""CPU tests of tests/rs_ref.py, the exact model behind the GPU tests of ecfft_poly_xgcd_partial and ecfft_rs_decode: the partial
row's identity, degree bracket and normalisation, and Gao's decoder against a brute-force nearest-codeword search over a tiny
prime."""
import itertools
import random

import numpy as np
import pytest

import gcd_ref as G
import poly_ref as R
import rs_ref as S

PRIMES = [97, R.P["m31"], R.P["secp256k1"]]


def rand_poly(p, n, rng):
    """n coefficients, degree exactly n - 1"""
    v = [rng.randrange(p) for _ in range(n)]
    if n:
        v[-1] = v[-1] or 1
    return v


def add(x, y, p):
    return G._add(x, y, p)


def check_row(p, a, b, stop, row):
    r, s, t, prev = row
    assert add(S._mul(s, a, p), S._mul(t, b, p), p) == G.trim(r)
    assert S.deg(r) < stop
    assert all(0 <= x < p for x in r + s + t)
    assert (t and t[-1] == 1) or (not t and s and s[-1] == 1)
    if s:                                                            # not row 1 (s_1 = 0): the remainder before it is not below stop
        assert prev >= stop


@pytest.mark.parametrize("p", PRIMES)
def test_partial_row_identity_and_bracket(p):
    rng = random.Random(p % 1000)
    for na, nb in ((2, 1), (9, 9), (33, 20), (20, 33), (40, 39)):
        a, b = rand_poly(p, na, rng), rand_poly(p, nb, rng)
        stops = sorted({0, 1, (na - 1) // 3, (na - 1 + 1) // 2 - 1, (na - 1 + 1) // 2, (na - 1 + 1) // 2 + 1, nb - 1, na, max(na, nb) + 3})
        many = S.partial_rows(p, a, b, stops)
        for stop in stops:
            row = S.partial_row(p, a, b, stop)
            assert row == many[stop]
            check_row(p, a, b, stop, row)


@pytest.mark.parametrize("p", PRIMES)
def test_partial_row_is_a_row_of_the_sequence(p):
    """against the sequence written out row by row: the selected row is the FIRST below stop, up to the scale"""
    rng = random.Random(7)
    a, b = rand_poly(p, 24, rng), rand_poly(p, 21, rng)
    seq = [(a, [1], []), (b, [], [1])]
    while seq[-1][0]:
        q, rem = G.divmod_school(seq[-2][0], seq[-1][0], p)
        seq.append((rem, G._sub(seq[-2][1], S._mul(q, seq[-1][1], p), p), G._sub(seq[-2][2], S._mul(q, seq[-1][2], p), p)))
    for stop in range(0, 26):
        j = next(i for i in range(1, len(seq)) if S.deg(seq[i][0]) < stop)
        r, s, t, prev = S.partial_row(p, a, b, stop)
        c = pow(seq[j][2][-1], p - 2, p)
        assert (r, s, t) == tuple(G._scale(x, c, p) for x in seq[j]) and prev == S.deg(seq[j - 1][0])


@pytest.mark.parametrize("p", PRIMES)
def test_abnormal_and_common_factor(p):
    rng = random.Random(11)
    g = rand_poly(p, 6, rng)
    g[-1] = 1
    qs = [rand_poly(p, d + 1, rng) for d in (2, 5, 1, 3, 4, 2)]
    hi, lo = g, []
    for q in reversed(qs):
        hi, lo = add(S._mul(q, hi, p), lo, p), hi
    a, b = hi, lo
    degs = [S.deg(a)]
    for q in qs:
        degs.append(degs[-1] - S.deg(q))
    assert degs[-1] == 5
    for stop in range(0, S.deg(a) + 2):
        row = S.partial_row(p, a, b, stop)
        check_row(p, a, b, stop, row)
        want = next(d for d in degs[1:] + [-1] if d < stop)             # the degrees of r_1 .. r_m, then the zero row
        assert S.deg(row[0]) == want
    r, s, t, _ = S.partial_row(p, a, b, 0)
    assert not r and S._mul(t, g, p) == G._scale(a, pow(a[-1], p - 2, p), p)      # t = +-a / g up to scale, and both are monic


@pytest.mark.parametrize("p", PRIMES)
def test_normalisation_cases(p):
    rng = random.Random(3)
    a, b = rand_poly(p, 8, rng), rand_poly(p, 5, rng)
    # b = 0: row 1 is (0, 0, 1) for every stop
    for stop in (0, 1, 8, 20):
        assert S.partial_row(p, a, [], stop) == ([], [], [1], 7)
    # a = 0: row 1 = (b, 0, 1) above deg b; from deg b down row 2 = (0, 1, 0)
    assert S.partial_row(p, [], b, 5) == (b, [], [1], -1)
    assert S.partial_row(p, [], b, 4) == ([], [1], [], 4) == S.partial_row(p, [], b, 0)
    # both zero
    assert S.partial_row(p, [], [], 0) == ([], [], [1], -1) == S.partial_row(p, [0, 0], [0], 3)
    # deg a < deg b: row 1 = (b, 0, 1), then row 2 = (a, 1, 0) scaled so that s is monic (it is), then the sequence of (b, a)
    assert S.partial_row(p, b, a, 8) == (a, [], [1], 4)
    assert S.partial_row(p, b, a, 7) == (b, [1], [], 7) == S.partial_row(p, b, a, 5)
    r, s, t, prev = S.partial_row(p, b, a, 4)
    q, rem = G.divmod_school(a, b, p)
    assert (r, s, t, prev) == (rem, G._scale(q, p - 1, p), [1], 4)
    # stop = 0: the zero row; t is a / gcd up to sign, made monic
    r, s, t, _ = S.partial_row(p, a, b, 0)
    assert not r and t[-1] == 1 and add(S._mul(s, a, p), S._mul(t, b, p), p) == []
    assert S.deg(t) <= S.deg(a) and S.deg(s) <= S.deg(b)
    # stop above both degrees: row 1
    assert S.partial_row(p, a, b, 9) == (b, [], [1], 7) == S.partial_row(p, a, b, 1000)
    # untrimmed and unreduced inputs
    assert S.partial_row(p, a + [0, 0], [x + p for x in b] + [0], 3) == S.partial_row(p, a, b, 3)


def brute_force(p, xs, ys, k):
    """every codeword within (m - k) // 2 of ys, as (message, distance): numpy over all p^k messages"""
    m = len(xs)
    msgs = np.array(list(itertools.product(range(p), repeat=k)), dtype=np.int64)[:, ::-1]       # coefficient 0 fastest
    V = np.array([[pow(x, j, p) for x in xs] for j in range(k)], dtype=np.int64)
    words = msgs @ V % p
    dist = (words != np.array(ys, dtype=np.int64)).sum(axis=1)
    hit = np.nonzero(dist <= (m - k) // 2)[0]
    return [([int(c) for c in msgs[i]], int(dist[i])) for i in hit]


@pytest.mark.parametrize("m,k", [(4, 1), (6, 2), (7, 3), (8, 2), (8, 3), (3, 3), (4, 3)])
def test_gao_against_nearest_codeword_search(m, k):
    p = 97
    rng = random.Random(100 * m + k)
    radius = (m - k) // 2
    for trial in range(12):
        xs = rng.sample(range(p), m)
        if trial == 0:
            xs[0] = 0
        f = [rng.randrange(p) for _ in range(k)]
        ys = S.evaluate(p, f, xs)
        e = [0, 1, radius, radius + 1, radius + 2, m][trial % 6]
        for pos in rng.sample(range(m), min(e, m)):
            ys[pos] = (ys[pos] + 1 + rng.randrange(p - 1)) % p
        near = brute_force(p, xs, ys, k)
        assert len(near) <= 1                                             # the radius is half the minimum distance
        msg, ne = S.gao_decode(p, xs, ys, k)
        if near:
            assert (msg, ne) == near[0]
            if e <= radius:
                assert msg == f and ne == e
        else:
            assert ne == -1 and msg == [0] * k


@pytest.mark.parametrize("p", PRIMES[1:])
def test_gao_large_primes(p):
    rng = random.Random(5)
    m, k = 24, 10
    xs = rng.sample(range(1, 10 ** 6), m)
    f = [rng.randrange(p) for _ in range(k)]
    for e in (0, 1, 7):
        ys = S.evaluate(p, f, xs)
        for pos in rng.sample(range(m), e):
            ys[pos] = (ys[pos] + 1) % p
        assert S.gao_decode(p, xs, ys, k) == (f, e)
    assert S.interpolate(p, xs, S.evaluate(p, f, xs)) == G.trim(f)
    assert S.evaluate(p, S.from_roots(p, xs), xs) == [0] * m
