"""TEST INFRASTRUCTURE — exact CPU references of poly_xgcd_partial / rs_decode, for tests/test_gpu_xgcd_partial.py,
tests/test_gpu_rsdecode.py and tests/test_rs_ref_host.py.

Imports only numpy, the standard library and tests/gcd_ref.py (int-list polynomials, schoolbook division).  Everything here is
generic in the prime p: polynomials are trimmed lists of Python ints, low to high, the zero polynomial the empty list.

- partial_row: the classical extended Euclidean sequence r_0 = a, r_1 = b, r_{i+1} = r_{i-1} - q_i r_i with (s_0, t_0) = (1, 0),
  (s_1, t_1) = (0, 1) (deg a < deg b: q_1 = 0, the sequence's own swap), run until the first row j >= 1 with deg r_j < stop
  (deg 0 = -1), that row scaled so that t is monic (s where t = 0).
- lagrange_basis / interpolate / from_roots / evaluate: schoolbook, quadratic.
- gao_decode: Gao's Reed-Solomon decoder on partial_row.
"""
import numpy as np

import gcd_ref as G


def deg(v):
    return len(G.trim(v)) - 1


def _mul(x, y, p):
    """schoolbook product of two int lists"""
    x, y = G.trim(x), G.trim(y)
    if not x or not y:
        return []
    if len(x) > len(y):
        x, y = y, x
    out = [0] * (len(x) + len(y) - 1)
    for i, c in enumerate(x):
        if c:
            for j, d in enumerate(y):
                out[i + j] += c * d
    return G.trim([v % p for v in out])


def _sub(x, y, p):
    return G._sub(x, y, p)


def partial_rows(p, a, b, stops):
    """{stop: (r, s, t, prev)} for every stop of `stops` in one pass over the sequence: the normalised row of the definition above
    as int lists and prev = the degree of the remainder before it (deg r < stop <= prev whenever the row is not row 1; prev is
    deg a for row 1)"""
    a, b = G.trim([x % p for x in a]), G.trim([x % p for x in b])
    r0, s0, t0 = a, [1], []
    r1, s1, t1 = b, [], [1]
    out = {}
    for stop in sorted(set(stops), reverse=True):
        while deg(r1) >= stop:                       # deg 0 = -1 < stop: the zero row always ends the loop
            q, rem = G.divmod_school(r0, r1, p)
            r0, r1 = r1, rem
            s0, s1 = s1, _sub(s0, _mul(q, s1, p), p)
            t0, t1 = t1, _sub(t0, _mul(q, t1, p), p)
        lead = t1[-1] if t1 else s1[-1]
        c = pow(lead, p - 2, p)
        out[stop] = (G._scale(r1, c, p), G._scale(s1, c, p), G._scale(t1, c, p), deg(r0))
    return out


def partial_row(p, a, b, stop):
    """(r, s, t, prev) for one stop"""
    return partial_rows(p, a, b, [stop])[stop]


def from_roots(p, xs):
    """prod (x - x_i)"""
    out = [1]
    for x in xs:
        nxt = [0] + out
        for i, c in enumerate(out):
            nxt[i] = (nxt[i] - x * c) % p
        out = nxt
    return out


def evaluate(p, f, xs):
    out = []
    for x in xs:
        v = 0
        for c in reversed(f):
            v = (v * x + c) % p
        out.append(v)
    return out


_lagrange = {}


def lagrange_basis(p, xs):
    """(g0, Q): g0 = prod (x - x_i) and the m x m object matrix whose row i holds the coefficients of g0 / (x - x_i) / g0'(x_i), the
    Lagrange basis polynomial of x_i: m inversions and m synthetic divisions, kept per point set"""
    key = (p, tuple(xs))
    if key not in _lagrange:
        m = len(xs)
        g0 = from_roots(p, xs)
        Q = np.zeros((m, m), dtype=object)
        for i, x in enumerate(xs):
            q, carry = [0] * m, 0
            for j in range(m, 0, -1):                # synthetic division of g0 by x - x_i
                carry = (g0[j] + carry * x) % p
                q[j - 1] = carry
            w = pow(evaluate(p, q, [x])[0], p - 2, p)             # g0'(x_i) = (g0 / (x - x_i))(x_i)
            Q[i] = [c * w % p for c in q]
        _lagrange.clear()                            # one point set at a time: the matrices are large
        _lagrange[key] = (g0, Q)
    return _lagrange[key]


def interpolate(p, xs, ys):
    """the polynomial of degree < len(xs) through (x_i, y_i): sum_i y_i L_i over the Lagrange basis"""
    _, Q = lagrange_basis(p, xs)
    return G.trim([int(c) % p for c in np.array([y % p for y in ys], dtype=object) @ Q])


def gao_decode(p, xs, ys, k):
    """(message, n_errors): message = the k coefficients (zero-padded int list) of the unique f, deg f < k, that differs from ys in
    at most (m - k) // 2 positions and n_errors = the number of those positions; ([0] * k, -1) when there is none.
    Gao: g0 = prod (x - x_i), g1 = the interpolant, the partial row of (g0, g1) with stop = ceil((m + k) / 2), f = r / t."""
    m = len(xs)
    assert 1 <= k <= m and len(ys) == m and len(set(x % p for x in xs)) == m
    g0, g1 = lagrange_basis(p, xs)[0], interpolate(p, xs, ys)
    r, _, t, _ = partial_row(p, g0, g1, (m + k + 1) // 2)
    f, rem = G.divmod_school(r, t, p)
    if rem or deg(f) >= k:
        return [0] * k, -1
    return f + [0] * (k - len(f)), deg(t)
