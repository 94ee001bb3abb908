"""TEST INFRASTRUCTURE — exact CPU references of seq_min_poly / seq_nth_term, for tests/test_gpu_seq.py and
tests/test_seq_ref_host.py.

Imports only numpy (object arrays of Python ints), the standard library and tests/rs_ref.py (the partial remainder row on
int-list polynomials).  Everything here is generic in the prime p: a sequence is a list of Python ints, a polynomial a list of
ints low to high.

- berlekamp_massey: the textbook algorithm, (L, monic C low to high): the linear complexity of the row and ONE polynomial of
  that degree that generates it, the unique one where 2 L <= N.
- euclid_min_poly: the route the library defines (MCA Alg. 12.9): h = sum s_i x^i, (r, ., t) = the partial row of (x^N, h) with
  stop = N // 2, d = max(1 + deg r, deg t); determined iff t(0) != 0 and 2 d <= N, and then (d, x^d t(1/x) / t(0)); else
  (-1, []).
- power_of_x / nth_terms: x^K mod C by square-and-multiply on schoolbook products, and s_K .. s_(K + nout - 1) from it
  (Fiduccia); iterate: the same terms by running the recurrence.
"""
import numpy as np

import rs_ref as S


def berlekamp_massey(p, s):
    """(L, C): C = [c_0, .., c_(L-1), 1] with s[i+L] + sum_j c_j s[i+j] = 0 for 0 <= i < N - L, L minimal"""
    s = [x % p for x in s]
    c, b = [1], [1]                      # connection polynomials, c[0] = 1: sum_i c[i] s[n-i] = 0
    L, m, bd = 0, 1, 1
    for n in range(len(s)):
        d = sum(c[i] * s[n - i] for i in range(min(L, len(c) - 1) + 1)) % p
        if d == 0:
            m += 1
            continue
        coef = d * pow(bd, p - 2, p) % p
        t = c[:]
        c = c + [0] * (len(b) + m - len(c))
        for i, v in enumerate(b):
            c[i + m] = (c[i + m] - coef * v) % p
        if 2 * L <= n:
            L, b, bd, m = n + 1 - L, t, d, 1
        else:
            m += 1
    c = (c + [0] * (L + 1))[:L + 1]
    return L, c[::-1]                    # C = x^L c(1/x)


def euclid_min_poly(p, s):
    """(L, C) where the row is determined, (-1, []) where it is not"""
    n = len(s)
    r, _, t, _ = S.partial_row(p, [0] * n + [1], [x % p for x in s], n // 2)
    d = max(1 + S.deg(r), S.deg(t))
    if not t or t[0] == 0 or 2 * d > n:
        return -1, []
    inv = pow(t[0], p - 2, p)
    t = t + [0] * (d + 1 - len(t))
    return d, [t[d - j] * inv % p for j in range(d + 1)]


def _mulmod(p, a, b, M):
    """a b mod (x^L + M) for residues of L coefficients (int lists) and the low coefficients M of the MONIC modulus as an object
    array: the schoolbook product row by row, then one elimination step per coefficient from 2 L - 2 down to L.  Sums are kept
    as exact integers and reduced mod p once per row."""
    L = len(M)
    bv = np.array(b, dtype=object)
    prod = np.zeros(2 * L, dtype=object)
    for i, x in enumerate(a):
        if x:
            prod[i:i + L] += x * bv
    for k in range(2 * L - 2, L - 1, -1):
        q = prod[k] % p
        if q:
            prod[k - L:k] -= q * M
    return [int(v) % p for v in prod[:L]]


def _shift(p, u, M):
    """x u mod (x^L + M)"""
    top = u[-1]
    return [((u[j - 1] if j else 0) - top * int(M[j])) % p for j in range(len(u))]


def power_of_x(p, C, K):
    """x^K mod C as L = len(C) - 1 coefficients, by square-and-multiply from the top bit of K; C[L] != 0, L >= 1"""
    C = [c % p for c in C]
    L = len(C) - 1
    assert L >= 1 and C[L] and K >= 0
    linv = pow(C[L], p - 2, p)
    M = np.array([c * linv % p for c in C[:L]], dtype=object)
    u = [1] + [0] * (L - 1)
    for i in range(K.bit_length() - 1, -1, -1):
        u = _mulmod(p, u, u, M)
        if (K >> i) & 1:
            u = _shift(p, u, M)
    return u


def nth_terms(p, C, init, K, nout, u=None):
    """[s_K, .., s_(K + nout - 1)] of the sequence with sum_{j<=L} C[j] s[i+j] = 0 and s[:L] = init; C[L] != 0, L >= 1.  u: a
    power_of_x(p, C, K) the caller already has"""
    C, init = [c % p for c in C], [x % p for x in init]
    L = len(C) - 1
    assert len(init) == L
    u = power_of_x(p, C, K) if u is None else list(u)
    linv = pow(C[L], p - 2, p)
    M = [c * linv % p for c in C[:L]]
    out = []
    for _ in range(nout):
        out.append(sum(a * b for a, b in zip(u, init)) % p)
        u = _shift(p, u, M)
    return out


def iterate(p, C, init, n):
    """the first n terms by running the recurrence"""
    C = [c % p for c in C]
    L = len(C) - 1
    linv = pow(C[L], p - 2, p)
    s = [x % p for x in init]
    while len(s) < n:
        i = len(s) - L
        s.append(-sum(C[j] * s[i + j] for j in range(L)) * linv % p)
    return s[:n]
