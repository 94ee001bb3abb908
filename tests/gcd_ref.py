"""TEST INFRASTRUCTURE — exact CPU references of poly_gcd / poly_xgcd, for tests/test_gpu_polygcd.py and tests/test_gcd_ref_host.py.

Imports only numpy, the standard library and tests/poly_ref.py (its Kronecker product mul_exact).  Polynomials are STANDARD-form
arrays in the element layout of the field, as in poly_ref; the zero polynomial is an array of any length that holds only zeros.

- eea: the classical extended Euclidean algorithm on Python ints, a restatement of utils::xgcd (src/utils.rs:147-182) line by line,
  with schoolbook division.  Quadratic in pure Python: for small sizes only.
- gcd: the monic gcd by the same remainder loop, in the convention of xgcd (gcd(0, b) = monic b; utils::gcd returns 0 there).
- from_quotients: (r0, r1) built BACKWARDS from r_m = g and r_{i-1} = q_i r_i + r_{i+1}.  By uniqueness of division with remainder,
  Euclid on (r0, r1) has exactly the quotient sequence qs and the gcd g, so abnormal sequences (quotients of any degree) of any
  size come with their answer; the cofactors follow from the same recurrence s_{i+1} = s_{i-1} - q_i s_i.
- check_xgcd: a s + b t = g by mul_exact, g monic, canonical residues, and the degree bounds that make (s, t) unique.
"""
import numpy as np

import poly_ref as R

P = R.P


# ---- polynomials as lists of ints, low to high, no trailing zeros ----------------------------------------------------------------------
def trim(v):
    v = [int(x) for x in v]
    while v and v[-1] == 0:
        v.pop()
    return v


def ints(field, a):
    """standard-form array -> trimmed list of ints"""
    return trim(R.to_ints(field, a)) if a.shape[0] else []


def arr(field, v, n=None):
    """list of ints -> standard-form array of n coefficients (default: as many as the list has), zero-padded"""
    n = len(v) if n is None else n
    assert len(trim(v)) <= n, (len(trim(v)), n)
    out = np.zeros(R.shape(field, n), R.dtype(field))
    k = min(len(v), n)
    if k:
        out[:k] = R.from_ints(field, [x % P[field] for x in v[:k]])
    return out


def deg(v):
    return len(trim(v)) - 1


def _sub(x, y, p):
    n = max(len(x), len(y))
    return trim([((x[i] if i < len(x) else 0) - (y[i] if i < len(y) else 0)) % p for i in range(n)])


def _add(x, y, p):
    n = max(len(x), len(y))
    return trim([((x[i] if i < len(x) else 0) + (y[i] if i < len(y) else 0)) % p for i in range(n)])


def _scale(x, c, p):
    return trim([v * c % p for v in x])


def mul(field, x, y):
    """product of two int lists through poly_ref.mul_exact"""
    x, y = trim(x), trim(y)
    if not x or not y:
        return []
    return trim(R.to_ints(field, R.mul_exact(field, arr(field, x), arr(field, y))))


def divmod_school(a, b, p):
    """(q, r) with a = b q + r, deg r < deg b, by long division on int lists (b != 0): ark-poly's divide_with_q_and_r"""
    a, b = trim(a), trim(b)
    assert b
    if len(a) < len(b):
        return [], a
    r = np.array(a, dtype=object)
    bb = np.array(b, dtype=object)
    nb, nq = len(b), len(a) - len(b) + 1
    inv = pow(b[-1], p - 2, p)
    q = [0] * nq
    for i in range(nq - 1, -1, -1):
        c = int(r[i + nb - 1]) * inv % p
        q[i] = c
        if c:
            r[i:i + nb] = (r[i:i + nb] - c * bb) % p
    return trim(q), trim([int(x) % p for x in r[:nb - 1]])


# ---- utils::xgcd restated ----------------------------------------------------------------------------------------------------------
def eea(field, a, b):
    """(s, t, g) of int lists exactly as utils::xgcd (src/utils.rs:147-182) computes them: the remainder loop on (old_r, r) and
    (old_s, s), t = (old_r - old_s a) / b (zero when b = 0), everything scaled by 1 / lc(old_r) (by 1 when old_r = 0)"""
    p = P[field]
    a, b = trim(a), trim(b)
    s, old_s, r, old_r = [], [1], b, a
    while r:
        q, rem = divmod_school(old_r, r, p)
        r, old_r = rem, r
        s, old_s = _sub(old_s, mul(field, q, s), p), s
    if b:
        t, rem = divmod_school(_sub(old_r, mul(field, old_s, a), p), b, p)
        assert not rem
    else:
        t = []
    c = pow(old_r[-1], p - 2, p) if old_r else 1
    return _scale(old_s, c, p), _scale(t, c, p), _scale(old_r, c, p)


def gcd(field, a, b):
    """the monic gcd of two int lists (gcd(0, 0) = 0), in xgcd's convention for a zero operand"""
    p = P[field]
    a, b = trim(a), trim(b)
    while b:
        a, b = b, divmod_school(a, b, p)[1]
    return _scale(a, pow(a[-1], p - 2, p), p) if a else []


# ---- a pair with a prescribed quotient sequence ----------------------------------------------------------------------------------------
def from_quotients(field, g, qs):
    """g: monic int list; qs = [q_1 .. q_m]: int lists, deg q_i >= 1 for i >= 2 and q_1 != 0.  Returns int lists (r0, r1, s, t):
    Euclid on (r0, r1) takes exactly the quotients qs, gcd(r0, r1) = g, and (s, t) are the cofactors utils::xgcd returns"""
    p = P[field]
    g = trim(g)
    assert g and g[-1] == 1 and all(trim(q) for q in qs) and all(deg(q) >= 1 for q in qs[1:])
    hi, lo = g, []                                   # r_m, r_{m+1}
    for q in reversed(qs):
        hi, lo = _add(mul(field, q, hi), lo, p), hi   # r_{i-1} = q_i r_i + r_{i+1}
    r0, r1 = hi, lo
    s0, s1, t0, t1 = [1], [], [], [1]
    for q in qs:
        s0, s1 = s1, _sub(s0, mul(field, q, s1), p)
        t0, t1 = t1, _sub(t0, mul(field, q, t1), p)
    return r0, r1, s0, t0


def rand_poly(field, n, seed, monic=False):
    """n coefficients (degree exactly n - 1) as an int list"""
    v = R.to_ints(field, R.rand_std(field, n, seed, specials=False))
    v[-1] = 1 if monic or v[-1] == 0 else v[-1]
    return v


# ---- the check ---------------------------------------------------------------------------------------------------------------------
def check_xgcd(field, a, b, s, t, g):
    """"" when (s, t, g) (standard-form arrays, zero-padded) is what xgcd(a, b) returns, else a message: canonical residues, g monic,
    a s + b t = g exactly, and deg s < deg b - deg g, deg t < deg a - deg g where those bounds are positive — which makes the
    cofactors unique — or the degenerate values of the Euclidean algorithm (b = 0: s = 1/lc(a), t = 0; a = 0 or b | a: s = 0,
    t = 1/lc(b))"""
    p = P[field]
    bad = R._noncanonical(field, [("s", s), ("t", t), ("g", g)])
    if bad:
        return bad
    A, B, S, T, G = (ints(field, x) for x in (a, b, s, t, g))
    if not A and not B:
        return "" if not (S or T or G) else "a = b = 0 must give s = t = g = 0"
    if not G or G[-1] != 1:
        return "g is not monic"
    if _add(mul(field, A, S), mul(field, B, T), p) != G:
        return "a s + b t != g"
    if not B:
        return "" if S == [pow(A[-1], p - 2, p)] and not T else "b = 0: expected s = 1/lc(a), t = 0"
    if deg(B) == deg(G):                                  # a = 0 or b | a
        return "" if not S and T == [pow(B[-1], p - 2, p)] else "b | a: expected s = 0, t = 1/lc(b)"
    if deg(S) >= deg(B) - deg(G):
        return f"deg s = {deg(S)} >= deg b - deg g = {deg(B) - deg(G)}"
    if deg(A) > deg(G) and deg(T) >= deg(A) - deg(G):
        return f"deg t = {deg(T)} >= deg a - deg g = {deg(A) - deg(G)}"
    if deg(A) == deg(G) and T:
        return "a | b: expected t = 0"
    return ""
