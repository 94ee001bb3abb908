"""The three-core EXIT level, proved with Python integers and nothing of the library.

One EXIT level takes the evaluations of P (deg P < n) on S = S0 u S1 (|S0| = |S1| = m = n/2) to the evaluations on S0 of
U = P mod X^m and V = P div X^m.  The level driver runs the Montgomery reduction over Z1, the vanishing polynomial of S1:

    core 1   t1 = e1/a1 on S1            --EXTEND S1->S0-->  g0        a = X^m on S
             h0 = (e0 - g0 a0)/Z1 on S0
    core 2   h0                          --EXTEND S0->S1-->  h1
    core 3   t1' = h1 C'1/a1 on S1       --EXTEND S1->S0-->  g0'       C' = Z1^2 mod X^m
             u0 = (h0 C'0 - g0' a0)/Z1 on S0
             v0 = (e0 - u0)/a0 on S0

EXTEND here is plain Lagrange interpolation (the interpolant of degree < m through m values, evaluated on the other moiety), so
the test shares no code and no table with the library; it runs over the secp256k1 prime and over 2^31 - 1.
"""
import random

import pytest

P_SECP = 2**256 - 2**32 - 977
P_M31 = 2**31 - 1


def inv(a, p):
    return pow(a % p, p - 2, p)


def poly_eval(c, x, p):
    r = 0
    for a in reversed(c):
        r = (r * x + a) % p
    return r


def poly_mul(a, b, p):
    r = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] = (r[i + j] + x * y) % p
    return r


def extend(vals, src, dst, p):
    """values on `src` of a polynomial of degree < len(src) -> its values on `dst` (Lagrange)"""
    out = []
    for t in dst:
        acc = 0
        for j, xj in enumerate(src):
            num = den = 1
            for k, xk in enumerate(src):
                if k != j:
                    num = num * (t - xk) % p
                    den = den * (xj - xk) % p
            acc = (acc + vals[j] * num % p * inv(den, p)) % p
        out.append(acc)
    return out


def exit_level_three_cores(e0, e1, S0, S1, p):
    m = len(S0)
    a0 = [pow(x, m, p) for x in S0]
    a1 = [pow(x, m, p) for x in S1]
    z1 = [1]
    for s in S1:
        z1 = poly_mul(z1, [(-s) % p, 1], p)
    z1_s0_inv = [inv(poly_eval(z1, x, p), p) for x in S0]
    cc = poly_mul(z1, z1, p)[:m]                                    # C' = Z1^2 mod X^m
    c0 = [poly_eval(cc, x, p) for x in S0]
    c1 = [poly_eval(cc, x, p) for x in S1]
    # core 1
    g0 = extend([e * inv(a, p) % p for e, a in zip(e1, a1)], S1, S0, p)
    h0 = [(e - g * a) * zi % p for e, g, a, zi in zip(e0, g0, a0, z1_s0_inv)]
    # core 2
    h1 = extend(h0, S0, S1, p)
    # core 3
    g0p = extend([h * c % p * inv(a, p) % p for h, c, a in zip(h1, c1, a1)], S1, S0, p)
    u0 = [(h * c - g * a) * zi % p for h, c, g, a, zi in zip(h0, c0, g0p, a0, z1_s0_inv)]
    v0 = [(e - u) * inv(a, p) % p for e, u, a in zip(e0, u0, a0)]
    return u0, v0


def check(p, n, coeffs, rng):
    m = n // 2
    pts = set()
    while len(pts) < n:
        x = rng.randrange(1, p)                                      # distinct and non-zero: the form's requirement
        pts.add(x)
    pts = list(pts)
    rng.shuffle(pts)
    S0, S1 = pts[0::2], pts[1::2]
    e0 = [poly_eval(coeffs, x, p) for x in S0]
    e1 = [poly_eval(coeffs, x, p) for x in S1]
    u0, v0 = exit_level_three_cores(e0, e1, S0, S1, p)
    lo, hi = coeffs[:m], coeffs[m:]
    assert u0 == [poly_eval(lo, x, p) for x in S0]
    assert v0 == [poly_eval(hi, x, p) for x in S0]


@pytest.mark.parametrize("p", [P_SECP, P_M31], ids=["secp256k1", "m31"])
@pytest.mark.parametrize("n", [4, 8, 16])
def test_three_core_level_random(p, n):
    rng = random.Random(1000 * n + p % 997)
    for _ in range(3):
        check(p, n, [rng.randrange(p) for _ in range(n)], rng)


@pytest.mark.parametrize("p", [P_SECP, P_M31], ids=["secp256k1", "m31"])
@pytest.mark.parametrize("n", [4, 8, 16])
def test_three_core_level_full_degree(p, n):
    """deg P = n - 1 exactly: the leading coefficient is non-zero"""
    rng = random.Random(77 * n + p % 991)
    c = [rng.randrange(p) for _ in range(n - 1)] + [rng.randrange(1, p)]
    check(p, n, c, rng)
    check(p, n, [0] * (n - 1) + [1], rng)                            # P = X^(n-1)


@pytest.mark.parametrize("p", [P_SECP, P_M31], ids=["secp256k1", "m31"])
@pytest.mark.parametrize("n", [4, 8, 16])
def test_three_core_level_zero_remainder(p, n):
    """P mod X^m = 0: P = X^m Q"""
    rng = random.Random(31 * n + p % 983)
    m = n // 2
    check(p, n, [0] * m + [rng.randrange(1, p) for _ in range(m)], rng)
    check(p, n, [0] * n, rng)                                        # and P = 0


@pytest.mark.parametrize("p", [P_SECP, P_M31], ids=["secp256k1", "m31"])
def test_three_core_level_low_degree(p):
    """deg P < m: V = 0 and U = P"""
    rng = random.Random(5)
    check(p, 8, [rng.randrange(p) for _ in range(4)] + [0] * 4, rng)
