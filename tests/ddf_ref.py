"""TEST INFRASTRUCTURE — an exact CPU model of ecfft_poly_squarefree and ecfft_poly_distinct_degree, for
tests/test_gpu_polyddf.py and tests/test_ddf_ref_host.py.

Imports only the standard library, tests/gcd_ref.py (trim, divmod_school), tests/powmod_ref.py (_conv) and tests/roots_ref.py
(monic, gcd, pow_mod).  Polynomials are lists of Python ints, low to high; every function takes the prime p itself, so that the
model can be compared with brute-force trial division at primes small enough to list every irreducible.

- squarefree_part: the monic f / gcd(f, f'); asserts p > deg f, so that f' = 0 only for constants (no p-th-power case).
- ddf: {d: g_d}, g_d the monic product of the irreducible factors of degree d of f.  The Frobenius iterates are plain repeated
  powers h_(i+1) = h_i^p mod s, which owes nothing to modular composition (the GPU's other route).  The reference's
  distinct_degree_factors (src/utils.rs:63) takes pow_mod(x^p, i) = x^(p i) instead of x^(p^i); the two agree at i = 1 only.
  Once deg f* < 2(i + 1), what is left of f* is irreducible of its own degree.
- pack / unpack: the layout of the C ABI: `degrees` (nd entries, degrees[d-1] = deg g_d; the zero polynomial: -1, 0, ...) and
  `factors` (nd entries: the g_d of positive degree in ascending d, each as its low deg g_d coefficients, then zeros).
- binomial_irreducible(n, a, p): x^n - a is irreducible over F_p iff for every prime q | n: q | p - 1 and a^((p-1)/q) != 1, and,
  when 4 | n, p = 1 mod 4 (Lidl-Niederreiter 3.75).  Both fields have p = 3 mod 4, so 4 | n never is.
- product: prod of int-list polynomials by a product tree.
"""
import gcd_ref as G
import powmod_ref as W
import roots_ref as RR


def derivative(f, p):
    return G.trim([j * f[j] % p for j in range(1, len(f))])


def squarefree_part(f, p):
    """the monic f / gcd(f, f'); [1] for a non-zero constant, None for the zero polynomial"""
    f = G.trim([v % p for v in f])
    if not f:
        return None
    assert p > len(f) - 1, "the model has no p-th-power case"
    if len(f) == 1:
        return [1]
    f = RR.monic(f, p)
    g = RR.gcd(f, derivative(f, p), p)
    q, r = G.divmod_school(f, g, p)
    assert not r and q[-1] == 1
    return q


def ddf(f, p):
    """{d: g_d} over the degrees with deg g_d > 0; {} for a non-zero constant, None for the zero polynomial"""
    s = squarefree_part(f, p)
    if s is None:
        return None
    out, fs, i = {}, s, 1
    h = None
    while len(fs) - 1 >= 2 * i:
        h = RR.pow_mod([0, 1], p, s, p) if h is None else RR.pow_mod(h, p, s, p)     # x^(p^i) mod s
        g = RR.gcd(fs, RR._sub(h, [0, 1], p), p)                  # h = x: the gcd with 0 is f* itself
        if len(g) > 1:
            out[i] = g
            fs, r = G.divmod_school(fs, g, p)
            assert not r
        i += 1
    if len(fs) > 1:
        out[len(fs) - 1] = fs
    return out


def pack(factors, nd):
    """(factors row, degrees row), nd entries each, of a ddf() result (None: the zero polynomial)"""
    degrees, row = [0] * nd, []
    if factors is None:
        degrees[0] = -1
    else:
        for d in sorted(factors):
            g = factors[d]
            assert g[-1] == 1 and (len(g) - 1) % d == 0
            degrees[d - 1] = len(g) - 1
            row += g[:-1]
    assert len(row) <= nd
    return row + [0] * (nd - len(row)), degrees


def unpack(row, degrees):
    """the inverse of pack: {d: g_d with its leading 1}, None for the zero polynomial"""
    if degrees[0] < 0:
        return None
    out, pos = {}, 0
    for d, n in enumerate(degrees, 1):
        if n > 0:
            out[d] = list(row[pos:pos + n]) + [1]
            pos += n
    return out


def _prime_divisors(n):
    out, q = [], 2
    while q * q <= n:
        if n % q == 0:
            out.append(q)
            while n % q == 0:
                n //= q
        q += 1
    if n > 1:
        out.append(n)
    return out


def binomial_irreducible(n, a, p):
    a %= p
    if n < 1 or a == 0:
        return False
    if n == 1:
        return True
    if n % 4 == 0 and p % 4 != 1:
        return False
    return all((p - 1) % q == 0 and pow(a, (p - 1) // q, p) != 1 for q in _prime_divisors(n))


def binomial(n, a, p):
    """x^n - a"""
    return [-a % p] + [0] * (n - 1) + [1]


def irreducible_binomials(n, count, p, start=2):
    """the first `count` values a >= start with x^n - a irreducible, as polynomials"""
    out, a = [], start
    while len(out) < count:
        if binomial_irreducible(n, a, p):
            out.append(binomial(n, a, p))
        a += 1
    return out


def product(polys, p):
    level = [list(q) for q in polys]
    if not level:
        return [1]
    while len(level) > 1:
        nxt = [W._conv(level[i], level[i + 1], p) for i in range(0, len(level) - 1, 2)]
        if len(level) & 1:
            nxt.append(level[-1])
        level = nxt
    return level[0]
