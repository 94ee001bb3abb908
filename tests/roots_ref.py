"""TEST INFRASTRUCTURE — an exact CPU restatement of ecfft_poly_find_roots, for tests/test_gpu_polyroots.py and
tests/test_polyroots_host.py.

Imports only the standard library, tests/gcd_ref.py (trim, divmod_school) and tests/powmod_ref.py (_conv).  Polynomials are
lists of Python ints, low to high; every function takes the prime p itself, so that the scheme can be compared with brute-force
evaluation at a prime small enough to try every element.

- linear_part: g = gcd(f, x^p - x mod f), the monic product of the DISTINCT linear factors of f whatever their multiplicities are
  (x^p - x is the squarefree product of all x - a).
- split: one attempt with the shift c on a monic product h of e >= 2 distinct linear factors: w = (x + c)^((p-1)/2) mod h,
  u = gcd(h, w - 1), v = h / u; a success when 0 < deg u < e.  p is odd.
- find_roots: the stack of pending factors of the GPU's leaf kernel: pop a factor; x + a yields -a; otherwise the next shift from
  an attempt counter that starts at 1 and is incremented after every attempt; on success u and v replace h (v on top).  Returns the
  sorted roots and the number of attempts; None for the zero polynomial (every element is a root; the C ABI reports -1).
- legendre_pair: the first pair 2 <= r < s whose shifted values r + c, s + c have EQUAL non-zero Legendre symbols for c = 1 .. nfail and
  different ones at c = nfail + 1: the quadratic (x - r)(x - s) fails exactly the first nfail shifts.
- product: f = k prod (x - r_i)^m_i prod (x^2 + c_j^2); the quadratics are irreducible when p = 3 mod 4.
"""
import gcd_ref as G
import powmod_ref as W

CAP = 64            # consecutive failed shifts of one factor after which the GPU call gives up


def monic(f, p):
    f = G.trim(f)
    c = pow(f[-1], p - 2, p)
    return [v * c % p for v in f]


def rem(a, b, p):
    return G.divmod_school(a, b, p)[1]


def gcd(a, b, p):
    """monic gcd of two int lists, not both zero"""
    a, b = G.trim(a), G.trim(b)
    while b:
        a, b = b, rem(a, b, p)
    return monic(a, p)


def pow_mod(base, e, f, p):
    """base^e mod f, left to right from the top set bit (e >= 1)"""
    base = rem(base, f, p)
    res = base
    for bit in bin(e)[3:]:
        res = rem(W._conv(res, res, p), f, p)
        if bit == "1":
            res = rem(W._conv(res, base, p), f, p)
    return res


def _sub(x, y, p):
    n = max(len(x), len(y))
    return G.trim([((x[i] if i < len(x) else 0) - (y[i] if i < len(y) else 0)) % p for i in range(n)])


def linear_part(f, p):
    """gcd(f, x^p - x mod f) for f != 0 (monic; [1] when f has no root)"""
    f = G.trim(f)
    assert f
    if len(f) == 1:
        return [1]
    return gcd(f, _sub(pow_mod([0, 1], p, f, p), [0, 1], p), p)


def split(h, c, p):
    """(u, v) of one attempt; u = gcd(h, (x + c)^((p-1)/2) - 1 mod h), v = h / u"""
    assert p & 1 and len(h) >= 3 and h[-1] == 1
    w = pow_mod([c % p, 1], (p - 1) // 2, h, p)
    u = gcd(h, _sub(w, [1], p), p)
    v, r = G.divmod_school(h, u, p)
    assert not r
    return u, v


def find_roots(f, p):
    """(sorted distinct roots, attempts), or None for the zero polynomial"""
    f = G.trim(f)
    if not f:
        return None
    stack, roots, c, fails = [linear_part(f, p)], [], 1, 0
    while stack:
        h = stack.pop()
        e = len(h) - 1
        if e == 0:
            continue
        if e == 1:
            roots.append(-h[0] % p)
            continue
        u, v = split(h, c, p)
        c += 1
        if 0 < len(u) - 1 < e:
            fails = 0
            stack += [u, v]
        else:
            fails += 1
            assert fails < CAP, "attempt cap"
            stack.append(h)
    return sorted(roots), c - 1


def legendre(a, p):
    s = pow(a % p, (p - 1) // 2, p)
    return -1 if s == p - 1 else s


def legendre_pair(p, nfail=4, start=2, span=4096):
    """in the order of r, then s: r = start, start + 1, ... (0 and 1 have cases of their own), s in (r, r + span)"""
    r = start
    while True:
        for s in range(r + 1, r + span):
            if all(legendre(r + c, p) == legendre(s + c, p) != 0 for c in range(1, nfail + 1)) and \
                    legendre(r + nfail + 1, p) * legendre(s + nfail + 1, p) == -1:
                return r, s
        r += 1


def product(p, roots_mult, quads, k=1):
    """k prod (x - r)^m prod (x^2 + c^2) for roots_mult = [(r, m), ...] and quads = [c, ...], by a product tree"""
    level = [[-r % p, 1] for r, m in roots_mult for _ in range(m)] + [[c * c % p, 0, 1] for c in quads]
    if not level:
        return [k % p]
    while len(level) > 1:
        nxt = [W._conv(level[i], level[i + 1], p) for i in range(0, len(level) - 1, 2)]
        if len(level) & 1:
            nxt.append(level[-1])
        level = nxt
    return [v * k % p for v in level[0]]
