"""TEST INFRASTRUCTURE — an exact CPU restatement of ecfft_division_polynomial and ecfft_curve_trace_mod, and of the CRT over
their residues that the C ABI does not have yet (Schoof's algorithm, examples/schoofs.rs of the reference), for
tests/test_gpu_schoof.py and tests/test_schoof_ref_host.py.

Imports only the standard library.  Polynomials are lists of Python ints, low to high, trimmed; every function takes the prime p.

- L(n): the number of coefficients of psi_n in the reference's convention (the factor 2y of an even index removed).
- divpoly(n, A, B, p): psi_n, NOT monic, memoised over the O(log n) indices the recurrence reaches.
- trace_mod(A, B, l, p, stats): t mod l with #E = p + 1 - t; -1 for a singular curve.  The order of operations is the GPU
  kernel's: per attempt on a modulus h (psi_l made monic at first) pi = (x^p, f^((p-1)/2) y), pi^2, Q = [p mod l](x, y) by
  repeated addition of (x, y), E = pi^2 + Q, then j pi for j = 1, 2, ... by repeated addition of pi, compared with E.  A
  denominator that is not invertible replaces h by the proper factor gcd(denominator, h) and the attempt starts over; equal a
  with b1 != +-b2 splits on gcd(b1 - b2, h), else gcd(b1 + b2, h).  There is no degree-1 shortcut.  stats (a dict, optional)
  counts 'splits', 'infinity' (E = O), 'deg1' (an attempt that ran on a modulus of degree 1) and lists the 'degrees' met.
- primes_for(p): 2, 3, 5, ... until the product exceeds 4 sqrt(p).
- cardinality(A, B, p): (#E, [t mod l ...]) by the incremental CRT of schoofs.rs:52-70; 0 for a singular curve.
- ec_add / ec_mul: the affine group law on y^2 = x^3 + A x + B (None = O), for N P = O and for psi_n's defining property.
- from_find_curve(a, bb, p): y^2 = x (x^2 + a x + bb) as (A, B) by x -> x - a/3.
"""
import math

P = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}
SECP256K1_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SMALL_MAX = 65          # ECFFT_SCHOOF_SMALL_MAX: coefficients of a modulus that one workgroup finishes


def trim(v):
    v = list(v)
    while v and v[-1] == 0:
        v.pop()
    return v


def add(x, y, p):
    n = max(len(x), len(y))
    return trim([((x[i] if i < len(x) else 0) + (y[i] if i < len(y) else 0)) % p for i in range(n)])


def sub(x, y, p):
    n = max(len(x), len(y))
    return trim([((x[i] if i < len(x) else 0) - (y[i] if i < len(y) else 0)) % p for i in range(n)])


def scale(x, c, p):
    return trim([v * c % p for v in x])


def mul(x, y, p):
    if not x or not y:
        return []
    out = [0] * (len(x) + len(y) - 1)
    for i, a in enumerate(x):
        if a:
            for j, b in enumerate(y):
                out[i + j] += a * b
    return trim([v % p for v in out])


def divmod_(a, b, p):
    a = [v % p for v in a]
    b = trim(b)
    assert b
    db = len(b) - 1
    inv = pow(b[-1], -1, p)
    q = [0] * max(len(a) - db, 0)
    for k in range(len(a) - 1 - db, -1, -1):
        c = a[k + db] * inv % p
        q[k] = c
        if c:
            for j in range(db + 1):
                a[k + j] = (a[k + j] - c * b[j]) % p
    return trim(q), trim(a[:db])


def rem(a, b, p):
    return divmod_(a, b, p)[1]


def monic(f, p):
    f = trim(f)
    return scale(f, pow(f[-1], -1, p), p)


def mulmod(x, y, h, p):
    return rem(mul(x, y, p), h, p)


def powmod(base, e, h, p):
    res = rem([1], h, p)
    base = rem(base, h, p)
    for bit in bin(e)[2:]:
        res = mulmod(res, res, h, p)
        if bit == "1":
            res = mulmod(res, base, h, p)
    return res


def xgcd_inv(a, h, p):
    """(g, s): the monic g = gcd(a, h) and s with s a = g mod h."""
    r0, r1 = trim(h), rem(a, h, p)
    s0, s1 = [], [1]
    while r1:
        q, r = divmod_(r0, r1, p)
        r0, r1 = r1, r
        s0, s1 = s1, sub(s0, mul(q, s1, p), p)
    c = pow(r0[-1], -1, p)
    return scale(r0, c, p), rem(scale(s0, c, p), h, p)


def gcd(a, b, p):
    a, b = trim(a), trim(b)
    while b:
        a, b = b, rem(a, b, p)
    return monic(a, p) if a else []


# ---- division polynomials --------------------------------------------------------------------
def L(n):
    if n < 2:
        return 1
    return (n * n - 1) // 2 + 1 if n & 1 else (n * n - 4) // 2 + 1


def divpoly_indices(n):
    """the indices the recurrence reaches from n, ascending (the base cases 0 .. 4 included where reached)"""
    seen, todo = set(), [n]
    while todo:
        k = todo.pop()
        if k in seen:
            continue
        seen.add(k)
        if k > 4:
            m = k // 2
            todo += [m - 1, m, m + 1, m + 2] + ([m - 2] if k % 2 == 0 else [])
    return sorted(seen)


def divpoly(n, A, B, p, memo=None):
    memo = {} if memo is None else memo
    f = [B % p, A % p, 0, 1]
    ff16 = scale(mul(f, f, p), 16, p)
    for k in divpoly_indices(n):
        if k in memo:
            continue
        if k == 0:
            v = []
        elif k <= 2:
            v = [1]
        elif k == 3:
            v = [-A * A % p, 12 * B % p, 6 * A % p, 0, 3]
        elif k == 4:
            v = [(-2 * A**3 - 16 * B * B) % p, -8 * A * B % p, -10 * A * A % p, 40 * B % p, 10 * A % p, 0, 2]
        else:
            m = k // 2
            if k % 2 == 0:
                t0 = mul(mul(memo[m - 1], memo[m - 1], p), memo[m + 2], p)
                t1 = mul(mul(memo[m + 1], memo[m + 1], p), memo[m - 2], p)
                v = mul(sub(t0, t1, p), memo[m], p)
            else:
                t0 = mul(memo[m + 2], mul(mul(memo[m], memo[m], p), memo[m], p), p)
                t1 = mul(memo[m - 1], mul(mul(memo[m + 1], memo[m + 1], p), memo[m + 1], p), p)
                v = sub(mul(ff16, t0, p), t1, p) if m % 2 == 0 else sub(t0, mul(ff16, t1, p), p)
        memo[k] = trim(v)
    return memo[n]


# ---- the affine group law on points of the field -----------------------------------------------
def ec_add(P1, P2, A, p):
    if P1 is None:
        return P2
    if P2 is None:
        return P1
    (x1, y1), (x2, y2) = P1, P2
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        m = (3 * x1 * x1 + A) * pow(2 * y1, -1, p) % p
    else:
        m = (y1 - y2) * pow(x1 - x2, -1, p) % p
    x3 = (m * m - x1 - x2) % p
    return x3, (m * (x1 - x3) - y1) % p


def ec_mul(n, Pt, A, p):
    res = None
    while n:
        if n & 1:
            res = ec_add(res, Pt, A, p)
        Pt = ec_add(Pt, Pt, A, p)
        n >>= 1
    return res


def sqrt_mod(v, p):
    """a square root of v for p = 3 mod 4, or None"""
    assert p % 4 == 3
    r = pow(v, (p + 1) // 4, p)
    return r if r * r % p == v % p else None


def from_find_curve(a, bb, p):
    """y^2 = x (x^2 + a x + bb) -> (A, B) of y^2 = x^3 + A x + B under x -> x - a/3"""
    i3, i27 = pow(3, -1, p), pow(27, -1, p)
    return (bb - a * a * i3) % p, (2 * a**3 * i27 - a * bb * i3) % p


# ---- Schoof ------------------------------------------------------------------------------------
class Split(Exception):
    def __init__(self, g):
        self.g = g


def _endo_add(P1, P2, h, f, A, p):
    """(a1, b1 y) + (a2, b2 y) in F_p[x]/(h); None = the point at infinity; raises Split(proper monic factor of h)"""
    (a1, b1), (a2, b2) = P1, P2
    dh = len(h) - 1
    if a1 == a2:
        if not add(b1, b2, p):
            return None
        if b1 == b2:
            num = add(scale(mulmod(a1, a1, h, p), 3, p), [A % p], p)
            den = scale(mulmod(f, b1, h, p), 2, p)
        else:
            for e in (sub(b1, b2, p), add(b1, b2, p)):
                g = gcd(e, h, p)
                if 0 < len(g) - 1 < dh:
                    raise Split(g)
            raise AssertionError("equal a, b1 != +-b2, and neither difference splits the modulus")
    else:
        num, den = sub(b1, b2, p), sub(a1, a2, p)
    g, inv = xgcd_inv(den, h, p)
    if len(g) - 1 > 0:
        assert len(g) - 1 < dh
        raise Split(g)
    r = mulmod(num, inv, h, p)
    a3 = sub(sub(mulmod(mulmod(r, r, h, p), f, h, p), a1, p), a2, p)
    b3 = sub(mulmod(r, sub(a1, a3, p), h, p), b1, p)
    return a3, b3


def _attempt(h, A, B, l, p, stats):
    x = rem([0, 1], h, p)
    f = rem([B % p, A % p, 0, 1], h, p)
    pa = powmod(x, p, h, p)
    pb = powmod(f, (p - 1) // 2, h, p)
    ea = powmod(pa, p, h, p)
    eb = mulmod(powmod(pb, p, h, p), pb, h, p)
    one = rem([1], h, p)
    Q = (x, one)
    for _ in range(p % l - 1):
        Q = _endo_add(Q, (x, one), h, f, A, p)
        assert Q is not None
    E = _endo_add((ea, eb), Q, h, f, A, p)
    if E is None:
        stats["infinity"] += 1
        return 0
    Pj = (pa, pb)
    for j in range(1, l):
        if Pj == E:
            return j
        if j + 1 < l:
            Pj = _endo_add(Pj, (pa, pb), h, f, A, p)
            if Pj is None:
                break
    return 0


def new_stats():
    return {"splits": 0, "infinity": 0, "deg1": 0, "degrees": []}


def is_singular(A, B, p):
    return (4 * A**3 + 27 * B * B) % p == 0


def is_odd_prime(l):
    return l >= 3 and l % 2 == 1 and all(l % q for q in range(3, int(math.isqrt(l)) + 1, 2))


def trace_mod(A, B, l, p, stats=None):
    stats = new_stats() if stats is None else stats
    if is_singular(A, B, p):
        return -1
    f = [B % p, A % p, 0, 1]
    if l == 2:
        xp = powmod([0, 1], p, f, p)
        return 0 if len(gcd(sub(xp, [0, 1], p), f, p)) > 1 else 1
    assert is_odd_prime(l)
    h = monic(divpoly(l, A, B, p), p)
    while True:
        stats["degrees"].append(len(h) - 1)
        if len(h) - 1 == 1:
            stats["deg1"] += 1
        try:
            return _attempt(h, A, B, l, p, stats)
        except Split as s:
            stats["splits"] += 1
            assert 0 < len(s.g) - 1 < len(h) - 1
            h = s.g


def primes_for(p):
    m, out, l = 1, [], 2
    while m * m <= 16 * p:                 # until the product exceeds 4 sqrt(p), exactly
        if l == 2 or is_odd_prime(l):
            out.append(l)
            m *= l
        l += 1
    return out


def crt(residues, primes):
    t, m = 0, 1
    for r, l in zip(residues, primes):
        t = (t + m * ((r - t) * pow(m, -1, l) % l)) % (m * l)
        m *= l
    return t - m if t > m // 2 else t


def cardinality(A, B, p, stats=None):
    if is_singular(A, B, p):
        return 0, []
    primes = primes_for(p)
    tr = [trace_mod(A, B, l, p, stats) for l in primes]
    return p + 1 - crt(tr, primes), tr
