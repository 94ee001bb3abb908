"""TEST INFRASTRUCTURE — exact CPU references of poly_pow_mod / poly_mul_mod, for tests/test_gpu_polypowmod.py and
tests/test_powmod_ref_host.py.

Imports only numpy, the standard library and tests/poly_ref.py (its Kronecker product mul_exact).  Everything works on STANDARD-form
arrays in the element layout of the field, as poly_ref does.

- Barrett: the reciprocal of the reversed modulus by Newton steps on Kronecker products, computed once per modulus; reduce() is then
  two products and a subtraction.  pow_mod / mul_mod are built on it (left-to-right square-and-multiply, utils::pow_mod).
- check_pow_mod / check_mul_mod: the comparisons as jobs of a process pool ("" when the result is right, else a message).
- from_roots: prod (x - r_i) by a product tree.
- pow_repeated: a^e by e - 1 products, each reduced by schoolbook long division — shares nothing with Barrett but mul_exact.
- exp_bits / exp_from_bytes: the exponent as the C ABI reads it (little-endian bytes, high zero bytes ignored).
- fused_step_model: the three-product modular step of the GPU's large regime restated on lists of ints (lengths 2d - 1, d - 1 and d,
  with the reversals), for a check against long division at a small prime.
"""
import numpy as np

import poly_ref as R

P = R.P


# ---- element-wise helpers on standard-form arrays --------------------------------------------------------------------------------------
def _sub(field, x, y):
    p = P[field]
    if field == "m31":
        return ((x.astype(np.uint64) + np.uint64(p) - y.astype(np.uint64)) % np.uint64(p)).astype(np.uint32)
    return R.from_ints(field, [(a - b) % p for a, b in zip(R.to_ints(field, x), R.to_ints(field, y))])


def _zeros(field, n):
    return np.zeros(R.shape(field, n), R.dtype(field))


def _pad(field, x, n):
    """the first n coefficients of x, zero-padded"""
    out = _zeros(field, n)
    k = min(n, x.shape[0])
    out[:k] = x[:k]
    return out


def const(field, v, n):
    """the constant polynomial v as n coefficients"""
    out = _zeros(field, n)
    if n:
        out[0] = R.from_ints(field, [v % P[field]])[0]
    return out


def inv_series(field, f, k):
    """1/f mod x^k (f[0] != 0) by Newton steps g' = g (2 - f g) on exact products"""
    p = P[field]
    g = R.from_ints(field, [pow(R.to_ints(field, f[:1])[0], p - 2, p)])
    n = 1
    while n < k:
        n2 = min(2 * n, k)
        t = _pad(field, R.mul_exact(field, _pad(field, f, n2), g), n2)
        u = _sub(field, const(field, 2, n2), t)
        g = _pad(field, R.mul_exact(field, g, u), n2)
        n = n2
    return g


class Barrett:
    """reduction modulo f (nm = d + 1 coefficients, f[d] != 0) of anything below 2d coefficients with one reciprocal"""

    def __init__(self, field, f):
        self.field, self.f, self.d = field, np.ascontiguousarray(f, R.dtype(field)), f.shape[0] - 1
        assert self.d >= 1 and R.to_ints(field, f[-1:])[0] != 0
        self._g, self._memo = {}, {}

    def recip(self, nq):
        """1/rev(f) mod x^nq"""
        if nq not in self._g:
            self._g[nq] = inv_series(self.field, _pad(self.field, self.f[::-1], nq), nq)
        return self._g[nq]

    def reduce(self, c):
        """c mod f as d coefficients"""
        field, d = self.field, self.d
        nq = c.shape[0] - d
        if nq <= 0:
            return _pad(field, c, d)
        g = self.recip(nq)
        q = _pad(field, R.mul_exact(field, np.ascontiguousarray(c[::-1][:nq]), g), nq)[::-1]      # rev(rev(c) g mod x^nq)
        m = min(nq, d)
        fq = _pad(field, R.mul_exact(field, self.f[:d], np.ascontiguousarray(q[:m])), d)
        return _sub(field, _pad(field, c, d), fq)

    def mul(self, x, y):
        """x y mod f; the last few products are remembered (a scan that repeats the prefix of an earlier one costs nothing)"""
        key = (x.tobytes(), y.tobytes())
        if key not in self._memo:
            if len(self._memo) >= 8:
                self._memo.pop(next(iter(self._memo)))
            self._memo[key] = self.reduce(R.mul_exact(self.field, x, y))
        return self._memo[key]


def mul_mod(field, a, b, f):
    return Barrett(field, f).mul(a, b)


def pow_mod(field, a, e, f, B=None):
    """a^e mod f, left to right from the top set bit (utils::pow_mod, src/utils.rs:194-211); d coefficients.  B: a Barrett(field, f)
    to reuse (its reciprocal is the expensive part at large sizes)"""
    B = B or Barrett(field, f)
    if e == 0:
        return const(field, 1, B.d)
    base = B.reduce(np.ascontiguousarray(a, R.dtype(field)))
    res = base
    for bit in bin(e)[3:]:
        res = B.mul(res, res)
        if bit == "1":
            res = B.mul(res, base)
    return res


def check_pow_mod(field, a, f, exps, outs):
    """outs[i] == a^exps[i] mod f for every exponent (one Barrett, so one reciprocal, for all of them)"""
    B = Barrett(field, f)
    for e, got in zip(exps, outs):
        bad = R._noncanonical(field, [("a^e mod f", got)]) or R._first_diff(field, got, pow_mod(field, a, e, f, B), f"a^{e} mod f")
        if bad:
            return bad
    return ""


def check_mul_mod(field, a, b, f, out):
    """out == a b mod f"""
    return R._noncanonical(field, [("a b mod f", out)]) or R._first_diff(field, out, mul_mod(field, a, b, f), "a b mod f")


def from_roots(field, roots):
    """prod (x - r_i) for a standard-form array of roots: len(roots) + 1 coefficients, monic"""
    p = P[field]
    level = [R.from_ints(field, [(-r) % p, 1]) for r in R.to_ints(field, roots)]
    while len(level) > 1:
        nxt = [R.mul_exact(field, level[i], level[i + 1]) for i in range(0, len(level) - 1, 2)]
        if len(level) & 1:
            nxt.append(level[-1])
        level = nxt
    return level[0]


# ---- independent of Barrett: long division -------------------------------------------------------------------------------------------
def long_division_rem(a, b, p):
    """a mod b on lists of ints (b[-1] != 0): len(b) - 1 coefficients"""
    nb, nq = len(b), max(len(a) - len(b) + 1, 0)
    r = np.array(a, dtype=object)
    bb = np.array(b, dtype=object)
    inv = pow(b[-1], p - 2, p)
    for i in range(nq - 1, -1, -1):
        c = int(r[i + nb - 1]) * inv % p
        if c:
            r[i:i + nb] = (r[i:i + nb] - c * bb) % p
    rem = [int(x) % p for x in r[:nb - 1]] + [0] * max(nb - 1 - len(a), 0)
    return rem[:nb - 1]


def pow_repeated(field, a, e, f):
    """a^e mod f by e - 1 products with a, each reduced by long division"""
    p, d = P[field], f.shape[0] - 1
    fi = R.to_ints(field, f)
    if e == 0:
        return const(field, 1, d)
    base = R.from_ints(field, long_division_rem(R.to_ints(field, a), fi, p))
    res = base
    for _ in range(e - 1):
        res = R.from_ints(field, long_division_rem(R.to_ints(field, R.mul_exact(field, res, base)), fi, p))
    return res


# ---- the exponent as the C ABI reads it ------------------------------------------------------------------------------------------------
def exp_bits(b):
    """little-endian exponent bytes -> (number of bits up to the top set one, bytes that hold them); high zero bytes do not count"""
    n = len(b)
    while n and b[n - 1] == 0:
        n -= 1
    if n == 0:
        return 0, 0
    nbits = 8 * n
    while not (b[(nbits - 1) >> 3] >> ((nbits - 1) & 7)) & 1:
        nbits -= 1
    return nbits, n


def exp_from_bytes(b):
    nbits, _ = exp_bits(b)
    return sum(((b[i >> 3] >> (i & 7)) & 1) << i for i in range(nbits))


def scan(b):
    """the squarings ('S') and multiplies ('M') of the left-to-right scan of the exponent bytes b"""
    nbits, _ = exp_bits(b)
    ops = []
    for i in range(nbits - 2, -1, -1):
        ops.append("S")
        if (b[i >> 3] >> (i & 7)) & 1:
            ops.append("M")
    return "".join(ops)


# ---- the fused step on lists --------------------------------------------------------------------------------------------------------
def _conv(x, y, p):
    if not x or not y:
        return []
    return [int(v) % p for v in np.convolve(np.array(x, dtype=object), np.array(y, dtype=object))]


def reciprocal_list(f, k, p):
    """1/f mod x^k by the schoolbook recurrence"""
    g = [0] * k
    if k:
        g[0] = pow(f[0], p - 2, p)
    for j in range(1, k):
        s = sum(f[i] * g[j - i] for i in range(1, min(j, len(f) - 1) + 1))
        g[j] = -g[0] * s % p
    return g


def fused_step_model(x, y, f, p):
    """x y mod f (x, y: d coefficients, f: d + 1) as the large regime computes it: g = 1/rev(f) mod x^(d-1);
       c = x y (2d - 1); t = rev(c) mod x^(d-1) = c[2d-2-j]; u = t g; q[j] = u[d-2-j] for j < d - 1; res = c[:d] - ((f mod x^d) q)[:d]"""
    d = len(f) - 1
    assert len(x) == d and len(y) == d and d >= 2
    g = reciprocal_list([f[d - j] for j in range(d - 1)], d - 1, p)
    c = _conv(x, y, p)
    assert len(c) == 2 * d - 1
    t = [c[2 * d - 2 - j] for j in range(d - 1)]
    u = _conv(t, g, p)
    assert len(u) == max(2 * d - 3, 0)
    q = [u[d - 2 - j] for j in range(d - 1)]
    w = _conv(f[:d], q, p)
    assert len(w) == (2 * d - 2 if q else 0)
    w += [0] * (d - len(w))
    return [(c[j] - w[j]) % p for j in range(d)]
