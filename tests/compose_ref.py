"""TEST INFRASTRUCTURE — exact CPU references of poly_compose_mod, for tests/test_gpu_polycompose.py and
tests/test_polycompose_host.py.

Imports only numpy, the standard library, tests/poly_ref.py and tests/powmod_ref.py.

- compose_mod: f(g) mod h by Horner's scheme on STANDARD-form arrays, every product the Kronecker product poly_ref.mul_exact reduced by
  powmod_ref.Barrett (one reciprocal per modulus).
- horner_long_division: the same on lists of ints with schoolbook long division — shares nothing with Barrett.
- chunking / brent_kung_model: the baby-step / giant-step schedule of the GPU's large regime restated on lists of ints: k =
  ceil(sqrt(nf)), k' = ceil(nf / k), the table B_t = g^t for t = 0 .. k, the chunk sums C_i = sum_t f[i k + t] B_t with a ragged last
  chunk, then res = C_(k'-1) and res = res B_k + C_i downwards.  It counts its modular products.
"""
import numpy as np

import poly_ref as R
import powmod_ref as W

P = R.P


def _add_const(field, res, c):
    """res[0] += c (standard form, one coefficient array c of length 1), in place"""
    p = P[field]
    if field == "m31":
        res[0] = np.uint32((int(res[0]) + int(c[0])) % p)
    else:
        res[0] = R.from_ints(field, [(R.to_ints(field, res[:1])[0] + R.to_ints(field, c)[0]) % p])[0]
    return res


def compose_mod(field, f, g, h, B=None):
    """f(g) mod h: d = len(h) - 1 coefficients.  B: a Barrett(field, h) to reuse"""
    B = B or W.Barrett(field, h)
    f = np.ascontiguousarray(f, R.dtype(field))
    gr = B.reduce(np.ascontiguousarray(g, R.dtype(field)))
    nf = f.shape[0]
    res = W._pad(field, f[nf - 1:nf], B.d)
    for i in range(nf - 2, -1, -1):
        res = B.reduce(R.mul_exact(field, res, gr))
        _add_const(field, res, f[i:i + 1])
    return res


def horner_long_division(f, g, h, p):
    """f(g) mod h on lists of ints: Horner with a schoolbook product and long division per coefficient"""
    d = len(h) - 1
    gr = W.long_division_rem(g, h, p)
    res = [f[-1] % p] + [0] * (d - 1)
    for c in reversed(f[:-1]):
        res = W.long_division_rem(W._conv(res, gr, p), h, p)
        res[0] = (res[0] + c) % p
    return res


def chunking(nf):
    """(k, k') = (ceil(sqrt(nf)), ceil(nf / k))"""
    k = 1
    while k * k < nf:
        k += 1
    return k, (nf + k - 1) // k


def brent_kung_model(f, g, h, p, stats=None):
    """f(g) mod h as the large regime schedules it; stats (a dict) receives the count of modular products"""
    d = len(h) - 1
    nf = len(f)
    k, kp = chunking(nf)
    products = 0
    gr = W.long_division_rem(g, h, p)
    mulmod = lambda x, y: W.long_division_rem(W._conv(x, y, p), h, p)
    B = [[1 % p] + [0] * (d - 1), gr]                         # B_0 = 1, B_1 = g
    top = k if kp > 1 else k - 1                              # B_k is the giant step: only a second chunk reads it
    for t in range(1, top):
        B.append(mulmod(B[t], gr))
        products += 1
    C = []
    for i in range(kp):
        row = [0] * d
        for t in range(k):
            if i * k + t < nf:                                # the last chunk may be ragged
                c = f[i * k + t]
                row = [(r + c * b) % p for r, b in zip(row, B[t])]
        C.append(row)
    res = C[kp - 1]
    for i in range(kp - 2, -1, -1):
        res = [(x + y) % p for x, y in zip(mulmod(res, B[k]), C[i])]
        products += 1
    if stats is not None:
        stats.update(k=k, kp=kp, products=products)
    return res
