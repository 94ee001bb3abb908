"""TEST INFRASTRUCTURE — exact CPU references of the polynomial operations (poly_mul, poly_divrem, poly_inv_series), for the tests of
tests/test_gpu_poly_regimes.py and tests/test_poly_ref_host.py.

Imports only numpy and the standard library, so worker processes (spawn) can import it without torch or the GPU library.  Every
function works on STANDARD-form values: numpy arrays in the element layout of the field (secp256k1 uint64[n, 4] little-endian limbs,
m31 uint32[n]) or Python ints.  The test modules convert in-memory (Montgomery) arrays with the oracle before handing them over.

- mul_exact: the product by Kronecker substitution on Python ints (slots of whole bytes wide enough for min(na, nb) (p-1)^2).
- check_mul / check_divrem / check_inv_series: exact checks built on it; each returns "" when the result is right, else a message
  naming the first wrong coefficient.  Every output coefficient must also be canonical (< p).
- sz_mul / sz_divrem / sz_inv_series: Schwartz-Zippel forms of the same identities at seeded points of [0, p), for sizes where the
  exact product is too slow.  `horner(coeffs, zs) -> values` may be passed (the oracle's); the default is horner() below.
- sz_mul_mod: r == x y mod f proved by a witness quotient q: x(z) y(z) == f(z) q(z) + r(z) with len(r) = deg f.
"""
import math

import numpy as np

P = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}
LIMBS = {"secp256k1": 4, "m31": 1}
_P_LIMBS = np.array([(P["secp256k1"] >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


# ---- layout <-> Python ints ----------------------------------------------------------------------------------------------------------
def shape(field, n):
    return (n, 4) if field == "secp256k1" else (n,)


def dtype(field):
    return np.uint64 if field == "secp256k1" else np.uint32


def to_ints(field, a):
    """standard-form array -> list of Python ints"""
    a = np.ascontiguousarray(a, dtype(field))
    if field == "m31":
        return [int(x) for x in a]
    raw = a.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(a.shape[0])]


def from_ints(field, ints):
    """list of Python ints (each in [0, 2^256) / [0, 2^32)) -> standard-form array"""
    if field == "m31":
        return np.array([int(x) for x in ints], dtype=np.uint32).reshape(shape(field, len(ints)))
    raw = b"".join(int(x).to_bytes(32, "little") for x in ints)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(ints), 4).copy()


def canonical(field, a):
    """bool mask of the coefficients < p"""
    a = np.ascontiguousarray(a, dtype(field))
    if field == "m31":
        return a < np.uint32(P["m31"])
    lt = np.zeros(a.shape[0], dtype=bool)
    eq = np.ones(a.shape[0], dtype=bool)
    for l in (3, 2, 1, 0):                                   # lexicographic from the top limb
        lt |= eq & (a[:, l] < _P_LIMBS[l])
        eq &= a[:, l] == _P_LIMBS[l]
    return lt


def _vals(field, a):
    """standard-form array -> values to compute with: uint64 (m31) or an object array of Python ints (secp256k1)"""
    if field == "m31":
        return np.ascontiguousarray(a, np.uint32).astype(np.uint64)
    return np.array(to_ints(field, a) if a.shape[0] else [], dtype=object)


def _from_vals(field, v):
    return v.astype(np.uint32) if field == "m31" else from_ints(field, list(v))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def rand_std(field, n, seed, specials=True):
    """n uniform elements of [0, p) in standard form (secp256k1: uniform 256-bit rows, the rare row >= p redrawn); with specials, 0, 1
    and p - 1 at seeded positions and a few runs of zero coefficients"""
    rng = np.random.default_rng(seed)
    if field == "m31":
        a = rng.integers(0, P["m31"], n, dtype=np.uint32)
    else:
        a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
        while True:
            bad = ~canonical(field, a)
            if not bad.any():
                break
            a[bad] = rng.integers(0, 2**64, size=(int(bad.sum()), 4), dtype=np.uint64)
    if specials and n >= 8:
        pm1 = from_ints(field, [P[field] - 1])[0]
        one = from_ints(field, [1])[0]
        k = max(1, n // 64)
        for v in (0, one, pm1):
            a[rng.integers(0, n, k)] = v
        for _ in range(3):                                   # runs of zero coefficients
            ln = int(rng.integers(1, max(2, min(300, n // 4))))
            s = int(rng.integers(0, n - ln))
            a[s:s + ln] = 0
    return a


def set_nonzero(field, a, idx):
    """a[idx] = 1 where it is 0 (a divisor's leading coefficient, a series' constant term)"""
    idx = np.atleast_1d(idx)
    if field == "m31":
        z = idx[a[idx] == 0]
        a[z] = 1
    else:
        z = idx[(a[idx] == 0).all(axis=1)]
        a[z] = from_ints(field, [1])[0]
    return a


# ---- the exact product ---------------------------------------------------------------------------------------------------------------
def slot_bytes(field, na, nb):
    """bytes per Kronecker slot: every product coefficient (a sum of min(na, nb) products of two values <= p - 1) fits"""
    return ((min(na, nb) * (P[field] - 1) ** 2).bit_length() + 7) // 8


def _pack(field, a, w):
    n = a.shape[0]
    eb = 32 if field == "secp256k1" else 4
    buf = np.zeros((n, w), dtype=np.uint8)
    buf[:, :eb] = np.ascontiguousarray(a).view(np.uint8).reshape(n, eb)
    return int.from_bytes(buf.tobytes(), "little")


def mul_exact(field, a, b):
    """a * b (standard-form arrays of na, nb coefficients) -> standard-form array of na + nb - 1 canonical coefficients"""
    p = P[field]
    na, nb = a.shape[0], b.shape[0]
    nc = na + nb - 1
    w = slot_bytes(field, na, nb)
    c = _pack(field, a, w) * _pack(field, b, w)
    raw = np.frombuffer(c.to_bytes(nc * w, "little"), dtype=np.uint8).reshape(nc, w)
    if field == "m31":                                        # 2^32 = 2 mod p: fold 32-bit words
        w4 = (w + 3) // 4 * 4
        words = np.zeros((nc, w4), dtype=np.uint8)
        words[:, :w] = raw
        words = words.view("<u4").astype(np.uint64)
        acc = np.zeros(nc, dtype=np.uint64)
        for k in range(words.shape[1]):
            acc += (words[:, k] % np.uint64(p)) << np.uint64(k)
        return (acc % np.uint64(p)).astype(np.uint32)
    rb = raw.tobytes()
    return from_ints(field, [int.from_bytes(rb[i * w:(i + 1) * w], "little") % p for i in range(nc)])


def _first_diff(field, got, want, what):
    got = np.ascontiguousarray(got, dtype(field))
    want = np.ascontiguousarray(want, dtype(field))
    if got.shape != want.shape:
        return f"{what}: shape {got.shape} != {want.shape}"
    bad = got != want if field == "m31" else (got != want).any(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        return f"{what}: {int(bad.sum())} coefficients differ, first at {i} of {got.shape[0]}"
    return ""


def _noncanonical(field, arrays):
    for name, x in arrays:
        ok = canonical(field, x)
        if not ok.all():
            return f"{name}: coefficient {int(np.argmin(ok))} is not canonical (>= p)"
    return ""


def check_mul(field, a, b, c):
    """c == a * b coefficient for coefficient (all standard form)"""
    return _noncanonical(field, [("c", c)]) or _first_diff(field, c, mul_exact(field, a, b), "a*b")


def _add_low(field, x, r):
    """x + r (r added to the low len(r) coefficients of x), standard form"""
    if r.shape[0] == 0:
        return x
    xv, rv = _vals(field, x), _vals(field, r)
    xv[:rv.shape[0]] = (xv[:rv.shape[0]] + rv) % (P[field] if field != "m31" else np.uint64(P[field]))
    return _from_vals(field, xv)


def check_divrem(field, a, b, q, r):
    """b q + r == a exactly, with len(q) = na - nb + 1 and len(r) = nb - 1; given deg r < deg b, (q, r) is unique"""
    na, nb = a.shape[0], b.shape[0]
    if q.shape[0] != max(na - nb + 1, 0) or r.shape[0] != nb - 1:
        return f"lengths {q.shape[0]}, {r.shape[0]} for na = {na}, nb = {nb}"
    bad = _noncanonical(field, [("q", q), ("r", r)])
    if bad:
        return bad
    if q.shape[0] == 0:                                        # na < nb: r = a, zero-padded
        want = np.zeros(shape(field, nb - 1), dtype(field))
        want[:na] = a
        return _first_diff(field, r, want, "r (na < nb)")
    return _first_diff(field, _add_low(field, mul_exact(field, b, q), r), a, "b*q + r")


def check_inv_series(field, f, g):
    """the low k = len(g) coefficients of (f mod x^k) g are exactly [1, 0, ..., 0]"""
    k = g.shape[0]
    bad = _noncanonical(field, [("g", g)])
    if bad:
        return bad
    want = np.zeros(shape(field, k), dtype(field))
    want[0] = from_ints(field, [1])[0]
    return _first_diff(field, mul_exact(field, f[:k], g)[:k], want, "(f mod x^k) g mod x^k")


def check_many(kind, field, count, first, *arrays):
    """one exact check ("mul": a, b, c; "divrem": a, b, q, r; "inv_series": f, g) on each of `count` pairs laid end to end in every
    array; pairs are numbered from `first` in the message"""
    fn = {"mul": check_mul, "divrem": check_divrem, "inv_series": check_inv_series}[kind]
    for i in range(count):
        rows = [x[i * (x.shape[0] // count):(i + 1) * (x.shape[0] // count)] for x in arrays]
        bad = fn(field, *rows)
        if bad:
            return f"pair {first + i}: {bad}"
    return ""


# ---- Schwartz-Zippel -----------------------------------------------------------------------------------------------------------------
def sz_count(field, D):
    """points t with (D / p)^t <= 2^-64 for an identity of degree < D"""
    if field == "secp256k1":
        return 2
    return math.ceil(64 / (31 - math.ceil(math.log2(max(D, 2)))))


def sz_points(field, t, seed):
    """t seeded points drawn uniformly from [0, p) (standard form)"""
    return rand_std(field, t, seed, specials=False)


def horner(field, coeffs, zs):
    """coeffs (standard form) at the points zs -> list of Python ints (m31: a power table in numpy; secp256k1: Horner on ints)"""
    p = P[field]
    out = []
    if field == "m31":
        c = np.ascontiguousarray(coeffs, np.uint32).astype(np.uint64)
        for z in to_ints(field, zs):
            pw = _powers_m31(z, c.shape[0])
            out.append(int(((c * pw) % np.uint64(p)).sum() % np.uint64(p)))
        return out
    cs = to_ints(field, coeffs)[::-1]
    for z in to_ints(field, zs):
        acc = 0
        for x in cs:
            acc = (acc * z + x) % p
        out.append(acc)
    return out


def _powers_m31(z, n):
    """z^0 .. z^(n-1) mod p as uint64 (blocks of 1024: a low table times a high table)"""
    p = np.uint64(P["m31"])
    B = 1024
    lo = np.ones(B, dtype=np.uint64)
    for i in range(1, B):
        lo[i] = lo[i - 1] * np.uint64(z) % p
    zb = int(lo[B - 1]) * z % P["m31"]
    nh = (n + B - 1) // B
    hi = np.ones(nh, dtype=np.uint64)
    for i in range(1, nh):
        hi[i] = hi[i - 1] * np.uint64(zb) % p
    return ((hi[:, None] * lo[None, :]) % p).reshape(-1)[:n]


def _powers_int(z, n, p):
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * z % p
    return pw


def sz_mul(field, a, b, c, zs, horner_fn=None):
    """a(z) b(z) == c(z) at every point"""
    h = horner_fn or (lambda x, y: horner(field, x, y))
    p = P[field]
    bad = _noncanonical(field, [("c", c)])
    if bad:
        return bad
    for i, (x, y, w) in enumerate(zip(h(a, zs), h(b, zs), h(c, zs))):
        if x * y % p != w % p:
            return f"a(z) b(z) != c(z) at point {i}"
    return ""


def sz_divrem(field, a, b, q, r, zs, horner_fn=None):
    """a(z) == b(z) q(z) + r(z) at every point; lengths and canonical form asserted separately"""
    h = horner_fn or (lambda x, y: horner(field, x, y))
    p = P[field]
    na, nb = a.shape[0], b.shape[0]
    if q.shape[0] != max(na - nb + 1, 0) or r.shape[0] != nb - 1:
        return f"lengths {q.shape[0]}, {r.shape[0]} for na = {na}, nb = {nb}"
    bad = _noncanonical(field, [("q", q), ("r", r)])
    if bad:
        return bad
    hq = h(q, zs) if q.shape[0] else [0] * len(zs)
    hr = h(r, zs) if r.shape[0] else [0] * len(zs)
    for i, (x, y, u, v) in enumerate(zip(h(a, zs), h(b, zs), hq, hr)):
        if x % p != (y * u + v) % p:
            return f"a(z) != b(z) q(z) + r(z) at point {i}"
    return ""


def sz_mul_mod(field, x, y, f, q, r, zs, horner_fn=None):
    """r == x y mod f, given a witness quotient q: x(z) y(z) == f(z) q(z) + r(z) at every point, with len(r) = len(f) - 1 and a
    nonzero leading coefficient of f.  The identity is one of polynomials of degree < len(x) + len(y) - 1; once it holds, deg r <
    deg f makes r THE remainder, wherever q came from (a wrong q cannot make a wrong r pass: f q + r determines r mod f)."""
    h = horner_fn or (lambda c, z: horner(field, c, z))
    p = P[field]
    nc, nm = x.shape[0] + y.shape[0] - 1, f.shape[0]
    if r.shape[0] != nm - 1 or q.shape[0] != max(nc - nm + 1, 0):
        return f"lengths {q.shape[0]}, {r.shape[0]} for a product of {nc} and nm = {nm}"
    if to_ints(field, f[nm - 1:])[0] == 0:
        return "the leading coefficient of f is zero"
    bad = _noncanonical(field, [("q", q), ("r", r)])
    if bad:
        return bad
    hq = h(q, zs) if q.shape[0] else [0] * len(zs)
    hr = h(r, zs) if r.shape[0] else [0] * len(zs)
    for i, (u, v, w, s, t) in enumerate(zip(h(x, zs), h(y, zs), h(f, zs), hq, hr)):
        if u * v % p != (w * s + t) % p:
            return f"x(z) y(z) != f(z) q(z) + r(z) at point {i}"
    return ""


def sz_inv_series(field, f, g, zs):
    """sum_{j<k} g_j z^j S_{k-j} == 1 with S_t = sum_{l < min(t, nf)} f_l z^l: the z-weighted sum of the coefficients of f g mod x^k,
    a polynomial in z of degree < k.  O(k + nf) per point: one power table and one prefix scan."""
    p = P[field]
    k, nf = g.shape[0], f.shape[0]
    bad = _noncanonical(field, [("g", g)])
    if bad:
        return bad
    n = max(k, min(nf, k))
    for i, z in enumerate(to_ints(field, zs)):
        if field == "m31":
            pp = np.uint64(p)
            pw = _powers_m31(z, n)
            fz = np.ascontiguousarray(f[:k], np.uint32).astype(np.uint64) * pw[:min(nf, k)] % pp
            S = np.concatenate([np.zeros(1, np.uint64), np.cumsum(fz) % pp])           # S[t] = sum_{l < t} f_l z^l (t <= nf)
            t = np.minimum(k - np.arange(k), min(nf, k))
            gz = np.ascontiguousarray(g, np.uint32).astype(np.uint64) * pw[:k] % pp
            tot = int(((gz * S[t]) % pp).sum() % pp)
        else:
            pw = _powers_int(z, n, p)
            fi, gi = to_ints(field, f[:k]), to_ints(field, g)
            S = [0] * (min(nf, k) + 1)
            for l in range(min(nf, k)):
                S[l + 1] = (S[l] + fi[l] * pw[l]) % p
            tot = 0
            for j in range(k):
                tot += gi[j] * pw[j] % p * S[min(k - j, nf)]
            tot %= p
        if tot != 1:
            return f"sum_j g_j z^j S_(k-j) != 1 at point {i}"
    return ""
