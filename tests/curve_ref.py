"""TEST INFRASTRUCTURE — Python model of the curve search: the control flow of the reference's find_curve.rs (double_point_x,
half_point_x, roots, fi_roots, cyclic_two_sylow_subgroup, find_curve) restated on Python ints, the candidate stream of
include/ecfft_hip.h, and point arithmetic on y^2 = x(x^2 + a x + bb) for the checks of the tests.

Imports only the standard library.  Everything is a STANDARD-form integer in [0, p).  p = 3 mod 4 throughout, so the square root is
the canonical v^((p+1)/4), accepted when its square is v (0 counts as a square, as sqrt().is_some() does); the two roots of a
quadratic come in the reference's order (-b + s)/2, (-b - s)/2.

`muls` (a one-element list, optional) counts field multiplications the way the device code spends them: an exponentiation is charged
SQRT_MULS[field] plus the squaring that checks it.
"""
P = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}
SQRT_MULS = {"secp256k1": 253 + 13, "m31": 29}
MASK64 = 2**64 - 1
MAX_INDEX = 2**60


# ---- the candidate stream ------------------------------------------------------------------------------------------------------------
def word(seed, c):
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def candidate(field, seed, index):
    """(a, bb) of candidate `index` of stream `seed`"""
    assert 0 <= index < MAX_INDEX
    p = P[field]
    if field == "m31":
        return (word(seed, 8 * index) & 0x7FFFFFFF) % p, (word(seed, 8 * index + 4) & 0x7FFFFFFF) % p
    a = sum(word(seed, 8 * index + j) << (64 * j) for j in range(4)) % p
    bb = sum(word(seed, 8 * index + 4 + j) << (64 * j) for j in range(4)) % p
    return a, bb


# ---- find_curve.rs -------------------------------------------------------------------------------------------------------------------
class _Count:
    def __init__(self, p, muls, sqrt_muls):
        self.p, self.muls, self.sqrt_muls = p, muls, sqrt_muls

    def mul(self, n=1):
        if self.muls is not None:
            self.muls[0] += n

    def sqrt(self, v):
        """Option<F>: the canonical root or None"""
        self.mul(self.sqrt_muls + 1)
        r = pow(v, (self.p + 1) // 4, self.p)
        return r if r * r % self.p == v else None


def _double_point_x_is_none(px, a, bb, p, c):
    c.mul(2)
    return px * (px * px + a * px + bb) % p == 0


def _roots(b, cc, p, c):
    """roots of x^2 + b x + cc"""
    c.mul(1)
    s = c.sqrt((b * b - 4 * cc) % p)
    if s is None:
        return None
    half = (p + 1) // 2
    c.mul(2)
    return [(-b + s) * half % p, (-b - s) * half % p]


def _fi_roots(i, qx, a, bb, p, c):
    c.mul(1)
    ds = c.sqrt((qx * qx + a * qx + bb) % p)
    if ds is None:
        return None
    x_coeff = -(2 * qx + (-1) ** i * 2 * ds) % p
    return _roots(x_coeff, bb, p, c)


def _half_point_x(qx, a, bb, p, c):
    roots = _fi_roots(1, qx, a, bb, p, c)
    if roots is None:
        roots = _fi_roots(2, qx, a, bb, p, c)
    if roots is None:
        return None
    for x in roots:
        c.mul(2)
        if c.sqrt(x * (x * x + a * x + bb) % p) is not None:
            return x
    return None


def two_sylow(a, bb, p, muls=None, sqrt_muls=0):
    """cyclic_two_sylow_subgroup: (n, x); (0, 0) when the 2-Sylow subgroup is not cyclic, bb is no square, or the curve is singular
    (bb = 0 or a zero discriminant, where the reference asserts)"""
    c = _Count(p, muls, sqrt_muls)
    c.mul(1)
    disc = (a * a - 4 * bb) % p
    if bb == 0 or disc == 0:
        return 0, 0
    b = c.sqrt(bb)
    if b is None or c.sqrt(disc) is not None:
        return 0, 0
    if c.sqrt((a + 2 * b) % p) is not None:
        p4x = b
    else:
        assert pow((a - 2 * b) % p, (p - 1) // 2, p) == 1, "unreachable!() in the reference"
        p4x = (-b) % p
    if _double_point_x_is_none(p4x, a, bb, p, c):
        return 1, 0
    k, acc = 2, p4x
    while True:
        x = _half_point_x(acc, a, bb, p, c)
        if x is None:
            return k, acc
        k, acc = k + 1, x


def two_sylow_field(field, a, bb, muls=None):
    return two_sylow(a, bb, P[field], muls, SQRT_MULS[field])


def find_curve(field, k, seed, start=0, max_candidates=1 << 20):
    """the smallest index in the window whose n >= max(k, 2): (index, n, a, bb, x), or None"""
    k = max(k, 2)
    for i in range(start, start + max_candidates):
        a, bb = candidate(field, seed, i)
        n, x = two_sylow_field(field, a, bb)
        if n >= k:
            return i, n, a, bb, x
    return None


# ---- points of y^2 = x (x^2 + a x + bb); None is the identity ------------------------------------------------------------------------
def rhs(x, a, bb, p):
    return x * (x * x + a * x + bb) % p


def sqrt_canon(v, p):
    r = pow(v, (p + 1) // 4, p)
    return r if r * r % p == v else None


def pt_double(pt, a, bb, p):
    if pt is None or pt[1] == 0:
        return None
    x, y = pt
    lam = (3 * x * x + 2 * a * x + bb) * pow(2 * y, -1, p) % p
    x3 = (lam * lam - a - 2 * x) % p
    return x3, (lam * (x - x3) - y) % p


def pt_double_n(pt, times, a, bb, p):
    for _ in range(times):
        pt = pt_double(pt, a, bb, p)
    return pt


def group_order(a, bb, p):
    """number of points, by the Legendre symbol of every right-hand side (small p only)"""
    squares = {x * x % p for x in range(1, p)}
    n = 1
    for x in range(p):
        v = rhs(x, a, bb, p)
        n += 1 if v == 0 else (2 if v in squares else 0)
    return n


def coset_offset(a, bb, n, p):
    """the point with the smallest integer x >= 1 whose y^2 is a non-zero square and whose 2^n multiple is not the identity; (0, 0)
    when n is the bit length of p: by the Hasse bound the group then has exactly 2^n points, all of them multiples of the generator"""
    if n == p.bit_length():
        return 0, 0
    x = 1
    while True:
        v = rhs(x, a, bb, p)
        y = sqrt_canon(v, p) if v else None
        if y is not None and pt_double_n((x, y), n, a, bb, p) is not None:
            return x, y
        x += 1


# the crate's secp256k1 curve, generator of order 2^36 and coset offset (the constants of src/lib.rs:45-59)
CRATE = {
    "a": 31172306031375832341232376275243462303334845584808513005362718476441963632613,
    "bb": 45508371059383884471556188660911097844526467659576498497548207627741160623272,
    "gen": (41293412487153066667050767300223451435019201659857889215769525847559135483332,
            73754924733368840065089190002333366411120578552679996887076912271884749237510),
    "offset": (105623886150579165427389078198493427091405550492761682382732004625374789850161,
               7709812624542158994629670452026922591039826164720902911013234773380889499231),
    "log_order": 36,
}

# first hits of the stream, as found with this model: (field, seed, k) -> (index, n); the tests recompute them
FIRST_HITS = {
    ("m31", 1, 6): (13, 10), ("m31", 1, 10): (13, 10), ("m31", 1, 12): (2631, 12), ("m31", 2, 6): (0, 6), ("m31", 2, 10): (2452, 10),
    ("secp256k1", 1, 6): (309, 8), ("secp256k1", 1, 10): (2338, 10), ("secp256k1", 1, 12): (2581, 13), ("secp256k1", 2, 10): (129, 10),
}
