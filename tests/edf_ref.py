"""TEST INFRASTRUCTURE — an exact CPU restatement of ecfft_poly_equal_degree, for tests/test_gpu_polyedf.py and
tests/test_edf_ref_host.py.

Imports only the standard library, tests/gcd_ref.py (trim, divmod_school), tests/powmod_ref.py (_conv), tests/roots_ref.py
(monic, rem, gcd, pow_mod) and tests/ddf_ref.py (product, binomials).  Polynomials are lists of Python ints, low to high; every
function takes the prime p itself, so that the model can be compared with trial division at primes small enough to list every
irreducible.

- frobenius(g, d, p): [h_0 .. h_(d-1)], h_i = x^(p^i) mod g, as plain repeated powers h_(i+1) = h_i^p mod g.
- norm(hs, c, g, p): N_c = prod_i (h_i + c) mod g.  Modulo an irreducible factor f_j of degree d of g it is the field norm of
  alpha_j + c: (-1)^d f_j(-c), an element of F_p.
- split(h, hs, g, c, p): one attempt on a divisor h of g: w = (N_c mod h)^((p-1)/2) mod h = (x + c)^((p^d - 1)/2), u = gcd(h, w - 1),
  v = h / u; a success when 0 < deg u < deg h.  p is odd.
- equal_degree(g, d, p): the stack of pending factors of the GPU's leaf kernel with the shifts 1, 2, 3, ... from one attempt counter.
  Returns (sorted factors with their leading 1, attempts, the longest run of consecutive failed shifts on one factor); None for the
  zero polynomial (-1 in the C ABI), -2 where d does not divide the degree, [] for a non-zero constant.
- pack / unpack: the layout of the C ABI: `factors` (nd entries: the factors in ascending order, which is Python's sorted on
  low-to-high coefficient lists, each as its low d coefficients, then zeros) and n_factors.
- shifted(q, s, p): q(x + s), irreducible with q and dense.
"""
import ddf_ref as D
import gcd_ref as G
import powmod_ref as W
import roots_ref as RR

CAP = 64            # consecutive failed shifts of one factor after which the GPU call gives up


def frobenius(g, d, p):
    hs = [RR.rem([0, 1], g, p)]
    for _ in range(1, d):
        hs.append(RR.pow_mod(hs[-1], p, g, p))
    return hs


def norm(hs, c, g, p):
    res = None
    for h in hs:
        y = list(h) + [0] * (1 - len(h))
        y[0] = (y[0] + c) % p
        y = G.trim(y)
        res = y if res is None else RR.rem(W._conv(res, y, p), g, p)
    return res


def split(h, hs, g, c, p):
    assert p & 1 and h[-1] == 1
    base = RR.rem(norm(hs, c, g, p), h, p)
    w = RR.pow_mod(base, (p - 1) // 2, h, p) if base else []
    u = RR.gcd(h, RR._sub(w, [1], p), p)
    v, r = G.divmod_school(h, u, p)
    assert not r
    return u, v


def equal_degree(g, d, p, cap=CAP):
    g = G.trim([v % p for v in g])
    if not g:
        return None
    n = len(g) - 1
    if n == 0:
        return [], 0, 0
    if n % d:
        return -2
    g = RR.monic(g, p)
    if n == d:
        return [g], 0, 0
    hs = frobenius(g, d, p)
    stack, out, c, fails, worst = [g], [], 1, 0, 0
    while stack:
        h = stack.pop()
        e = len(h) - 1
        if e == d:
            out.append(h)
            continue
        u, v = split(h, hs, g, c, p)
        c += 1
        if 0 < len(u) - 1 < e:
            assert (len(u) - 1) % d == 0
            fails = 0
            stack += [u, v]
        else:
            fails += 1
            worst = max(worst, fails)
            if fails >= cap:
                raise OverflowError("attempt cap")
            stack.append(h)
    return sorted(out), c - 1, worst


def pack(factors, nd, d):
    """(factors row of nd entries, n_factors) of a list of monic factors of degree d (None: the zero polynomial; -2 passes through)"""
    if factors is None or factors == -2:
        return [0] * nd, -1 if factors is None else -2
    row = []
    for q in sorted(factors):
        assert len(q) == d + 1 and q[-1] == 1
        row += q[:-1]
    assert len(row) <= nd
    return row + [0] * (nd - len(row)), len(factors)


def unpack(row, n, d):
    return [list(row[i * d:(i + 1) * d]) + [1] for i in range(max(n, 0))]


def shifted(q, s, p):
    """q(x + s) by Horner"""
    res = []
    for coef in reversed(q):
        res = W._conv(res, [s % p, 1], p) if res else []
        res = res + [0] * (1 - len(res))
        res[0] = (res[0] + coef) % p
    return G.trim(res)


def irreducibles(d, count, p):
    """`count` distinct dense monic irreducibles of degree d: the binomials x^d - a and their shifts (x + s)^d - a, s = 1, 2, ...
    (d = 1: x - a only)"""
    if d == 1:
        return [[-a % p, 1] for a in range(2, 2 + count)]
    nb = max(1, (count + 3) // 4)
    bins = D.irreducible_binomials(d, nb, p)
    out, s = [], 0
    while len(out) < count:
        out += [shifted(q, s, p) for q in bins]
        s += 1
    out = out[:count]
    assert len({tuple(q) for q in out}) == count
    return out


def case(d, r, p, k=3):
    """(g, want) of a test input known by construction: g = k prod q over the first r of irreducibles(d, ., p); want = sorted(q)"""
    qs = irreducibles(d, r, p)
    return [v * k % p for v in D.product(qs, p)], sorted(qs)


# The (d, r) that tests/test_gpu_polyedf.py passes to the GPU through case(), by test; tests/test_edf_ref_host.py runs the model on
# every one it can afford (all of M31; secp256k1 at d <= 9 and at most 71 coefficients) and holds them to the cap condition.
GPU_ONE_FACTOR = [(1, 1), (2, 1), (63, 1)]
GPU_LINEAR = [(1, 2), (1, 64)]
GPU_SMALL_SPLITS = [(2, 2), (2, 32), (3, 21), (7, 9), (9, 7), (21, 3)]
GPU_MIXED_ROWS = [(3, 5), (3, 2), (3, 9), (2, 4)]
GPU_LARGE_FIRST = [(2, 33), (1, 66)]
GPU_LARGE_BOTH = {"secp256k1": [(7, 10), (3, 100)], "m31": [(7, 10), (3, 100), (21, 4)]}      # both iterate methods forced
GPU_LARGE_SHIPPED = {"secp256k1": [(21, 4), (63, 2), (2, 160)], "m31": [(63, 2), (2, 160)]}


def gpu_cases(field):
    """every (d, r) of the GPU tests for the field, without repeats"""
    both = GPU_ONE_FACTOR + GPU_LINEAR + GPU_SMALL_SPLITS + GPU_MIXED_ROWS + GPU_LARGE_FIRST
    out = []
    for dr in both + GPU_LARGE_BOTH[field] + GPU_LARGE_SHIPPED[field]:
        if dr not in out:
            out.append(dr)
    return out
