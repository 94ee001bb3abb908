"""TEST INFRASTRUCTURE — an exact CPU model of ecfft_poly_squarefree_decompose and ecfft_poly_factor, for
tests/test_gpu_polyfactor.py and tests/test_factor_ref_host.py.

Imports only the standard library, tests/gcd_ref.py (trim, divmod_school), tests/roots_ref.py (monic, gcd, _sub), tests/ddf_ref.py
(derivative, ddf, product) and tests/edf_ref.py (equal_degree, irreducibles).  Polynomials are lists of Python ints, low to high;
every function takes the prime p itself.

- yun(f, p): Yun's squarefree decomposition, the loop of the GPU as it is written: with f made monic, a_0 = gcd(f, f'), b = f / a_0,
  c = f' / a_0, d = c - b'; for i = 1, 2, ... while deg b > 0: a_i = gcd(b, d) (gcd(b, 0) = b), b <- b / a_i, c <- d / a_i,
  d <- c - b'.  Returns ({i: a_i with its leading 1, for deg a_i > 0}, the leading coefficient, the number of iterations); None for
  the zero polynomial.  Asserts p > deg f: derivatives vanish for constants only and there is no p-th-power case.
- factor(f, p): yun, then ddf_ref.ddf and edf_ref.equal_degree per part.  Returns ([(q with its leading 1, e), ...] in ascending
  (e, deg q, coefficients), the leading coefficient, the longest run of consecutive failed shifts on one factor); None for zero.
- case(spec, p, k): a spec is a list of (d, r, e): r distinct irreducibles of degree d, each at multiplicity e.  The irreducibles of
  one degree come from ONE call of edf_ref.irreducibles(d, total for d, p), sliced in the order of the spec (its choice depends on
  the count).  Returns (f = k prod q^e, the expected [(q, e), ...] in the order above).
- parts_of(want): the expected decomposition {e: the product of the q at multiplicity e} of an expected factor list.
- pack_decompose / pack_factor: the layouts of the C ABI.
"""
import ddf_ref as D
import edf_ref as E
import gcd_ref as G
import roots_ref as RR


def _exact(a, b, p):
    q, r = G.divmod_school(a, b, p)
    assert not r
    return q


def yun(f, p):
    f = G.trim([v % p for v in f])
    if not f:
        return None
    assert p > len(f) - 1, "the model has no p-th-power case"
    lead = f[-1]
    if len(f) == 1:
        return {}, lead, 0
    f = RR.monic(f, p)
    fd = D.derivative(f, p)
    a0 = RR.gcd(f, fd, p)
    b, c = _exact(f, a0, p), _exact(fd, a0, p)
    d = RR._sub(c, D.derivative(b, p), p)
    parts, i = {}, 0
    while len(b) > 1:
        i += 1
        a = RR.gcd(b, d, p)                                   # d = 0: the gcd is b itself
        if len(a) > 1:
            parts[i] = a
        b = _exact(b, a, p)
        c = _exact(d, a, p) if d else []
        d = RR._sub(c, D.derivative(b, p), p)
    assert sum(i * (len(a) - 1) for i, a in parts.items()) == len(f) - 1
    return parts, lead, i


def order(factors):
    """[(q, e), ...] in the order of the C ABI: ascending (e, deg q, coefficients low to high)"""
    return sorted(factors, key=lambda qe: (qe[1], len(qe[0]), qe[0]))


def factor(f, p):
    y = yun(f, p)
    if y is None:
        return None
    parts, lead, _ = y
    out, worst = [], 0
    for e, a in parts.items():
        for d, g in D.ddf(a, p).items():
            qs, _, w = E.equal_degree(g, d, p)
            worst = max(worst, w)
            out += [(q, e) for q in qs]
    return order(out), lead, worst


def case(spec, p, k=3):
    total = {}
    for d, r, e in spec:
        total[d] = total.get(d, 0) + r
    pool = {d: E.irreducibles(d, n, p) for d, n in total.items()}
    used = {d: 0 for d in total}
    want, polys = [], []
    for d, r, e in spec:
        for q in pool[d][used[d]:used[d] + r]:
            want.append((q, e))
            polys += [q] * e
        used[d] += r
    f = [v * k % p for v in D.product(polys, p)]
    return f, order(want)


def multiply_back(factors, lead, p):
    polys = [q for q, e in factors for _ in range(e)]
    return [v * lead % p for v in D.product(polys, p)]


def parts_of(want, p):
    by_e = {}
    for q, e in want:
        by_e.setdefault(e, []).append(q)
    return {e: D.product(qs, p) for e, qs in by_e.items()}


def pack_decompose(parts, nd):
    """(parts row, degrees row), nd entries each, of a yun() decomposition {i: a_i} (None: the zero polynomial)"""
    degrees, row = [0] * nd, []
    if parts is None:
        degrees[0] = -1
    else:
        for i in sorted(parts):
            a = parts[i]
            assert a[-1] == 1 and len(a) > 1
            degrees[i - 1] = len(a) - 1
            row += a[:-1]
    assert len(row) <= nd
    return row + [0] * (nd - len(row)), degrees


def pack_factor(factors, nd):
    """(factors row, fdeg row, fmult row, n_factors), the rows of nd entries, of a factor list (None: the zero polynomial)"""
    if factors is None:
        return [0] * nd, [0] * nd, [0] * nd, -1
    row, fdeg, fmult = [], [], []
    for q, e in order(factors):
        assert q[-1] == 1 and len(q) > 1 and e >= 1
        row += q[:-1]
        fdeg.append(len(q) - 1)
        fmult.append(e)
    n = len(fdeg)
    assert len(row) <= nd
    return row + [0] * (nd - len(row)), fdeg + [0] * (nd - n), fmult + [0] * (nd - n), n


def unpack_factor(row, fdeg, fmult, n):
    out, pos = [], 0
    for j in range(max(n, 0)):
        out.append((list(row[pos:pos + fdeg[j]]) + [1], fmult[j]))
        pos += fdeg[j]
    return out


def degree(spec):
    return sum(d * r * e for d, r, e in spec)


# The specs of tests/test_gpu_polyfactor.py.  Small regime (at most 65 coefficients, any tree):
SMALL = {
    "S1": [(1, 3, 1), (1, 2, 2), (2, 2, 1), (2, 1, 3), (3, 1, 2)],   # degree 23: three multiplicities, three degrees, a split inside a part
    "S2": [(1, 10, 1), (1, 9, 2), (3, 2, 2), (2, 6, 1)],             # degree 52: 27 factors
    "S3": [(1, 1, 64)],                                              # degree 64: K iterations, the limit of 65 coefficients
    "S4": [(1, 1, 1), (1, 1, 3)],                                    # degree 4: a gap at multiplicity 2
    "S5": [(2, 32, 1)],                                              # degree 64: squarefree, the largest small split
    "S6": [(1, 1, e) for e in range(1, 11)],                         # degree 55: ten parts, the most a small row can have
}
# Large regime, with the leaves of the tree the rule asks for:
LARGE = {
    "L1": ([(1, 33, 2)], 256),                                       # degree 66: large Yun, a small part
    "L2": ([(2, 35, 1), (1, 3, 2), (3, 1, 3)], 256),                 # degree 85: a part of degree 70 through edf_one_large's rounds
    "L3": ([(1, 40, 1), (2, 20, 2), (7, 5, 1), (1, 6, 4)], 512),     # degree 179: a part of degree 75 that needs distinct-degree splitting
}
assert [degree(s) for s in SMALL.values()] == [23, 52, 64, 4, 64, 55]
assert [degree(s) for s, _ in LARGE.values()] == [66, 85, 179]
