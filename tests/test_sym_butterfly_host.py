"""CPU proof, on Python integers, of the symmetric butterflies.

A chain of good isogenies psi_k(x) = (x - b_k)^2 / x over a small prime carries two interleaved point sets S0, S1 (the moieties of
a tree).  In the coordinate sigma_k = (x - c1_k)/(x - c2_k) of each layer (c1, c2 = the critical points of psi_k, +-b_k here) the
two pre-images of a layer point have opposite sigma, so the stage tables p0 = sigma(s0), p1 = -p0, np0 = -p0, dinv = 1/(p1 - p0)
are tables of the general two-multiply butterflies on which

    recombine (A, B) -> (A + p0 B, A - p0 B)        decompose (a, b) -> q1 = dinv (b - a), q0 = (a + b)/2

give the same values with one multiply, provided the weights carry one factor (s_k - c2_k) per layer on top of the general
basis' W = prod v_k(s_k)^(h_k - 1).  EXTEND = weights . recombine(target) . decompose(source) . 1/weights is checked against direct
evaluation of the polynomial in the general basis, in the symmetric basis under the general butterflies, and in the symmetric basis
under the one-multiply butterflies; the mirror of host_curve.h critical_points is checked on the good isogeny and on a map whose
discriminant is a non-residue."""
import random

P = 1000003            # = 3 mod 4
LOG_E = 4              # 16 points per moiety, four layers


def inv(a):
    return pow(a % P, P - 2, P)


def sqrt(a):
    a %= P
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a else None


def critical_points(num, den):
    """mirror of host_curve.h critical_points: roots of N'D - N D', or None when they are not two finite rational points"""
    n0, n1, n2 = num
    d0, d1, d2 = den
    A = (n2 * d1 - n1 * d2) % P
    Bh = (n2 * d0 - n0 * d2) % P
    C = (n1 * d0 - n0 * d1) % P
    if A == 0:
        return None
    disc = (Bh * Bh - A * C) % P
    r = sqrt(disc) if disc else None
    if r is None:
        return None
    return (r - Bh) * inv(A) % P, (-r - Bh) * inv(A) % P


def good_map(b):
    return (b * b % P, -2 * b % P, 1), (0, 1, 0)


def psi(b, x):
    return (x - b) ** 2 * inv(x) % P


def lift(b, t):
    """the two pre-images of t under psi_b, or None: x^2 - (2b + t) x + b^2 = 0"""
    r = sqrt(t * (t + 4 * b))
    if not r:
        return None
    i2 = inv(2)
    return (2 * b + t + r) * i2 % P, (2 * b + t - r) * i2 % P


def build_chain(rng, log_m):
    """layers[k] = the 2^(log_m - k) points of layer k of a tree with 2^log_m leaves, layers[k+1][j] = psi_k(layers[k][j]) =
    psi_k(layers[k][j + half]); bs[k] = b_k.  Built from the root downwards, b_k redrawn until every point of layer k+1 lifts."""
    while True:
        layers, bs = [[rng.randrange(1, P)]], []
        ok = True
        for _ in range(log_m):
            for _try in range(200000):
                b = rng.randrange(1, P)
                pre = []
                for t in layers[0]:
                    pre.append(lift(b, t))
                    if pre[-1] is None:
                        break
                if pre[-1] is not None:
                    lo, hi = [p[0] for p in pre], [p[1] for p in pre]
                    if len(set(lo + hi)) == 2 * len(pre) and 0 not in lo + hi:
                        break
            else:
                ok = False
                break
            layers.insert(0, lo + hi)
            bs.insert(0, b)
        if ok:
            return layers, bs


def moiety_chain(layers, sg):
    """layer k of moiety sg: the points of index = sg mod 2 (the stage tables of device_tree.h build_tree)"""
    return [lay[sg::2] for lay in layers[:-1]]


def tables(chain, bs, sym):
    """per stage k: p0, p1, np0, dinv over the h_k pairs; and the weights of the e leaves"""
    e = len(chain[0])
    st = []
    for k, pts in enumerate(chain):
        h = len(pts) // 2
        if h == 0:
            break
        c1, c2 = critical_points(*good_map(bs[k])) if sym else (None, None)
        co = (lambda x: (x - c1) * inv(x - c2) % P) if sym else (lambda x: x)
        p0 = [co(pts[i]) for i in range(h)]
        p1 = [co(pts[i + h]) for i in range(h)]
        st.append((p0, p1, [-v % P for v in p0], [inv(b - a) for a, b in zip(p0, p1)]))
    w = []
    for i in range(e):
        W = 1
        for k in range(len(st)):
            h = len(chain[k]) // 2
            s = chain[k][i % len(chain[k])]
            W = W * pow(s, h - 1, P) % P                    # v_k(x) = x, h_k - 1 times
            if sym:
                W = W * (s - critical_points(*good_map(bs[k]))[1]) % P
        w.append(W)
    return st, w


def extend(vals, src, tgt, sym_bfly, mults):
    """EXTEND of one vector from the source tables to the target tables; mults[0] counts butterfly multiplies"""
    (sst, sw), (tst, tw) = src, tgt
    e = len(vals)
    x = [v * inv(wi) % P for v, wi in zip(vals, sw)]
    i2 = inv(2)
    for k, (p0, p1, np0, dinv) in enumerate(sst):             # decompose, large distance first
        h = len(p0)
        for blk in range(0, e, 2 * h):
            for i in range(h):
                a, b = x[blk + i], x[blk + i + h]
                q1 = dinv[i] * (b - a) % P
                if sym_bfly:
                    q0 = (a + b) * i2 % P; mults[0] += 1      # the halving is a shift, not a multiply
                else:
                    q0 = (a + np0[i] * q1) % P; mults[0] += 2
                x[blk + i], x[blk + i + h] = q0, q1
    for k in range(len(tst) - 1, -1, -1):                      # recombine
        p0, p1, _, _ = tst[k]
        h = len(p0)
        for blk in range(0, e, 2 * h):
            for i in range(h):
                A, B = x[blk + i], x[blk + i + h]
                if sym_bfly:
                    m = p0[i] * B % P; mults[0] += 1
                    x[blk + i], x[blk + i + h] = (A + m) % P, (A - m) % P
                else:
                    mults[0] += 2
                    x[blk + i], x[blk + i + h] = (A + p0[i] * B) % P, (A + p1[i] * B) % P
    return [v * wi % P for v, wi in zip(x, tw)]


def evaluate(coeffs, pts):
    return [sum(c * pow(x, j, P) for j, c in enumerate(coeffs)) % P for x in pts]


def test_critical_points_of_the_good_isogeny_are_plus_minus_b():
    rng = random.Random(1)
    for _ in range(20):
        b = rng.randrange(1, P)
        cp = critical_points(*good_map(b))
        assert cp is not None and set(cp) == {b, -b % P}


def test_rationality_test_rejects_a_non_residue_discriminant():
    # Velu-shaped map (x^2 - x0 x + t)/(x - x0): critical points x0 +- sqrt(t)
    rng = random.Random(2)
    seen = {True: 0, False: 0}
    while min(seen.values()) < 5:
        x0, t = rng.randrange(P), rng.randrange(1, P)
        cp = critical_points((t, -x0 % P, 1), (-x0 % P, 1, 0))
        r = sqrt(t)
        seen[r is not None] += 1
        if r is None:
            assert cp is None
        else:
            assert cp is not None and set(cp) == {(x0 + r) % P, (x0 - r) % P}
    assert critical_points((1, 2, 0), (3, 1, 0)) is None        # no quadratic term: a critical point at infinity


def test_opposite_sigma_on_every_pair():
    layers, bs = build_chain(random.Random(3), LOG_E + 1)
    for sg in (0, 1):
        st, _ = tables(moiety_chain(layers, sg), bs, True)
        for p0, p1, np0, dinv in st:
            assert all((a + b) % P == 0 for a, b in zip(p0, p1))
            assert np0 == p1 and all(d * (-2 * a) % P == 1 for a, d in zip(p0, dinv))


def test_extend_exact_in_every_basis_and_form():
    rng = random.Random(4)
    layers, bs = build_chain(rng, LOG_E + 1)
    e = 1 << LOG_E
    S = [layers[0][sg::2] for sg in (0, 1)]
    gen = [tables(moiety_chain(layers, sg), bs, False) for sg in (0, 1)]
    sym = [tables(moiety_chain(layers, sg), bs, True) for sg in (0, 1)]
    for trial in range(4):
        coeffs = [rng.randrange(P) for _ in range(e)] if trial else [0] * (e - 1) + [1]
        for src in (0, 1):
            vals, want = evaluate(coeffs, S[src]), evaluate(coeffs, S[1 - src])
            m_gen, m_mix, m_sym = [0], [0], [0]
            assert extend(vals, gen[src], gen[1 - src], False, m_gen) == want      # today's form
            assert extend(vals, sym[src], sym[1 - src], False, m_mix) == want      # symmetric tables, general butterflies
            assert extend(vals, sym[src], sym[1 - src], True, m_sym) == want       # symmetric tables, one multiply per pair
            assert m_gen[0] == m_mix[0] == 2 * e * LOG_E and m_sym[0] == e * LOG_E
