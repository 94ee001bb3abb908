"""TEST INFRASTRUCTURE — an exact Python-int model of the short-Weierstrass front end (include/ecfft_hip.h: ecfft_curve_point_mul,
ecfft_curve_point_two_adicity, ecfft_curve_find_generator, ecfft_build_ec_fftree), for tests/test_gpu_ecpoint.py,
tests/test_gpu_ectree.py, tests/test_ectree_host.py and tests/test_ec_ref_host.py.

Imports the standard library, tests/schoof_ref.py (the affine group law ec_add / ec_mul), tests/roots_ref.py (find_roots) and
tests/curve_ref.py (sqrt_canon).  The curve is y^2 = x^3 + A x + B over F_p; a point is (x, y) in standard form, None is the identity.

- on_curve, is_singular, neg, mul (double-and-add on the affine law: the affine result is unique, so any correct chain gives it).
- two_adicity(P, A, p, cap): the smallest i <= cap with 2^i P = O, else -1 (src/utils.rs:356-365 with a cap).
- candidates(A, B, p, start): x = start, start + 1, ... whose x^3 + A x + B is a non-zero square, with the canonical root.
- find_generator(A, B, order, p, start, max_candidates): (v, gen, offset, x) as the header defines them, None when the window holds
  no generator; raises ValueError when a candidate shows that `order` is not the curve's.
- velu_chain(A, B, gen, log_n, p): the log_n rational maps ((num0, num1, num2), (den0, den1, den2)) of build_ec_fftree
  (src/ec.rs:526-543), gen of order 2^log_n.
- leaves(A, B, gen, log_order, offset, n, p): x of offset + i * 2^(log_order - log2 n) gen.
- CRATE_M31: the constants of src/lib.rs:198-215.
"""
import json
import os

import curve_ref
import roots_ref
import schoof_ref as S

P = S.P
MAX_TWO_ADICITY = {"secp256k1": 258, "m31": 34}          # 8 * element bytes + 2
CRATE_M31 = {"A": 1, "B": 0, "gen": (1273083559, 804329170), "offset": (1048755163, 279503108), "log_order": 28}
# the published generator and group order of secp256k1, y^2 = x^3 + 7
SECP256K1_G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
               0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
SECP256K1_ORDER = S.SECP256K1_ORDER


def fixture():
    """tests/golden/ec_curves.json: [{field, A, B, order}] with Python ints"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ec_curves.json")) as f:
        return [{"field": c["field"], "A": int(c["A"]), "B": int(c["B"]), "order": int(c["order"])} for c in json.load(f)["curves"]]


def rhs(x, A, B, p):
    return (x * x * x + A * x + B) % p


def on_curve(pt, A, B, p):
    return pt is None or (pt[1] * pt[1] - rhs(pt[0], A, B, p)) % p == 0


is_singular = S.is_singular


def neg(pt, p):
    return None if pt is None else (pt[0], -pt[1] % p)


def add(P1, P2, A, p):
    return S.ec_add(P1, P2, A, p)


def mul(k, pt, A, p):
    return S.ec_mul(k, pt, A, p)


def v2(n):
    return (n & -n).bit_length() - 1


def two_adicity(pt, A, p, cap):
    for i in range(cap + 1):
        if pt is None:
            return i
        if i < cap:
            pt = add(pt, pt, A, p)
    return -1


def double_n(pt, times, A, p):
    for _ in range(times):
        pt = add(pt, pt, A, p)
    return pt


def candidate(x, A, B, p):
    """the point (x, canonical root) when x^3 + A x + B is a non-zero square, else None"""
    f = rhs(x, A, B, p)
    if f == 0:
        return None
    y = curve_ref.sqrt_canon(f, p)
    return None if y is None else (x, y)


def find_generator(A, B, order, p, start=1, max_candidates=1 << 12):
    assert order > 0 and start >= 1
    v = v2(order)
    m = order >> v
    if v == 0:
        return None
    gen = off = x_gen = None
    for x in range(start, start + max_candidates):
        R = candidate(x, A, B, p)
        if R is None:
            continue
        if gen is None:
            G = mul(m, R, A, p)
            t = two_adicity(G, A, p, v)
            if t < 0:
                raise ValueError("not the order of this curve")
            if t == v:
                gen, x_gen = G, x
        if off is None and double_n(R, v + 1, A, p) is not None:
            off = R
        if gen is not None and off is not None:
            break
    if gen is None:
        return None
    return v, gen, off if off is not None else (0, 0), x_gen


def velu_chain(A, B, gen, log_n, p, cap=300):
    """the maps of build_ec_fftree for a generator of order 2^log_n: at each level the roots of x^3 + a x + b ascending, the first
    Velu 2-isogeny whose image of the generator has two-adicity one lower; None when some level has none"""
    maps, a, b, g = [], A % p, B % p, gen
    for _ in range(log_n):
        roots, _ = roots_ref.find_roots([b, a, 0, 1], p)
        tg = two_adicity(g, a, p, cap)
        for x0 in roots:
            t = (3 * x0 * x0 + a) % p
            a2, b2 = (a - 5 * t) % p, (b - 7 * x0 * t) % p
            dx = None if g is None else (g[0] - x0) % p
            if not dx:
                gp = None
            else:
                dx2 = dx * dx % p
                gp = ((g[0] * g[0] - x0 * g[0] + t) * pow(dx, -1, p) % p, (dx2 - t) * pow(dx2, -1, p) * g[1] % p)
            tp = two_adicity(gp, a2, p, cap)
            if tg >= 0 and tp >= 0 and tg == tp + 1:
                maps.append(((t, -x0 % p, 1), (-x0 % p, 1, 0)))
                a, b, g = a2, b2, gp
                break
        else:
            return None
    return maps


def leaves(A, B, gen, log_order, offset, n, p):
    g = double_n(gen, log_order - (n.bit_length() - 1), A, p)
    out, acc = [], offset
    for _ in range(n):
        out.append(acc[0])
        acc = add(acc, g, A, p)
    return out


def layers(lv, maps, p):
    """the layers below the leaves: layer k + 1 = psi_k(first half of layer k)"""
    out, cur = [lv], lv
    for num, den in maps:
        half = cur[:len(cur) // 2]
        cur = [(num[0] + num[1] * x + num[2] * x * x) * pow(den[0] + den[1] * x + den[2] * x * x, -1, p) % p for x in half]
        out.append(cur)
    return out
