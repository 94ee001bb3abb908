"""Writes tests/golden/ec_curves.json: (field, A, B, order) of the curves y^2 = x^3 + A x + B that the tests of the short-Weierstrass
front end run on.  Run from the repository root: python tests/golden/gen_ec_curves.py (about 10 s, CPU only).

- M31 (1, 6) and (1, 3): counted by the CPU model of Schoof's algorithm, tests/schoof_ref.py cardinality.
- M31 (1, 0): p = 3 mod 4, so y^2 = x^3 + x is supersingular and has p + 1 = 2^31 points.
- secp256k1 (1, 0) and (p - 1, 0): supersingular for the same reason, p + 1 points each (the first with one point of order 2, the
  second with three).
- secp256k1 (0, 1): a twist of y^2 = x^3 + 7 (j = 0).  With t = p + 1 - N the trace of that curve and 4 p = t^2 + 3 s^2, the six
  twists have the traces +-t, +-(t + 3 s) / 2, +-(t - 3 s) / 2; the order is the one of the six that annihilates points of the curve.

Every order is then checked again: it lies in the Hasse interval and [order] R = O for several points R of the curve.
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ec_ref as E  # noqa: E402
import schoof_ref as S  # noqa: E402


def points(A, B, p, count):
    out, x = [], 1
    while len(out) < count:
        R = E.candidate(x, A, B, p)
        if R is not None:
            out.append(R)
        x += 1
    return out


def checked(field, A, B, order):
    p = S.P[field]
    assert not S.is_singular(A, B, p)
    assert (order - p - 1) ** 2 <= 4 * p, "outside the Hasse interval"
    for R in points(A, B, p, 6):
        assert E.mul(order, R, A, p) is None, (field, A, B, order)
    return {"field": field, "A": str(A), "B": str(B), "order": str(order)}


def j0_twist_order(B, p, n7):
    t = p + 1 - n7
    s2, r = divmod(4 * p - t * t, 3)
    s = math.isqrt(s2)
    assert r == 0 and s * s == s2
    traces = [t, -t, (t + 3 * s) // 2, -(t + 3 * s) // 2, (t - 3 * s) // 2, -(t - 3 * s) // 2]
    pts = points(0, B, p, 4)
    hits = [p + 1 - tr for tr in traces if all(E.mul(p + 1 - tr, R, 0, p) is None for R in pts)]
    assert len(hits) == 1, hits
    return hits[0]


def main():
    m31, secp = S.P["m31"], S.P["secp256k1"]
    curves = [
        checked("m31", 1, 6, S.cardinality(1, 6, m31)[0]),
        checked("m31", 1, 3, S.cardinality(1, 3, m31)[0]),
        checked("m31", 1, 0, m31 + 1),
        checked("secp256k1", 1, 0, secp + 1),
        checked("secp256k1", secp - 1, 0, secp + 1),
        checked("secp256k1", 0, 1, j0_twist_order(1, secp, S.SECP256K1_ORDER)),
    ]
    with open(os.path.join(HERE, "ec_curves.json"), "w") as f:
        json.dump({"comment": "written by tests/golden/gen_ec_curves.py: curves y^2 = x^3 + A x + B and their numbers of points", "curves": curves}, f, indent=1)
        f.write("\n")
    for c in curves:
        print(c["field"], c["A"] if len(c["A"]) < 12 else "p-1", c["B"], c["order"])


if __name__ == "__main__":
    main()
