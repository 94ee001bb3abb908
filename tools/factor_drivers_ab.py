#!/usr/bin/env python3
"""Large-regime calls of the factor drivers for an A/B of two source trees with the processes ALTERNATING (two processes run one
after the other drift by more than the spread inside either): one process per tree and turn, each printing one JSON line of
medians in ms.  ROOT is the tree whose built library is measured (default: this one).  Inputs, on a tree of 4096 leaves:
    roots_R    poly_find_roots of prod (x - r_i) over R seeded distinct roots (R + 1 coefficients, all roots), device-resident
    mul_R      poly_mul of that polynomial with itself: a call the drivers do not touch, the control
    edf_D_N    poly_equal_degree(g, D) of tests/edf_ref.case(D, N / D): N / D irreducibles of degree D, host arrays
Each call is made twice unmeasured, then `reps` times between device synchronisations (host clock); the figure is the median.
reps: M31 15 (edf_2_1024 and edf_7_252: 9); secp256k1 5 (edf_2_1024: 2).
usage: factor_drivers_ab.py [ROOT]"""
import json
import os
import sys
import time

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ecfft_amd  # noqa: E402
import edf_ref  # noqa: E402
import polyroots_time as PT  # noqa: E402


def med(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 4)


def main():
    out = {}
    plan = {"m31": {"roots": [(256, 15), (1024, 15)], "edf": [(2, 256, 15), (2, 1024, 9), (7, 252, 9)]},
            "secp256k1": {"roots": [(256, 5)], "edf": [(2, 256, 5), (2, 1024, 2)]}}
    for field, todo in plan.items():
        p = PT.P[field]
        t = ecfft_amd.FIELDS[field].build_fftree(4096)
        a = 0x9E3779B1 if field == "m31" else 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95
        for r, reps in todo["roots"]:
            roots = [(a * (i + 1) + 12345) % p for i in range(r)]
            f = PT.dev(field, PT.trimmed(PT.product(field, t, [[-x % p, 1] for x in roots], 2)))
            out[f"{field}/roots_{r}"] = med(lambda: t.poly_find_roots(f), reps)
            out[f"{field}/mul_{r}"] = med(lambda: t.poly_mul(f, f), 15)
        for d, n, reps in todo["edf"]:
            g = PT.mem(field, edf_ref.case(d, n // d, p)[0])
            out[f"{field}/edf_{d}_{n}"] = med(lambda: t.poly_equal_degree(g, d), reps)
        del t
    print(json.dumps(out))


if __name__ == "__main__":
    main()
