#!/usr/bin/env python3
"""ecfft_poly_eval_points against poly_mul(G) and ENTER_G, in one process on warmed shapes, device-resident data (host clock after a
device synchronise, median of `reps` calls, the variants alternating call by call):
    eval          FFTree.poly_eval_points(f, x, count): nf coefficients at m random points, G = max(64, next_pow2(nf))
    eval_2x       the same points with 2 * count polynomials
    leaves        FFTree.poly_eval_points of 64-coefficient polynomials at the same points and count: no tree, k_eval_leaves alone
    poly_mul_G    FFTree.poly_mul of two G/2-coefficient operands, count pairs: the yardstick
    enter_G       FFTree.enter of count vectors of G coefficients
The phase split of one call is read from these.  The subproduct tree and the node reciprocals (phase A) do not depend on count, the
descent and the leaves scale with it: phase A = 2 eval - eval_2x, descent = eval - phase A - leaves.
usage: polyeval_time.py [reps] > profiles/polyeval/polyeval_time.json ; prints one JSON object"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecfft_amd  # noqa: E402

CASES = [("secp256k1", 16, 16, 1), ("secp256k1", 20, 20, 1), ("secp256k1", 18, 18, 8), ("secp256k1", 10, 20, 1),
         ("m31", 22, 22, 1)]   # (field, log nf, log m, count)


def rand_dev(field, rows, seed):
    rng = np.random.default_rng(seed)
    if field == "m31":
        return torch.from_numpy(rng.integers(0, 2**31 - 1, rows, dtype=np.uint32).view(np.int32)).cuda()
    a = rng.integers(0, 2**64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)                                  # < 2^255 < p: a reduced residue
    return torch.from_numpy(a.view(np.int64)).cuda()


def run_case(field, log_nf, log_m, count, reps):
    nf, m = 1 << log_nf, 1 << log_m
    G = max(64, nf)
    t = ecfft_amd.FIELDS[field].build_fftree(G)
    f, f2, x = rand_dev(field, count * nf, 1), rand_dev(field, 2 * count * nf, 2), rand_dev(field, m, 3)
    f64 = rand_dev(field, count * 64, 4)
    a, b = rand_dev(field, count * (G // 2), 5), rand_dev(field, count * (G // 2), 6)
    c = rand_dev(field, count * G, 7)
    ops = {"eval": lambda: t.poly_eval_points(f, x, count=count),
           "eval_2x": lambda: t.poly_eval_points(f2, x, count=2 * count),
           "leaves": lambda: t.poly_eval_points(f64, x, count=count),
           "poly_mul_G": lambda: t.poly_mul(a, b, count=count),
           "enter_G": lambda: t.enter(c, count=count)}
    for _ in range(2):
        for fn in ops.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in ops}
    for _ in range(reps):
        for k, fn in ops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    phase_a = 2 * med["eval"] - med["eval_2x"]
    split = {"tree_and_reciprocals": phase_a, "descent": med["eval"] - phase_a - med["leaves"], "leaves": med["leaves"]}
    P = -(-m // G) * G
    node_bytes = 4 * P * max(G.bit_length() - 7, 0) * t.field.elem_bytes    # M^ and G^: 4 P elements per level d = 64 .. G/2
    del t
    torch.cuda.empty_cache()
    return {"field": field, "nf": nf, "m": m, "count": count, "G": G, "reps": reps,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_ms": {k: round(min(v), 4) for k, v in ts.items()},
            "eval_over_poly_mul_G": round(med["eval"] / med["poly_mul_G"], 3),
            "eval_over_enter_G": round(med["eval"] / med["enter_G"], 3),
            "phase_split_ms": {k: round(v, 4) for k, v in split.items()},
            "node_data_bytes": node_bytes}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    torch.zeros(1, device="cuda")
    out = {"device": ecfft_amd.device_info(0), "cases": [run_case(f, a, b, c, reps) for f, a, b, c in CASES]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
