#!/usr/bin/env python3
"""ecfft_poly_interpolate against poly_eval_points, poly_mul(P) and EXIT_P, in one process on warmed shapes, device-resident data
(host clock after a device synchronise, median of `reps` calls, the variants alternating call by call):
    interp        FFTree.poly_interpolate(x, y, count): m = P distinct points, count value vectors
    interp_2x     the same points with 2 * count value vectors
    eval          FFTree.poly_eval_points(f, x, count) with nf = m at the same points: the inverse operation, the yardstick
    eval_2x       the same with 2 * count polynomials
    poly_mul_P    FFTree.poly_mul of two P/2-coefficient operands, count pairs
    exit_P        FFTree.exit of count vectors of P evaluations
The subproduct tree and the weights depend only on the points, the leaves, the ascent and the EXIT scale with count:
shared = 2 T(c) - T(2c), per vector = (T(2c) - T(c)) / c, for interp and for eval alike.
usage: polyinterp_time.py [reps] > profiles/polyinterp/polyinterp_time.json ; prints one JSON object"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecfft_amd  # noqa: E402

CASES = [("secp256k1", 16, 1), ("secp256k1", 20, 1), ("secp256k1", 18, 8), ("m31", 22, 1)]   # (field, log m, count)


def rand_dev(field, rows, seed):
    rng = np.random.default_rng(seed)
    if field == "m31":
        return torch.from_numpy(rng.integers(0, 2**31 - 1, rows, dtype=np.uint32).view(np.int32)).cuda()
    a = rng.integers(0, 2**64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)                                  # < 2^255 < p: a reduced residue
    return torch.from_numpy(a.view(np.int64)).cuda()


def distinct_dev(field, rows, seed):
    """pairwise distinct points: M31 an arithmetic progression mod p, shuffled (random draws collide); secp256k1 random, checked"""
    rng = np.random.default_rng(seed)
    if field != "m31":
        x = rand_dev(field, rows, seed)
        assert np.unique(x.cpu().numpy(), axis=0).shape[0] == rows
        return x
    p = 2**31 - 1
    a, b = int(rng.integers(1, p)), int(rng.integers(0, p))
    x = ((np.arange(rows, dtype=np.uint64) * np.uint64(a) + np.uint64(b)) % np.uint64(p)).astype(np.uint32)
    return torch.from_numpy(x[rng.permutation(rows)].view(np.int32)).cuda()


def run_case(field, log_m, count, reps):
    m = 1 << log_m
    P = max(64, m)
    t = ecfft_amd.FIELDS[field].build_fftree(P)
    x = distinct_dev(field, m, 3)
    y, y2 = rand_dev(field, count * m, 1), rand_dev(field, 2 * count * m, 2)
    a, b = rand_dev(field, count * (P // 2), 5), rand_dev(field, count * (P // 2), 6)
    ops = {"interp": lambda: t.poly_interpolate(x, y, count=count),
           "interp_2x": lambda: t.poly_interpolate(x, y2, count=2 * count),
           "eval": lambda: t.poly_eval_points(y, x, count=count),
           "eval_2x": lambda: t.poly_eval_points(y2, x, count=2 * count),
           "poly_mul_P": lambda: t.poly_mul(a, b, count=count),
           "exit_P": lambda: t.exit(y, count=count)}
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
    split = {"interp_shared": 2 * med["interp"] - med["interp_2x"], "interp_per_vector": (med["interp_2x"] - med["interp"]) / count,
             "eval_shared": 2 * med["eval"] - med["eval_2x"], "eval_per_polynomial": (med["eval_2x"] - med["eval"]) / count}
    del t
    torch.cuda.empty_cache()
    return {"field": field, "m": m, "count": count, "P": P, "reps": reps,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_ms": {k: round(min(v), 4) for k, v in ts.items()},
            "interp_over_eval": round(med["interp"] / med["eval"], 3),
            "interp_over_poly_mul_P": round(med["interp"] / med["poly_mul_P"], 3),
            "split_ms": {k: round(v, 4) for k, v in split.items()}}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    torch.zeros(1, device="cuda")
    out = {"device": ecfft_amd.device_info(0), "cases": [run_case(f, a, c, reps) for f, a, c in CASES]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
