#!/usr/bin/env python3
"""ecfft_poly_gcd / ecfft_poly_xgcd against the Euclid loop a user could write before them from ecfft_poly_divrem, and against
ecfft_poly_mul at the same size, in one process on warmed shapes, device-resident data (host clock after a device synchronise,
median of `reps` calls, the variants alternating call by call, the whole measurement repeated `blocks` times to see the spread
between medians):
    gcd, xgcd     FFTree.poly_gcd / poly_xgcd(a, b): n and n - 1 coefficients, seeded random (coprime, the normal degree sequence)
    euclid        r_{i+1} = r_{i-1} mod r_i by one FFTree.poly_divrem per remainder until the remainder has no coefficients (each
                  remainder of a normal sequence is one coefficient shorter, so its row is already trimmed); only up to `euclid_max`
                  coefficients, and with one rep per block above 1024, because it is n calls of a full division each
    poly_mul_N    FFTree.poly_mul of two n-coefficient operands: the unit
A case whose first call takes longer than 2 s is measured with reps = blocks = 1 and no further warm-up.
usage: polygcd_time.py [reps [blocks [euclid_max [max_log_secp [max_log_m31]]]]] > profiles/polygcd/polygcd_time.json ; prints one JSON object"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecfft_amd  # noqa: E402
from ecfft_amd import fftree as FT  # noqa: E402


def sizes(max_log):
    g = FT.GCD_SMALL_MAX
    return sorted({16, 64, g // 2, g, g + 1, 2 * g} | {1 << k for k in range(10, max_log + 1, 2)} | {1 << max_log})


def rand_dev(field, rows, seed):
    rng = np.random.default_rng(seed)
    if field == "m31":
        return torch.from_numpy(rng.integers(1, 2**31 - 1, rows, dtype=np.uint32).view(np.int32)).cuda()
    a = rng.integers(0, 2**64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)                                  # < 2^255 < p: a reduced residue
    a[:, 0] |= np.uint64(1)                                   # nonzero
    return torch.from_numpy(a.view(np.int64)).cuda()


def run_case(field, t, n, reps, blocks, euclid_max):
    a, b = rand_dev(field, n, 1), rand_dev(field, n - 1, 2)

    def euclid():
        r0, r1 = a, b
        while r1.shape[0] > 1:
            r0, r1 = r1, t.poly_divrem(r0, r1)[1]
        return r1

    ops = {"gcd": lambda: t.poly_gcd(a, b), "xgcd": lambda: t.poly_xgcd(a, b), "poly_mul_N": lambda: t.poly_mul(a, a)}
    if n <= euclid_max:
        ops["euclid"] = euclid
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g, deg = ops["gcd"]()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    if first > 2.0:
        reps = blocks = 1                                     # the first call was the warm-up
    else:
        for fn in ops.values():
            fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in ops}
    for _ in range(blocks):
        ts = {k: [] for k in ops}
        for i in range(reps):
            for k, fn in ops.items():
                if k == "euclid" and n > 1024 and i:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for k in ops:
            meds[k].append(float(np.median(ts[k])))
    med = {k: float(np.median(v)) for k, v in meds.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in meds.items()}
    out = {"field": field, "n": n, "reps": reps, "blocks": blocks, "deg_gcd": int(deg[0]),
           "median_ms": {k: round(v, 4) for k, v in med.items()}, "spread_ms": spread,
           "block_medians_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
           "gcd_over_poly_mul_N": round(med["gcd"] / med["poly_mul_N"], 2), "xgcd_over_poly_mul_N": round(med["xgcd"] / med["poly_mul_N"], 2)}
    if "euclid" in med:
        out["euclid_over_gcd"] = round(med["euclid"] / med["gcd"], 2)
        out["euclid_over_xgcd"] = round(med["euclid"] / med["xgcd"], 2)
    return out


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    reps, blocks, euclid_max, logs = arg(1, 5), arg(2, 3), arg(3, 4096), {"secp256k1": arg(4, 19), "m31": arg(5, 21)}
    torch.zeros(1, device="cuda")
    cases = []
    for field in ("secp256k1", "m31"):
        t = ecfft_amd.FIELDS[field].build_fftree(2 << logs[field])
        for n in sizes(logs[field]):
            cases.append(run_case(field, t, n, reps, blocks, euclid_max))
            print(json.dumps(cases[-1]), file=sys.stderr, flush=True)
        del t
        torch.cuda.empty_cache()
    print(json.dumps({"device": ecfft_amd.device_info(0), "small_max": FT.GCD_SMALL_MAX, "euclid_max": euclid_max, "cases": cases}))


if __name__ == "__main__":
    main()
