#!/usr/bin/env python3
"""ecfft_poly_pow_mod against the same power composed from ecfft_poly_mul + ecfft_poly_divrem, and against ecfft_poly_mul at the
same N, in one process on warmed shapes, device-resident data (host clock after a device synchronise, median of `reps` calls, the
variants alternating call by call, the whole measurement repeated `blocks` times to see the spread between medians):
    pow_mod       FFTree.poly_pow_mod(a, e, f): d = nm - 1 coefficients per residue, e of B bits (seeded, top bit set)
    composed      the same left-to-right scan over the same bits from the public calls the library had before: per modular product
                  one poly_mul and one poly_divrem (which recomputes the reciprocal of the modulus every time)
    setup         FFTree.poly_pow_mod(a, 1, f): everything pow_mod does once per call (reduce, reciprocal, the three kept lifts)
    poly_mul_N    FFTree.poly_mul of two N/2-coefficient operands, N = next_pow2(2d - 1): the yardstick
The number of modular products comes from the exponent's own bits: B - 1 squarings and popcount(e) - 1 multiplies.
usage: polypowmod_time.py [reps [blocks]] > profiles/polypowmod/polypowmod_time.json ; prints one JSON object"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecfft_amd  # noqa: E402

# (field, d, count, exponent bits)
CASES = [("secp256k1", 1 << 19, 1, 8), ("secp256k1", 1 << 15, 1, 32), ("secp256k1", 1 << 10, 1, 64), ("secp256k1", 64, 1, 64),
         ("secp256k1", 16, 1, 64), ("secp256k1", 1 << 18, 8, 8), ("m31", 1 << 23, 1, 8), ("m31", 1 << 12, 1, 64)]


def rand_dev(field, rows, seed):
    rng = np.random.default_rng(seed)
    if field == "m31":
        return torch.from_numpy(rng.integers(1, 2**31 - 1, rows, dtype=np.uint32).view(np.int32)).cuda()
    a = rng.integers(0, 2**64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)                                  # < 2^255 < p: a reduced residue
    a[:, 0] |= np.uint64(1)                                   # nonzero
    return torch.from_numpy(a.view(np.int64)).cuda()


def exponent(bits, seed):
    rng = np.random.default_rng(seed)
    e = 1 << (bits - 1)
    for i in range(bits - 1):
        e |= int(rng.integers(0, 2)) << i
    return e


def run_case(field, d, count, bits, reps, blocks):
    N = 1
    while N < 2 * d - 1:
        N <<= 1
    t = ecfft_amd.FIELDS[field].build_fftree(max(N, 2))
    a, f = rand_dev(field, count * d, 1), rand_dev(field, count * (d + 1), 2)
    h, hh = rand_dev(field, count * max(N // 2, 1), 3), rand_dev(field, count * max(N // 2, 1), 4)
    e = exponent(bits, 5)
    scan = bin(e)[3:]
    steps = len(scan) + scan.count("1")                       # squarings + multiplies of the scan below the top bit

    def composed():
        res = a
        for bit in scan:
            res = t.poly_divrem(t.poly_mul(res, res, count=count), f, count=count)[1]
            if bit == "1":
                res = t.poly_divrem(t.poly_mul(res, a, count=count), f, count=count)[1]
        return res

    ops = {"pow_mod": lambda: t.poly_pow_mod(a, e, f, count=count), "composed": composed,
           "setup": lambda: t.poly_pow_mod(a, 1, f, count=count), "poly_mul_N": lambda: t.poly_mul(h, hh, count=count)}
    same = bool(torch.equal(ops["pow_mod"](), composed()))
    for fn in ops.values():
        fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in ops}
    for _ in range(blocks):
        ts = {k: [] for k in ops}
        for _ in range(reps):
            for k, fn in ops.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for k in ops:
            meds[k].append(float(np.median(ts[k])))
    med = {k: float(np.median(v)) for k, v in meds.items()}
    a_steps = [m / steps for m in meds["pow_mod"]]
    b_steps = [m / steps for m in meds["composed"]]
    spread = max(max(a_steps) - min(a_steps), max(b_steps) - min(b_steps))
    del t
    torch.cuda.empty_cache()
    return {"field": field, "d": d, "N": N, "count": count, "exp_bits": bits, "modular_products": steps, "reps": reps, "blocks": blocks,
            "same_bytes": same,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "block_medians_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
            "pow_mod_ms_per_product": round(med["pow_mod"] / steps, 5),
            "pow_mod_ms_per_product_without_setup": round((med["pow_mod"] - med["setup"]) / steps, 5),
            "composed_ms_per_product": round(med["composed"] / steps, 5),
            "spread_ms_per_product": round(spread, 5),
            "below_composed_by_more_than_spread": bool(min(b_steps) - max(a_steps) > spread),
            "composed_over_pow_mod": round(med["composed"] / med["pow_mod"], 3),
            "product_over_poly_mul_N": round((med["pow_mod"] - med["setup"]) / steps / med["poly_mul_N"], 3),
            "composed_product_over_poly_mul_N": round(med["composed"] / steps / med["poly_mul_N"], 3)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    torch.zeros(1, device="cuda")
    out = {"device": ecfft_amd.device_info(0), "cases": [run_case(f, d, c, b, reps, blocks) for f, d, c, b in CASES]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
