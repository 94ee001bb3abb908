#!/usr/bin/env python3
"""ecfft_poly_divrem and ecfft_poly_inv_series against ecfft_poly_mul at the same N, in one process on warmed shapes, device-resident
data (host clock after a device synchronise, median of `reps` calls, the variants alternating call by call):
    divrem        FFTree.poly_divrem(a, b): q and r, na = 2^a, nb = 2^b + 1 (nq = nr = 2^b, N = 2^a)
    inv_series    FFTree.poly_inv_series(rev(b), nq): the reciprocal alone (base case + Newton steps)
    base          FFTree.poly_inv_series(rev(b), 64): the k_series_base launch alone (no transform)
    q_product     FFTree.poly_mul of two nq-coefficient operands: the quotient product (N = next_pow2(2 nq - 1))
    r_product     FFTree.poly_mul of nr and min(nq, nr) coefficients: the remainder product
    poly_mul_N    FFTree.poly_mul of two N/2-coefficient operands: the yardstick
The phase split of one divrem is read from these: base case, Newton steps = inv_series - base, quotient product, remainder product,
and the rest (reversals, the subtraction, the flag read-back).
usage: polydiv_time.py [reps] > profiles/polydiv/polydiv_time.json ; prints one JSON object"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecfft_amd  # noqa: E402

CASES = [("secp256k1", 20, 19, 1), ("secp256k1", 16, 15, 1), ("secp256k1", 19, 18, 8), ("m31", 24, 23, 1)]   # (field, a, b, count)


def rand_dev(field, rows, seed):
    rng = np.random.default_rng(seed)
    if field == "m31":
        return torch.from_numpy(rng.integers(1, 2**31 - 1, rows, dtype=np.uint32).view(np.int32)).cuda()
    a = rng.integers(0, 2**64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)                                  # < 2^255 < p: a reduced residue
    a[:, 0] |= np.uint64(1)                                   # nonzero
    return torch.from_numpy(a.view(np.int64)).cuda()


def run_case(field, log_a, log_b, count, reps):
    na, nb = 1 << log_a, (1 << log_b) + 1
    nq, nr = na - nb + 1, nb - 1
    N = 1 << log_a
    t = ecfft_amd.FIELDS[field].build_fftree(N)
    a, b = rand_dev(field, count * na, 1), rand_dev(field, count * nb, 2)
    fr = torch.flip(b.view(count, nb, -1), [1]).reshape(b.shape).contiguous()    # rev(b), count rows
    x, y = rand_dev(field, count * nq, 3), rand_dev(field, count * nq, 4)
    mq = min(nq, nr)
    xr, yr = rand_dev(field, count * nr, 5), rand_dev(field, count * mq, 6)
    h, hh = rand_dev(field, count * (N // 2), 7), rand_dev(field, count * (N // 2), 8)
    ops = {"divrem": lambda: t.poly_divrem(a, b, count=count),
           "inv_series": lambda: t.poly_inv_series(fr, nq, count=count),
           "base": lambda: t.poly_inv_series(fr, 64, count=count),
           "q_product": lambda: t.poly_mul(x, y, count=count),
           "r_product": lambda: t.poly_mul(xr, yr, count=count),
           "poly_mul_N": lambda: t.poly_mul(h, hh, count=count)}
    for _ in range(2):
        for f in ops.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in ops}
    for _ in range(reps):
        for k, f in ops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    split = {"base_case": med["base"], "newton_steps": med["inv_series"] - med["base"], "quotient_product": med["q_product"],
             "remainder_product": med["r_product"]}
    split["rest"] = med["divrem"] - sum(split.values())
    del t
    torch.cuda.empty_cache()
    return {"field": field, "na": na, "nb": nb, "nq": nq, "nr": nr, "N": N, "count": count, "reps": reps,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_ms": {k: round(min(v), 4) for k, v in ts.items()},
            "divrem_over_poly_mul_N": round(med["divrem"] / med["poly_mul_N"], 3),
            "inv_series_over_poly_mul_N": round(med["inv_series"] / med["poly_mul_N"], 3),
            "phase_split_ms": {k: round(v, 4) for k, v in split.items()}}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    torch.zeros(1, device="cuda")
    out = {"device": ecfft_amd.device_info(0), "cases": [run_case(f, a, b, c, reps) for f, a, b, c in CASES]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
