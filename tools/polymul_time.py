#!/usr/bin/env python3
"""ecfft_poly_mul against the transforms it is made of, in one process on warmed shapes, device-resident data (host clock after a
device synchronise, median of `reps` calls, the variants alternating call by call):
    poly_mul          FFTree.poly_mul(a, b): both operands entered at N/2 and lifted, k_poly_pointwise, EXIT_N
    enter_exit        the same-size ENTER_N + EXIT_N of one zero-padded operand (the floor the lifted form aims at)
    naive             what a user writes by hand: ENTER_N of both zero-padded operands, the pointwise product (here ecfft_poly_mul on
                      count * N length-1 "polynomials", i.e. k_poly_pointwise plus a device copy of each operand and of the result),
                      EXIT_N
    naive_no_product  the naive composition without its product step (2 ENTER_N + EXIT_N): a lower bound of any hand-written form
plus the per-class split of one poly_mul call from ecfft_profile_read (HIP events around every launch; the product kernel is the
"pointwise" class), and a check that poly_mul and the naive composition agree element for element.
usage: polymul_time.py [reps] > profiles/.../polymul_time.json ; prints one JSON object"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecfft_amd  # noqa: E402

CASES = [("secp256k1", 19, 1), ("secp256k1", 15, 1), ("m31", 23, 1), ("secp256k1", 19, 8)]   # (field, log2 operand length, count)


def rand_dev(field, rows, seed):
    rng = np.random.default_rng(seed)
    if field == "m31":
        return torch.from_numpy(rng.integers(0, 2**31 - 1, rows, dtype=np.uint32).view(np.int32)).cuda()
    a = rng.integers(0, 2**64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)                                  # < 2^255 < p: a reduced residue
    return torch.from_numpy(a.view(np.int64)).cuda()


def padded(x, count, n, N):
    out = torch.zeros((count * N,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    out.view(count, N, -1)[:, :n] = x.view(count, n, -1)
    return out


def run_case(field, log_n, count, reps):
    n = 1 << log_n
    N = 2 * n                                                 # N = next_pow2(2n - 1)
    t = ecfft_amd.FIELDS[field].build_fftree(N)
    a, b = rand_dev(field, count * n, 1), rand_dev(field, count * n, 2)
    ap, bp = padded(a, count, n, N), padded(b, count, n, N)

    def poly_mul():
        return t.poly_mul(a, b, count=count)

    def enter_exit():
        return t.exit(t.enter(ap, count=count), count=count)

    def naive():
        ea, eb = t.enter(ap, count=count), t.enter(bp, count=count)
        return t.exit(t.poly_mul(ea, eb, count=count * N), count=count)

    def naive_no_product():
        ea, eb = t.enter(ap, count=count), t.enter(bp, count=count)
        return t.exit(ea, count=count), eb

    ops = {"poly_mul": poly_mul, "enter_exit": enter_exit, "naive": naive, "naive_no_product": naive_no_product}
    for _ in range(3):
        for f in ops.values():
            f()
    torch.cuda.synchronize()
    c, cn = poly_mul(), naive()
    torch.cuda.synchronize()
    agree = bool(torch.equal(c.view(count, 2 * n - 1, -1), cn.view(count, N, -1)[:, :2 * n - 1])) and \
        not bool(cn.view(count, N, -1)[:, 2 * n - 1:].any())
    ts = {k: [] for k in ops}
    for _ in range(reps):
        for k, f in ops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    # per-class split of poly_mul (and of the same-size ENTER + EXIT) from the HIP events around every launch
    split = {}
    for k in ("poly_mul", "enter_exit"):
        t.profile(True)
        for _ in range(reps):
            ops[k]()
        torch.cuda.synchronize()
        cls = t.profile_read()
        t.profile(False)
        split[k] = {r["name"]: {"ms": round(r["ms"] / reps, 4), "launches": r["launches"] // reps,
                                "alg_GB_s": round(r["alg_bytes"] / (r["ms"] * 1e-3) / 1e9, 1) if r["ms"] else None}
                    for r in cls if r["launches"]}
    prod_ms = split["poly_mul"].get("pointwise", {}).get("ms")
    del t
    torch.cuda.empty_cache()
    return {"field": field, "na": n, "nb": n, "N": N, "count": count, "reps": reps, "bit_exact_vs_naive": agree,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_ms": {k: round(min(v), 4) for k, v in ts.items()},
            "poly_mul_over_enter_exit": round(med["poly_mul"] / med["enter_exit"], 4),
            "poly_mul_over_naive": round(med["poly_mul"] / med["naive"], 4),
            "product_kernel_us": None if prod_ms is None else round(prod_ms * 1e3, 1),
            "class_split_ms": split}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    torch.zeros(1, device="cuda")
    out = {"device": ecfft_amd.device_info(0), "cases": [run_case(f, ln, c, reps) for f, ln, c in CASES]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
