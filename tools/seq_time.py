#!/usr/bin/env python3
"""ecfft_seq_min_poly and ecfft_seq_nth_term against the same results composed from the calls that existed before them, in one
process on warmed shapes (host clock after a device synchronise, median of `reps` calls, the variants alternating call by call,
the whole measurement repeated `blocks` times to see the spread between medians).
  min_poly cases (rows of N uniform terms, N even: linear complexity N / 2, the longest remainder sequence that is determined):
    seq_min_poly    FFTree.seq_min_poly(seq, count): all rows in one call, device tensors in and out
    xgcd_partial    FFTree.poly_xgcd_partial(x^N rows, seq, N / 2, count) on operands already staged: the device part of composed
    composed        what a caller had to do: stage count rows of x^N, FFTree.poly_xgcd_partial, read t and the degrees back, decide
                    the verdict, invert t(0) and reverse t on the host through the standard-form converters, upload C
  nth_term cases (random monic C of degree L, random initial terms, one index K shared by the rows, nout = 1):
    seq_nth_term    FFTree.seq_nth_term(C, init, K, count)
    pow_mod         FFTree.poly_pow_mod(x rows, K, C, count) alone: the device part of composed
    composed        pow_mod, a download and the dot product with the initial terms on the host (numpy for M31, Python integers
                    through the converters for secp256k1), upload
A composed variant whose host part handles more than 2^16 elements runs once per block, not `reps` times.  Results are checked:
both routes return the same bytes, and every order is N / 2.
usage: seq_time.py [reps [blocks]] > profiles/seq/seq_time.json ; prints one JSON object"""
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

MIN_POLY = [(64, 1), (64, 64), (64, 4096), (254, 1), (254, 64), (254, 4096), (1024, 1), (4096, 1)]
NTH_TERM = [(16, 1), (16, 4096), (64, 1), (64, 4096), (256, 1), (256, 8), (1024, 1), (1024, 8)]


def rand_np(field, rows, seed):
    rng = np.random.default_rng(seed)
    if field == "m31":
        return rng.integers(1, 2**31 - 1, rows, dtype=np.uint32)
    a = rng.integers(0, 2**64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)                                  # < 2^255 < p: a reduced residue
    a[:, 0] |= np.uint64(1)                                   # nonzero
    return a


def dev(field, x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if field == "m31" else np.int64)).cuda()


def host(F, x):
    return x.cpu().numpy().view(F.dtype)


def measure(ops, once, reps, blocks):
    """ops: name -> callable; once: the names that run once per block.  -> (median ms, block medians)"""
    for fn in ops.values():
        fn()
    torch.cuda.synchronize()
    meds = {name: [] for name in ops}
    for _ in range(blocks):
        ts = {name: [] for name in ops}
        for i in range(reps):
            for name, fn in ops.items():
                if name in once and i:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        for name in ops:
            meds[name].append(float(np.median(ts[name])))
    return {name: float(np.median(v)) for name, v in meds.items()}, meds


def report(case, med, meds, new, base):
    spread = {name: max(v) - min(v) for name, v in meds.items()}
    case.update({"median_ms": {k: round(v, 4) for k, v in med.items()}, "spread_ms": {k: round(v, 4) for k, v in spread.items()},
                 "block_medians_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
                 "composed_over_" + new: round(med["composed"] / med[new], 2), base + "_over_" + new: round(med[base] / med[new], 2),
                 # the one condition of the small regime: not slower than composed by more than the spread this run records
                 "new_minus_composed_ms": round(med[new] - med["composed"], 4),
                 "not_slower_than_composed_within_spread": bool(med[new] - med["composed"] <= spread[new] + spread["composed"])})
    return case


def tree_for(F, leaves):
    size = 4
    while size < leaves:
        size <<= 1
    return F.build_fftree(size), size


def min_poly_case(field, n, count, reps, blocks):
    F = ecfft_amd.FIELDS[field]
    p = F.MODULUS[field]
    t, size = tree_for(F, 2 * n + 1)
    nh = n // 2 + 1
    seq = dev(field, rand_np(field, count * n, 10 + n))
    xn_row = F.from_ints([0] * n + [1])

    def stage():
        return dev(field, np.tile(xn_row, (count,) + (1,) * (xn_row.ndim - 1)))

    xn = stage()

    def composed():
        r, s, tt, deg = t.poly_xgcd_partial(stage(), seq, n // 2, count=count)
        th = host(F, tt)
        out = np.zeros_like(th[:count * nh])
        orders = np.full(count, -1, np.int64)
        for b in range(count):
            d = max(int(deg[b, 0]) + 1, int(deg[b, 2]))
            if 2 * d > n:
                continue
            row = F.to_ints(th[b * (n + 1):b * (n + 1) + d + 1])
            if row[0] == 0:
                continue
            inv = pow(row[0], p - 2, p)
            out[b * nh:b * nh + d + 1] = F.from_ints([c * inv % p for c in reversed(row)])
            orders[b] = d
        return dev(field, out), orders

    ops = {"seq_min_poly": lambda: t.seq_min_poly(seq, count=count),
           "xgcd_partial": lambda: t.poly_xgcd_partial(xn, seq, n // 2, count=count), "composed": composed}
    mp, orders = ops["seq_min_poly"]()
    cmp_, corders = composed()
    assert (orders == n // 2).all() and (corders == orders).all() and torch.equal(mp, cmp_), "the two routes disagree"
    med, meds = measure(ops, {"composed"} if count * n > 1 << 16 else set(), reps, blocks)
    case = {"call": "seq_min_poly", "field": field, "n_terms": n, "count": count, "tree": size, "reps": reps, "blocks": blocks,
            "regime": "small" if n <= FT.SEQ_SMALL_MAX else "large", "us_per_row": round(1e3 * med["seq_min_poly"] / count, 3)}
    del t
    torch.cuda.empty_cache()
    return report(case, med, meds, "seq_min_poly", "xgcd_partial")


def nth_term_case(field, L, count, kname, K, reps, blocks):
    F = ecfft_amd.FIELDS[field]
    p = F.MODULUS[field]
    t, size = tree_for(F, 2 * L - 1 if L > 64 else 4)
    cp = rand_np(field, count * (L + 1), 20 + L)
    one = F.from_ints([1])
    for b in range(count):
        cp[b * (L + 1) + L] = one[0]
    cp = dev(field, cp)
    init_np = rand_np(field, count * L, 30 + L)
    init = dev(field, init_np)
    x = dev(field, np.tile(F.from_ints([0, 1]), (count,) + (1,) * (one.ndim - 1)))

    def composed():
        u = host(F, t.poly_pow_mod(x, K, cp, count=count))
        if field == "m31":
            prod = (u.astype(np.uint64) * init_np.astype(np.uint64)) % np.uint64(p)
            out = (prod.reshape(count, L).sum(axis=1) % np.uint64(p)).astype(np.uint32)
        else:
            ui, si = F.to_ints(u), F.to_ints(init_np)
            out = F.from_ints([sum(a * b for a, b in zip(ui[b * L:(b + 1) * L], si[b * L:(b + 1) * L])) % p for b in range(count)])
        return dev(field, out)

    ops = {"seq_nth_term": lambda: t.seq_nth_term(cp, init, K, count=count), "pow_mod": lambda: t.poly_pow_mod(x, K, cp, count=count),
           "composed": composed}
    assert torch.equal(ops["seq_nth_term"](), composed()), "the two routes disagree"
    med, meds = measure(ops, {"composed"} if count * L > 1 << 16 and field != "m31" else set(), reps, blocks)
    case = {"call": "seq_nth_term", "field": field, "order": L, "count": count, "index": kname, "index_bits": K.bit_length(), "tree": size,
            "reps": reps, "blocks": blocks, "regime": "small" if L + 1 <= FT.SEQ_TERM_SMALL_MAX else "large",
            "us_per_row": round(1e3 * med["seq_nth_term"] / count, 3)}
    del t
    torch.cuda.empty_cache()
    return report(case, med, meds, "seq_nth_term", "pow_mod")


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    reps, blocks = arg(1, 5), arg(2, 3)
    torch.zeros(1, device="cuda")
    cases = []

    def add(case):
        cases.append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)

    for field in ("secp256k1", "m31"):
        p = ecfft_amd.FIELDS[field].MODULUS[field]
        for n, count in MIN_POLY:
            add(min_poly_case(field, n, count, reps, blocks))
        for L, count in NTH_TERM:
            for kname, K in (("64-bit", 2**64 - 59), ("field-sized", p - 2)):
                add(nth_term_case(field, L, count, kname, K, reps, blocks))
    small = [c for c in cases if c["regime"] == "small" and c["count"] >= 64]
    print(json.dumps({"device": ecfft_amd.device_info(0), "seq_small_max": FT.SEQ_SMALL_MAX, "seq_term_small_max": FT.SEQ_TERM_SMALL_MAX,
                      "small_regime_count_ge_64_not_slower_than_composed": all(c["not_slower_than_composed_within_spread"] for c in small),
                      "cases": cases}))


if __name__ == "__main__":
    main()
