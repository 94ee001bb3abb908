#!/usr/bin/env python3
"""ecfft_rs_decode and ecfft_poly_xgcd_partial against the only alternative there was before them, composed from public calls, in
one process on warmed shapes, device-resident data (host clock after a device synchronise, median of `reps` calls, the variants
alternating call by call, the whole measurement repeated `blocks` times to see the spread between medians).  Every row carries
floor((m - k) / 2) errors, the most the code corrects, so the remainder sequence runs its full length.
    rs_decode       FFTree.rs_decode(points, values, k, count): all rows in one call
    xgcd_partial    FFTree.poly_xgcd_partial(g0, g1, ceil((m + k) / 2)) on the rows' interpolants: the part of rs_decode it exposes
    the decoder composed from public calls, in its two parts:
    interpolate     ONE FFTree.poly_interpolate for all rows
    euclid_rows     per row the Euclid loop r_{i+1} = r_{i-1} mod r_i by one FFTree.poly_divrem per remainder, stopped by reading
                    the remainder's degree back; the cofactor t_{i+1} = t_{i-1} - q_i t_i is kept by FFTree.poly_mul (the library
                    has no public addition, so the sum of the two products is read out of ONE product: (t_i + x^N t_{i-1})
                    (1 - q_i x^N) holds it in its coefficients N .. 2N - 1, and -q_i is the product of q_i with the constant
                    -1); a final FFTree.poly_divrem gives f = r / t.  g0 is computed once, outside the clock.  Above `rows_max`
                    rows only that many are run (`euclid_rows_measured`); the rows are independent and run one after another.
    composed_ms = interpolate + euclid_rows * count / euclid_rows_measured: measured where all rows were run, else scaled.
Results are checked: rs_decode returns the messages that were encoded and floor((m - k) / 2) errors per row, and so does composed.
usage: rsdecode_time.py [reps [blocks [rows_max]]] > profiles/rsdecode/rsdecode_time.json ; prints one JSON object"""
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

SHAPES = {"secp256k1": [(255, 223, 1), (255, 223, 4096), (1024, 768, 1)], "m31": [(255, 223, 1), (255, 223, 4096), (4096, 3072, 1)]}


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


def vanishing(F, pts_np):
    """prod (x - x_i) as in-memory elements, on the host"""
    p, out = F.MODULUS[F.name], [1]
    for x in F.to_ints(pts_np):
        nxt = [0] + out
        for i, c in enumerate(out):
            nxt[i] = (nxt[i] - x * c) % p
        out = nxt
    return F.from_ints(out)


def true_len(x):
    """coefficients up to the last nonzero one: a degree read-back"""
    nz = (x != 0) if x.dim() == 1 else (x != 0).any(dim=1)
    idx = torch.nonzero(nz)
    return int(idx.max()) + 1 if idx.numel() else 0


def composed_row(t, g0, g1, stop, one, minus_one, N):
    """(f, deg t) of one row by public calls only, or None where the division leaves a remainder"""
    zeros = lambda n: torch.zeros((n,) + tuple(g0.shape[1:]), dtype=g0.dtype, device=g0.device)
    pad = lambda x: torch.cat([x, zeros(N - x.shape[0])])
    r0, r1 = g0, g1[:true_len(g1)]
    t0, t1 = zeros(N), pad(one)
    while r1.shape[0] - 1 >= stop:
        q, rem = t.poly_divrem(r0, r1)
        r0, r1 = r1, rem[:true_len(rem)]
        step = torch.cat([one, zeros(N - 1), t.poly_mul(q, minus_one)])
        t0, t1 = t1, t.poly_mul(torch.cat([t1, t0]), step)[N:2 * N].contiguous()
    lt = true_len(t1)
    if r1.shape[0] < lt:
        return None if r1.shape[0] else (zeros(0), lt - 1)
    f, rem = t.poly_divrem(r1, t1[:lt].contiguous())
    return (f, lt - 1) if true_len(rem) == 0 else None


def run_case(field, m, k, count, reps, blocks, rows_max):
    F = ecfft_amd.FIELDS[field]
    size = 4
    while size < 4 * (m + 1):
        size <<= 1
    t = F.build_fftree(size)
    e, stop, N = (m - k) // 2, (m + k + 1) // 2, m + 1
    pts_np = rand_np(field, m, 1)
    pts = dev(field, pts_np)
    g0 = dev(field, vanishing(F, pts_np))
    one, minus_one = dev(field, F.from_ints([1])), dev(field, F.from_ints([F.MODULUS[field] - 1]))
    msg = dev(field, rand_np(field, count * k, 2))
    words = t.poly_eval_points(msg, pts, count=count).cpu().numpy().copy()
    rng, noise = np.random.default_rng(3), rand_np(field, count * e + 1, 4)
    for b in range(count):
        pos = rng.choice(m, e, replace=False) + b * m
        words[pos] = noise[b * e:(b + 1) * e]
    words = torch.from_numpy(words).cuda()
    rows = min(count, rows_max)

    g1_all = t.poly_interpolate(pts, words, count=count)
    g0_all = g0.repeat((count,) + (1,) * (g0.dim() - 1))

    def euclid_rows():
        return [composed_row(t, g0, g1_all[b * m:(b + 1) * m], stop, one, minus_one, N) for b in range(rows)]

    ops = {"rs_decode": lambda: t.rs_decode(pts, words, k, count=count),
           "xgcd_partial": lambda: t.poly_xgcd_partial(g0_all, g1_all, stop, count=count),
           "interpolate": lambda: t.poly_interpolate(pts, words, count=count), "euclid_rows": euclid_rows}
    message, n_err = ops["rs_decode"]()
    assert torch.equal(message, msg) and (n_err == e).all(), "rs_decode did not return the encoded messages"
    for b, got in enumerate(ops["euclid_rows"]()):
        assert got is not None and got[1] == e and torch.equal(got[0], msg[b * k:(b + 1) * k]), "the composed decoder disagrees"
    ops["xgcd_partial"]()
    torch.cuda.synchronize()
    meds = {name: [] for name in ops}
    for _ in range(blocks):
        ts = {name: [] for name in ops}
        for i in range(reps):
            for name, fn in ops.items():
                if name == "euclid_rows" and i and (m > 1024 or rows > 1):
                    continue                                  # hundreds of synchronous calls: once per block
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        for name in ops:
            meds[name].append(float(np.median(ts[name])))
    med = {name: float(np.median(v)) for name, v in meds.items()}
    composed = med["interpolate"] + med["euclid_rows"] * count / rows
    out = {"field": field, "m": m, "k": k, "count": count, "errors_per_row": e, "tree": size, "reps": reps, "blocks": blocks,
           "euclid_rows_measured": rows, "median_ms": {name: round(v, 4) for name, v in med.items()},
           "spread_ms": {name: round(max(v) - min(v), 4) for name, v in meds.items()},
           "block_medians_ms": {name: [round(x, 4) for x in v] for name, v in meds.items()},
           "composed_ms": round(composed, 4), "composed_is_scaled": rows < count,
           "composed_over_rs_decode": round(composed / med["rs_decode"], 2),
           "rs_decode_us_per_row": round(1e3 * med["rs_decode"] / count, 3)}
    del t
    torch.cuda.empty_cache()
    return out


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    reps, blocks, rows_max = arg(1, 5), arg(2, 3), arg(3, 8)
    torch.zeros(1, device="cuda")
    cases = []
    for field in ("secp256k1", "m31"):
        for m, k, count in SHAPES[field]:
            cases.append(run_case(field, m, k, count, reps, blocks, rows_max))
            print(json.dumps(cases[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"device": ecfft_amd.device_info(0), "rs_small_max": FT.RS_SMALL_MAX, "rows_max": rows_max, "cases": cases}))


if __name__ == "__main__":
    main()
