#!/usr/bin/env python3
"""ecfft_rs_encode and ecfft_rs_decode_erasures against what a caller had before them, in one process on warmed shapes,
device-resident data (host clock after a device synchronise, median of `reps` calls, the variants alternating call by call, the
whole measurement repeated `blocks` times to see the spread between medians).
Decoder, three kinds of received words per shape (e0 = floor((m - k) / 2), the most the code corrects without erasures):
    clean       no erasure, e0 errors per row
                  rs_decode            FFTree.rs_decode: the decoder these words do not need more than
                  erasures_nomask      FFTree.rs_decode_erasures(erased=None)
                  erasures_zero_mask   FFTree.rs_decode_erasures with an all-zero mask: what the new prologue costs such a word
    mixed       s = e0 erasures and floor((m - s - k) / 2) errors per row, the mask of every row drawn on its own
    erased      s = m - k erasures, no error
                  erasures             FFTree.rs_decode_erasures on all rows in one call, coefficients out
                  erasures_codeword    the same with the re-encoded codeword out
                  per_mask             the path a caller had: per row (every mask is distinct) the kept points and values gathered
                                       with an index built on the host, and ONE FFTree.rs_decode call on them.  Above `rows_max`
                                       rows only that many are run and the time is scaled (`per_mask_is_scaled`).
Encoder:
    rs_encode       FFTree.rs_encode on all rows
    composed        FFTree.poly_interpolate at the first k points, then FFTree.poly_eval_points at the other m - k
Results are checked before anything is timed: every decoder path returns the coefficients of the data that were encoded (and the
codeword form the codeword that was sent), both encoder paths return the same parity.
usage: rscodec_time.py [reps [blocks [rows_max]]] > profiles/rscodec/rscodec_time.json ; prints one JSON object"""
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


def measure(ops, reps, blocks, once=()):
    """{name: (median of block medians, spread, block medians)} in ms; the names in `once` run once per block"""
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
    return {name: (float(np.median(v)), max(v) - min(v), v) for name, v in meds.items()}


def report(res):
    return {"median_ms": {n: round(v[0], 4) for n, v in res.items()}, "spread_ms": {n: round(v[1], 4) for n, v in res.items()},
            "block_medians_ms": {n: [round(x, 4) for x in v[2]] for n, v in res.items()}}


def run_case(field, m, k, count, reps, blocks, rows_max):
    F = ecfft_amd.FIELDS[field]
    size = 4
    while size < 4 * (m + 1):
        size <<= 1
    t = F.build_fftree(size)
    e0 = (m - k) // 2
    pts_np = rand_np(field, m, 1)
    pts = dev(field, pts_np)
    data = dev(field, rand_np(field, count * k, 2))
    rows = min(count, rows_max)
    out = {"field": field, "m": m, "k": k, "count": count, "tree": size, "reps": reps, "blocks": blocks}

    # ---- encoder ----
    def composed_encode():
        coef = t.poly_interpolate(pts[:k], data, count=count)
        return coef, t.poly_eval_points(coef, pts[k:], count=count)

    sent = t.rs_encode(pts, data, k, count=count)
    coef, par = composed_encode()
    sent2 = sent.reshape((count, m) + tuple(sent.shape[1:]))
    assert torch.equal(sent2[:, :k].reshape(data.shape), data), "rs_encode does not carry the data through"
    assert torch.equal(sent2[:, k:].reshape(par.shape), par), "rs_encode and the composed encoder disagree"
    res = measure({"rs_encode": lambda: t.rs_encode(pts, data, k, count=count), "composed": composed_encode}, reps, blocks)
    out["encode"] = report(res)
    out["encode"]["composed_over_rs_encode"] = round(res["composed"][0] / res["rs_encode"][0], 2)
    out["encode"]["rs_encode_us_per_row"] = round(1e3 * res["rs_encode"][0] / count, 3)

    # ---- decoder ----
    def received(s, e, seed):
        """(words on the device, mask on the host): s positions of every row lost and filled with noise, e of the others changed"""
        rng = np.random.default_rng(seed)
        words, mask = sent.cpu().numpy().copy(), np.zeros((count, m), np.uint8)
        noise = rand_np(field, count * (s + e) + 1, seed + 1)
        for b in range(count):
            pos = rng.choice(m, s + e, replace=False)
            mask[b, pos[:s]] = 1
            words[pos + b * m] = noise[b * (s + e):(b + 1) * (s + e)]
        return torch.from_numpy(words).cuda(), mask

    def per_mask(words, mask):
        """today's path on the first `rows` rows: a host-built index per row, a gather, one rs_decode call"""
        got = []
        for b in range(rows):
            idx = torch.from_numpy(np.nonzero(mask[b] == 0)[0]).cuda()
            got.append(t.rs_decode(pts[idx].contiguous(), words[b * m:(b + 1) * m][idx].contiguous(), k))
        return got

    words, mask = received(0, e0, 10)
    zero = torch.from_numpy(mask.reshape(-1)).cuda()
    ops = {"rs_decode": lambda: t.rs_decode(pts, words, k, count=count),
           "erasures_nomask": lambda: t.rs_decode_erasures(pts, words, None, k, count=count),
           "erasures_zero_mask": lambda: t.rs_decode_erasures(pts, words, zero, k, count=count)}
    for name, fn in ops.items():
        msg, n_err = fn()
        assert torch.equal(msg, coef) and (n_err == e0).all(), f"{name} did not return the encoded data"
    res = measure(ops, reps, blocks)
    out["clean"] = report(res)
    out["clean"].update({"erasures": 0, "errors": e0, "zero_mask_over_rs_decode": round(res["erasures_zero_mask"][0] / res["rs_decode"][0], 3)})

    for kind, s in (("mixed", e0), ("erased", m - k)):
        e = (m - s - k) // 2
        words, mask = received(s, e, 20 + s)
        dmask = torch.from_numpy(mask.reshape(-1)).cuda()
        ops = {"erasures": lambda: t.rs_decode_erasures(pts, words, dmask, k, count=count),
               "erasures_codeword": lambda: t.rs_decode_erasures(pts, words, dmask, k, count=count, codeword=True),
               "per_mask": lambda: per_mask(words, mask)}
        msg, n_err = ops["erasures"]()
        assert torch.equal(msg, coef) and (n_err == e).all(), "rs_decode_erasures did not return the encoded data"
        word, n_err = ops["erasures_codeword"]()
        assert torch.equal(word, sent) and (n_err == e).all(), "rs_decode_erasures did not return the codeword that was sent"
        for b, (msg, n_err) in enumerate(ops["per_mask"]()):
            assert torch.equal(msg, coef[b * k:(b + 1) * k]) and n_err[0] == e, "the per-mask path did not return the encoded data"
        res = measure(ops, reps, blocks, once=("per_mask",) if m > 1024 else ())
        scaled = res["per_mask"][0] * count / rows
        out[kind] = report(res)
        out[kind].update({"erasures": s, "errors": e, "per_mask_rows_measured": rows, "per_mask_ms": round(scaled, 4), "per_mask_is_scaled": rows < count,
                          "per_mask_over_erasures": round(scaled / res["erasures"][0], 2),
                          "erasures_us_per_row": round(1e3 * res["erasures"][0] / count, 3)})
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
