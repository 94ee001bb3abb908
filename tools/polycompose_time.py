#!/usr/bin/env python3
"""ecfft_poly_compose_mod against Horner's scheme written from the public ecfft_poly_mul_mod and against a fresh modular power at the
same size, in one process on warmed shapes, device-resident data (host clock after a device synchronise, median of `reps` calls, the
variants alternating call by call, the whole measurement repeated `blocks` times to see the spread between medians).  nf = ng = d,
count = 1, a random modulus of d + 1 coefficients; then a sweep of short f (nf = 2 .. 16 at d = 64 and 256) for the smallest nf from
which the call stays below Horner by more than the spread:
    compose       FFTree.poly_compose_mod(f, g, h)
    horner        res = f[nf-1]; res = poly_mul_mod(res, g, h), res[0] += f[i] for i = nf - 2 .. 0 (the constant is added on the host: one
                  element each way per step).  Not run from the first size on at which one call exceeds `horner_max_s` seconds.
    pow_mod       FFTree.poly_pow_mod(a, p, h): what a caller without composition pays per Frobenius iterate
From ecfft_profile_read, one profiled call each (HIP events around every launch; not the timed calls):
    exit_launches          launches of the k_exit_low class in one compose call, and in one with nf = 2, which runs the same setup and no
                           modular product; their difference next to the schedule's 3 (k + k' - 2).  (One per batched EXIT where the
                           low levels of an EXIT are fused; a field whose EXIT of N runs level by level shows 0.)
    launches               the same for the launches of all classes together, next to (k + k' - 2) times the launches of one product
                           with a kept operand (poly_pow_mod with exponents 255 and 128: seven multiplies apart); the one lift of the
                           giant step comes on top
    pointwise_ms           the `pointwise` class of the compose call: pads, pointwise products and subtractions of every product, and
                           k_compose_rows.  The class does not separate one kernel; k_compose_rows' own time is read from a kernel trace
                           (profiles/README.md)
usage: polycompose_time.py [reps [blocks [horner_max_s [max_log_secp [max_log_m31]]]]] > profiles/polycompose/polycompose_time.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ecfft_amd  # noqa: E402

P = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}


def rand_dev(field, rows, seed):
    rng = np.random.default_rng(seed)
    if field == "m31":
        return torch.from_numpy(rng.integers(1, 2**31 - 1, rows, dtype=np.uint32).view(np.int32)).cuda()
    a = rng.integers(0, 2**64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)                                  # < 2^255 < p: a reduced residue
    a[:, 0] |= np.uint64(1)                                   # nonzero
    return torch.from_numpy(a.view(np.int64)).cuda()


def stored_ints(field, x):
    """the stored numbers (in-memory form) of a device tensor as Python ints: adding two of them mod p is the field's addition"""
    raw = x.cpu().numpy().tobytes()
    w = 4 if field == "m31" else 32
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def stored_tensor(field, v, like):
    w = 4 if field == "m31" else 32
    a = np.frombuffer(int(v).to_bytes(w, "little"), dtype=np.int32 if field == "m31" else np.int64).copy()
    return torch.from_numpy(a).reshape((1,) + tuple(like.shape[1:])).to(like.device)


def chunking(nf):
    k = 1
    while k * k < nf:
        k += 1
    return k, (nf + k - 1) // k


def classes_of(t, fn):
    """the kernel classes of one profiled call of fn, by name"""
    fn()
    t.profile(True)
    fn()
    c = {c["name"]: c for c in t.profile_read()}
    t.profile(False)
    return c


def run_case(field, d, nf, reps, blocks, horner_ok, horner_max_s, full=True):
    p = P[field]
    N = 2
    while N < 2 * d - 1:
        N <<= 1
    t = ecfft_amd.FIELDS[field].build_fftree(N)
    f, g, h, a = rand_dev(field, nf, 1), rand_dev(field, d, 2), rand_dev(field, d + 1, 3), rand_dev(field, d, 4)
    fi = stored_ints(field, f)

    def horner():
        res = torch.zeros_like(g)
        res[0:1] = f[nf - 1:nf]
        for i in range(nf - 2, -1, -1):
            res = t.poly_mul_mod(res, g, h)
            res[0:1] = stored_tensor(field, (stored_ints(field, res[0:1])[0] + fi[i]) % p, res)
        return res

    ops = {"compose": lambda: t.poly_compose_mod(f, g, h)}
    if full:
        ops["pow_mod"] = lambda: t.poly_pow_mod(a, p, h)
    want = ops["compose"]()
    horner_first_s, same = None, None
    if horner_ok:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = horner()
        torch.cuda.synchronize()
        horner_first_s = time.perf_counter() - t0
        same = bool(torch.equal(got, want))
        if horner_first_s <= horner_max_s:
            ops["horner"] = horner
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
    spread = {k: max(v) - min(v) for k, v in meds.items()}
    k, kp = chunking(nf)
    out = {"field": field, "d": d, "nf": nf, "N": N, "k": k, "k_prime": kp, "modular_products": (k - 1) + (kp - 1), "horner_products": nf - 1,
           "pow_mod_products": p.bit_length() - 1 + bin(p).count("1") - 1, "reps": reps, "blocks": blocks,
           "median_ms": {n: round(v, 4) for n, v in med.items()}, "spread_ms": {n: round(v, 4) for n, v in spread.items()},
           "block_medians_ms": {n: [round(x, 4) for x in v] for n, v in meds.items()}}
    if full:
        out["compose_over_pow_mod"] = round(med["compose"] / med["pow_mod"], 4)
    if horner_first_s is not None:
        out["horner_same_bytes"] = same
        out["horner_first_call_s"] = round(horner_first_s, 3)
    if "horner" in med:
        out["horner_over_compose"] = round(med["horner"] / med["compose"], 2)
        out["below_horner_by_more_than_spread"] = bool(min(meds["horner"]) - max(meds["compose"]) > max(spread["horner"], spread["compose"]))
    if full and d > 64:                                       # the large regime: the schedule as the profiler saw it
        two = lambda: t.poly_compose_mod(f[:2], g, h)
        c1, c2 = classes_of(t, ops["compose"]), classes_of(t, two)
        ex, ex2, pw, pw2 = c1["k_exit_low"], c2["k_exit_low"], c1["pointwise"], c2["pointwise"]
        m255, m128 = (classes_of(t, lambda e=e: t.poly_pow_mod(a, e, h)) for e in (255, 128))
        total = lambda c: sum(v["launches"] for v in c.values())
        per_product = (total(m255) - total(m128)) / 7
        out.update({"exit_launches": ex["launches"], "exit_launches_nf2": ex2["launches"],
                    "exit_launches_of_products": ex["launches"] - ex2["launches"], "expected_3_k_kp_2": 3 * (k + kp - 2),
                    "launches": total(c1), "launches_nf2": total(c2), "launches_per_product": round(per_product, 2),
                    "launches_of_products_over_per_product": round((total(c1) - total(c2)) / per_product, 2), "expected_k_kp_2": k + kp - 2,
                    "pointwise_ms": round(pw["ms"], 4), "pointwise_ms_nf2": round(pw2["ms"], 4)})
    elif full:
        pw = classes_of(t, ops["compose"])["pointwise"]
        out["pointwise_ms"] = round(pw["ms"], 4)              # k_compose_small, the one launch of the call
    del t
    torch.cuda.empty_cache()
    return out, "horner" in med


def crossing(cases, key):
    """the smallest d from which `compose` stays above the other column (None: never in the table)"""
    first = None
    for c in cases:
        if key not in c["median_ms"]:
            continue
        if c["median_ms"]["compose"] >= c["median_ms"][key]:
            first = first if first is not None else c["d"]
        else:
            first = None
    return first


def main():
    arg = lambda i, dflt, conv: conv(sys.argv[i]) if len(sys.argv) > i else dflt
    reps, blocks, horner_max_s = arg(1, 5, int), arg(2, 3, int), arg(3, 4.0, float)
    max_log = {"secp256k1": arg(4, 12, int), "m31": arg(5, 14, int)}
    torch.zeros(1, device="cuda")
    cases = []
    for field in ("secp256k1", "m31"):
        horner_ok = True
        for d in (16, 64, 256, 1 << 10, 1 << 12, 1 << 14):
            if d > (1 << max_log[field]):
                continue
            c, ran = run_case(field, d, d, reps, blocks, horner_ok, horner_max_s)
            horner_ok = horner_ok and ran
            cases.append(c)
            print(json.dumps(c), file=sys.stderr, flush=True)
    # the smallest nf at which the call is below Horner by more than the spread: short f against residues of both regimes
    sweep = []
    for field in ("secp256k1", "m31"):
        for d in (64, 256):
            for nf in (2, 3, 4, 5, 8, 16):
                sweep.append(run_case(field, d, nf, reps, blocks, True, horner_max_s, full=False)[0])
    smallest = {}
    for c in sweep:
        key = f"{c['field']} d={c['d']}"
        if c.get("below_horner_by_more_than_spread") and key not in smallest:
            smallest[key] = c["nf"]
        elif not c.get("below_horner_by_more_than_spread"):
            smallest.pop(key, None)
    by_field = {f: [c for c in cases if c["field"] == f] for f in ("secp256k1", "m31")}
    out = {"device": ecfft_amd.device_info(0), "cases": cases, "nf_sweep": sweep, "below_horner_from_nf": smallest,
           "compose_not_below_pow_mod_from_d": {f: crossing(v, "pow_mod") for f, v in by_field.items()},
           "compose_not_below_horner_from_d": {f: crossing(v, "horner") for f, v in by_field.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
