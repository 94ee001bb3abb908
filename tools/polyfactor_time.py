#!/usr/bin/env python3
"""ecfft_poly_factor against the factorisation a caller composed from the public calls that existed before it, in one process on
warmed shapes, host arrays on both sides (host clock around synchronous calls, median of `reps` calls, the two alternating call by
call, the whole measurement repeated `blocks` times to see the spread between medians).

Inputs are built from a spec, a list of (d, r, e): r distinct irreducibles of degree d, each at multiplicity e (the shapes of
tests/factor_ref.py: linear factors x - a, binomials x^d - a and their shifts); f = 3 prod q^e, `count` copies laid end to end.
    factor     FFTree.poly_factor(f, count): one call for all rows.
    baseline   per row: poly_distinct_degree(f), poly_equal_degree(g_d, d) per non-empty d (FFTree.poly_irreducible_factors), then
               the multiplicity of every factor by repeated poly_divrem of f until a remainder is not zero (the check on the host).
               The tool first asserts that it finds the factors and multiplicities of `factor`.  It makes count x (1 + degrees +
               divisions) synchronous calls; above `max_rows` rows it is timed on the first `max_rows` rows and scaled to count
               (baseline_rows_timed < count says so).
    launches   from ecfft_profile_read, one profiled call, all classes together (factor only).
usage: polyfactor_time.py [reps [blocks [max_rows]]] > profiles/polyfactor/polyfactor_time.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecfft_amd  # noqa: E402
from ecfft_amd import fftree as FT  # noqa: E402

P = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1}
SPECS = {
    "S1": [(1, 3, 1), (1, 2, 2), (2, 2, 1), (2, 1, 3), (3, 1, 2)],
    "S2": [(1, 10, 1), (1, 9, 2), (3, 2, 2), (2, 6, 1)],
    "L2": [(2, 35, 1), (1, 3, 2), (3, 1, 3)],
    "L3": [(1, 40, 1), (2, 20, 2), (7, 5, 1), (1, 6, 4)],
}
SHAPES = [("S1", 1), ("S1", 64), ("S1", 4096), ("S2", 1), ("S2", 64), ("S2", 4096), ("L2", 1), ("L3", 1)]


def conv(x, y, p):
    return [int(v) % p for v in np.convolve(np.array(x, dtype=object), np.array(y, dtype=object))]


def product(polys, p):
    level = [list(q) for q in polys]
    while len(level) > 1:
        nxt = [conv(level[i], level[i + 1], p) for i in range(0, len(level) - 1, 2)]
        if len(level) & 1:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def irreducibles(d, count, p):
    """x - a for d = 1; otherwise (x + s)^d - a for the first a >= 2 with a^((p-1)/q) != 1 for the prime q = d (2, 3 or 7: q | p - 1
    in both fields), s = 0, 1, ..."""
    if d == 1:
        return [[-a % p, 1] for a in range(2, 2 + count)]
    assert d in (2, 3, 7) and (p - 1) % d == 0
    nb, bins, a = max(1, (count + 3) // 4), [], 2
    while len(bins) < nb:
        if pow(a, (p - 1) // d, p) != 1:
            bins.append(a)
        a += 1
    out, s = [], 0
    while len(out) < count:
        xs = product([[s % p, 1]] * d, p)
        for a in bins:
            out.append([(xs[0] - a) % p] + xs[1:])
        s += 1
    return out[:count]


def build(spec, p):
    """(f, [(q, e), ...] in the call's order)"""
    total = {}
    for d, r, e in spec:
        total[d] = total.get(d, 0) + r
    pool = {d: irreducibles(d, n, p) for d, n in total.items()}
    used = {d: 0 for d in total}
    want, polys = [], []
    for d, r, e in spec:
        for q in pool[d][used[d]:used[d] + r]:
            want.append((q, e))
            polys += [q] * e
        used[d] += r
    return [3 * v % p for v in product(polys, p)], sorted(want, key=lambda qe: (qe[1], len(qe[0]), qe[0]))


class Host:
    """int lists <-> the crate's form"""
    def __init__(self, field):
        self.F, self.field, self.p = ecfft_amd.FIELDS[field], field, P[field]

    def mem(self, ints):
        w = 4 if self.field == "m31" else 32
        raw = b"".join(int(v).to_bytes(w, "little") for v in ints)
        std = np.frombuffer(raw, dtype=self.F.dtype).reshape(self.F.shape(len(ints))).copy()
        return self.F.from_standard(std)

    def ints(self, x):
        raw = self.F.to_standard(np.ascontiguousarray(x)).tobytes()
        w = 4 if self.field == "m31" else 32
        return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def baseline_row(t, fm):
    """[(q with its leading 1, e), ...] of one row from the calls that existed before poly_factor, and the number of calls"""
    out, calls = [], 1
    by_d = t.poly_irreducible_factors(fm)
    calls += len(by_d)
    for d, qs in by_d.items():
        for q in qs:
            cur, e = fm, 0
            while cur.shape[0] >= q.shape[0]:
                quo, rem = t.poly_divrem(cur, q)
                calls += 1
                if np.ascontiguousarray(rem).view(np.uint8).any():
                    break
                cur, e = quo, e + 1
            out.append((q, e))
    return out, calls


def timed(ops, reps, blocks):
    meds = {k: [] for k in ops}
    for _ in range(blocks):
        ts = {k: [] for k in ops}
        for _ in range(reps):
            for k, fn in ops.items():
                t0 = time.perf_counter()
                fn()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for k in ops:
            meds[k].append(float(np.median(ts[k])))
    return ({k: float(np.median(v)) for k, v in meds.items()}, {k: max(v) - min(v) for k, v in meds.items()},
            {k: [round(x, 4) for x in v] for k, v in meds.items()})


def run_case(field, name, count, reps, blocks, max_rows):
    p, H = P[field], Host(field)
    f, want = build(SPECS[name], p)
    nf = len(f)
    N = 4
    while nf > FT.FACTOR_SMALL_MAX and N < 2 * nf - 1:
        N <<= 1
    t = ecfft_amd.FIELDS[field].build_fftree(max(N, 256))                 # the baseline's poly_divrem needs a tree at every size
    row = H.mem(f)
    fm = np.concatenate([row] * count)
    factor = lambda: t.poly_factor(fm, count=count)
    fac, fdeg, fmult, n, lead = factor()
    got = [(H.ints(q), e) for q, e in t.factor_unpack(fac[:nf - 1], fdeg[0], fmult[0], n[0])]
    assert got == want and n.tolist() == [len(want)] * count and H.ints(lead) == [3] * count
    assert fac.tobytes() == np.ascontiguousarray(fac[:nf - 1]).tobytes() * count
    base, calls = baseline_row(t, row)
    assert sorted(((H.ints(q), e) for q, e in base), key=lambda qe: (qe[1], len(qe[0]), qe[0])) == want, "the baseline must find the same factors"
    rows_timed = min(count, max_rows)

    def baseline():
        for _ in range(rows_timed):
            baseline_row(t, row)
    med, spread, blocks_ms = timed({"factor": factor, "baseline": baseline}, reps, blocks)
    scale = count / rows_timed
    med["baseline"] *= scale
    spread["baseline"] *= scale
    t.profile(True)
    factor()
    launches = sum(c["launches"] for c in t.profile_read())
    t.profile(False)
    out = {"field": field, "spec": name, "degree": nf - 1, "factors": len(want), "count": count, "N": N,
           "regime": "small" if nf <= FT.FACTOR_SMALL_MAX else "large", "baseline_calls_per_row": calls, "baseline_rows_timed": rows_timed,
           "reps": reps, "blocks": blocks, "median_ms": {k: round(v, 4) for k, v in med.items()},
           "spread_ms": {k: round(v, 4) for k, v in spread.items()}, "block_medians_ms": blocks_ms, "launches": {"factor": launches},
           "baseline_over_factor": round(med["baseline"] / med["factor"], 2),
           "factor_below_baseline_by_more_than_the_spread": bool(med["baseline"] - med["factor"] > max(spread["factor"], spread["baseline"]))}
    del t
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    max_rows = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    cases = []
    for field in ("secp256k1", "m31"):
        for name, count in SHAPES:
            c = run_case(field, name, count, reps, blocks, max_rows)
            cases.append(c)
            print(f"{field} {name} count={count}: factor {c['median_ms']['factor']:.3f} ms ({c['launches']['factor']} launches), baseline "
                  f"{c['median_ms']['baseline']:.3f} ms ({c['baseline_over_factor']}x, {c['baseline_calls_per_row']} calls per row)",
                  file=sys.stderr, flush=True)
    print(json.dumps({"device": ecfft_amd.device_info(0), "cases": cases}, indent=1))


if __name__ == "__main__":
    main()
