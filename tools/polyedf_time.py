#!/usr/bin/env python3
"""ecfft_poly_equal_degree against the reference's formulation of equal-degree splitting written from the public calls a caller had
before it, in one process on warmed shapes, host arrays on both sides (host clock around synchronous calls, median of `reps` calls,
the two alternating call by call, the whole measurement repeated `blocks` times to see the spread between medians).

Inputs are built: g = prod of r = n // d distinct irreducibles of degree d, the binomials x^d - a and their shifts (x + s)^d - a.
    edf        FFTree.poly_equal_degree(g, d)
    baseline   a stack of pending factors; per split w = poly_pow_mod(x + c, (p^d - 1)/2, u) (utils::equal_degree_factorization's
               exponent, d times the bits of p), poly_gcd(u, w - 1) (the subtraction on the host), poly_divrem; the shifts c = 1, 2,
               3, ... from one counter.  The tool first asserts that its factors, sorted, give the bytes of `edf`.  Where one call of
               it takes longer than `cap_s` seconds it is run once and not timed in blocks (baseline_blocks = false); where its
               estimated count of modular products, r times the products of one power, exceeds `max_products` it is not run at
               all (baseline = null): minutes per call for secp256k1 at n = 1024.
    launches   from ecfft_profile_read, one profiled call each, all classes together.
    iterates   the Frobenius iterates the call takes beyond h_1: d - 2 (none for a row that is one factor).
    rounds, leaves, leaf_factors, direct_factors   the host rounds of the large regime replayed from the quadratic characters of
               (-1)^d f_j(-c) of the built factors (no hook): one shift per round, pieces of one factor going straight to the
               output, pieces of degree <= 64 to the leaf launch.  The small regime is one leaf and no round.
usage: polyedf_time.py [reps [blocks [cap_s [max_products]]]] > profiles/polyedf/polyedf_time.json"""
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
NS = [16, 64, 256, 1024]
DS = [2, 7]


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
    """(x + s)^d - a for the first a >= 2 with a^((p-1)/q) != 1 for the prime q = d (2 or 7: q | p - 1 in both fields), s = 0, 1, ..."""
    assert d in (2, 7) and (p - 1) % d == 0
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


LEAF = 64            # a piece of at most this degree is finished by the workgroup kernel


def plus_one(q, c, p):
    """the splitting element is +1 modulo the irreducible q at the shift c: the norm (-1)^d q(-c) is a non-zero square"""
    v = 0
    for coef in reversed(q):
        v = (v * (-c) + coef) % p
    return pow((-1) ** (len(q) - 1) * v % p, (p - 1) // 2, p) == 1


def rounds_and_leaves(qs, d, p):
    """the host rounds of the large regime replayed on the sets of factors, from the characters of (-1)^d f_j(-c) alone: one shift
    per round for all pending sets; a piece of one factor goes to the output, one of degree <= LEAF to the leaves, the rest stay
    pending.  Returns (rounds, leaves, leaf factors, factors that went straight to the output); a row of degree <= LEAF is one leaf."""
    if len(qs) == 1:
        return 0, 0, 0, 1
    if len(qs) * d <= LEAF:
        return 0, 1, len(qs), 0
    pending, leaves, direct, c = [qs], [], 0, 0
    while pending:
        c += 1
        nxt = []
        for s in pending:
            u = [q for q in s if plus_one(q, c, p)]
            v = [q for q in s if not plus_one(q, c, p)]
            for part in ([u, v] if u and v else [s]):
                if len(part) == 1:
                    direct += 1
                elif len(part) * d <= LEAF:
                    leaves.append(part)
                else:
                    nxt.append(part)
        pending = nxt
    return c, len(leaves), sum(len(x) for x in leaves), direct


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


def baseline(t, H, gm, d):
    """the factors of the monic g (d + 1 coefficients each, crate form, discovery order) and the number of attempts"""
    p = H.p
    exp = (p ** d - 1) // 2
    stack, out, c = [gm], [], 1
    while stack:
        u = stack.pop()
        e = u.shape[0] - 1
        if e == d:
            out.append(u)
            continue
        w = H.ints(t.poly_pow_mod(H.mem([c, 1]), exp, u))
        w[0] = (w[0] - 1) % p
        g, dg = t.poly_gcd(u, H.mem(w))
        c += 1
        n = int(dg[0])
        if 0 < n < e:
            a = np.ascontiguousarray(g[:n + 1])
            stack += [a, t.poly_divrem(u, a)[0]]
        else:
            assert c < 4096
            stack.append(u)
    return out, c - 1


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


def launches_of(t, fn):
    t.profile(True)
    fn()
    n = sum(c["launches"] for c in t.profile_read())
    t.profile(False)
    return n


def run_case(field, d, n, reps, blocks, cap_s, max_products):
    p, H = P[field], Host(field)
    r = n // d
    qs = irreducibles(d, r, p)
    g = product(qs, p)
    ng = len(g)
    N = 4
    while ng > FT.EDF_SMALL_MAX and N < 2 * ng - 1:
        N <<= 1
    t = ecfft_amd.FIELDS[field].build_fftree(max(N, 256))                 # the baseline's poly_divrem needs a tree at every size
    gm = H.mem(g)
    edf = lambda: t.poly_equal_degree(gm, d)
    want, cnt = edf()
    assert cnt[0] == r
    bits = p.bit_length() - 1 + bin(p >> 1).count("1") - 1                # products of one power with (p - 1) / 2
    ebits = ((p ** d - 1) // 2).bit_length() - 1 + bin((p ** d - 1) // 2).count("1") - 1
    runs = r * ebits <= max_products
    first_s, attempts, same = 0.0, None, None
    if runs:
        t0 = time.perf_counter()
        facs, attempts = baseline(t, H, gm, d)
        first_s = time.perf_counter() - t0
        rows = sorted(H.ints(q)[:d] for q in facs)
        same = bool(H.mem([v for q in rows for v in q]).tobytes() == np.ascontiguousarray(want[:r * d]).tobytes())
        assert same, "the baseline from the public calls, sorted, must give the bytes of the call"
    assert H.ints(want[:r * d]) == [v for q in sorted(q[:d] for q in qs) for v in q]
    edf()
    ops = {"edf": edf}
    in_blocks = runs and first_s <= cap_s
    if in_blocks:
        ops["baseline"] = lambda: baseline(t, H, gm, d)
    med, spread, blocks_ms = timed(ops, reps, blocks)
    if runs and not in_blocks:
        med["baseline"], spread["baseline"], blocks_ms["baseline"] = first_s * 1e3, 0.0, [round(first_s * 1e3, 4)]
    rounds, nleaf, leaf_factors, direct = rounds_and_leaves(qs, d, p)
    out = {"field": field, "d": d, "n": r * d, "r": r, "N": N, "regime": "small" if ng <= FT.EDF_SMALL_MAX else "large",
           "iterates": max(d - 2, 0) if r > 1 else 0, "rounds": rounds, "leaves": nleaf, "leaf_factors": leaf_factors, "direct_factors": direct, "baseline_attempts": attempts, "baseline_same_bytes": same, "baseline_blocks": in_blocks,
           "products_per_attempt": {"edf": d - 1 + bits, "baseline": ebits}, "reps": reps, "blocks": blocks,
           "median_ms": {k: round(v, 4) for k, v in med.items()}, "spread_ms": {k: round(v, 4) for k, v in spread.items()},
           "block_medians_ms": blocks_ms, "launches": {"edf": launches_of(t, edf)}}
    if runs:
        out["baseline_over_edf"] = round(med["baseline"] / med["edf"], 2)
        out["edf_below_baseline_by_more_than_the_spread"] = bool(med["baseline"] - med["edf"] > max(spread["edf"], spread["baseline"]))
    else:
        out["baseline"] = None
    if in_blocks:
        out["launches"]["baseline"] = launches_of(t, ops["baseline"])
    del t
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    cap_s = float(sys.argv[3]) if len(sys.argv) > 3 else 5.0
    max_products = int(sys.argv[4]) if len(sys.argv) > 4 else 150000
    cases = []
    for field in ("secp256k1", "m31"):
        for d in DS:
            for n in NS:
                c = run_case(field, d, n, reps, blocks, cap_s, max_products)
                cases.append(c)
                b = c["median_ms"].get("baseline")
                print(f"{field} d={d} n={c['n']}: edf {c['median_ms']['edf']:.3f} ms, baseline "
                      + (f"{b:.3f} ms ({c['baseline_over_edf']}x){'' if c['baseline_blocks'] else ' [once]'}" if b is not None else "not run"),
                      file=sys.stderr, flush=True)
    print(json.dumps({"device": ecfft_amd.device_info(0), "cases": cases}, indent=1))


if __name__ == "__main__":
    main()
