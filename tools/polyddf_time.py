#!/usr/bin/env python3
"""ecfft_poly_distinct_degree against the same factorisation written from the public calls a caller had before it (poly_gcd,
poly_divrem, poly_pow_mod, poly_compose_mod), and the two ways its large regime can take a Frobenius iterate, in one process on
warmed shapes, host arrays on both sides (host clock around synchronous calls, median of `reps` calls, the variants alternating
call by call, the whole measurement repeated `blocks` times to see the spread between medians).  Needs the hooks build
(ecfft_test_ddf_iterate forces the iterate method).

Inputs are built, so the number of iterates is known: A = (deg - 14) distinct linear factors times (x^7 - a1)(x^7 - a2), whose loop
runs to i = 7 and takes 6 iterates; B = (deg - 6) linear factors times (x^3 - b1)(x^3 - b2): 2 iterates.  Both are monic and
squarefree of degree deg, so A costs exactly four more iterations (gcd and iterate) than B.
    ddf            FFTree.poly_distinct_degree(A), the shipped rule
    baseline       g = poly_gcd(f, f') (f' on the host), s = f / g, h = h_1 = poly_pow_mod(x, p, s); per degree i: poly_gcd(f*, h - x)
                   (the subtraction on the host), poly_divrem where the gcd is not 1, h = poly_compose_mod(h, h_1, s).  The tool first
                   asserts that it gives the bytes of `ddf`.
    kept / power   (deg > 64) the call with the iterate forced to the kept composition / the fresh power, on A and on B; both give
                   the bytes of `ddf`.  iteration_ms = (T(A) - T(B)) / 4 is one gcd and one iterate of that kind.
    compose_mod, pow_mod, gcd   (deg > 64) the public calls a caller pays per iterate: poly_compose_mod(h_1, h_1, s), poly_pow_mod(h_1, p, s)
                   and poly_gcd(s, h_1 - x); iterate_ms = iteration_ms - gcd.
    launches       from ecfft_profile_read, one profiled call each: all classes together; per iteration as above.
`rule` is what ddf_iterate_composes picks from the counts of modular products (k' - 1 against bits + popcount(p) - 2); `measured` is
the faster of kept / power on A by more than the spread, else "tie".
usage: polyddf_time.py [reps [blocks]] > profiles/polyddf/polyddf_time.json"""
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
DEGS = [16, 64, 256, 1024]


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


def irreducible_binomials(n, count, p):
    """x^n - a for the first a >= 2 with a^((p-1)/q) != 1 for every prime q | n (n = 3 or 7: q | p - 1 in both fields)"""
    assert n in (3, 7) and (p - 1) % n == 0
    out, a = [], 2
    while len(out) < count:
        if pow(a, (p - 1) // n, p) != 1:
            out.append([-a % p] + [0] * (n - 1) + [1])
        a += 1
    return out


def build(field, deg, n):
    p = P[field]
    a = 0x9E3779B1 if field == "m31" else 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95
    lin = [[-((a * (i + 1) + 1) % p) % p, 1] for i in range(deg - 2 * n)]
    f = product(lin + irreducible_binomials(n, 2, p), p)
    assert len(f) == deg + 1
    return f


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


def baseline(t, H, fm, nf):
    """(factors, degrees) in the layout of poly_distinct_degree, for a monic f of nf > 2 coefficients, from the public calls"""
    p = H.p
    fi = H.ints(fm)
    g, dg = t.poly_gcd(fm, H.mem([j * fi[j] % p for j in range(1, nf)]))
    s = fm if dg[0] == 0 else t.poly_divrem(fm, np.ascontiguousarray(g[:dg[0] + 1]))[0]
    ds = s.shape[0] - 1
    h1 = t.poly_pow_mod(H.mem([0, 1]), p, s)
    h, fs, e, i, rows, degrees = h1, s, ds, 1, [], np.zeros(nf - 1, np.int64)
    while e >= 2 * i:
        w = H.ints(h)
        w[1] = (w[1] - 1) % p
        g, dg = t.poly_gcd(fs, H.mem(w))
        n = int(dg[0])
        if n > 0:
            degrees[i - 1] = n
            rows.append(g[:n])
            if n < e:
                fs = t.poly_divrem(fs, np.ascontiguousarray(g[:n + 1]))[0]
            e -= n
        if e < 2 * (i + 1):
            break
        h = t.poly_compose_mod(h, h1, s)
        i += 1
    if e > 0:
        degrees[e - 1] = e
        rows.append(fs[:e])
    fac = np.zeros_like(fm[:nf - 1])
    cat = np.concatenate(rows)
    fac[:cat.shape[0]] = cat
    return fac, degrees, s, h1


def timed(ops, reps, blocks):
    for fn in ops.values():
        fn()
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
    fn()
    t.profile(True)
    fn()
    n = sum(c["launches"] for c in t.profile_read())
    t.profile(False)
    return n


def chunking(nf):
    k = 1
    while k * k < nf:
        k += 1
    return k, (nf + k - 1) // k


def run_case(L, field, deg, reps, blocks):
    p, H = P[field], Host(field)
    nf = deg + 1
    N = 4
    while nf > FT.DDF_SMALL_MAX and N < 2 * nf - 1:
        N <<= 1
    t = ecfft_amd.FIELDS[field].build_fftree(max(N, 256))                 # the baseline's poly_divrem needs a tree at every size
    A, B = H.mem(build(field, deg, 7)), H.mem(build(field, deg, 3))
    force = L.ecfft_test_ddf_iterate

    def ddf(f, mode=0):
        assert force(mode) == 0
        try:
            return t.poly_distinct_degree(f)
        finally:
            force(0)

    want = ddf(A)
    assert want[1][0].tolist()[:7] == [deg - 14, 0, 0, 0, 0, 0, 14], want[1][0].tolist()[:7]
    bfac, bdeg, s, h1 = baseline(t, H, A, nf)
    same = bool(bfac.tobytes() == want[0].tobytes() and np.array_equal(bdeg, want[1][0]))
    assert same, "the baseline from the public calls must give the bytes of the call"
    ops = {"ddf": lambda: ddf(A), "baseline": lambda: baseline(t, H, A, nf)}
    large = deg > 64
    if large:
        for mode, name in ((1, "kept"), (2, "power")):
            assert ddf(A, mode)[0].tobytes() == want[0].tobytes()
            ops[name + "_A"] = lambda m=mode: ddf(A, m)
            ops[name + "_B"] = lambda m=mode: ddf(B, m)
        w = H.ints(h1)
        w[1] = (w[1] - 1) % p
        wm = H.mem(w)
        ops["compose_mod"] = lambda: t.poly_compose_mod(h1, h1, s)
        ops["pow_mod"] = lambda: t.poly_pow_mod(h1, p, s)
        ops["gcd"] = lambda: t.poly_gcd(s, wm)
    med, spread, blocks_ms = timed(ops, reps, blocks)
    k, kp = chunking(deg)
    power_products = p.bit_length() + bin(p).count("1") - 2
    out = {"field": field, "deg": deg, "N": N, "iterates_A": 6, "iterates_B": 2, "baseline_same_bytes": same, "reps": reps, "blocks": blocks,
           "median_ms": {n: round(v, 4) for n, v in med.items()}, "spread_ms": {n: round(v, 4) for n, v in spread.items()},
           "block_medians_ms": blocks_ms, "baseline_over_ddf": round(med["baseline"] / med["ddf"], 2)}
    if large:
        it = {n: (med[n + "_A"] - med[n + "_B"]) / 4 for n in ("kept", "power")}
        la = {n: launches_of(t, ops[n]) for n in ("kept_A", "kept_B", "power_A", "power_B", "compose_mod", "pow_mod", "gcd", "baseline")}
        noise = max(spread["kept_A"], spread["power_A"])
        measured = "tie" if abs(med["kept_A"] - med["power_A"]) <= noise else ("kept" if med["kept_A"] < med["power_A"] else "power")
        rule = "kept" if kp - 1 <= power_products else "power"
        out.update({"k": k, "k_prime": kp, "products_per_iterate": {"kept": kp - 1, "power": power_products, "compose_mod": k + kp - 2},
                    "iteration_ms": {n: round(v, 4) for n, v in it.items()},
                    "iterate_ms": {"kept": round(it["kept"] - med["gcd"], 4), "power": round(it["power"] - med["gcd"], 4),
                                   "compose_mod": round(med["compose_mod"], 4), "pow_mod": round(med["pow_mod"], 4)},
                    "kept_over_compose_mod": round((it["kept"] - med["gcd"]) / med["compose_mod"], 3),
                    "launches": la,
                    "launches_per_iterate": {"kept": (la["kept_A"] - la["kept_B"]) / 4 - la["gcd"], "power": (la["power_A"] - la["power_B"]) / 4 - la["gcd"],
                                             "compose_mod": la["compose_mod"], "pow_mod": la["pow_mod"]},
                    "rule": rule, "measured": measured, "rule_agrees": measured in (rule, "tie")})
    del t
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    cases = []
    with FT.use_hooks_library() as L:
        for field in ("secp256k1", "m31"):
            for deg in DEGS:
                c = run_case(L, field, deg, reps, blocks)
                cases.append(c)
                print(f"{field} deg={deg}: ddf {c['median_ms']['ddf']:.3f} ms, baseline {c['median_ms']['baseline']:.3f} ms"
                      + (f", iteration kept {c['iteration_ms']['kept']:.3f} / power {c['iteration_ms']['power']:.3f} ms, rule {c['rule']}, "
                         f"measured {c['measured']}" if "rule" in c else ""), file=sys.stderr, flush=True)
    verdict = {f"{c['field']} deg={c['deg']}": {"rule": c["rule"], "measured": c["measured"], "rule_agrees": c["rule_agrees"]} for c in cases if "rule" in c}
    print(json.dumps({"device": ecfft_amd.device_info(0), "cases": cases, "iterate_rule": verdict}, indent=1))


if __name__ == "__main__":
    main()
