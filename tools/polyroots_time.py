#!/usr/bin/env python3
"""ecfft_poly_find_roots against the same recursion a user could write before it from the public calls, and against
ecfft_poly_mul at the same size, in one process on warmed shapes, device-resident data (host clock after a device synchronise,
median of `reps` calls, the variants alternating call by call, the whole measurement repeated `blocks` times to see the spread
between medians).  Inputs: r seeded distinct roots times a rootless cofactor of r/4 quadratics x^2 + c^2 (irreducible, p = 3 mod 4
in both fields), built with poly_mul; nf = r + 2 (r/4) + 1.
    find_roots    FFTree.poly_find_roots(f)
    composed      the same recursion from the PUBLIC calls, depth-first: g = poly_gcd(f, poly_pow_mod(x, p, f) - x), then per split
                  one poly_pow_mod((x + c), (p-1)/2, h), one poly_gcd and one poly_divrem, shifts 1, 2, 3, ...; only while one call of it
                  stays under `composed_max_s` seconds
    poly_mul_N    FFTree.poly_mul of two nf-coefficient operands: the unit
    leaf_ms       the `pointwise` class of ecfft_profile_read for ONE small-regime call on the leaf factors of this input (the factors
                  of at most 64 roots that the rounds end with, recomputed here from the Legendre symbols of r + c, as rows of
                  ROOTS_SMALL_MAX): k_roots_small and k_roots_rank.  An UPPER bound of the leaf launch inside find_roots: as rows of
                  their own the factors also run the Frobenius scan
    rounds        the number of shifts the host rounds use until every factor has at most 64 roots (from the same symbols)
A case whose first call takes longer than 2 s is measured with reps = blocks = 1 and no further warm-up.
usage: polyroots_time.py [reps [blocks [composed_max_s [max_log_secp [max_log_m31]]]]] > profiles/polyroots/polyroots_time.json ; prints one JSON object"""
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

P = {"m31": 2**31 - 1, "secp256k1": 2**256 - 2**32 - 977}
LEAF = FT.ROOTS_SMALL_MAX - 1


def std(field, ints):
    """Python ints -> standard-form array in the field's element layout"""
    if field == "m31":
        return np.array(ints, dtype=np.uint32)
    return np.array([[(v >> (64 * k)) & (2**64 - 1) for k in range(4)] for v in ints], dtype=np.uint64).reshape(len(ints), 4)


def mem(field, ints):
    return ecfft_amd.FIELDS[field].from_standard(std(field, ints))


def ints_of(field, a):
    s = ecfft_amd.FIELDS[field].to_standard(a)
    if field == "m31":
        return [int(v) for v in s]
    return [sum(int(s[i, k]) << (64 * k) for k in range(4)) for i in range(s.shape[0])]


def product(field, t, leaves, width):
    """the product of len(leaves) polynomials of `width` coefficients each (rows of ints) by a batched product tree of poly_mul;
    the list is filled up to a power of two with the constant 1, so the result may carry high zeros"""
    n = 1
    while n < len(leaves):
        n <<= 1
    rows = leaves + [[1] + [0] * (width - 1)] * (n - len(leaves))
    cur = mem(field, [v for r in rows for v in r])
    while n > 1:
        w = cur.shape[0] // n
        v = cur.reshape((n // 2, 2, w) + cur.shape[1:])
        cur = t.poly_mul(np.ascontiguousarray(v[:, 0]).reshape((-1,) + cur.shape[1:]), np.ascontiguousarray(v[:, 1]).reshape((-1,) + cur.shape[1:]), count=n // 2)
        n //= 2
    return cur


def trimmed(a):
    nz = np.flatnonzero(a.reshape(a.shape[0], -1).any(axis=1))
    return np.ascontiguousarray(a[:nz[-1] + 1])


def legendre(a, p):
    s = pow(a % p, (p - 1) // 2, p)
    return -1 if s == p - 1 else s


def rounds_and_leaves(roots, p):
    """the host rounds replayed on the root sets: one shift per round for all sets of more than LEAF roots"""
    pending, leaves, c = ([roots] if len(roots) > LEAF else []), ([roots] if len(roots) <= LEAF else []), 0
    while pending:
        c += 1
        nxt = []
        for s in pending:
            u = [r for r in s if legendre(r + c, p) == 1]
            v = [r for r in s if legendre(r + c, p) != 1]
            for part in ([u, v] if u and v else [s]):
                (nxt if len(part) > LEAF else leaves).append(part)
        pending = nxt
    return c, leaves


def dev(field, a):
    return torch.from_numpy(a.view(np.int64) if field == "secp256k1" else a.view(np.int32)).cuda()


class Composed:
    """the recursion from the public calls on device tensors; single coefficients are fixed up through the host"""

    def __init__(self, field, t):
        self.field, self.t, self.p = field, t, P[field]
        self.F = ecfft_amd.FIELDS[field]

    def const(self, v):
        return dev(self.field, mem(self.field, [v % self.p]))

    def add_at(self, w, i, v):
        """w[i] += v (one element through the host)"""
        x = w[i:i + 1].cpu().numpy().view(self.F.dtype).reshape(self.F.shape(1))
        w[i:i + 1] = dev(self.field, mem(self.field, [(ints_of(self.field, x)[0] + v) % self.p]))

    def roots(self, f):
        t, p = self.t, self.p
        x = dev(self.field, mem(self.field, [0, 1]))
        w = t.poly_pow_mod(x, p, f)
        self.add_at(w, 1, -1)
        g, deg = t.poly_gcd(f, w)
        stack, out, c = [g[:int(deg[0]) + 1]], [], 1
        while stack:
            h = stack.pop()
            e = h.shape[0] - 1
            if e <= 0:
                continue
            if e == 1:
                out.append(h[0:1])                            # the root is -h[0]; negating and ordering are left out of the time
                continue
            w = t.poly_pow_mod(dev(self.field, mem(self.field, [c, 1])), (p - 1) // 2, h)
            self.add_at(w, 0, -1)
            c += 1
            u, du = t.poly_gcd(h, w)
            du = int(du[0])
            if 0 < du < e:
                u = u[:du + 1].contiguous()
                stack += [u, t.poly_divrem(h, u)[0]]
            else:
                stack.append(h)
        return out


def run_case(field, t, r, reps, blocks, state):
    p = P[field]
    a = 0x9E3779B1 if field == "m31" else 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95
    roots = [(a * (i + 1) + 12345) % p for i in range(r)]
    nq = max(r // 4, 1)
    lin = trimmed(product(field, t, [[-x % p, 1] for x in roots], 2))
    quad = trimmed(product(field, t, [[c * c % p, 0, 1] for c in range(1, nq + 1)], 3))
    fh = t.poly_mul(lin, quad)
    f = dev(field, fh)
    nf = fh.shape[0]
    assert nf == r + 2 * nq + 1
    nrounds, leaves = rounds_and_leaves(roots, p)
    comp = Composed(field, t)
    ops = {"find_roots": lambda: t.poly_find_roots(f), "poly_mul_N": lambda: t.poly_mul(f, f)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got, n = ops["find_roots"]()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    assert int(n[0]) == r and ints_of(field, got[:r].cpu().numpy().view(comp.F.dtype).reshape(comp.F.shape(r))) == sorted(roots)
    if not state["composed_off"]:
        t0 = time.perf_counter()
        out = comp.roots(f)
        torch.cuda.synchronize()
        first_c = time.perf_counter() - t0
        assert len(out) == r
        if first_c > state["composed_max_s"]:
            state["composed_off"] = True                      # this size is still reported (one call); larger ones are not run
        ops["composed"] = lambda: comp.roots(f)
    if first > 2.0 or state["composed_off"] and "composed" in ops:
        reps = blocks = 1
    else:
        for fn in ops.values():
            fn()
    torch.cuda.synchronize()
    meds = {k: [] for k in ops}
    for _ in range(blocks):
        ts = {k: [] for k in ops}
        for i in range(reps):
            for k, fn in ops.items():
                if k == "composed" and r > 64 and i:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for k in ops:
            meds[k].append(float(np.median(ts[k])))
    med = {k: float(np.median(v)) for k, v in meds.items()}
    # the leaf factors as rows of the small regime, profiled
    F = comp.F
    lrows = np.zeros(F.shape(len(leaves) * (LEAF + 1)), F.dtype)
    for i, s in enumerate(leaves):
        lrows[i * (LEAF + 1):i * (LEAF + 1) + len(s) + 1] = trimmed(product(field, t, [[-v % p, 1] for v in s], 2))
    lf = dev(field, lrows)
    t.poly_find_roots(lf, count=len(leaves))
    t.profile(True)
    t.poly_find_roots(lf, count=len(leaves))
    leaf_ms = [c["ms"] for c in t.profile_read() if c["name"] == "pointwise"][0]
    t.profile(False)
    out = {"field": field, "roots": r, "nf": nf, "reps": reps, "blocks": blocks, "rounds": nrounds, "leaf_factors": len(leaves),
           "leaf_ms": round(leaf_ms, 4), "median_ms": {k: round(v, 4) for k, v in med.items()},
           "spread_ms": {k: round(max(v) - min(v), 4) for k, v in meds.items()},
           "block_medians_ms": {k: [round(x, 4) for x in v] for k, v in meds.items()},
           "find_roots_over_poly_mul_N": round(med["find_roots"] / med["poly_mul_N"], 2), "leaf_share": round(leaf_ms / med["find_roots"], 3)}
    if "composed" in med:
        out["composed_over_find_roots"] = round(med["composed"] / med["find_roots"], 2)
    return out


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    reps, blocks, logs = arg(1, 5), arg(2, 3), {"secp256k1": arg(4, 12), "m31": arg(5, 14)}
    torch.zeros(1, device="cuda")
    cases = []
    for field in ("secp256k1", "m31"):
        t = ecfft_amd.FIELDS[field].build_fftree(4 << logs[field])
        state = {"composed_off": False, "composed_max_s": float(arg(3, 4))}
        for r in sorted({16, 64, 256} | {1 << k for k in range(10, logs[field] + 1, 2)} | {1 << logs[field]}):
            cases.append(run_case(field, t, r, reps, blocks, state))
            print(json.dumps(cases[-1]), file=sys.stderr, flush=True)
        del t
        torch.cuda.empty_cache()
    print(json.dumps({"device": ecfft_amd.device_info(0), "small_max": FT.ROOTS_SMALL_MAX, "cases": cases}))


if __name__ == "__main__":
    main()
