#!/usr/bin/env python3
"""ecfft_curve_trace_mod against the same algorithm written from the public calls a caller had before it, in one process on warmed
shapes, host arrays on both sides (host clock around synchronous calls, median of `reps` calls, the two alternating call by call,
the whole measurement repeated `blocks` times to see the spread between medians), and ecfft_division_polynomial on its own.

    trace      FFTree.curve_trace_mod(A, B, l) for l = 3, 5, 7, 11 (the small regime: one workgroup per curve, one launch), with
               count = 1 and with count = 64 copies of the curve in one call
    baseline   ONE curve: psi_l by FFTree.division_polynomial, made monic on the host; pi by two poly_pow_mod; pi^2 by two
               poly_compose_mod and one poly_mul_mod; the group law of examples/schoofs.rs:237-273 with poly_mul_mod for the products
               and poly_xgcd for the inverse, sums and differences of rows in Python on the host (numpy for M31, ints for
               secp256k1): the ratios are against a caller who composes the calls from Python; Q = [p mod l](x, y) and j pi by repeated
               sums, as the kernel takes them.  The curves are ones whose modulus never splits, (8, 81) over M31 and (0, 7) over
               secp256k1, and the tool first asserts that the baseline returns the residue of `trace`.  For count = 64 the
               baseline is not run: baseline_64_ms is 64 times the one-curve median (a caller's loop).
    trace_large  the same pair for l = 13 .. 31 (the large regime: one curve per call on a tree of 1024 leaves), 2 calls per block, 2 blocks
    cardinality  M31 (8, 81) and secp256k1 (0, 7): curve_trace_mod per prime of the rule, each timed once, until cap_s seconds are
               spent; where every prime ran, their CRT must be the known order (secp256k1: the published one), and where they took
               at most 60 s together the full curve_cardinality is run once more for its wall time and must return that order;
               otherwise the residues reached, checked against the published order
    divpoly    FFTree.division_polynomial(A, B, n) for n = 11, 17, 31, 103 with count = 1 and 8 (device work plus the host staging)
usage: schoof_time.py [reps [blocks [cap_s]]] > profiles/schoof/schoof_time.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecfft_amd  # noqa: E402

CURVE = {"m31": (8, 81), "secp256k1": (0, 7)}
LS = [3, 5, 7, 11]
LARGE_LS = [13, 17, 19, 23, 29, 31]
SECP256K1_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
ORDER = {"m31": 2147489041, "secp256k1": SECP256K1_ORDER}


class Base:
    """Schoof's attempt on one modulus from the public calls; rows are host arrays of d elements"""

    def __init__(self, t, fld, A, B, l):
        self.t, self.f, self.p, self.l, self.A = t, fld, fld.MODULUS[fld.name], l, A
        p = self.p
        a_el, b_el = fld.from_ints([A]), fld.from_ints([B])
        psi = fld.to_ints(t.division_polynomial(a_el, b_el, l))
        inv = pow(psi[-1], -1, p)
        self.h = fld.from_ints([v * inv % p for v in psi])
        self.d = len(psi) - 1
        self.x = self.row([0, 1])
        self.one = self.row([1])
        self.fx = self.row([B, A, 0, 1])
        self.A_raw = self.raw(a_el)[0]

    def row(self, ints):
        return self.f.from_ints(list(ints) + [0] * (self.d - len(ints)))

    def raw(self, u):
        """the stored numbers of a row as Python ints (sums and differences are the same in the crate's form)"""
        if self.f.limbs == 1:
            return [int(v) for v in u]
        b = np.ascontiguousarray(u).tobytes()
        n = self.f.dtype.itemsize * self.f.limbs
        return [int.from_bytes(b[i:i + n], "little") for i in range(0, len(b), n)]

    def unraw(self, vals):
        if self.f.limbs == 1:
            return np.array(vals, self.f.dtype)
        n = self.f.dtype.itemsize * self.f.limbs
        return np.frombuffer(b"".join(v.to_bytes(n, "little") for v in vals), self.f.dtype).reshape(self.f.shape(len(vals))).copy()

    def lin(self, u, v, sign):
        p = self.p
        if self.f.limbs == 1:
            return ((u.astype(np.int64) + sign * v.astype(np.int64)) % p).astype(self.f.dtype)
        return self.unraw([(a + sign * b) % p for a, b in zip(self.raw(u), self.raw(v))])

    def mul(self, u, v):
        return self.t.poly_mul_mod(u, v, self.h)

    def add(self, P1, P2):
        (a1, b1), (a2, b2) = P1, P2
        if np.array_equal(a1, a2):
            if not np.ascontiguousarray(self.lin(b1, b2, 1)).view(np.uint8).any():
                return None
            assert np.array_equal(b1, b2), "the timed curves do not split"
            sq = self.raw(self.mul(a1, a1))
            num = self.unraw([(3 * v + (self.A_raw if i == 0 else 0)) % self.p for i, v in enumerate(sq)])
            den = self.mul(self.fx, b1)
            den = self.lin(den, den, 1)
        else:
            num, den = self.lin(b1, b2, -1), self.lin(a1, a2, -1)
        s, _, _, deg = self.t.poly_xgcd(den, self.h)
        assert deg[0] == 0, "the timed curves do not split"
        r = self.mul(num, s[:self.d])
        a3 = self.lin(self.lin(self.mul(self.mul(r, r), self.fx), a1, -1), a2, -1)
        b3 = self.lin(self.mul(r, self.lin(a1, a3, -1)), b1, -1)
        return a3, b3

    def trace(self):
        t, p, l = self.t, self.p, self.l
        pa = t.poly_pow_mod(self.x, p, self.h)
        pb = t.poly_pow_mod(self.fx, (p - 1) // 2, self.h)
        ea = t.poly_compose_mod(pa, pa, self.h)
        eb = self.mul(t.poly_compose_mod(pb, pa, self.h), pb)
        Q = (self.x, self.one)
        for _ in range(p % l - 1):
            Q = self.add(Q, (self.x, self.one))
        E = self.add((ea, eb), Q)
        if E is None:
            return 0
        Pj = (pa, pb)
        for j in range(1, l):
            if np.array_equal(Pj[0], E[0]) and np.array_equal(Pj[1], E[1]):
                return j
            if j + 1 < l:
                Pj = self.add(Pj, (pa, pb))
        return 0


def med(xs):
    return float(np.median(xs))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    cap_s = float(sys.argv[3]) if len(sys.argv) > 3 else 120.0
    out = {"device": ecfft_amd.device_info(0), "reps": reps, "blocks": blocks, "cap_s": cap_s, "trace": [], "trace_large": [], "cardinality": [], "divpoly": []}
    for name in ("m31", "secp256k1"):
        fld = ecfft_amd.FIELDS[name]
        t = fld.build_fftree(256)
        A, B = CURVE[name]
        for l in LS:
            a1, b1 = fld.from_ints([A]), fld.from_ints([B])
            a64, b64 = fld.from_ints([A] * 64), fld.from_ints([B] * 64)
            want = int(t.curve_trace_mod(a1, b1, l)[0])
            assert t.curve_trace_mod(a64, b64, l).tolist() == [want] * 64
            base = lambda: Base(t, fld, A, B, l).trace()
            assert base() == want, (name, l)
            one = lambda: t.curve_trace_mod(a1, b1, l)
            many = lambda: t.curve_trace_mod(a64, b64, l)
            m1, m64, mb = [], [], []
            for _ in range(blocks):
                x1, x64, xb = [], [], []
                for _ in range(reps):
                    x1.append(timed(one)); xb.append(timed(base)); x64.append(timed(many))
                m1.append(med(x1)); m64.append(med(x64)); mb.append(med(xb))
            out["trace"].append({"field": name, "l": l, "degree": (l * l - 1) // 2, "residue": want,
                                 "trace_1_ms": m1, "trace_64_ms": m64, "baseline_1_ms": mb, "baseline_64_ms": 64 * med(mb),
                                 "ratio_1": med(mb) / med(m1), "ratio_64": 64 * med(mb) / med(m64)})
            print(json.dumps(out["trace"][-1]), file=sys.stderr, flush=True)
        del t
        # the large regime: one curve per call, the baseline as above (2 calls per block, 2 blocks)
        t = fld.build_fftree(1024)
        a1, b1 = fld.from_ints([A]), fld.from_ints([B])
        for l in LARGE_LS:
            want = int(t.curve_trace_mod(a1, b1, l)[0])
            base = lambda: Base(t, fld, A, B, l).trace()
            try:
                assert base() == want, (name, l)
                splits = False
            except AssertionError as ex:
                if "do not split" not in str(ex):
                    raise
                splits = True                                    # the baseline has no restart: it is not timed at this l
            one = lambda: t.curve_trace_mod(a1, b1, l)
            m1, mb = [], []
            for _ in range(2):
                x1, xb = [], []
                for _ in range(2):
                    x1.append(timed(one))
                    if not splits:
                        xb.append(timed(base))
                m1.append(med(x1))
                if not splits:
                    mb.append(med(xb))
            out["trace_large"].append({"field": name, "l": l, "degree": (l * l - 1) // 2, "residue": want, "trace_1_ms": m1,
                                       "baseline_1_ms": mb or None, "ratio_1": med(mb) / med(m1) if mb else None})
            print(json.dumps(out["trace_large"][-1]), file=sys.stderr, flush=True)
        del t
        # one full count: per-l times from single calls until `cap_s` seconds are spent, then the whole call where they all ran
        t = fld.build_fftree(512 if name == "m31" else 1 << 14)
        primes, per_l, spent = t.schoof_primes(), [], 0.0
        for l in primes:
            if spent > cap_s:
                break
            ms = timed(lambda: per_l.append([l, int(t.curve_trace_mod(a1, b1, l)[0])]))
            per_l[-1].append(ms)
            spent += ms / 1e3
        card = {"field": name, "curve": [A, B], "primes": primes, "per_l": per_l, "complete": len(per_l) == len(primes), "order": None, "wall_ms": None}
        if name == "secp256k1":
            card["residues_match_published_order"] = all(r == (fld.MODULUS[name] + 1 - SECP256K1_ORDER) % l for l, r, _ in per_l)
        card["per_l_total_ms"] = sum(x[2] for x in per_l)
        if card["complete"]:
            tt, m = 0, 1
            for l, r, _ in per_l:                                # the CRT of schoofs.rs:52-70 on the residues of the single calls
                tt = (tt + m * ((r - tt) * pow(m, -1, l) % l)) % (m * l)
                m *= l
            card["order"] = str(fld.MODULUS[name] + 1 - (tt - m if tt > m // 2 else tt))
            assert card["order"] == str(ORDER[name]), card
            if spent <= 60.0:                                    # the whole call once more, where that stays short
                full = []
                card["wall_ms"] = timed(lambda: full.append(t.curve_cardinality(a1, b1)[0]))
                assert full[0] == ORDER[name], full
        out["cardinality"].append(card)
        print(json.dumps(card), file=sys.stderr, flush=True)
        del t
        t = fld.build_fftree(8192)
        for n in (11, 17, 31, 103):
            for count in (1, 8):
                a, b = fld.from_ints([A] * count), fld.from_ints([B + i for i in range(count)])
                fn = lambda: t.division_polynomial(a, b, n)
                fn()
                ms = [med([timed(fn) for _ in range(reps)]) for _ in range(blocks)]
                out["divpoly"].append({"field": name, "n": n, "coefficients": t.division_polynomial_len(n), "count": count, "ms": ms})
                print(json.dumps(out["divpoly"][-1]), file=sys.stderr, flush=True)
        del t
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
