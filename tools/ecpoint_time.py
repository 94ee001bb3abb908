#!/usr/bin/env python3
"""Times of the short-Weierstrass front end (ecfft_curve_point_mul, ecfft_curve_find_generator, ecfft_build_ec_fftree), in one
process on warmed shapes, host arrays (host clock around the synchronous calls, so the copies to and from the device are inside;
median of `reps` calls, the whole measurement repeated `blocks` times to see the spread between medians).

    point_mul    count = 1, 64, 2^12, 2^16, 2^20 points of one curve with a random scalar of 4, 32 and 40 bytes per row, both
                 fields.  Beside each time the field multiplications it stands for, from the formula counts of the Jacobian
                 coordinates (curve_points.h: 10 per doubling, 11 per mixed addition):
                   useful_muls  per row 10 per bit of the longest scalar + 11 per set bit of the row's own + the final inversion
                   issued_muls  per row 21 per bit + the inversion: a wave runs the addition at every bit where ANY of its 64 lanes
                                has the bit set, which with a random scalar per row is every bit
                 and the rates useful_per_s / issued_per_s next to `ceiling_per_s`, ecfft_mul_ceiling at the waves per SIMD that
                 the kernel's registers allow (`OCCUPANCY`, from the code object: DESIGN.md 5.14).
    find_generator  ecfft_curve_find_generator on M31 (1, 6) and secp256k1 (1, 0) with the orders of tests/golden/ec_curves.json
    build_ec_fftree n = 2^12 over M31 with the crate's constants, end to end, beside ecfft_build_fftree(2^12)
usage: ecpoint_time.py [reps [blocks]] > profiles/ecpoint/ecpoint_time.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecfft_amd  # noqa: E402

COUNTS = [1, 64, 1 << 12, 1 << 16, 1 << 20]
WIDTHS = [4, 32, 40]
CURVE = {"m31": (1, 6), "secp256k1": (1, 0)}
BASE_X = {"m31": 2, "secp256k1": 3}                     # the first candidates of large order (tests/test_ec_ref_host.py)
OCCUPANCY = {"m31": 8, "secp256k1": 2}                  # waves per SIMD of k_point_mul: 20 and 187 VGPRs
INV_MULS = {"m31": 64 + 30, "secp256k1": 255 + 15}      # F::inv, field_m31.h / field_secp256k1.h
M31_CRATE = {"A": 1, "B": 0, "gen": (1273083559, 804329170), "offset": (1048755163, 279503108), "log_order": 28}


def med(xs):
    return float(np.median(xs))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def medians(fn, reps, blocks):
    fn()
    return [med([timed(fn) for _ in range(reps)]) for _ in range(blocks)]


def fixture_order(field, A, B):
    with open(os.path.join(ROOT, "tests", "golden", "ec_curves.json")) as f:
        return next(int(c["order"]) for c in json.load(f)["curves"] if (c["field"], int(c["A"]), int(c["B"])) == (field, A, B))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    out = {"device": ecfft_amd.device_info(0), "reps": reps, "blocks": blocks, "point_mul": [], "find_generator": [], "build_ec_fftree": []}
    for name in ("m31", "secp256k1"):
        fld = ecfft_amd.FIELDS[name]
        p = fld.MODULUS[name]
        A, B = CURVE[name]
        a_el, b_el = fld.from_ints([A]), fld.from_ints([B])
        x = BASE_X[name]
        f = (x**3 + A * x + B) % p
        y = pow(f, (p + 1) // 4, p)
        assert y * y % p == f
        base = fld.from_ints([x, y])
        ceiling = fld.mul_ceiling(OCCUPANCY[name])
        rng = np.random.default_rng(5)
        # 2^20 points of the curve: random multiples of the base, made by the call itself
        big = COUNTS[-1]
        pts, inf = fld.curve_point_mul(a_el, b_el, np.tile(base, (big,) + (1,) * (base.ndim - 1)), rng.integers(0, 256, (big, 4), dtype=np.uint8))
        assert not inf.any()
        for count in COUNTS:
            P = pts[:2 * count]
            for nb in WIDTHS:
                k = rng.integers(0, 256, (count, nb), dtype=np.uint8)
                k[:, -1] |= 0x80                                   # every scalar has all 8 nb bits, so the count of doublings is known
                nbits = 8 * nb
                ones = int(np.unpackbits(k).sum())
                r = reps if count < (1 << 20) else max(1, reps - 1)
                ms = medians(lambda: fld.curve_point_mul(a_el, b_el, P, k), r, blocks)
                useful = count * (10 * nbits + INV_MULS[name] + 4) + 11 * ones
                issued = count * (21 * nbits + INV_MULS[name] + 4)
                row = {"field": name, "count": count, "scalar_bytes": nb, "ms": ms, "useful_muls": useful, "issued_muls": issued,
                       "useful_per_s": useful / (med(ms) * 1e-3), "issued_per_s": issued / (med(ms) * 1e-3), "ceiling_per_s": ceiling,
                       "waves_per_simd": OCCUPANCY[name]}
                out["point_mul"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        order = fixture_order(name, A, B)
        got = fld.curve_find_generator(a_el, b_el, order)
        row = {"field": name, "curve": [A, B], "log_order": got["log_order"], "x": got["x"],
               "ms": medians(lambda: fld.curve_find_generator(a_el, b_el, order), reps, blocks)}
        out["find_generator"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    fld, cr, n = ecfft_amd.FIELDS["m31"], M31_CRATE, 1 << 12
    args = (fld.from_ints([cr["A"]]), fld.from_ints([cr["B"]]), fld.from_ints(list(cr["gen"])), cr["log_order"], fld.from_ints(list(cr["offset"])))
    row = {"field": "m31", "n": n, "build_ec_fftree_ms": medians(lambda: fld.build_ec_fftree(n, *args), reps, blocks),
           "build_fftree_ms": medians(lambda: fld.build_fftree(n), reps, blocks)}
    out["build_ec_fftree"].append(row)
    print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
