#!/usr/bin/env python3
"""Throughput of the curve search (ecfft_find_curve) on the GPU, in one process, host clock around the synchronous call.
    full scan     a scan that cannot hit: k = 8 * element bytes, 2^22 candidates (secp256k1) / 2^26 (M31) of stream `seed`; one warm-up
                  call, then `blocks` calls, the median.  candidates_per_s from it.
    mul share     field multiplies per second of the scan over ecfft_mul_ceiling of the field (4 waves per SIMD): the multiplies are
                  those the Python model (tests/curve_ref.py) counts for the first `sample` candidates of the same stream, scaled to the
                  scan (an exponentiation is charged its addition chain plus the squaring that checks it)
    stage_lengths entries every stage read during ONE scan (hooks build of the library: ecfft_curve_search_stats): bb square,
                  discriminant, point of order 4, then the halving rounds.  What keeps lanes busy: each launch is dense over its queue.
    stage_ms      host milliseconds around each stage of that scan (launch + the read of the queue length that waits for it)
    cpu baseline  the host instantiation of the same steps (tests/cpp/curve_host.cpp, -O2, one core) on 2^16 candidates
    search        one real search per field, k = 24: its wall time, index and n
usage: findcurve_time.py [blocks [seed]] > profiles/findcurve/findcurve_time.json ; prints one JSON object"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes  # noqa: E402
import torch  # noqa: E402,F401
import ecfft_amd  # noqa: E402
from ecfft_amd import fftree as FT  # noqa: E402
import curve_ref as R  # noqa: E402

SCAN_LOG = {"secp256k1": 22, "m31": 26}
SAMPLE = {"secp256k1": 1 << 12, "m31": 1 << 14}


def cpu_baseline(seed):
    """{field: candidates per second} of the host instantiation on one core"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "curve_host")
        subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "curve_host.cpp"),
                        "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True, capture_output=True)
        out = subprocess.run([exe, str(seed), str(1 << 16), "time"], check=True, capture_output=True, text=True).stdout
    return {ln.split()[0]: float(ln.split()[2]) for ln in out.splitlines() if "candidates_per_s" in ln}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    res = {"device": FT.device_info(), "seed": seed, "blocks": blocks, "cpu_candidates_per_s": cpu_baseline(seed), "fields": []}
    for field in ("secp256k1", "m31"):
        F = ecfft_amd.FIELDS[field]
        k_never, count = 8 * F.elem_bytes, 1 << SCAN_LOG[field]
        scan = lambda: F.find_curve(k_never, seed, max_candidates=count)
        assert scan() is None                                                        # warm-up; nothing reaches n = 8 * bytes
        secs = sorted(timed(scan)[0] for _ in range(blocks))
        med = statistics.median(secs)
        muls = [0]
        for i in range(SAMPLE[field]):
            R.two_sylow_field(field, *R.candidate(field, seed, i), muls=muls)
        muls_per_cand = muls[0] / SAMPLE[field]
        ceiling = F.mul_ceiling(4)
        with FT.use_hooks_library() as L:
            assert ecfft_amd.FIELDS[field].find_curve(k_never, seed, max_candidates=count) is None        # warm-up of this build
            L.ecfft_curve_search_stats(None, None, 0, 1)
            assert ecfft_amd.FIELDS[field].find_curve(k_never, seed, max_candidates=count) is None
            lens, stage_s = (ctypes.c_uint64 * 300)(), (ctypes.c_double * 300)()
            n_len = L.ecfft_curve_search_stats(lens, stage_s, 300, 1)
        stage = [int(v) for v in lens[:n_len]]
        while stage and stage[-1] == 0:
            stage.pop()
        ms = [round(1e3 * stage_s[i], 3) for i in range(len(stage))]
        t_search, hit = timed(lambda: F.find_curve(24, seed, max_candidates=1 << 34))
        res["fields"].append({
            "field": field, "scan_candidates": count, "scan_s": [round(s, 5) for s in secs], "scan_median_s": round(med, 5),
            "candidates_per_s": round(count / med, 1), "model_muls_per_candidate": round(muls_per_cand, 2), "model_sample": SAMPLE[field],
            "mul_per_s": round(count * muls_per_cand / med, 1), "mul_ceiling_per_s": round(ceiling, 1),
            "share_of_mul_ceiling": round(count * muls_per_cand / med / ceiling, 4),
            "gpu_over_one_cpu_core": round(count / med / res["cpu_candidates_per_s"][field], 1),
            "stage_lengths": {"bb_square": stage[0], "discriminant": stage[1], "order4": stage[2], "halving_rounds": stage[3:]},
            "stage_ms": {"bb_square": ms[0], "discriminant": ms[1], "order4": ms[2], "halving_rounds": ms[3:], "halving_total": round(sum(ms[3:]), 3)},
            "search_k24": None if hit is None else {"seconds": round(t_search, 4), "index": hit["index"], "n": hit["n"]},
        })
    print(json.dumps(res))


if __name__ == "__main__":
    main()
