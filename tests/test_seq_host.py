"""CPU test of the host-side staging of ecfft_seq_min_poly / ecfft_seq_nth_term (ecfft_amd/csrc/seq_host.h: the bit length of the
index, the size arithmetic that must not wrap) by a stand-alone program, tests/cpp/seq_host.cpp, built with AddressSanitizer and
UBSan: indices in heap buffers of exactly their length, shapes up to SIZE_MAX against 128-bit arithmetic."""
import os
import subprocess

from conftest import ROOT


def test_index_bits_and_size_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "seq_host")
    src = os.path.join(ROOT, "tests", "cpp", "seq_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", src, "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SEQ_HOST_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "index bit lengths" in r.stdout and "size arithmetic" in r.stdout
