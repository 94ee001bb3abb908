"""CPU test of the exact model of seq_min_poly / seq_nth_term (tests/seq_ref.py), which tests/test_gpu_seq.py compares the GPU
with: the Euclid route the library defines agrees with textbook Berlekamp-Massey on every row with 2 L <= N and reports every row
with 2 L > N as undetermined; nth_terms equals the recurrence run term by term."""
import random

import pytest

import seq_ref as Q

PRIMES = {"secp256k1": 2**256 - 2**32 - 977, "m31": 2**31 - 1, "p2": 2, "p3": 3, "p7": 7}


def rows_of(p, n, rng):
    """recurrent rows of random order 0 .. n, the zero row, one non-zero term first, in the middle or last, uniform rows"""
    rows = [[0] * n]
    for pos in {0, n // 2, n - 1}:
        rows.append([1 + rng.randrange(p - 1) if i == pos else 0 for i in range(n)])
    for _ in range(3):
        rows.append([rng.randrange(p) for _ in range(n)])
    for _ in range(6):
        L = rng.randrange(n + 1)
        C = [rng.randrange(p) for _ in range(L)] + [1]
        rows.append(Q.iterate(p, C, [rng.randrange(p) for _ in range(L)], n) if L else [0] * n)
    return rows


@pytest.mark.parametrize("name", sorted(PRIMES))
def test_euclid_route_is_berlekamp_massey(name):
    p, rng = PRIMES[name], random.Random(len(name) + PRIMES[name] % 1000)
    determined = undetermined = 0
    for n in range(1, 41):
        for s in rows_of(p, n, rng):
            L, C = Q.berlekamp_massey(p, s)
            assert len(C) == L + 1 and C[L] == 1
            assert all((sum(C[j] * s[i + j] for j in range(L + 1))) % p == 0 for i in range(n - L)), (n, s)
            got = Q.euclid_min_poly(p, s)
            if 2 * L <= n:
                assert got == (L, C), (n, s, L, C, got)
                determined += 1
            else:
                assert got == (-1, []), (n, s, L, got)
                undetermined += 1
    assert determined > 100 and undetermined > 100


def test_the_edges_of_the_definition():
    p = PRIMES["m31"]
    assert Q.euclid_min_poly(p, [0]) == (0, [1]) and Q.euclid_min_poly(p, [5]) == (-1, [])
    assert Q.euclid_min_poly(p, [0, 0, 0, 0]) == (0, [1])
    assert Q.euclid_min_poly(p, [3, 6, 12, 24]) == (1, [p - 2, 1])
    assert Q.euclid_min_poly(p, [0, 0, 1, 1, 2, 3, 5, 8]) == (3, [0, p - 1, p - 1, 1])       # x (x^2 - x - 1): c_0 = 0
    assert Q.euclid_min_poly(p, [0, 0, 1, 1, 2]) == (-1, [])                     # the same with N = 5 < 2 L
    assert Q.euclid_min_poly(p, [0, 1, 1, 2, 3, 5, 8, 13]) == (2, [p - 1, p - 1, 1])
    assert Q.euclid_min_poly(p, [0, 0, 0, 0, 0, 7]) == (-1, [])


@pytest.mark.parametrize("name", sorted(PRIMES))
def test_nth_terms_is_the_recurrence(name):
    p, rng = PRIMES[name], random.Random(77)
    for L in (1, 2, 3, 7):
        for monic in (True, False):
            C = [rng.randrange(p) for _ in range(L)] + [1 if monic else 1 + rng.randrange(p - 1)]
            init = [rng.randrange(p) for _ in range(L)]
            want = Q.iterate(p, C, init, 306)
            for K in range(301):
                assert Q.nth_terms(p, C, init, K, 1) == want[K:K + 1], (L, K)
            for K in (0, 1, L, 150, 300):
                assert Q.nth_terms(p, C, init, K, 5) == want[K:K + 5], (L, K)
    assert Q.nth_terms(p, [0, 0, 1], [0, 0], 10**6, 2) == [0, 0]


def test_both_calls_are_declared_in_the_header_and_the_three_mirrors():
    import os
    import re
    from conftest import ROOT
    read = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    header, py = read("include", "ecfft_hip.h"), read("ecfft_amd", "fftree.py")
    hpp, rs = read("include", "ecfft_fftree.hpp"), read("bindings", "rust", "src", "lib.rs")
    for name in ("ecfft_seq_min_poly", "ecfft_seq_nth_term"):
        assert re.search(r"^int %s\(" % name, header, re.M) and '"%s"' % name in py and name + "(" in hpp and "pub fn %s(" % name in rs
    assert "def seq_min_poly(" in py and "def seq_nth_term(" in py and "pub fn seq_min_poly(" in rs and "pub fn seq_nth_term(" in rs
    assert " min_poly(const std::vector<Elem>& seq" in hpp and " nth_term(const std::vector<Elem>& char_poly" in hpp
    small = {k: int(v) for k, v in re.findall(r"#define ECFFT_(SEQ_SMALL_MAX|SEQ_TERM_SMALL_MAX|GCD_SMALL_MAX|COMPOSE_SMALL_MAX)\s+(\d+)", header)}
    assert small["SEQ_SMALL_MAX"] == small["GCD_SMALL_MAX"] - 1 == 255 and small["SEQ_TERM_SMALL_MAX"] == small["COMPOSE_SMALL_MAX"] == 65
    assert "SEQ_SMALL_MAX = 255" in py and "SEQ_TERM_SMALL_MAX = 65" in py
