"""CPU tests of tests/rs_codec_ref.py, the exact model behind the GPU tests of ecfft_rs_encode and ecfft_rs_decode_erasures: the
decoder against a brute-force nearest-codeword search on the kept positions over a tiny prime, the identity that lets the
workgroup kernel keep the tables of ALL points under a mask per row, the systematic encoder, and the presence of both calls in the
header and its mirrors."""
import os
import random
import re

import numpy as np
import pytest

import poly_ref as R
import rs_codec_ref as C
import rs_ref as S
from conftest import ROOT

PRIMES = [97, R.P["m31"], R.P["secp256k1"]]


def corrupt(p, ys, positions, rng):
    for pos in positions:
        ys[pos] = (ys[pos] + 1 + rng.randrange(p - 1)) % p


def make_row(p, xs, k, s, e, rng):
    """(data polynomial, received word, mask): a random codeword with s erased positions holding garbage and e errors among the kept"""
    m = len(xs)
    f = [rng.randrange(p) for _ in range(k)]
    ys = S.evaluate(p, f, xs)
    lost = rng.sample(range(m), s)
    erased = [1 if i in lost else 0 for i in range(m)]
    for pos in lost:
        ys[pos] = rng.randrange(p)
    keep = C.kept_positions(erased)
    corrupt(p, ys, rng.sample(keep, min(e, len(keep))), rng)
    return f, ys, erased


def test_decoder_against_nearest_codeword_search_on_the_kept_positions():
    """m = 8, k = 2 over p = 97: every codeword, its distance on the kept positions; a unique codeword within floor((m' - k) / 2)
    must be returned with its distance, anything else is -1"""
    p, m, k = 97, 8, 2
    rng = random.Random(820)
    msgs = np.array([[a, b] for b in range(p) for a in range(p)], dtype=np.int64)
    inside = outside = short = 0
    for trial in range(90):
        xs = rng.sample(range(p), m)
        if trial % 7 == 0 and 0 not in xs:
            xs[rng.randrange(m)] = 0
        s = rng.randrange(0, m + 1) if trial % 9 else m - k + 1 + trial % 2
        s = min(s, m)
        mk = m - s
        radius = (mk - k) // 2 if mk >= k else 0
        e = rng.choice([0, radius, radius + 1, radius + 2, rng.randrange(0, mk + 1)])
        f, ys, erased = make_row(p, xs, k, s, e, rng)
        keep = C.kept_positions(erased)
        out, ne = C.gao_decode_erasures(p, xs, ys, erased, k)
        word, ne2 = C.gao_decode_erasures(p, xs, ys, erased, k, codeword=True)
        assert ne2 == ne and len(out) == k and len(word) == m
        if mk < k:
            assert ne == -1 and out == [0] * k and word == [0] * m
            short += 1
            continue
        V = np.array([[pow(xs[i], j, p) for i in keep] for j in range(k)], dtype=np.int64)
        dist = ((msgs @ V % p) != np.array([ys[i] for i in keep], dtype=np.int64)).sum(axis=1)
        hit = np.nonzero(dist <= radius)[0]
        assert len(hit) <= 1
        if len(hit):
            assert out == [int(c) for c in msgs[hit[0]]] and ne == int(dist[hit[0]])
            assert word == S.evaluate(p, out, xs)
            if e <= radius:
                assert out == f and ne == e
            inside += 1
        else:
            assert ne == -1 and out == [0] * k and word == [0] * m
            outside += 1
    assert inside >= 20 and outside >= 10 and short >= 5


SHAPES = {97: [(8, 2), (15, 7), (12, 4), (2, 1), (9, 9)], R.P["m31"]: [(15, 7), (40, 20)], R.P["secp256k1"]: [(15, 7), (40, 20)]}


@pytest.mark.parametrize("p", PRIMES)
def test_full_interpolant_against_kept_locator_gives_the_punctured_row(p):
    """the identity of the workgroup kernel: (r, t) of (g0', interpolant over all points with erased symbols as 0) at stop' is (r, t) of
    (g0', interpolant over the kept points) — inside and beyond the radius, and with deg g1 = deg g0' (one erasure)"""
    rng = random.Random(p % 991)
    for m, k in SHAPES[p]:
        for trial in range(10):
            xs = rng.sample(range(min(p, 10 ** 9)), m)
            s = min([0, 1, m - k, (m - k) // 2, rng.randrange(0, m - k + 1)][trial % 5], m - k)
            mk = m - s
            e = [0, (mk - k) // 2, (mk - k) // 2 + 1, rng.randrange(0, mk + 1)][trial % 4]
            f, ys, erased = make_row(p, xs, k, s, e, rng)
            full, punct = C.identity_rows(p, xs, ys, erased, k)
            assert full == punct, (m, k, s, e)
            r, t = full
            q, rem = S.G.divmod_school(r, t, p)
            want = C.gao_decode_erasures(p, xs, ys, erased, k)
            if rem or S.deg(q) >= k:
                assert want[1] == -1
            else:
                assert want == (q + [0] * (k - len(q)), S.deg(t))


@pytest.mark.parametrize("p", PRIMES)
def test_systematic_encoder(p):
    rng = random.Random(31)
    for m, k in ((15, 7), (7, 7), (5, 1), (20, 19)):
        xs = rng.sample(range(min(p, 10 ** 9)), m)
        data = [rng.randrange(p) for _ in range(k)]
        word = C.encode_systematic(p, xs, data)
        assert len(word) == m and word[:k] == data
        f = S.interpolate(p, xs[:k], data)
        assert S.deg(f) < k and word == S.evaluate(p, f, xs)
        # a codeword of the code that rs_decode_erasures decodes: with all the parity erased the data alone give it back
        erased = [0] * k + [1] * (m - k)
        assert C.gao_decode_erasures(p, xs, word, erased, k, codeword=True) == (word, 0)


def test_header_and_mirrors_declare_the_codec():
    header = open(os.path.join(ROOT, "include", "ecfft_hip.h")).read()
    for name in ("ecfft_rs_encode", "ecfft_rs_decode_erasures"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+ECFFT_RS_OUT_COEFFS\s+0\b", header) and re.search(r"#define\s+ECFFT_RS_OUT_CODEWORD\s+1\b", header)
    hpp = open(os.path.join(ROOT, "include", "ecfft_fftree.hpp")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in ("rs_encode", "rs_decode_erasures"):
        assert re.search(r"\b%s\s*\(" % name, hpp), name
        assert re.search(r"pub fn %s\s*\(" % name, rust) and re.search(r"pub fn ecfft_%s\s*\(" % name, rust), name
    from ecfft_amd import fftree as FT
    assert callable(FT.FFTree.rs_encode) and callable(FT.FFTree.rs_decode_erasures)
    assert "ecfft_rs_encode" in FT.EXPORTS and "ecfft_rs_decode_erasures" in FT.EXPORTS
    assert (FT.RS_OUT_COEFFS, FT.RS_OUT_CODEWORD) == (0, 1)
