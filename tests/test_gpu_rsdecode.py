"""GPU tests of ecfft_rs_decode (Gao's Reed-Solomon decoder): k_rs_prepare + k_rs_decode_small (code length m <= RS_SMALL_MAX, a
received word per workgroup, on any tree) and the large regime (the interpolation body, the partial xgcd driver and the division
body, row by row).  Codewords come from the library's own encoder, poly_eval_points; verdict and message are compared byte for
byte, through the oracle's standard-form converters, with the exact model of tests/rs_ref.py.  Beyond the decoding radius the model
decides what is expected — a failure or another codeword."""
import ctypes
import random

import numpy as np
import pytest

import gcd_ref as G
import poly_ref as R
import rs_ref as S
from conftest import std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P
SMALL = [(8, 4), (64, 32), (255, 223), (255, 1), (16, 16)]
LARGE = {"secp256k1": (300, 200), "m31": (1100, 900)}

_trees = {}


def tree(field, n):
    import ecfft_amd
    if (field, n) not in _trees:
        _trees[(field, n)] = ecfft_amd.FIELDS[field].build_fftree(n)
    return _trees[(field, n)]


def to_std(F, x):
    x = np.ascontiguousarray(x, F.dtype)
    out = np.empty_like(x)
    if x.shape[0]:
        F._to_std(x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), x.shape[0])
    return out


def to_ints(F, field, x):
    return R.to_ints(field, to_std(F, x))


def from_ints(F, field, v):
    return std_to_field(F, G.arr(field, v, len(v)))


def make_points(F, field, m, seed):
    """m distinct points in scrambled order: 0, the four leaves of the smallest tree, the rest seeded"""
    p, rng = P[field], random.Random(seed)
    pts = [0] + to_ints(F, field, tree(field, 4).leaves())
    while len(pts) < m:
        x = rng.randrange(p)
        if x not in pts:
            pts.append(x)
    pts = pts[:m]
    rng.shuffle(pts)
    return pts


def encode(F, field, xs, msgs, k):
    """the codewords of the messages (int lists) at xs, by poly_eval_points on a tree that holds k coefficients"""
    n = 64
    while n < k:
        n <<= 1
    f = from_ints(F, field, [c for msg in msgs for c in msg])
    return to_ints(F, field, tree(field, n).poly_eval_points(f, from_ints(F, field, xs), count=len(msgs)))


def received(F, field, xs, k, errors, seed):
    """(messages, words): one seeded message per entry of `errors`, its codeword with that many positions changed at seeded places"""
    p, m, rng = P[field], len(xs), random.Random(seed)
    msgs = [[rng.randrange(p) for _ in range(k)] for _ in errors]
    flat = encode(F, field, xs, msgs, k)
    words = []
    for i, e in enumerate(errors):
        w = flat[i * m:(i + 1) * m]
        assert m > 300 or w == S.evaluate(p, msgs[i], xs)                   # the encoder itself, where the model is quick
        for pos in rng.sample(range(m), min(e, m)):
            w[pos] = (w[pos] + 1 + rng.randrange(p - 1)) % p
        words.append(w)
    return msgs, words


def decode_and_check(F, field, t, xs, words, k, msgs=None, errors=None, device=False):
    """rs_decode on the words against the model; within the radius also against the messages themselves"""
    p, m, count = P[field], len(xs), len(words)
    pts, vals = from_ints(F, field, xs), from_ints(F, field, [y for w in words for y in w])
    if device:
        import torch
        message, n_err = t.rs_decode(torch.from_numpy(pts).cuda(), torch.from_numpy(vals).cuda(), k, count=count)
        assert message.is_cuda
        message = message.cpu().numpy()
    else:
        message, n_err = t.rs_decode(pts, vals, k, count=count)
    assert message.shape[0] == count * k and n_err.shape == (count,) and n_err.dtype == np.int64
    message = to_std(F, message)
    want = [S.gao_decode(p, xs, w, k) for w in words]
    for i, (msg, ne) in enumerate(want):
        assert n_err[i] == ne, (i, n_err[i], ne)
        assert np.array_equal(message[i * k:(i + 1) * k], G.arr(field, msg, k)), i
        if msgs is not None and errors[i] <= (m - k) // 2:
            assert msg == msgs[i] and ne == errors[i]
    return [w[1] for w in want]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m,k", SMALL)
def test_small_regime(oracle_mod, field, m, k):
    """e = 0, 1, the radius and one beyond it, all four rows in one call on a tree of four leaves"""
    F, t = oracle_mod.field(field), tree(field, 4)
    rad = (m - k) // 2
    xs = make_points(F, field, m, 100 * m + k)
    errors = [0, 1, rad, rad + 1]
    msgs, words = received(F, field, xs, k, errors, m + k)
    decode_and_check(F, field, t, xs, words, k, msgs, errors)


@pytest.mark.parametrize("field", FIELDS)
def test_large_regime(oracle_mod, field):
    m, k = LARGE[field]
    n = 4
    while n < 2 * m + 1:
        n <<= 1
    F, t = oracle_mod.field(field), tree(field, n)
    rad = (m - k) // 2
    xs = make_points(F, field, m, 7)
    errors = [0, 1, rad, rad + 1]
    msgs, words = received(F, field, xs, k, errors, 8)
    decode_and_check(F, field, t, xs, words, k, msgs, errors)
    with pytest.raises(ValueError, match="too small"):                 # one size below next_pow2(2 m + 1), checked before anything runs
        tree(field, n // 2).rs_decode(from_ints(F, field, xs), from_ints(F, field, words[0]), k)


@pytest.mark.parametrize("field", FIELDS)
def test_failing_row_among_good_ones(oracle_mod, field):
    """rows of different error counts in one call, one of them far beyond the radius, and the all-zero word; then the same call on
    device tensors"""
    m, k = 64, 32
    F, t = oracle_mod.field(field), tree(field, 4)
    xs = make_points(F, field, m, 21)
    errors = [3, 16, 24, 0, 9]
    msgs, words = received(F, field, xs, k, errors, 22)
    words.append([0] * m)
    verdicts = decode_and_check(F, field, t, xs, words, k)
    assert verdicts == [3, 16, -1, 0, 9, 0]
    assert decode_and_check(F, field, t, xs, words, k, device=True) == verdicts


@pytest.mark.parametrize("field", FIELDS)
def test_more_rows_than_one_wave_of_workgroups(oracle_mod, field):
    """600 rows of a short code in one call: every row its own error count"""
    m, k = 12, 4
    F, t = oracle_mod.field(field), tree(field, 4)
    xs = make_points(F, field, m, 31)
    errors = [i % 6 for i in range(600)]
    msgs, words = received(F, field, xs, k, errors, 32)
    decode_and_check(F, field, t, xs, words, k, msgs, errors)


def test_argument_errors(oracle_mod):
    from ecfft_amd import fftree as FT
    assert FT.RS_SMALL_MAX == 255
    field = "m31"
    F, t = oracle_mod.field(field), tree(field, 4)
    xs = [5, 9, 11, 2, 7, 3]
    word = from_ints(F, field, S.evaluate(P[field], [1, 2], xs))
    with pytest.raises(ValueError):
        t.rs_decode(from_ints(F, field, [5, 9, 11, 2, 9, 3]), word, 2)          # two equal points, found on the device
    with pytest.raises(ValueError):
        t.rs_decode(from_ints(F, field, xs), word, 7)                           # k > m
    with pytest.raises(ValueError):
        t.rs_decode(from_ints(F, field, xs), word, 0)
    message, n_err = t.rs_decode(from_ints(F, field, xs), word, 2)              # the context keeps working
    assert n_err[0] == 0 and to_ints(F, field, message) == [1, 2]
    big = list(range(1, 301))
    with pytest.raises(ValueError):                                             # two equal points in the large regime
        tree(field, 1024).rs_decode(from_ints(F, field, big[:-1] + [1]), from_ints(F, field, big), 100)
