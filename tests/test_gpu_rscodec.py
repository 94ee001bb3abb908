"""GPU tests of the Reed-Solomon codec: ecfft_rs_encode (k_rs_encode_prepare + k_rs_encode_small; above RS_SMALL_MAX the
interpolation and evaluation bodies) and ecfft_rs_decode_erasures (k_rs_prepare + k_rs_decode_ee_small, a received word and its
mask per workgroup; above RS_SMALL_MAX the rows one after another on their compacted points).  Every result is compared byte for
byte, through the oracle's standard-form converters, with the exact model of tests/rs_codec_ref.py: Gao's decoder on the kept
positions, which also decides the rows beyond the radius."""
import ctypes
import random

import numpy as np
import pytest

import gcd_ref as G
import poly_ref as R
import rs_codec_ref as C
import rs_ref as S
from conftest import std_to_field

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
P = R.P
# (erasures, errors) of the small regime at m = 15, k = 7: (8, 0) leaves m' = k, (2, 4) and (1, 4) are beyond the radius, (9, 0) leaves m' < k
PAIRS = [(0, 0), (0, 4), (8, 0), (2, 3), (4, 2), (6, 1), (2, 4), (1, 4), (9, 0)]

_trees = {}
_models = {}


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


def make_points(field, m, seed):
    """m distinct points in scrambled order, 0 among them"""
    p, rng = P[field], random.Random(seed)
    pts = [0]
    while len(pts) < m:
        x = rng.randrange(p)
        if x not in pts:
            pts.append(x)
    rng.shuffle(pts)
    return pts


def make_rows(field, xs, k, pairs, seed):
    """(codewords, words, masks) as int lists, one row per (erasures, errors) pair: a seeded codeword, s positions marked lost and
    filled with garbage, e of the kept ones changed"""
    p, m, rng = P[field], len(xs), random.Random(seed)
    clean, words, masks = [], [], []
    for s, e in pairs:
        c = S.evaluate(p, [rng.randrange(p) for _ in range(k)], xs)
        lost = set(rng.sample(range(m), s))
        w = [rng.randrange(p) if i in lost else c[i] for i in range(m)]
        for pos in rng.sample([i for i in range(m) if i not in lost], e):
            w[pos] = (w[pos] + 1 + rng.randrange(p - 1)) % p
        clean.append(c); words.append(w); masks.append([1 if i in lost else 0 for i in range(m)])
    return clean, words, masks


def model(key, field, xs, words, masks, k):
    """[(message, n_errors, codeword)] of the rows by the exact model, computed once per case"""
    if key not in _models:
        p, out = P[field], []
        for w, e in zip(words, masks):
            msg, ne = C.gao_decode_erasures(p, xs, w, e, k)
            out.append((msg, ne, S.evaluate(p, msg, xs) if ne >= 0 else [0] * len(xs)))
        _models[key] = out
    return _models[key]


def decode(F, field, t, xs, words, masks, k, codeword, device=False):
    """rs_decode_erasures on int rows -> (rows of standard-form output, n_errors)"""
    m, count = len(xs), len(words)
    pts, vals = from_ints(F, field, xs), from_ints(F, field, [y for w in words for y in w])
    er = None if masks is None else np.array(masks, dtype=np.uint8).reshape(-1)
    if device:
        import torch
        out, n_err = t.rs_decode_erasures(torch.from_numpy(pts).cuda(), torch.from_numpy(vals).cuda(),
                                          None if er is None else torch.from_numpy(er).cuda(), k, count=count, codeword=codeword)
        assert out.is_cuda
        out = out.cpu().numpy()
    else:
        out, n_err = t.rs_decode_erasures(pts, vals, er, k, count=count, codeword=codeword)
    no = m if codeword else k
    assert out.shape[0] == count * no and n_err.shape == (count,) and n_err.dtype == np.int64
    return to_std(F, out), n_err


def check(F, field, t, key, xs, words, masks, k, codeword, device=False):
    want = model(key, field, xs, words, masks, k)
    out, n_err = decode(F, field, t, xs, words, masks, k, codeword, device)
    no = len(xs) if codeword else k
    for i, (msg, ne, word) in enumerate(want):
        assert n_err[i] == ne, (i, n_err[i], ne)
        assert np.array_equal(out[i * no:(i + 1) * no], G.arr(field, word if codeword else msg, no)), i
    return [w[1] for w in want]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("codeword", [False, True])
def test_small_regime_mixed_rows_in_one_call(oracle_mod, field, codeword):
    """m = 15, k = 7: 70 rows, every row its own mask, the nine pairs first; host arrays, then device tensors"""
    m, k = 15, 7
    F, t = oracle_mod.field(field), tree(field, 4)
    xs = make_points(field, m, 1507)
    pairs = (PAIRS * 8)[:70]
    clean, words, masks = make_rows(field, xs, k, pairs, 1508)
    verdicts = check(F, field, t, ("mixed", field), xs, words, masks, k, codeword)
    for i, (s, e) in enumerate(pairs):
        if 2 * e <= m - s - k:                                         # within the radius: the codeword that was sent
            assert verdicts[i] == e and model(("mixed", field), field, xs, words, masks, k)[i][2] == clean[i]
        if m - s < k:
            assert verdicts[i] == -1
    assert verdicts[6] == -1 and verdicts[7] == -1                      # beyond the radius: what the model gave on these inputs
    assert check(F, field, t, ("mixed", field), xs, words, masks, k, codeword, device=True) == verdicts


@pytest.mark.parametrize("field", FIELDS)
def test_full_width_of_the_workgroup(oracle_mod, field):
    m, k = 255, 223
    F, t = oracle_mod.field(field), tree(field, 4)
    xs = make_points(field, m, 255223)
    pairs = [(10, 11), (32, 0), (0, 16), (33, 0)]
    clean, words, masks = make_rows(field, xs, k, pairs, 255)
    for codeword in (False, True):
        assert check(F, field, t, ("full", field), xs, words, masks, k, codeword, device=codeword) == [11, 0, 16, -1]
    assert [w[2] for w in model(("full", field), field, xs, words, masks, k)[:3]] == clean[:3]


@pytest.mark.parametrize("field", FIELDS)
def test_shortest_codes(oracle_mod, field):
    F, t, p = oracle_mod.field(field), tree(field, 4), P[field]
    for codeword in (False, True):
        assert check(F, field, t, ("m1", field), [5], [[77], [0], [p - 1]], [[0], [0], [1]], 1, codeword) == [0, 0, -1]
        xs = [3, 0]
        words, masks = [[9, 123], [456, 11], [8, 8], [1, 2]], [[0, 1], [1, 0], [0, 0], [1, 1]]
        assert check(F, field, t, ("m2", field), xs, words, masks, 1, codeword) == [0, 0, 0, -1]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m,k", [(15, 7), (64, 32), (255, 223), (300, 200)])
def test_without_erasures_it_is_rs_decode(oracle_mod, field, m, k):
    """erased = None and an all-zero mask: the bytes of rs_decode, message and verdict, at 0, 1, the radius and one error beyond it;
    (300, 200) is the large regime, on the smallest tree its rule allows"""
    F, t = oracle_mod.field(field), tree(field, 1024 if m > 255 else 4)
    rad = (m - k) // 2
    xs = make_points(field, m, 100 * m + k)
    clean, words, masks = make_rows(field, xs, k, [(0, 0), (0, 1), (0, rad), (0, rad + 1)], m + k)
    pts, vals = from_ints(F, field, xs), from_ints(F, field, [y for w in words for y in w])
    message, n_err = t.rs_decode(pts, vals, k, count=4)
    assert list(n_err[:3]) == [0, 1, rad]
    for er in (None, np.zeros(4 * m, np.uint8), np.zeros(4 * m, bool)):
        out, ne = t.rs_decode_erasures(pts, vals, er, k, count=4)
        assert out.tobytes() == message.tobytes() and np.array_equal(ne, n_err)
    word, ne = t.rs_decode_erasures(pts, vals, None, k, count=4, codeword=True)
    assert np.array_equal(ne, n_err)
    for i in range(4):
        want = S.evaluate(P[field], to_ints(F, field, message[i * k:(i + 1) * k]), xs) if n_err[i] >= 0 else [0] * m
        assert np.array_equal(to_std(F, word[i * m:(i + 1) * m]), G.arr(field, want, m)), i


@pytest.mark.parametrize("field", FIELDS)
def test_large_regime(oracle_mod, field):
    """m = 300, k = 200 on the smallest tree the rule allows; (60, 10) leaves m' = 240, below the small bound"""
    m, k = 300, 200
    F, t = oracle_mod.field(field), tree(field, 1024)
    xs = make_points(field, m, 300200)
    pairs = [(20, 40), (100, 0), (60, 10), (0, 50), (30, 36)]
    clean, words, masks = make_rows(field, xs, k, pairs, 300)
    for codeword in (False, True):
        verdicts = check(F, field, t, ("large", field), xs, words, masks, k, codeword, device=codeword)
        assert verdicts[:4] == [40, 0, 10, 50]
    want = model(("large", field), field, xs, words, masks, k)
    assert [w[2] for w in want[:4]] == clean[:4]


@pytest.mark.parametrize("field", FIELDS)
def test_large_regime_compaction_boundaries(oracle_mod, field):
    """m = 300, k = 200, erasures only, one call: m' = 300 (a clean row), 256 (the first length that is interpolated on the tree),
    255 (the last one for the compacted small kernels), 200 (m' = k) and 199 (m' < k: skipped)"""
    m, k = 300, 200
    F, t = oracle_mod.field(field), tree(field, 1024)
    xs = make_points(field, m, 300256)
    clean, words, masks = make_rows(field, xs, k, [(0, 0), (44, 0), (45, 0), (100, 0), (101, 0)], 256)
    for codeword in (False, True):
        assert check(F, field, t, ("bounds", field), xs, words, masks, k, codeword) == [0, 0, 0, 0, -1]
    assert [w[2] for w in model(("bounds", field), field, xs, words, masks, k)[:4]] == clean[:4]


ENC = [(15, 7), (255, 223), (7, 7), (5, 1), (300, 200)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m,k", ENC)
def test_encoder(oracle_mod, field, m, k):
    """against the model and against poly_interpolate + poly_eval_points, one row and 33 rows, host arrays and device tensors"""
    import torch
    p = P[field]
    F, t, big = oracle_mod.field(field), tree(field, 1024 if m > 255 else 4), tree(field, 1024)
    xs = make_points(field, m, 7 * m + k)
    rng = random.Random(m - k)
    pts = from_ints(F, field, xs)
    for count in (1, 33):
        data = [[rng.randrange(p) for _ in range(k)] for _ in range(count)]
        flat = from_ints(F, field, [y for d in data for y in d])
        word = t.rs_encode(pts, flat, k, count=count)
        assert word.shape[0] == count * m
        std = to_std(F, word)
        for b in range(count):
            assert np.array_equal(std[b * m:(b + 1) * m], G.arr(field, C.encode_systematic(p, xs, data[b]), m)), b
            assert np.array_equal(std[b * m:b * m + k], G.arr(field, data[b], k))
        dev = t.rs_encode(torch.from_numpy(pts).cuda(), torch.from_numpy(flat).cuda(), k, count=count)
        assert dev.is_cuda and dev.cpu().numpy().tobytes() == word.tobytes()
        if k < m:
            coef = big.poly_interpolate(pts[:k], flat, count=count)
            par = big.poly_eval_points(coef, pts[k:], count=count)
            for b in range(count):
                assert par[b * (m - k):(b + 1) * (m - k)].tobytes() == word[b * m + k:(b + 1) * m].tobytes()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m,k,n", [(15, 7, 4), (255, 223, 4), (300, 200, 1024)])
def test_round_trip(oracle_mod, field, m, k, n):
    """rs_encode, then erasures and errors within the radius, then rs_decode_erasures(codeword=True): the codeword that was sent"""
    p = P[field]
    F, t = oracle_mod.field(field), tree(field, n)
    xs = make_points(field, m, m * k)
    rng = random.Random(m + 3 * k)
    pts = from_ints(F, field, xs)
    budget = [(m - k, 0), (0, (m - k) // 2), ((m - k) // 2, (m - k) // 4), (1, (m - k - 1) // 2)]
    count = len(budget)
    data = from_ints(F, field, [rng.randrange(p) for _ in range(count * k)])
    sent = t.rs_encode(pts, data, k, count=count)
    recv, mask = sent.copy(), np.zeros((count, m), np.uint8)
    junk = from_ints(F, field, [rng.randrange(p) for _ in range(count * m)])
    rows = to_ints(F, field, sent)
    for b, (s, e) in enumerate(budget):
        lost = rng.sample(range(m), s)
        bad = rng.sample([i for i in range(m) if i not in lost], e)
        mask[b, lost] = 1
        for i in lost:
            recv[b * m + i] = junk[b * m + i]
        for i in bad:
            recv[b * m + i] = from_ints(F, field, [(rows[b * m + i] + 1 + rng.randrange(p - 1)) % p])[0]
    word, n_err = t.rs_decode_erasures(pts, recv, mask, k, count=count, codeword=True)
    assert list(n_err) == [e for _, e in budget]
    assert word.tobytes() == sent.tobytes()
    coef, n_err = t.rs_decode_erasures(pts, recv, mask, k, count=count)
    assert list(n_err) == [e for _, e in budget]
    for b in range(count):
        assert S.evaluate(p, to_ints(F, field, coef[b * k:(b + 1) * k]), xs[:k]) == to_ints(F, field, data[b * k:(b + 1) * k])


def test_argument_errors(oracle_mod):
    from ecfft_amd import fftree as FT
    field = "m31"
    F, t, p = oracle_mod.field(field), tree(field, 4), P[field]
    xs = [5, 9, 11, 2, 7, 3]
    word = from_ints(F, field, S.evaluate(p, [1, 2], xs))
    none = np.zeros(6, np.uint8)
    for k in (0, 7):                                                            # k = 0, k > m
        with pytest.raises(ValueError):
            t.rs_decode_erasures(from_ints(F, field, xs), word, none, k)
        with pytest.raises(ValueError):
            t.rs_encode(from_ints(F, field, xs), from_ints(F, field, list(range(k))), k)
    pts, out, n_err = from_ints(F, field, xs), np.zeros(6, F.dtype), np.zeros(1, np.int64)
    call = lambda form, ne: t._L.ecfft_rs_decode_erasures(t._h, pts.ctypes.data, 6, word.ctypes.data, none.ctypes.data, 2, out.ctypes.data, form, ne, 1,
                                                          FT.MEM_HOST, None)
    assert call(2, n_err.ctypes.data) == FT.ERR_BAD_ARG and call(-1, n_err.ctypes.data) == FT.ERR_BAD_ARG          # an unknown out_form
    assert call(FT.RS_OUT_COEFFS, None) == FT.ERR_BAD_ARG                                                          # n_errors is required
    assert call(FT.RS_OUT_COEFFS, n_err.ctypes.data) == FT.OK and n_err[0] == 0
    twice = from_ints(F, field, [5, 9, 11, 2, 9, 3])                           # points 1 and 4 are equal
    with pytest.raises(ValueError):
        t.rs_decode_erasures(twice, word, none, 2)
    with pytest.raises(ValueError):                                             # also when one of the two is erased in every row
        t.rs_decode_erasures(twice, np.concatenate([word, word]), np.array([0, 0, 0, 0, 1, 0] * 2, np.uint8), 2, count=2)
    for k in (2, 5, 6):                                                         # a data and a parity point, two data points, k = m
        with pytest.raises(ValueError):
            t.rs_encode(twice, word[:k], k)
    with pytest.raises(ValueError):                                             # two parity points
        t.rs_encode(from_ints(F, field, [5, 9, 11, 2, 7, 2]), word[:3], 3)
    out, n_err = t.rs_decode_erasures(pts, word, np.array([1, 0, 0, 1, 0, 0], np.uint8), 2, codeword=True)         # the context keeps working
    assert n_err[0] == 0 and out.tobytes() == word.tobytes()
    assert t.rs_encode(pts, word[:2], 2).tobytes() == word.tobytes()
    # the large regime: equal points (one of them erased), and trees that are too small, checked before anything runs
    big = list(range(1, 301))
    vals, dup = from_ints(F, field, big), from_ints(F, field, big[:-1] + [1])
    lost = np.zeros(300, np.uint8)
    lost[299] = 1
    with pytest.raises(ValueError):
        tree(field, 1024).rs_decode_erasures(dup, vals, lost, 100)
    with pytest.raises(ValueError):
        tree(field, 1024).rs_encode(dup, vals[:100], 100)
    with pytest.raises(ValueError, match="too small"):
        tree(field, 512).rs_decode_erasures(vals, vals, lost, 100)
    with pytest.raises(ValueError, match="too small"):
        tree(field, 64).rs_encode(vals, vals[:100], 100)
    assert tree(field, 128).rs_encode(vals, vals[:100], 100).shape[0] == 300     # next_pow2(k) leaves are enough
    out, n_err = tree(field, 1024).rs_decode_erasures(vals, vals, lost, 2)       # f = x at the points 1 .. 300
    assert n_err[0] == 0 and to_ints(F, field, out) == [0, 1]
