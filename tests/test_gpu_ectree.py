"""GPU tests of trees on short-Weierstrass curves (include/ecfft_hip.h: ecfft_curve_find_generator, ecfft_build_ec_fftree) against the
exact Python-int model tests/ec_ref.py: the generator search on the curves of tests/golden/ec_curves.json, and trees built from its
own outputs.  Every expectation is an equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import curve_ref
import ec_ref as E
import schoof_ref

pytestmark = pytest.mark.gpu

CYCLIC = [("m31", 1, 6), ("m31", 1, 3), ("m31", 1, 0), ("secp256k1", 1, 0)]


def field_of(field):
    import ecfft_amd
    return ecfft_amd.FIELDS[field]


def curve(field, A, B):
    return next(c for c in E.fixture() if (c["field"], c["A"], c["B"]) == (field, A, B))


def ints_of(field, arr):
    return field_of(field).to_ints(arr)


def gpu_find(field, A, B, order, **kw):
    F = field_of(field)
    r = F.curve_find_generator(F.from_ints([A]), F.from_ints([B]), order, **kw)
    if r is None:
        return None
    return r["log_order"], tuple(ints_of(field, r["gen"])), tuple(ints_of(field, r["offset"])), r["x"]


@functools.lru_cache(maxsize=None)
def model_find(field, A, B, order, start=1, max_candidates=200):
    return E.find_generator(A, B, order, E.P[field], start, max_candidates)


# ---- find_generator ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,A,B", CYCLIC)
@pytest.mark.parametrize("start", [1, 2])
def test_find_generator_matches_the_model(field, A, B, start):
    p, order = E.P[field], curve(field, A, B)["order"]
    want = model_find(field, A, B, order, start)
    assert want is not None
    v, gen, off, x = want
    assert v == E.v2(order) and E.two_adicity(gen, A, p, v) == v
    got = gpu_find(field, A, B, order, start=start, max_candidates=200)
    assert got == want
    # other windows, which the scan cuts into other batches (64, 256, ... candidates): the same answer wherever it is defined
    for mx in (x - start + 1, 64, 65, 321, 1000):
        assert gpu_find(field, A, B, order, start=start, max_candidates=mx) == model_find(field, A, B, order, start, mx)
    if x > start:
        assert gpu_find(field, A, B, order, start=start, max_candidates=x - start) is None          # the window ends before the winner
    if off == (0, 0):
        assert order == 1 << v                                                                      # a 2-group has no coset offset
    else:
        assert E.double_n(off, v + 1, A, p) is not None


def test_find_generator_answers_of_the_issue():
    """x = 3 (the second valid candidate) on secp256k1 (1, 0), a generator of order 16; x = 2 on M31 (1, 6) and (1, 3)"""
    v, gen, off, x = gpu_find("secp256k1", 1, 0, curve("secp256k1", 1, 0)["order"])
    assert (v, x) == (4, 3)
    assert gpu_find("m31", 1, 6, curve("m31", 1, 6)["order"])[3] == 2 and gpu_find("m31", 1, 3, curve("m31", 1, 3)["order"])[3] == 2
    assert gpu_find("m31", 1, 0, 1 << 31)[2] == (0, 0)


@pytest.mark.parametrize("field,A,B", [("secp256k1", -1, 0), ("secp256k1", 0, 1)])
def test_find_generator_on_a_2_sylow_subgroup_that_is_not_cyclic(field, A, B):
    p = E.P[field]
    order = curve(field, A % p, B)["order"]
    assert model_find(field, A % p, B, order) is None
    assert gpu_find(field, A % p, B, order, max_candidates=200) is None
    assert gpu_find(field, A % p, B, order, start=2, max_candidates=70) is None


@pytest.mark.parametrize("field,A,B", [("m31", 1, 6), ("secp256k1", 1, 0), ("secp256k1", 0, 1)])
def test_find_generator_rejects_a_wrong_order(field, A, B):
    order = curve(field, A, B)["order"]
    with pytest.raises(ValueError):
        gpu_find(field, A, B, order + 2)
    assert gpu_find(field, A, B, order + 1) is None                   # an odd order: nothing to look for


# ---- build_ec_fftree -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 64, 4096])
def test_the_crates_m31_constants_give_build_fftree(n):
    from ecfft_amd import fftree as FT
    F, cr = field_of("m31"), E.CRATE_M31
    t = F.build_ec_fftree(n, F.from_ints([cr["A"]]), F.from_ints([cr["B"]]), F.from_ints(list(cr["gen"])), cr["log_order"], F.from_ints(list(cr["offset"])))
    ref = F.build_fftree(n)
    assert t.n == ref.n == n
    m = n
    while m >= 2:
        for which in range(11):
            assert t.table(which, m).tobytes() == ref.table(which, m).tobytes(), (which, m)
        m //= 2
    for k in range(n.bit_length() - 1):
        for got, want in zip(t.rational_map(k), ref.rational_map(k)):
            assert got.tobytes() == want.tobytes()


@functools.lru_cache(maxsize=None)
def found(field, A, B):
    F = field_of(field)
    r = F.curve_find_generator(F.from_ints([A]), F.from_ints([B]), curve(field, A, B)["order"])
    return r


@pytest.mark.parametrize("field,A,B,sizes", [("secp256k1", 1, 0, [2, 4, 8, 16]), ("m31", 1, 6, [2, 4, 8, 16, 32, 64])])
def test_trees_from_find_generators_own_outputs(field, A, B, sizes):
    F, p = field_of(field), E.P[field]
    r = found(field, A, B)
    v, gen, off = r["log_order"], tuple(ints_of(field, r["gen"])), tuple(ints_of(field, r["offset"]))
    assert v == sizes[-1].bit_length() - 1
    rng = np.random.default_rng(31)
    for n in sizes:
        t = F.build_ec_fftree(n, F.from_ints([A]), F.from_ints([B]), r["gen"], v, r["offset"])
        assert t.n == n
        leaves = ints_of(field, t.leaves())
        assert leaves == E.leaves(A, B, gen, v, off, n, p) and len(set(leaves)) == n
        g = E.double_n(gen, v - (n.bit_length() - 1), A, p)
        maps = E.velu_chain(A, B, g, n.bit_length() - 1, p)
        for k, (num, den) in enumerate(maps):
            gn, gd = t.rational_map(k)
            assert (tuple(ints_of(field, gn)), tuple(ints_of(field, gd))) == (num, den)
        coeffs = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)]
        evals = t.enter(F.from_ints(coeffs))

        def horner(x):
            acc = 0
            for c in reversed(coeffs):
                acc = (acc * x + c) % p
            return acc
        assert ints_of(field, evals) == [horner(x) for x in leaves]
        assert ints_of(field, t.exit(evals)) == coeffs
    assert F.build_ec_fftree(2 * sizes[-1], F.from_ints([A]), F.from_ints([B]), r["gen"], v, r["offset"]) is None       # ECFFT_ERR_TREE_TOO_LARGE


@pytest.mark.parametrize("n", [64, 4096])
def test_the_crates_good_curve_in_short_weierstrass_form(n):
    """y^2 = x (x^2 + a x + bb) carried to (A, B) by x -> x - a/3, generator and offset shifted with it: the leaves are the crate's plus a/3"""
    F, p, cr = field_of("secp256k1"), E.P["secp256k1"], curve_ref.CRATE
    A, B = schoof_ref.from_find_curve(cr["a"], cr["bb"], p)
    sh = cr["a"] * pow(3, -1, p) % p
    gen, off = ((cr["gen"][0] + sh) % p, cr["gen"][1]), ((cr["offset"][0] + sh) % p, cr["offset"][1])
    t = F.build_ec_fftree(n, F.from_ints([A]), F.from_ints([B]), F.from_ints(list(gen)), cr["log_order"], F.from_ints(list(off)))
    ref = F.build_fftree(n)
    assert ints_of("secp256k1", t.leaves()) == [(x + sh) % p for x in ints_of("secp256k1", ref.leaves())]


def test_build_ec_fftree_error_rows():
    """every row of the header's table, one thing wrong at a time, on a machine where a good call succeeds"""
    import ecfft_amd
    FT, L = ecfft_amd.fftree, ecfft_amd.lib()
    field, A, B = "secp256k1", 1, 0
    F, p = field_of(field), E.P[field]
    r = found(field, A, B)
    v, gen, off = r["log_order"], tuple(ints_of(field, r["gen"])), tuple(ints_of(field, r["offset"]))
    one = lambda val: F.from_ints([val])
    pt = lambda xy: F.from_ints(list(xy))

    def call(n=16, a=A, b=B, g=gen, m=v, o=off, out=True):
        h = C.c_void_p()
        aa, bb, gg, oo = one(a), one(b), pt(g), pt(o)
        rc = L.ecfft_build_ec_fftree(F.id, n, aa.ctypes.data, bb.ctypes.data, gg.ctypes.data, m, oo.ctypes.data, 0, C.byref(h) if out else None)
        if h.value:
            L.ecfft_ctx_destroy(h)
        return rc

    assert call() == FT.OK
    assert call(n=12) == FT.ERR_NOT_POW2
    assert call(n=32) == FT.ERR_TREE_TOO_LARGE
    g2 = E.add(gen, gen, A, p)
    assert call(n=8, g=g2, m=v - 1) == FT.OK                             # twice the generator is a generator of half the order
    bad = {
        "singular curve": dict(a=0, b=0),
        "generator off the curve": dict(g=(gen[0], (gen[1] + 1) % p)),
        "offset off the curve": dict(o=((off[0] + 1) % p, off[1])),
        "generator of half the order": dict(g=g2),
        "order claimed too small": dict(m=v - 1, n=8),
        "order claimed too large": dict(m=v + 1),
        "offset in the subgroup": dict(o=gen),
        "offset whose double is in the subgroup": dict(g=g2, m=v - 1, o=gen, n=8),
        "order zero": dict(m=0, n=1),
        "order above the field": dict(m=257),
        "no handle": dict(out=False),
    }
    for what, kw in bad.items():
        assert call(**kw) == FT.ERR_BAD_ARG, what
