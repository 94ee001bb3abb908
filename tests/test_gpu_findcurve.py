"""GPU tests of the curve search (include/ecfft_hip.h: ecfft_curve_two_sylow, ecfft_find_curve, ecfft_build_fftree_on_curve) against the
Python model tests/curve_ref.py, which restates the reference's find_curve.rs.  Every expectation is an equality: the square-root
convention of the header makes n, the generator and the offset bit-exact."""
import functools

import numpy as np
import pytest

import curve_ref as R
import poly_ref

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]


def field_of(field):
    import ecfft_amd
    return ecfft_amd.FIELDS[field]


def crate_form(field, ints):
    return field_of(field).from_standard(poly_ref.from_ints(field, ints))


def ints_of(field, arr):
    return poly_ref.to_ints(field, field_of(field).to_standard(arr))


@functools.lru_cache(maxsize=None)
def model_rows(field, seed=1, count=4096):
    """(a, bb, n, x) of candidates 0 .. count-1, computed once per session"""
    out = []
    for i in range(count):
        a, bb = R.candidate(field, seed, i)
        out.append((a, bb) + R.two_sylow_field(field, a, bb))
    return out


def sylow(field, curves):
    """[(n, x)] from the GPU for [(a, bb)]"""
    n, x = field_of(field).curve_two_sylow(crate_form(field, [c[0] for c in curves]), crate_form(field, [c[1] for c in curves]))
    assert n.dtype == np.uint32
    return list(zip([int(v) for v in n], ints_of(field, x)))


def order_is_exactly(field, a, bb, x, n):
    p = R.P[field]
    y = R.sqrt_canon(R.rhs(x, a, bb, p), p)
    return y is not None and R.pt_double_n((x, y), n - 1, a, bb, p) == (0, 0)


# ---- curve_two_sylow ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_two_sylow_of_the_first_4096_candidates(field):
    rows = model_rows(field)
    assert sylow(field, [r[:2] for r in rows]) == [r[2:] for r in rows]


def test_two_sylow_of_the_crates_curve():
    a, bb = R.CRATE["a"], R.CRATE["bb"]
    (n, x), = sylow("secp256k1", [(a, bb)])
    assert n == 36 and order_is_exactly("secp256k1", a, bb, x, 36)
    assert (n, x) == R.two_sylow_field("secp256k1", a, bb)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("count", [63, 64, 65])
def test_two_sylow_queue_tails(field, count):
    rows = model_rows(field)[100:100 + count]
    assert sylow(field, [r[:2] for r in rows]) == [r[2:] for r in rows]


@pytest.mark.parametrize("field", FIELDS)
def test_two_sylow_singular_curves_and_a_zero(field):
    p = R.P[field]
    curves = [(5, 0), (0, 0), (2, 1), (p - 2, 1), (6, 9), (0, 1), (0, 4), (0, 9), (0, p - 1), (0, 3), (1, 1), (p - 1, p - 1)]
    curves += [r[:2] for r in model_rows(field)[:53]]          # so that live curves share the waves of the dead ones
    want = [R.two_sylow_field(field, a, bb) for a, bb in curves]
    assert want[:5] == [(0, 0)] * 5                              # bb = 0 and zero discriminants
    assert sylow(field, curves) == want


# ---- find_curve --------------------------------------------------------------------------------------------------------------------------
def found(field, r):
    """the dict of Field.find_curve as standard-form integers"""
    if r is None:
        return None
    one = lambda k: ints_of(field, r[k])[0]
    return {"index": r["index"], "n": r["n"], "a": one("a"), "bb": one("bb"), "gen": tuple(ints_of(field, r["gen"])), "offset": tuple(ints_of(field, r["offset"]))}


def model_found(field, k, seed, start=0, max_candidates=1 << 20):
    m = R.find_curve(field, k, seed, start, max_candidates)
    if m is None:
        return None
    i, n, a, bb, x = m
    p = R.P[field]
    return {"index": i, "n": n, "a": a, "bb": bb, "gen": (x, R.sqrt_canon(R.rhs(x, a, bb, p), p)), "offset": R.coset_offset(a, bb, n, p)}


@pytest.mark.parametrize("key", sorted(R.FIRST_HITS))
def test_find_curve_first_hits(key):
    field, seed, k = key
    got = found(field, field_of(field).find_curve(k, seed))
    assert got == model_found(field, k, seed)
    assert (got["index"], got["n"]) == R.FIRST_HITS[key]


@pytest.mark.parametrize("field,seed,k", [("m31", 1, 12), ("secp256k1", 1, 10)])
def test_find_curve_windows(field, seed, k):
    F = field_of(field)
    want = model_found(field, k, seed)
    hit = want["index"]
    assert found(field, F.find_curve(k, seed, start=hit, max_candidates=1)) == want
    assert F.find_curve(k, seed, start=0, max_candidates=hit) is None
    assert found(field, F.find_curve(k, seed, start=0, max_candidates=hit + 1)) == want
    nxt = model_found(field, k, seed, start=hit + 1)
    assert nxt["index"] > hit
    assert found(field, F.find_curve(k, seed, start=hit + 1)) == nxt
    assert found(field, F.find_curve(k, seed, max_candidates=100000)) == want       # another cut into batches: the same answer
    assert found(field, F.find_curve(0, seed, max_candidates=1 << 12)) == model_found(field, 2, seed)    # k below 2 is 2


@pytest.mark.parametrize("field,k,log_max", [("m31", 20, 26), ("secp256k1", 16, 22)])
def test_find_curve_deeper(field, k, log_max):
    """the window holds 16 hits on average; only the returned curve is checked against the model"""
    got = found(field, field_of(field).find_curve(k, 1, max_candidates=1 << log_max))
    assert got is not None
    assert (got["a"], got["bb"]) == R.candidate(field, 1, got["index"])
    n, x = R.two_sylow_field(field, got["a"], got["bb"])
    assert got["n"] == n >= k and got["gen"][0] == x
    assert order_is_exactly(field, got["a"], got["bb"], x, n)
    assert got["offset"] == R.coset_offset(got["a"], got["bb"], n, R.P[field])
    if got["offset"] == (0, 0):
        # the whole group is the cyclic one of 2^n points: no coset offset exists, and the header's recipe builds the tree
        p, F = R.P[field], field_of(field)
        assert n == p.bit_length()
        t = F.build_fftree_on_curve(256, crate_form(field, [got["a"]]), crate_form(field, [got["bb"]]),
                                    crate_form(field, list(R.pt_double(got["gen"], got["a"], got["bb"], p))), n - 1, crate_form(field, list(got["gen"])))
        assert len(set(ints_of(field, t.leaves()))) == 256


# ---- build_fftree_on_curve -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1 << 8, 1 << 12])
def test_build_on_the_crates_curve_is_build_fftree(n):
    from ecfft_amd import fftree as FT
    F, cr = field_of("secp256k1"), R.CRATE
    t = F.build_fftree_on_curve(n, crate_form("secp256k1", [cr["a"]]), crate_form("secp256k1", [cr["bb"]]), crate_form("secp256k1", list(cr["gen"])),
                                cr["log_order"], crate_form("secp256k1", list(cr["offset"])))
    ref = F.build_fftree(n)
    assert t.n == ref.n == n
    assert t.table(FT.TBL_F).tobytes() == ref.table(FT.TBL_F).tobytes()
    for k in range(n.bit_length() - 1):
        for got, want in zip(t.rational_map(k), ref.rational_map(k)):
            assert got.tobytes() == want.tobytes()


@functools.lru_cache(maxsize=None)
def found_tree(field, n=1 << 8):
    F = field_of(field)
    r = F.find_curve(12, 1)
    return r, F.build_fftree_on_curve(n, r["a"], r["bb"], r["gen"], r["n"], r["offset"])


@pytest.mark.parametrize("field", FIELDS)
def test_tree_on_a_found_curve(field):
    F, p, n = field_of(field), R.P[field], 1 << 8
    r, t = found_tree(field)
    assert (r["index"], r["n"]) == R.FIRST_HITS[(field, 1, 12)] and t.n == n
    leaves = ints_of(field, t.leaves())
    assert len(set(leaves)) == n
    rng = np.random.default_rng(12)
    coeffs = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(n)]
    evals = t.enter(crate_form(field, coeffs))

    def horner(x):
        acc = 0
        for c in reversed(coeffs):
            acc = (acc * x + c) % p
        return acc
    assert ints_of(field, evals) == [horner(x) for x in leaves]
    assert ints_of(field, t.exit(evals)) == coeffs
    a, b = poly_ref.rand_std(field, 100, 1), poly_ref.rand_std(field, 157, 2)
    c = t.poly_mul(F.from_standard(a), F.from_standard(b))
    assert poly_ref.check_mul(field, a, b, F.to_standard(c)) == ""
    assert F.build_fftree_on_curve(1 << r["n"], r["a"], r["bb"], r["gen"], r["n"], r["offset"]) is None       # ECFFT_ERR_TREE_TOO_LARGE
