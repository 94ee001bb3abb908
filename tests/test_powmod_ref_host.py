"""CPU tests of tests/powmod_ref.py, the exact reference of tests/test_gpu_polypowmod.py: the Barrett pow_mod / mul_mod against
repeated multiplication with long division, the Frobenius identity a^p = a mod a modulus that splits into distinct linear factors,
the list model of the GPU's fused three-product step against long division at a small prime, and the exponent byte parsing."""
import numpy as np
import pytest

import poly_ref as R
import powmod_ref as W

FIELDS = ["secp256k1", "m31"]


def modulus(field, nm, seed, lead=None):
    f = R.rand_std(field, nm, seed)
    R.set_nonzero(field, f, nm - 1)
    if lead is not None:
        f[nm - 1] = R.from_ints(field, [lead])[0]
    return f


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d,na", [(1, 1), (1, 5), (2, 1), (2, 2), (3, 7), (7, 3), (17, 17), (17, 18), (40, 100), (65, 64), (65, 200)])
def test_matches_repeated_multiplication(field, d, na):
    f = modulus(field, d + 1, 10 * d + na)
    a = R.rand_std(field, na, 3 * d + na)
    for e in (0, 1, 2, 3, 4, 5, 11, 16):
        got, want = W.pow_mod(field, a, e, f), W.pow_repeated(field, a, e, f)
        assert got.shape == want.shape == R.shape(field, d)
        assert np.array_equal(got, want), e


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("na,nb,nm", [(1, 1, 2), (5, 9, 3), (30, 30, 31), (30, 31, 31), (64, 64, 65), (100, 3, 40), (3, 3, 20), (90, 120, 70)])
def test_mul_mod_matches_long_division(field, na, nb, nm):
    p = R.P[field]
    f = modulus(field, nm, na + nb, lead=p - 1 if nm & 1 else None)
    a, b = R.rand_std(field, na, na), R.rand_std(field, nb, nb + 1)
    want = W.long_division_rem(R.to_ints(field, R.mul_exact(field, a, b)), R.to_ints(field, f), p)
    assert R.to_ints(field, W.mul_mod(field, a, b, f)) == want


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("d,na", [(5, 5), (65, 30), (65, 140), (300, 300)])
def test_frobenius_on_a_split_modulus(field, d, na):
    """f = prod (x - r_i), the r_i distinct: a^p = a mod every x - r_i, hence mod f"""
    roots = R.rand_std(field, d, 7 * d, specials=False)
    assert len(set(R.to_ints(field, roots))) == d
    f = W.from_roots(field, roots)
    assert f.shape[0] == d + 1 and R.to_ints(field, f[-1:]) == [1]
    assert all(v == 0 for v in R.horner(field, f, roots[:3]))
    a = R.rand_std(field, na, d + na)
    assert np.array_equal(W.pow_mod(field, a, R.P[field], f), W.Barrett(field, f).reduce(a))


@pytest.mark.parametrize("p", [7, 97, 65537])
@pytest.mark.parametrize("d", [2, 3, 4, 5, 8, 9, 33])
def test_fused_step_model_matches_long_division(p, d):
    rng = np.random.default_rng(p + d)
    for lead in (1, p - 1, int(rng.integers(1, p))):
        f = [int(v) for v in rng.integers(0, p, d)] + [lead]
        for zero_const in (False, True):
            if zero_const:
                f[0] = 0
            x, y = [int(v) for v in rng.integers(0, p, d)], [int(v) for v in rng.integers(0, p, d)]
            prod = [int(v) % p for v in np.convolve(np.array(x, dtype=object), np.array(y, dtype=object))]
            assert W.fused_step_model(x, y, f, p) == W.long_division_rem(prod, f, p)
            assert W.fused_step_model(x, x, f, p) == W.long_division_rem(W._conv(x, x, p), f, p)


def test_exponent_bytes():
    assert W.exp_bits(b"") == (0, 0)
    assert W.exp_bits(b"\x00") == (0, 0) and W.exp_bits(bytes(40)) == (0, 0)
    assert W.exp_bits(b"\x01") == (1, 1) and W.exp_bits(b"\x01\x00\x00") == (1, 1)
    assert W.exp_bits(b"\x80") == (8, 1) and W.exp_bits(b"\x00\x01") == (9, 2) and W.exp_bits(b"\xff\x7f\x00") == (15, 2)
    for e in (0, 1, 2, 3, 255, 256, 2**31 - 1, 2**64, R.P["secp256k1"], 2**300 + 12345):
        b = e.to_bytes((e.bit_length() + 7) // 8, "little")
        for pad in (0, 1, 9):
            assert W.exp_bits(b + bytes(pad)) == (e.bit_length(), len(b))
            assert W.exp_from_bytes(b + bytes(pad)) == e
    assert W.scan(b"") == "" and W.scan(b"\x01") == "" and W.scan(b"\x02") == "S" and W.scan(b"\x03") == "SM"
    assert W.scan(b"\x0b\x00") == "SSMSM"                        # 1011
    e = R.P["secp256k1"]
    ops = W.scan(e.to_bytes(32, "little"))
    assert ops.count("S") == 255 and ops.count("M") == bin(e).count("1") - 1


@pytest.mark.parametrize("field", ["secp256k1", "m31"])
def test_pool_checks_accept_and_reject(field):
    """check_pow_mod / check_mul_mod (the pool jobs of the regime tests): "" for the right result, a message for one changed coefficient"""
    a, b = R.rand_std(field, 70, 1), R.rand_std(field, 33, 2)
    f = R.set_nonzero(field, R.rand_std(field, 31, 3), 30)
    exps = [0, 1, 2, 3, 0b101101]
    outs = [W.pow_repeated(field, a, e, f) for e in exps]
    assert W.check_pow_mod(field, a, f, exps, outs) == ""
    wrong = [o.copy() for o in outs]
    wrong[4][29] = wrong[4][28]
    assert "45" in W.check_pow_mod(field, a, f, exps, wrong)
    m = W.mul_mod(field, a, b, f)
    p = R.P[field]
    assert R.to_ints(field, m) == W.long_division_rem(R.to_ints(field, R.mul_exact(field, a, b)), R.to_ints(field, f), p)
    assert W.check_mul_mod(field, a, b, f, m) == ""
    m[0] = m[1]
    assert W.check_mul_mod(field, a, b, f, m) != ""
