"""GPU tests of point arithmetic on short-Weierstrass curves (include/ecfft_hip.h: ecfft_curve_point_mul,
ecfft_curve_point_two_adicity) against the exact Python-int model tests/ec_ref.py.  The affine result of a multiplication is unique,
so every expectation is an equality."""
import functools

import numpy as np
import pytest

import ec_ref as E

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
COUNTS = [1, 63, 64, 65, 257]          # wave tails: the kernels run one point per lane of 64-lane workgroups
POOL = 257


def field_of(field):
    import ecfft_amd
    return ecfft_amd.FIELDS[field]


def curves_of(field):
    return [c for c in E.fixture() if c["field"] == field]


def curve(field, A, B):
    return next(c for c in curves_of(field) if (c["A"], c["B"]) == (A, B))


def pack_points(field, pts):
    """[(x, y) | None] -> (crate-form array, inf bytes); the point at infinity carries an x, y that must not be read"""
    flat = []
    for q in pts:
        flat += [12345, 67890] if q is None else list(q)
    return field_of(field).from_ints(flat), np.array([q is None for q in pts], np.uint8)


def unpack_points(field, out, inf):
    v = field_of(field).to_ints(out)
    res = []
    for i, f in enumerate(inf):
        if f:
            assert (v[2 * i], v[2 * i + 1]) == (0, 0)
            res.append(None)
        else:
            res.append((v[2 * i], v[2 * i + 1]))
    return res


def gpu_mul(field, curves, pts, scalars, nbytes, with_inf=None):
    """[k_i] P_i on the GPU: curves [(A, B)] and scalars [int], each one for all rows or one per row"""
    F = field_of(field)
    P, inf = pack_points(field, pts)
    use_inf = with_inf if with_inf is not None else bool(inf.any())
    out, inf_out = F.curve_point_mul(F.from_ints([c[0] for c in curves]), F.from_ints([c[1] for c in curves]), P, scalars, scalar_bytes=nbytes,
                                     inf=inf if use_inf else None)
    assert inf_out.dtype == np.uint8 and out.shape == P.shape
    return unpack_points(field, out, inf_out)


def model_mul(field, curves, pts, scalars):
    p, n = E.P[field], len(pts)
    cs = curves if len(curves) == n else curves * n
    ks = scalars if len(scalars) == n else scalars * n
    return [E.mul(k, q, c[0], p) for c, q, k in zip(cs, pts, ks)]


@functools.lru_cache(maxsize=None)
def base_points(field, A, B, count):
    """`count` finite points of the curve: the multiples R, 2 R, ... of its first candidate point R whose order exceeds `count`"""
    p = E.P[field]
    for x in range(1, 100):
        R = E.candidate(x, A, B, p)
        if R is None:
            continue
        out, acc = [], R
        while acc is not None and len(out) < count:
            out.append(acc)
            acc = E.add(acc, R, A, p)
        if len(out) == count:
            return out
    raise AssertionError("no point of large order among the first candidates")


@functools.lru_cache(maxsize=None)
def pool(field):
    """POOL rows (curve, point, 40-byte scalar), the curves of the fixture in turn, with the model's products for each scalar width;
    computed once per session and shared by every test that needs random rows"""
    rng = np.random.default_rng(2024 if field == "m31" else 2025)
    cs = curves_of(field)
    rows = []
    for i in range(POOL):
        c = cs[i % len(cs)]
        q = base_points(field, c["A"], c["B"], POOL // len(cs) + 1)[i // len(cs)]
        rows.append(((c["A"], c["B"]), q, int.from_bytes(rng.bytes(40), "little")))
    want = {nb: [E.mul(k % (1 << (8 * nb)), q, c[0], E.P[field]) for c, q, k in rows] for nb in (4, 8, 32, 40)}
    return rows, want


# ---- point_mul ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("nbytes", [4, 8, 32, 40])
@pytest.mark.parametrize("count", COUNTS)
def test_point_mul_random_rows(field, count, nbytes):
    """a curve, a point and a scalar per row"""
    rows, want = pool(field)
    rows = rows[:count]
    got = gpu_mul(field, [r[0] for r in rows], [r[1] for r in rows], [r[2] % (1 << (8 * nbytes)) for r in rows], nbytes)
    assert got == want[nbytes][:count]


@pytest.mark.parametrize("field", FIELDS)
def test_point_mul_shared_curve_and_shared_scalar(field):
    c = curves_of(field)[0]
    p, cv, count = E.P[field], (c["A"], c["B"]), 65
    pts = list(base_points(field, c["A"], c["B"], count))
    rng = np.random.default_rng(7)
    ks = [int.from_bytes(rng.bytes(8), "little") for _ in range(count)]
    assert gpu_mul(field, [cv], pts, ks, 8) == model_mul(field, [cv], pts, ks)                       # one curve, a scalar per row
    assert gpu_mul(field, [cv], pts, ks[:1], 8) == model_mul(field, [cv], pts, ks[:1])               # one curve, one scalar
    assert gpu_mul(field, [cv] * count, pts, ks[:1], 8) == model_mul(field, [cv], pts, ks[:1])       # a curve per row, one scalar
    assert E.mul(ks[0], pts[3], cv[0], p) is not None


@pytest.mark.parametrize("field", FIELDS)
def test_point_mul_special_scalars(field):
    """0, 1, 2, the order and its neighbours, and 40 bytes of 0xFF, on every curve of the fixture"""
    for c in curves_of(field):
        cv, order = (c["A"], c["B"]), c["order"]
        ks = [0, 1, 2, order, order - 1, order + 1, 2**320 - 1]
        pts = list(base_points(field, c["A"], c["B"], 3))
        rows_p = [q for q in pts for _ in ks]
        rows_k = ks * len(pts)
        got = gpu_mul(field, [cv], rows_p, rows_k, 40)
        assert got == model_mul(field, [cv], rows_p, rows_k)
        for i, q in enumerate(pts):
            r = got[i * len(ks):(i + 1) * len(ks)]
            assert r[0] is None and r[1] == q and r[3] is None and r[4] == E.neg(q, E.P[field]) and r[5] == q


def small_order_bases(field, A, B):
    """points of order 2, 4, 8 and 16 from the model's generator of the curve"""
    p, order = E.P[field], curve(field, A, B)["order"]
    v, gen, _, _ = E.find_generator(A, B, order, p)
    assert v >= 4
    return [E.double_n(gen, v - j, A, p) for j in (1, 2, 3, 4)]


@pytest.mark.parametrize("field,A,B", [("m31", 1, 6), ("m31", 1, 3), ("m31", 1, 0), ("secp256k1", 1, 0)])
def test_point_mul_bases_of_order_2_4_8_16(field, A, B):
    """every scalar from 0 to 40 on bases of small 2-power order: the accumulator meets infinity, the base and its negative, and a
    doubling meets y = 0"""
    bases = small_order_bases(field, A, B)
    p = E.P[field]
    assert bases[0][1] == 0 and [E.two_adicity(q, A, p, 8) for q in bases] == [1, 2, 3, 4]
    pts = [q for q in bases for _ in range(41)]
    ks = list(range(41)) * len(bases)
    assert gpu_mul(field, [(A, B)], pts, ks, 1) == model_mul(field, [(A, B)], pts, ks)


@pytest.mark.parametrize("field,A,B,odd", [("m31", 1, 6, 7), ("m31", 1, 6, 13), ("secp256k1", 0, 1, 3)])
def test_point_mul_bases_of_small_odd_order(field, A, B, odd):
    """every scalar from 0 to 40 on a base of order 7, 13 or 3: the accumulator equals the base or its negative inside the addition"""
    p, order = E.P[field], curve(field, A, B)["order"]
    assert order % odd == 0
    base = next(q for q in (E.mul(order // odd, R, A, p) for R in base_points(field, A, B, 40)) if q is not None)
    assert E.mul(odd, base, A, p) is None
    ks = list(range(41))
    want = model_mul(field, [(A, B)], [base] * 41, ks)
    assert want[odd] is None and want[odd + 1] == base and want[odd - 1] == E.neg(base, p)
    assert gpu_mul(field, [(A, B)], [base] * 41, ks, 1) == want
    assert gpu_mul(field, [(A, B)], [base] * 41, ks, 40) == want


@pytest.mark.parametrize("field", FIELDS)
def test_point_mul_bases_at_infinity(field):
    c = curves_of(field)[0]
    cv = (c["A"], c["B"])
    pts = list(base_points(field, c["A"], c["B"], 4))
    rows = [None, pts[0], None, pts[1], pts[2], None, pts[3]] * 10
    ks = [(3 * i + 1) for i in range(len(rows))]
    want = model_mul(field, [cv], rows, ks)
    assert [w is None for w in want[:7]] == [True, False, True, False, False, True, False]
    assert gpu_mul(field, [cv], rows, ks, 2) == want
    assert gpu_mul(field, [cv], pts, ks[:4], 2, with_inf=True) == model_mul(field, [cv], pts, ks[:4])     # flags given, none set


def test_point_mul_on_secp256k1_itself():
    """y^2 = x^3 + 7: the published generator times the published group order is the identity; 2 G and 3 G are the model's"""
    p, G, N = E.P["secp256k1"], E.SECP256K1_G, E.SECP256K1_ORDER
    assert E.on_curve(G, 0, 7, p)
    got = gpu_mul("secp256k1", [(0, 7)], [G] * 5, [N, 2, 3, N - 1, N + 1], 32)
    assert got == [None, E.mul(2, G, 0, p), E.mul(3, G, 0, p), E.neg(G, p), G]


@pytest.mark.parametrize("field", FIELDS)
def test_point_mul_errors(field):
    import ecfft_amd
    from ecfft_amd import fftree as FT
    F, L = field_of(field), ecfft_amd.lib()
    c = curves_of(field)[0]
    cv, p = (c["A"], c["B"]), E.P[field]
    pts = list(base_points(field, c["A"], c["B"], 70))
    with pytest.raises(ValueError):                                   # a point off the curve, in the second wave
        gpu_mul(field, [cv], pts[:66] + [(pts[66][0], (pts[66][1] + 1) % p)] + pts[67:], [5], 1)
    with pytest.raises(ValueError):                                   # a singular curve among good ones: y^2 = x^3 - 3 x + 2 at (1, 0)
        gpu_mul(field, [cv] * 3 + [(p - 3, 2)], pts[:3] + [(1, 0)], [5], 1)
    with pytest.raises(ValueError):                                   # the singular curve y^2 = x^3 with the point (0, 0)
        gpu_mul(field, [(0, 0)], [(0, 0)], [5], 1)
    P, _ = pack_points(field, pts[:3])
    A, B = F.from_ints([cv[0]]), F.from_ints([cv[1]])
    out, io = np.zeros_like(P), np.zeros(3, np.uint8)
    k = np.zeros(3 * 41, np.uint8)
    call = lambda nc=1, nk=1, kb=4: L.ecfft_curve_point_mul(F.id, 0, A.ctypes.data, B.ctypes.data, nc, P.ctypes.data, None, k.ctypes.data, nk, kb,
                                                            out.ctypes.data, io.ctypes.data, 3)
    assert call() == FT.OK
    for bad in (dict(kb=0), dict(kb=41), dict(nc=2), dict(nk=2), dict(nc=0), dict(nk=0)):
        assert call(**bad) == FT.ERR_BAD_ARG, bad


# ---- point_two_adicity -------------------------------------------------------------------------------------------------------------------
def gpu_adic(field, curves, pts, cap=None):
    F = field_of(field)
    P, inf = pack_points(field, pts)
    out = F.curve_point_two_adicity(F.from_ints([c[0] for c in curves]), F.from_ints([c[1] for c in curves]), P, cap=cap, inf=inf if inf.any() else None)
    assert out.dtype == np.int32
    return [int(v) for v in out]


@pytest.mark.parametrize("field,A,B", [("m31", 1, 6), ("m31", 1, 3), ("m31", 1, 0), ("secp256k1", 1, 0)])
def test_two_adicity_of_generators_and_their_doublings(field, A, B):
    p, order = E.P[field], curve(field, A, B)["order"]
    v, gen, _, _ = E.find_generator(A, B, order, p)
    pts = [E.double_n(gen, j, A, p) for j in range(v + 1)]
    assert pts[-1] is None and pts[-2][1] == 0
    assert gpu_adic(field, [(A, B)], pts) == [v - j for j in range(v + 1)]
    assert gpu_adic(field, [(A, B)], pts, cap=v) == [v - j for j in range(v + 1)]
    assert gpu_adic(field, [(A, B)], pts, cap=v - 1) == [-1] + [v - j for j in range(1, v + 1)]      # the cap cuts the search
    assert gpu_adic(field, [(A, B)], pts, cap=0) == [-1] * v + [0]


@pytest.mark.parametrize("field", FIELDS)
def test_two_adicity_of_mixed_rows(field):
    """a curve per row over wave tails: points with an odd part in their order give -1 at the cap, infinity gives 0"""
    rows, _ = pool(field)
    p, cap = E.P[field], E.MAX_TWO_ADICITY[field]
    for count in (63, 65):
        pts = [None if i % 9 == 4 else r[1] for i, r in enumerate(rows[:count])]
        want = [E.two_adicity(q, r[0][0], p, cap) for q, r in zip(pts, rows)]
        assert 0 in want and -1 in want
        assert gpu_adic(field, [r[0] for r in rows[:count]], pts) == want
    c = curves_of(field)[0]
    odd = c["order"] >> E.v2(c["order"])
    if odd > 1:
        q = next(q for q in (E.mul(1 << E.v2(c["order"]), R, c["A"], p) for R in base_points(field, c["A"], c["B"], 8)) if q)
        assert gpu_adic(field, [(c["A"], c["B"])], [q]) == [-1]


@pytest.mark.parametrize("field", FIELDS)
def test_two_adicity_errors(field):
    c = curves_of(field)[0]
    cv, p = (c["A"], c["B"]), E.P[field]
    pts = list(base_points(field, c["A"], c["B"], 3))
    with pytest.raises(ValueError):
        gpu_adic(field, [cv], [pts[0], (pts[1][0], (pts[1][1] + 1) % p), pts[2]])
    with pytest.raises(ValueError):
        gpu_adic(field, [(0, 0)], [(0, 0)])
    with pytest.raises(ValueError):
        gpu_adic(field, [cv], pts, cap=E.MAX_TWO_ADICITY[field] + 1)
    with pytest.raises(ValueError):
        gpu_adic(field, [cv, cv], pts)
