"""CPU tests of the model tests/ec_ref.py itself, so that the GPU tests compare against something checked: the crate's M31 constants,
the Velu chain against the rational maps the product's host construction returns, and the curves of tests/golden/ec_curves.json."""
import pytest

import ec_ref as E


@pytest.fixture(scope="module")
def prod():
    import ecfft_amd
    ecfft_amd.build.build()
    return ecfft_amd


def test_the_crates_m31_constants():
    p, cr = E.P["m31"], E.CRATE_M31
    assert E.on_curve(cr["gen"], cr["A"], cr["B"], p) and E.on_curve(cr["offset"], cr["A"], cr["B"], p)
    assert E.two_adicity(cr["gen"], cr["A"], p, 34) == 28
    assert E.two_adicity(cr["offset"], cr["A"], p, 34) == 31
    assert E.two_adicity(cr["offset"], cr["A"], p, 30) == -1          # the cap cuts the search


def test_the_chain_of_the_crates_m31_curve_is_the_products(prod):
    p, cr, n = E.P["m31"], E.CRATE_M31, 4096
    f, num, den = prod.m31.build_points(n)
    g = E.double_n(cr["gen"], cr["log_order"] - 12, cr["A"], p)
    maps = E.velu_chain(cr["A"], cr["B"], g, 12, p)
    assert len(maps) == 12
    for k, (mn, md) in enumerate(maps):
        assert tuple(int(v) for v in num[3 * k:3 * k + 3]) == mn and tuple(int(v) for v in den[3 * k:3 * k + 3]) == md
    lv = E.leaves(cr["A"], cr["B"], cr["gen"], cr["log_order"], cr["offset"], n, p)
    assert [int(v) for v in f[n:]] == lv
    assert [int(v) for v in f[n // 2:n]] == E.layers(lv, maps, p)[1]


def test_the_group_law_against_brute_force_on_a_small_prime():
    """p = 103: [k] P by double-and-add equals k - 1 additions, and the order of every point divides the number of points"""
    p, A, B = 103, 1, 6
    pts = [(x, y) for x in range(p) for y in range(p) if (y * y - E.rhs(x, A, B, p)) % p == 0]
    order = len(pts) + 1
    for q in pts[::7]:
        acc = None
        for k in range(1, 30):
            acc = E.add(acc, q, A, p)
            assert E.mul(k, q, A, p) == acc
        assert E.mul(order, q, A, p) is None
        assert E.two_adicity(q, A, p, 10) <= E.v2(order)


FOUND = {("m31", 1, 6): (6, 2), ("m31", 1, 3): (5, 2), ("m31", 1, 0): (31, None), ("secp256k1", 1, 0): (4, 3)}


@pytest.mark.parametrize("c", E.fixture(), ids=lambda c: f"{c['field']}-{c['A'] % 1000}-{c['B']}")
def test_the_curves_of_the_fixture(c):
    field, A, B, order = c["field"], c["A"], c["B"], c["order"]
    p = E.P[field]
    assert not E.is_singular(A, B, p) and (order - p - 1) ** 2 <= 4 * p
    pts = [q for q in (E.candidate(x, A, B, p) for x in range(1, 30)) if q]
    assert all(E.on_curve(q, A, B, p) and E.mul(order, q, A, p) is None for q in pts[:5])
    fg = E.find_generator(A, B, order, p, max_candidates=200)
    if (field, A, B) not in FOUND:
        assert fg is None                          # full 2-torsion, or a 2-Sylow subgroup Z2 x Z2: no point of order 2^v
        return
    v, gen, off, x = fg
    want_v, want_x = FOUND[(field, A, B)]
    assert v == want_v == E.v2(order) and (want_x is None or x == want_x)
    assert E.two_adicity(gen, A, p, v) == v
    if order == 1 << v:
        assert off == (0, 0)
        off, gen, v = gen, E.double_n(gen, 2, A, p), v - 2
    assert E.double_n(off, v + 1, A, p) is not None
    depth = min(v, 8)
    maps = E.velu_chain(A, B, E.double_n(gen, v - depth, A, p), depth, p)
    assert maps is not None and len(maps) == depth           # the chain exists to full depth
    log_n = min(depth, 4)
    n = 1 << log_n
    lv = E.leaves(A, B, gen, v, off, n, p)
    assert len(set(lv)) == n                                  # the leaves are distinct, and no layer meets the pole of its map
    layers = E.layers(lv, E.velu_chain(A, B, E.double_n(gen, v - log_n, A, p), log_n, p), p)
    assert [len(layer) for layer in layers] == [n >> k for k in range(log_n + 1)]
    with pytest.raises(ValueError):
        E.find_generator(A, B, order + 2, p)
