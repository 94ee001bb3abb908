"""TEST INFRASTRUCTURE — the exact CPU model of the Reed-Solomon codec (rs_encode / rs_decode_erasures), for
tests/test_gpu_rscodec.py and tests/test_rs_codec_ref_host.py.  Built on tests/rs_ref.py and generic in the prime p: polynomials
are lists of Python ints, low to high.

- encode_systematic: interpolation at the first k points, then evaluation at all m.
- gao_decode_erasures: rs_ref.gao_decode on the kept points and values (the punctured code), -1 when fewer than k are kept; the
  k coefficients of f or its m symbols at all points.
- full_interpolant / identity_rows: the two sides of the identity behind the workgroup kernel: the partial row of
  (g0', interpolant over ALL points with the erased symbols read as 0) against that of (g0', interpolant over the kept points).
"""
import rs_ref as S


def encode_systematic(p, xs, data):
    """the m symbols f(x_0), ..., f(x_{m-1}) of the f of degree < k = len(data) with f(x_i) = data[i], i < k"""
    k = len(data)
    assert 1 <= k <= len(xs)
    f = S.interpolate(p, list(xs[:k]), data)
    return S.evaluate(p, f, xs)


def kept_positions(erased):
    return [i for i, e in enumerate(erased) if not e]


def gao_decode_erasures(p, xs, ys, erased, k, codeword=False):
    """(out, n_errors): Gao's decoder on the kept positions.  out = the k coefficients of f (zero-padded), or with codeword its m
    symbols at all of xs; a zero row and -1 where fewer than k symbols are kept or no codeword lies in the radius"""
    m = len(xs)
    assert len(ys) == m and len(erased) == m and 1 <= k <= m
    keep = kept_positions(erased)
    no = m if codeword else k
    if len(keep) < k:
        return [0] * no, -1
    msg, ne = S.gao_decode(p, [xs[i] for i in keep], [ys[i] for i in keep], k)
    if ne < 0:
        return [0] * no, -1
    return (S.evaluate(p, msg, xs) if codeword else msg), ne


def full_interpolant(p, xs, ys, erased):
    """the interpolant over ALL m points of the row with its erased symbols read as 0"""
    return S.interpolate(p, list(xs), [0 if e else y for y, e in zip(ys, erased)])


def identity_rows(p, xs, ys, erased, k):
    """((r, t) from the full interpolant, (r, t) of the punctured code): the partial rows, t monic, of (g0', g1) with
    stop' = ceil((m' + k) / 2), for g1 = the full interpolant and for g1 = the interpolant over the kept points"""
    keep = kept_positions(erased)
    mk = len(keep)
    assert mk >= k
    kx, ky = [xs[i] for i in keep], [ys[i] for i in keep]
    g0k = S.from_roots(p, kx)
    stop = (mk + k + 1) // 2
    full = S.partial_row(p, g0k, full_interpolant(p, xs, ys, erased), stop)
    punct = S.partial_row(p, g0k, S.interpolate(p, kx, ky), stop)
    return (full[0], full[2]), (punct[0], punct[2])
