"""GPU tests of the return codes of the context-bound entry points that have no error test of their own: one valid small call in host
memory and the same call on CUDA tensors in device memory (both ECFFT_OK, equal results), then every single bad argument that applies,
each with its exact code.  Bad arguments are only ever paired with host buffers and ECFFT_MEM_HOST (or an unknown memory kind), and
every length that does not fit the buffers is one that an argument check rejects before anything runs."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ["secp256k1", "m31"]
N = 64                                   # leaves of the test tree


def rand_elems(field, n, seed):
    rng = np.random.default_rng(seed)
    if field == "m31":
        return rng.integers(1, 2**31 - 1, n, dtype=np.uint32)
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(1)
    return a


def _deg_ptr(a):
    return ctypes.byref(a["deg"]) if a["deg"] is not None else None


# name: (input buffers {key: elements}, output buffers {key: elements}, call(L, h, ptrs, mem, stream, args), default args,
#        bad cases [(label, overrides of ptrs / args, expected code)]); an in-place buffer (the shard calls) is an input
CASES = {
    "enter": ({"x": 16}, {"y": 16},
              lambda L, h, p, mem, s, a: L.ecfft_enter(h, p["x"], p["y"], a["n"], mem, s), {"n": 16},
              [("null in", {"x": None}, "ERR_BAD_ARG"), ("null out", {"y": None}, "ERR_BAD_ARG"),
               ("not pow2", {"n": 12}, "ERR_NOT_POW2"), ("zero", {"n": 0}, "ERR_NOT_POW2"),
               ("too small", {"n": 2 * N}, "ERR_TREE_TOO_SMALL"), ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
    "exit": ({"x": 16}, {"y": 16},
             lambda L, h, p, mem, s, a: L.ecfft_exit(h, p["x"], p["y"], a["n"], mem, s), {"n": 16},
             [("null in", {"x": None}, "ERR_BAD_ARG"), ("null out", {"y": None}, "ERR_BAD_ARG"),
              ("not pow2", {"n": 12}, "ERR_NOT_POW2"), ("too small", {"n": 2 * N}, "ERR_TREE_TOO_SMALL"),
              ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
    "enter_many": ({"x": 16}, {"y": 16},
                   lambda L, h, p, mem, s, a: L.ecfft_enter_many(h, p["x"], p["y"], a["n"], a["count"], mem, s), {"n": 8, "count": 2},
                   [("null in", {"x": None}, "ERR_BAD_ARG"), ("null out", {"y": None}, "ERR_BAD_ARG"),
                    ("not pow2", {"n": 6}, "ERR_NOT_POW2"), ("count", {"count": 0}, "ERR_BAD_ARG"),
                    ("too small", {"n": 2 * N, "count": 1}, "ERR_TREE_TOO_SMALL"), ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
    "exit_many": ({"x": 16}, {"y": 16},
                  lambda L, h, p, mem, s, a: L.ecfft_exit_many(h, p["x"], p["y"], a["n"], a["count"], mem, s), {"n": 8, "count": 2},
                  [("null in", {"x": None}, "ERR_BAD_ARG"), ("null out", {"y": None}, "ERR_BAD_ARG"),
                   ("not pow2", {"n": 6}, "ERR_NOT_POW2"), ("count", {"count": 0}, "ERR_BAD_ARG"),
                   ("too small", {"n": 2 * N, "count": 1}, "ERR_TREE_TOO_SMALL"), ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
    "extend": ({"x": 32}, {"y": 32},
               lambda L, h, p, mem, s, a: L.ecfft_extend(h, p["x"], p["y"], a["e"], a["moiety"], a["count"], mem, s),
               {"e": 16, "moiety": 1, "count": 2},
               [("null in", {"x": None}, "ERR_BAD_ARG"), ("null out", {"y": None}, "ERR_BAD_ARG"),
                ("not pow2", {"e": 12}, "ERR_NOT_POW2"), ("count", {"count": 0}, "ERR_BAD_ARG"),
                ("too small", {"e": N, "count": 1}, "ERR_TREE_TOO_SMALL"), ("moiety", {"moiety": 2}, "ERR_BAD_ARG"),
                ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
    "mextend": ({"x": 32}, {"y": 32},
                lambda L, h, p, mem, s, a: L.ecfft_mextend(h, p["x"], p["y"], a["e"], a["moiety"], a["count"], mem, s),
                {"e": 16, "moiety": 0, "count": 2},
                [("null in", {"x": None}, "ERR_BAD_ARG"), ("null out", {"y": None}, "ERR_BAD_ARG"),
                 ("not pow2", {"e": 12}, "ERR_NOT_POW2"), ("count", {"count": 0}, "ERR_BAD_ARG"),
                 ("too small", {"e": N, "count": 1}, "ERR_TREE_TOO_SMALL"), ("moiety", {"moiety": 2}, "ERR_BAD_ARG"),
                 ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
    "redc": ({"x": 16, "a": 16}, {"y": 16},
             lambda L, h, p, mem, s, a: L.ecfft_redc(h, p["x"], p["a"], p["y"], a["n"], a["moiety"], mem, s), {"n": 16, "moiety": 0},
             [("null evals", {"x": None}, "ERR_BAD_ARG"), ("null a", {"a": None}, "ERR_BAD_ARG"), ("null out", {"y": None}, "ERR_BAD_ARG"),
              ("not pow2", {"n": 12}, "ERR_NOT_POW2"), ("too small", {"n": 2 * N}, "ERR_TREE_TOO_SMALL"),
              ("moiety", {"moiety": 2}, "ERR_BAD_ARG"), ("mem", {"mem": 7}, "ERR_BAD_ARG"), ("size-1 tree", {"n": 1}, "ERR_BAD_ARG")]),
    "modular_reduce": ({"x": 16, "a": 16, "c": 16}, {"y": 16},
                       lambda L, h, p, mem, s, a: L.ecfft_modular_reduce(h, p["x"], p["a"], p["c"], p["y"], a["n"], mem, s), {"n": 16},
                       [("null evals", {"x": None}, "ERR_BAD_ARG"), ("null a", {"a": None}, "ERR_BAD_ARG"),
                        ("null c", {"c": None}, "ERR_BAD_ARG"), ("null out", {"y": None}, "ERR_BAD_ARG"),
                        ("not pow2", {"n": 12}, "ERR_NOT_POW2"), ("too small", {"n": 2 * N}, "ERR_TREE_TOO_SMALL"),
                        ("mem", {"mem": 7}, "ERR_BAD_ARG"), ("size-1 tree", {"n": 1}, "ERR_BAD_ARG")]),
    "vanish": ({"x": 16}, {"y": 32},
               lambda L, h, p, mem, s, a: L.ecfft_vanish(h, p["x"], p["y"], a["n"], mem, s), {"n": 16},
               [("null in", {"x": None}, "ERR_BAD_ARG"), ("null out", {"y": None}, "ERR_BAD_ARG"),
                ("not pow2", {"n": 12}, "ERR_NOT_POW2"), ("too small", {"n": N}, "ERR_TREE_TOO_SMALL"),
                ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
    "degree": ({"x": 16}, {},
               lambda L, h, p, mem, s, a: L.ecfft_degree(h, p["x"], a["n"], mem, s, _deg_ptr(a)), {"n": 16},
               [("null in", {"x": None}, "ERR_BAD_ARG"), ("null degree", {"deg": None}, "ERR_BAD_ARG"),
                ("not pow2", {"n": 12}, "ERR_NOT_POW2"), ("too small", {"n": 2 * N}, "ERR_TREE_TOO_SMALL"),
                ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
    "table_fma": ({"x": 8, "a": 8}, {"y": 8},
                  lambda L, h, p, mem, s, a: L.ecfft_table_fma(h, p["y"], p["x"], p["a"], a["cnt"], a["m"], a["which"], a["off"], a["stride"],
                                                               a["mode"], mem, s),
                  {"cnt": 8, "m": 16, "which": 3, "off": 1, "stride": 2, "mode": 1},
                  [("null out", {"y": None}, "ERR_BAD_ARG"), ("null x", {"x": None}, "ERR_BAD_ARG"),
                   ("not pow2", {"m": 12}, "ERR_NOT_POW2"), ("too small", {"m": 2 * N}, "ERR_TREE_TOO_SMALL"),
                   ("cnt 0 before mem", {"cnt": 0, "mem": 7}, "OK"), ("mem", {"mem": 7}, "ERR_BAD_ARG"),
                   ("table", {"which": 0}, "ERR_BAD_ARG"), ("range", {"off": 2}, "ERR_BAD_ARG"),
                   ("mode", {"mode": 4}, "ERR_BAD_ARG"), ("null y", {"a": None}, "ERR_BAD_ARG")]),
    "extend_top_cyclic": ({"b": 8}, {},
                          lambda L, h, p, mem, s, a: L.ecfft_extend_top_cyclic(h, p["b"], a["e"], a["moiety"], a["log_p"], a["rank"], a["rec"], mem, s),
                          {"e": 16, "moiety": 1, "log_p": 1, "rank": 1, "rec": 0},
                          [("null", {"b": None}, "ERR_BAD_ARG"), ("not pow2", {"e": 12}, "ERR_NOT_POW2"),
                           ("too small", {"e": N}, "ERR_TREE_TOO_SMALL"), ("moiety", {"moiety": 2}, "ERR_BAD_ARG"),
                           ("ranks", {"log_p": 4}, "ERR_BAD_ARG"), ("rank", {"rank": 2}, "ERR_BAD_ARG"),
                           ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
    "extend_local_block": ({"b": 8}, {},
                           lambda L, h, p, mem, s, a: L.ecfft_extend_local_block(h, p["b"], a["e"], a["moiety"], a["log_p"], mem, s),
                           {"e": 16, "moiety": 0, "log_p": 1},
                           [("null", {"b": None}, "ERR_BAD_ARG"), ("not pow2", {"e": 12}, "ERR_NOT_POW2"),
                            ("too small", {"e": N}, "ERR_TREE_TOO_SMALL"), ("moiety", {"moiety": 2}, "ERR_BAD_ARG"),
                            ("ranks", {"log_p": 4}, "ERR_BAD_ARG"), ("mem", {"mem": 7}, "ERR_BAD_ARG")]),
}

_trees = {}


def tree(field):
    import ecfft_amd
    if field not in _trees:
        _trees[field] = (ecfft_amd.FIELDS[field].build_fftree(N), ecfft_amd.FIELDS[field].build_extend_shard(1024, 1, 0))
    return _trees[field]


def _buffers(field, name, seed):
    ins, outs = CASES[name][:2]
    bufs = {k: rand_elems(field, n, seed + i) for i, (k, n) in enumerate(ins.items())}
    bufs.update({k: np.zeros_like(rand_elems(field, n, 0)) for k, n in outs.items()})
    return bufs


def _call(t, name, ptrs, mem, stream, over=None):
    call, defaults = CASES[name][2], CASES[name][3]
    over = over or {}
    p = {k: over.get(k, v) for k, v in ptrs.items()}
    a = {k: over.get(k, v) for k, v in defaults.items()}
    a["deg"] = over.get("deg", ctypes.c_size_t(12345))
    rc = call(t._L, t._h, p, over.get("mem", mem), stream, a)
    return rc, a["deg"]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_and_device_calls_agree(field, name):
    import torch
    from ecfft_amd import fftree as FT
    t, _ = tree(field)
    host = _buffers(field, name, 7)
    dev_in = {k: v.copy() for k, v in host.items()}
    rc, deg_h = _call(t, name, {k: v.ctypes.data for k, v in host.items()}, FT.MEM_HOST, None)
    assert rc == FT.OK
    v = np.int64 if field != "m31" else np.int32           # torch has no unsigned 64-bit tensors: same bytes, signed view
    tens = {k: torch.from_numpy(x.view(v)).cuda() for k, x in dev_in.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rc, deg_d = _call(t, name, {k: x.data_ptr() for k, x in tens.items()}, FT.MEM_DEVICE, s.cuda_stream)
    s.synchronize()
    assert rc == FT.OK
    for k, x in tens.items():
        assert np.array_equal(x.cpu().numpy().view(host[k].dtype), host[k]), k
    assert deg_d.value == deg_h.value
    if name == "degree":
        assert deg_h.value < 16


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_bad_arguments(field, name):
    from ecfft_amd import fftree as FT
    t, shard = tree(field)
    bufs = _buffers(field, name, 11)
    ptrs = {k: v.ctypes.data for k, v in bufs.items()}
    for label, over, want in CASES[name][4]:
        rc, _ = _call(t, name, ptrs, FT.MEM_HOST, None, over)
        assert rc == getattr(FT, want), (label, rc)
    rc, _ = _call(shard, name, ptrs, FT.MEM_HOST, None)    # a shard-only context serves its split transform and nothing else
    assert rc == FT.ERR_BAD_ARG
    rc, _ = _call(t, name, ptrs, FT.MEM_HOST, None)          # the context still works
    assert rc == FT.OK
