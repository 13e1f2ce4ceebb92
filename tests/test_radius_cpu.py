"""Radius search, CPU tier: the C ABI entry point exists and refuses bad arguments before any device call, the
radius -> exact integer bound conversion is pinned on its edge values, and the shard merge equals the radius result over
the concatenated rows (oracle)."""
import ctypes as C
import math

import numpy as np
import pytest

from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G
from metrovector_amd.sharded import merge_radius

from _radius import oracle_radius

INT32_MAX, INT32_MIN = 2**31 - 1, -2**31


def _call(corpus=None, metric=0, q=None, qdtype=0, qdim=4, nq=1, radii=None, m=4, counts=True, sc=True, idx=True):
    q = np.zeros(qdim * max(nq, 1), np.float32) if q is None else q
    radii = np.ones(max(nq, 1), np.float32) if radii is None else np.asarray(radii, np.float32)
    cnt = np.zeros(max(nq, 1), np.uint64)
    s = np.zeros(max(nq * m, 1), np.float32)
    i = np.zeros(max(nq * m, 1), np.uint64)
    p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    rc = _lib.gpu().mvfgpu_search_radius(corpus, metric, q.ctypes.data_as(C.c_void_p), qdtype, qdim, nq,
                                         radii.ctypes.data_as(C.c_void_p), m, p(cnt, counts), p(s, sc), p(i, idx), None)
    return rc, _lib.gpu().mvfgpu_last_error_message().decode()


def test_search_radius_is_exported():
    lib = _lib.gpu()
    assert hasattr(lib, "mvfgpu_search_radius") and hasattr(lib, "mvfgpu_selftest_radius_bound")
    assert hasattr(G.GpuCorpus, "search_radius")


def test_refusals_precede_any_device_call():
    INV = 12
    rc, msg = _call(corpus=None)
    assert rc == INV and "corpus is NULL" in msg
    rc, msg = _call(radii=[float("nan")])
    assert rc == INV and "NaN" in msg
    rc, msg = _call(nq=3, radii=[1.0, float("nan"), 2.0])
    assert rc == INV and "query 1" in msg
    rc, msg = _call(m=2**31 + 1)
    assert rc == INV and "max_per_query" in msg
    rc, msg = _call(counts=False)
    assert rc == INV and "NULL" in msg
    rc, msg = _call(sc=False)
    assert rc == INV and "NULL" in msg
    rc, msg = _call(m=0, sc=False, idx=False)  # counts only: entry buffers may be NULL -> the corpus check refuses next
    assert rc == INV and "corpus is NULL" in msg
    rc, msg = _call(metric=7)
    assert rc == INV and "metric" in msg
    rc, msg = _call(nq=0)
    assert rc == INV and "nq" in msg


def test_python_layer_refuses_a_nan_radius_and_a_negative_max():
    c = G.GpuCorpus(0)  # a NULL handle: nothing may reach the device
    c._h = C.c_void_p(None)
    with pytest.raises(E.InvalidArgument, match="NaN"):
        c.search_radius(np.zeros(4, np.float32), float("nan"), 3)
    with pytest.raises(E.InvalidArgument):
        c.search_radius(np.zeros(4, np.float32), 1.0, -1)


def _l2_bound_brute(r):
    """largest R >= 0 with sqrtf(R) <= r, by a window search around r^2 (numpy's f32 sqrt is correctly rounded)"""
    if r < 0:
        return -1
    if math.isinf(r) or r * r > 2.2e9:
        return INT32_MAX
    c = int(r * r)
    lo = max(0, c - 4096)
    R = np.arange(lo, min(INT32_MAX, c + 4096) + 1, dtype=np.int64)
    ok = np.sqrt(R.astype(np.float32)) <= np.float32(r)
    assert ok[0] and not ok[-1]
    return int(R[ok].max())


def _ip_bound_brute(r):
    """smallest R with (float)R >= r"""
    if r == -math.inf:
        return INT32_MIN
    if r > 2.0**31:
        return INT32_MAX
    c = int(math.floor(r))
    R = np.arange(max(INT32_MIN, c - 512), min(INT32_MAX, c + 512) + 1, dtype=np.int64)
    ok = R.astype(np.float32) >= np.float32(r)
    return int(R[ok].min())


def _mid(a, b):
    """an f32 strictly between two f32 values, when there is one"""
    a, b = np.float32(a), np.float32(b)
    m = np.nextafter(a, b)
    assert a < m < b
    return float(m)


@pytest.mark.parametrize("dtype", [G.INT8, G.UINT8])
def test_l2_raw_bound_edges(dtype):
    f = lambda r: G.radius_bound(dtype, G.L2, r)[1]  # noqa: E731
    assert f(0.0) == 0 and f(-0.0) == 0
    assert f(-1e-30) == -1 and f(-math.inf) == -1
    assert f(math.inf) == INT32_MAX
    for s in (1, 2, 3, 17, 255, 4096, 46340):  # exact squares are included
        assert f(float(s)) == _l2_bound_brute(float(s)) >= s * s  # (past 2^24 several integers share the float of s^2)
        assert s > 2048 or f(float(s)) == s * s
        assert f(float(np.nextafter(np.float32(s), np.float32(0)))) == _l2_bound_brute(float(np.nextafter(np.float32(s), np.float32(0))))
    for R in (2, 10, 1000, 123456, 16777217, 2_000_000_000):  # between two representable sqrtf results
        lo, hi = np.sqrt(np.float32(R)), np.sqrt(np.float32(R + 1))
        if lo < hi and np.nextafter(lo, hi) < hi:
            r = _mid(lo, hi)
            assert f(r) == _l2_bound_brute(r)
        assert f(float(lo)) == _l2_bound_brute(float(lo))
    assert f(1.5) == 2 and f(2.9999998) == 8
    # the key is the exact integer's (mvf_common.h): L2 key = R ^ 0x80000000
    assert G.radius_bound(dtype, G.L2, 3.0)[0] == (9 ^ 0x80000000)


@pytest.mark.parametrize("dtype", [G.INT8, G.UINT8])
def test_ip_raw_bound_edges(dtype):
    f = lambda r: G.radius_bound(dtype, G.INNER_PRODUCT, r)[1]  # noqa: E731
    assert f(0.0) == 0 and f(-0.0) == 0
    assert f(2.5) == 3 and f(-2.5) == -2 and f(7.0) == 7 and f(-7.0) == -7
    assert f(-math.inf) == INT32_MIN
    assert f(math.inf) == INT32_MAX and f(3e9) == INT32_MAX  # nothing can match: no dot product reaches INT32_MAX
    assert f(16777216.0) == 16777216
    assert f(16777218.0) == 16777218  # (float)16777217 == 16777216 < 16777218
    for r in (1e-30, -1e-30, 12345.678, -98765.5, 1.5e9, -1.5e9):
        assert f(r) == _ip_bound_brute(r)
    assert G.radius_bound(dtype, G.INNER_PRODUCT, 2.5)[0] == (~(3 ^ 0x80000000) & 0xFFFFFFFF)


def test_float_bounds_are_the_score_keys():
    def ord_key(x):
        b = int(np.float32(x + 0.0).view(np.uint32))
        return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)
    for dt in (G.FLOAT32, G.FLOAT16):
        for r in (0.0, 1.0, -2.5, math.inf, -math.inf, 1e-38):
            assert G.radius_bound(dt, G.L2, r) == (ord_key(r), 0)
            assert G.radius_bound(dt, G.INNER_PRODUCT, r) == (ord_key(-r), 0)
            assert G.radius_bound(dt, G.COSINE, r) == (ord_key(-r), 0)
    assert G.radius_bound(G.INT8, G.COSINE, 0.5) == (ord_key(-0.5), 0)  # cosine of integer rows is a float score
    with pytest.raises(E.InvalidArgument, match="NaN"):
        G.radius_bound(G.INT8, G.L2, float("nan"))


@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("dtype,metric", [(G.FLOAT32, G.L2), (G.FLOAT32, G.COSINE), (G.INT8, G.INNER_PRODUCT),
                                          (G.UINT8, G.L2), (G.FLOAT16, G.INNER_PRODUCT)])
def test_merge_radius_equals_the_radius_over_the_concatenated_rows(oracle, nshards, dtype, metric):
    n, dim, nq, m = 997, 13, 5, 40
    rows = oracle.synth_rows(71, 0, n, dim, dtype)
    qs = oracle.synth_queries(72, nq, dim, dtype)
    dead = np.zeros(n, bool)
    dead[::11] = True
    bounds = np.linspace(0, n, nshards + 1).astype(int)
    radii = []
    for q in qs:  # ~60 matches: more than max_per_query, so the merge has to cut
        s = oracle.scores(rows, dtype, metric, q)[0]
        s = np.sort(s[~dead]) if metric == 0 else np.sort(s[~dead])[::-1]
        radii.append(float(s[59]))
    parts = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        cnt = np.zeros(nq, np.uint64)
        S = np.zeros((nq, m), np.float32)
        I = np.zeros((nq, m), np.uint64)
        R = np.zeros((nq, m), np.int32)
        for j, q in enumerate(qs):
            c, S[j], I[j], R[j] = oracle_radius(oracle, rows[a:b], dtype, metric, q, radii[j], m, dead=dead[a:b], index_base=a)
            cnt[j] = c
        parts.append(G.RadiusResult(cnt, S, I, R))
    got = merge_radius(parts, metric, dtype, m)
    for j, q in enumerate(qs):
        c, S, I, R = oracle_radius(oracle, rows, dtype, metric, q, radii[j], m, dead=dead)
        assert int(got.counts[j]) == c and c >= 60
        assert (got.indices[j] == I).all()
        assert (got.scores[j].view(np.uint32) == S.view(np.uint32)).all()
        assert (got.raw[j] == R).all()


def test_routing_self_test_pins_the_crossover():
    for dt in (G.FLOAT16, G.INT8, G.UINT8):  # only Float32 rows have the batched radius route
        assert {G.radius_route(dt, nq) for nq in (1, 4, 16, 1024)} == {0}
        assert G.radius_route(dt, 1024, 2) == 0
    assert [G.radius_route(G.FLOAT32, nq) for nq in (1, 2, 4, 15, 16, 17, 1024, 100000)] == [0, 0, 0, 0, 1, 1, 1, 1]
    assert G.radius_route(G.FLOAT32, 1024, 1) == 0  # scan path 1: the streaming kernel
    for path in (2, 3, 5):
        assert G.radius_route(G.FLOAT32, 1, path) == 1 and G.radius_route(G.FLOAT32, 1024, path) == 1
    assert G.radius_route(G.FLOAT32, 15, 4) == 0 and G.radius_route(G.FLOAT32, 16, 6) == 1
    with pytest.raises(E.InvalidArgument):
        G.radius_route(G.FLOAT32, 0)
