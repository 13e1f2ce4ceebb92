"""Diversified re-ranking, CPU tier (include/mvf_gpu_mmr.h; DESIGN.md §3 "Diversified re-ranking"): the walk on the host
(mvfgpu_selftest_mmr_walk, D0's arithmetic) against the numpy walk of tests/_mmr.py, one case a fused multiply-subtract gets
wrong, the refusals that need no device, and the header's functions against the entry classes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

import _mmr as MM
import _streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT
METRICS = [G.L2, G.INNER_PRODUCT, G.COSINE]
LAMBDAS = [0.0, 0.3, 1.0]


def _check(metric, rel, sim, lam, k):
    rel, sim = np.asarray(rel, np.float32), np.asarray(sim, np.float32)
    m = rel.size
    order, obj, n = G.mmr_walk(rel, sim, metric, lam, k)
    want_o, want_obj = MM.numpy_walk(metric, rel, sim.reshape(m, m), lam, k)
    assert n == min(k, m) == len(want_o)
    assert order[:n].tolist() == want_o, f"metric {metric} lambda {lam} k {k}: picks {order[:8]} != {want_o[:8]}"
    assert obj[:n].tobytes() == want_obj.tobytes(), f"metric {metric} lambda {lam} k {k}: objective bits"
    assert (order[n:] == 0xFFFFFFFF).all() and (obj[n:] == MM.pad_score(metric)).all()
    assert len(set(order[:n].tolist())) == n


def _ks(m):
    return sorted({1, m, m + 3})


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", [1, 2, 37, 1024])
def test_walk_on_random_scores(metric, m):
    rng = np.random.default_rng(100 * m + metric)
    rel = rng.standard_normal(m).astype(np.float32)
    sim = rng.standard_normal((m, m)).astype(np.float32)
    if metric == G.L2:
        rel, sim = np.abs(rel), np.abs(sim)
    for lam in LAMBDAS:
        for k in (_ks(m) if m < 1024 else [1, 40, m + 3] if lam == 0.3 else [40]):
            _check(metric, rel, sim, lam, k)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("lam", LAMBDAS)
def test_walk_on_special_values(metric, lam):
    m = 24
    rng = np.random.default_rng(7 + metric)
    base_rel = rng.standard_normal(m).astype(np.float32)
    base_sim = rng.standard_normal((m, m)).astype(np.float32)
    worlds = {}
    rel, sim = base_rel.copy(), base_sim.copy()
    rel[[3, 11]] = np.nan                       # NaN in rel
    worlds["nan rel"] = (rel, sim)
    rel, sim = base_rel.copy(), base_sim.copy()
    sim[5, :] = np.nan                          # a NaN row: the pick 5 moves no red
    sim[:, 9] = np.nan                          # a NaN column: red(9) stays -inf
    worlds["nan row and column of sim"] = (rel, sim)
    worlds["all nan"] = (np.full(m, np.nan, np.float32), np.full((m, m), np.nan, np.float32))
    rel, sim = base_rel.copy(), base_sim.copy()
    rel[[1, 2]] = [np.inf, -np.inf]
    sim[4, 6], sim[4, 7], sim[8, :] = np.inf, -np.inf, np.inf
    worlds["infinities"] = (rel, sim)
    rel = np.where(np.arange(m) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    sim = np.where((np.arange(m)[:, None] + np.arange(m)[None, :]) % 3 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    worlds["signed zeros tie"] = (rel, sim)
    worlds["all equal"] = (np.full(m, 0.25, np.float32), np.full((m, m), 0.5, np.float32))
    for name, (rel, sim) in worlds.items():
        for k in _ks(m) + [5]:
            _check(metric, rel, sim, lam, k)
    # all equal: pure position order
    order, _, n = G.mmr_walk(*worlds["all equal"], metric, lam, m)
    assert order.tolist() == list(range(m)) and n == m
    order, _, _ = G.mmr_walk(*worlds["signed zeros tie"], metric, 1.0, m)
    assert order.tolist() == list(range(m)), "-0.0 and +0.0 tie: position order at lambda = 1"


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def test_the_objective_is_never_fused():
    """Three rows under InnerProduct, lambda = 0.3f.  Row 0 is picked first.  Row 1 has red = 0, so its objective is the one
    product a rel(1) = 0xBEE28038 in either form.  Row 2's objective is 0xBEE28038 too as (a rel) - (b red) with three roundings
    -- a tie, which position 1 wins -- but 0xBEE28037, one ulp larger, as fma(a, rel, -(b red)): the fused form picks row 2.
    The inputs were found by a numpy search and CHECKED to distinguish the two forms (exact rational arithmetic); the
    assertions below repeat that check in float64, where a rel is exact and the one subtraction rounds once to f32."""
    a = np.float32(0.3)
    b = np.float32(1.0) - a
    rel = np.array([2.0, _f32(0xBFBCC02E), _f32(0x3EED7547)], np.float32)
    sim = np.zeros((3, 3), np.float32)
    sim[0, 2] = _f32(0x3F54AB92)
    two = (a * rel[2]) - (b * sim[0, 2])
    fused = np.float32(np.float64(a) * np.float64(rel[2]) - np.float64(b * sim[0, 2]))
    assert two.view(np.uint32) == 0xBEE28038 and fused.view(np.uint32) == 0xBEE28037, "the case distinguishes the two forms"
    assert (a * rel[1]).view(np.uint32) == 0xBEE28038
    order, obj, n = G.mmr_walk(rel, sim, G.INNER_PRODUCT, 0.3, 2)
    assert n == 2 and order.tolist() == [0, 1], "a fused multiply-subtract picks row 2"
    assert obj.view(np.uint32).tolist() == [(a * rel[0]).view(np.uint32), 0xBEE28038]
    assert MM.numpy_walk(G.INNER_PRODUCT, rel, sim, 0.3, 2)[0] == [0, 1]
    order, obj, _ = G.mmr_walk(rel, sim, G.INNER_PRODUCT, 0.3, 3)
    assert order.tolist() == [0, 1, 2] and obj.view(np.uint32)[2] == 0xBEE28038


def _walk_rc(rel=True, sim=True, m=3, metric=0, lam=0.5, k=2, order=True):
    r, s = np.zeros(max(m, 1), np.float32), np.zeros(max(m * m, 1), np.float32)
    o, ob = np.zeros(max(k, 1) if k < 1 << 20 else 1, np.uint32), np.zeros(max(k, 1) if k < 1 << 20 else 1, np.float32)
    p = lambda arr, on: arr.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    rc = lib.mvfgpu_selftest_mmr_walk(p(r, rel), p(s, sim), m, metric, lam, k, p(o, order), p(ob, True))
    return rc, lib.mvfgpu_last_error_message().decode()


def test_the_walk_refuses_bad_arguments():
    assert _walk_rc()[0] == 2
    rc, msg = _walk_rc(metric=7)
    assert rc == -INV and "metric" in msg
    rc, msg = _walk_rc(k=0)
    assert rc == -INV and "k must be" in msg
    for kw in (dict(rel=False), dict(sim=False), dict(order=False)):
        rc, msg = _walk_rc(**kw)
        assert rc == -INV and "NULL" in msg, kw
    for lam in (float("nan"), -0.001, 1.001, float("inf")):
        rc, msg = _walk_rc(lam=lam)
        assert rc == -INV and "lambda" in msg, lam
    rc, msg = _walk_rc(m=0, rel=False, sim=False, k=3)
    assert rc == 0
    with pytest.raises(E.InvalidArgument, match="MVFGPU_MMR_MAX_CANDIDATES"):
        G.mmr_walk(np.zeros(1025, np.float32), np.zeros((1025, 1025), np.float32), 0, 0.5, 1)
    with pytest.raises(E.InvalidArgument, match="lambda"):
        G.mmr_walk(np.zeros(2, np.float32), np.zeros((2, 2), np.float32), 0, 2.0, 1)
    with pytest.raises(E.InvalidArgument):
        G.mmr_walk(np.zeros(3, np.float32), np.zeros((2, 2), np.float32), 0, 0.5, 1)
    assert G.mmr_walk(np.zeros(1, np.float32), np.zeros((1, 1), np.float32), 0, 0.0, 1)[0].tolist() == [0]
    assert G.mmr_walk(np.zeros(1, np.float32), np.zeros((1, 1), np.float32), 0, 1.0, 1)[0].tolist() == [0]


def _call(device=False, timer=False, corpus=None, metric=0, q=True, qdtype=0, qdim=4, nq=1, cand=True, m=3, k=2, lam=0.5, sc=True,
          idx=True, ms=True):
    qa = np.zeros(qdim * max(nq, 1), np.float32)
    ca = np.zeros(max(nq * m, 1), np.uint64)
    s = np.zeros(max(nq * k, 1) if k < 1 << 20 else 1, np.float32)
    i = np.zeros(max(nq * k, 1) if k < 1 << 20 else 1, np.uint64)
    out_ms = np.zeros(2, np.float32)
    p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    if timer:
        rc = lib.mvfgpu_selftest_mmr_stage_ms(corpus, metric, p(qa, q), qdtype, qdim, nq, p(ca, cand), m, k, lam, p(s, sc), p(i, idx),
                                              None, None, None, None, p(out_ms, ms))
    elif device:
        rc = lib.mvfgpu_search_mmr_device(corpus, metric, p(qa, q), qdtype, qdim, nq, p(ca, cand), m, k, lam, p(s, sc), p(i, idx),
                                          None, None, None, None)
    else:
        rc = lib.mvfgpu_search_mmr(corpus, metric, p(qa, q), qdtype, qdim, nq, p(ca, cand), m, k, lam, p(s, sc), p(i, idx), None,
                                   None, None)
    return rc, lib.mvfgpu_last_error_message().decode()


FORMS = [dict(), dict(device=True), dict(timer=True)]


@pytest.mark.parametrize("form", FORMS, ids=["host", "device", "timer"])
def test_refusals_precede_any_device_call(form):
    """the candidate search's checks in its order and with its messages; a bad lambda or list length is looked at only behind
    them (`corpus is NULL` comes first: tests/test_gpu_mmr.py holds those two on a live handle)"""
    rc, msg = _call(**form, corpus=None)
    assert rc == INV and msg == "corpus is NULL"
    rc, msg = _call(**form, metric=7)
    assert rc == INV and "metric" in msg
    rc, msg = _call(**form, nq=0)
    assert rc == INV and "nq" in msg
    rc, msg = _call(**form, k=0)
    assert rc == INV and "k must be" in msg
    rc, msg = _call(**form, k=2**31 + 1)
    assert rc == INV and "k must be" in msg
    for kw in (dict(q=False), dict(sc=False), dict(idx=False)):
        rc, msg = _call(**form, **kw)
        assert rc == INV and "NULL" in msg, kw
    rc, msg = _call(**form, cand=False)
    assert rc == INV and "candidates" in msg
    rc, msg = _call(**form, cand=False, m=0)  # nothing listed: no list needed -> the handle check refuses next
    assert rc == INV and msg == "corpus is NULL"
    for kw in (dict(lam=float("nan")), dict(lam=1.5), dict(m=5000)):  # behind the handle check
        rc, msg = _call(**form, **kw)
        assert rc == INV and msg == "corpus is NULL", kw
    if form.get("timer"):
        rc, msg = _call(**form, ms=False)
        assert rc == INV and "NULL" in msg


def test_python_layer():
    assert hasattr(G.GpuCorpus, "search_mmr") and hasattr(G.GpuCorpus, "search_mmr_device") and hasattr(G.GpuCorpus, "mmr_walk")
    assert callable(M.diversify_top_k) and callable(M.find_top_k_diverse)
    assert "diversify_top_k" in M.__all__ and "find_top_k_diverse" in M.__all__
    assert G.MMR_MAX_CANDIDATES == 1024
    c = G.GpuCorpus(0)  # a NULL handle: nothing may reach the device
    c._h = C.c_void_p(None)
    q = np.zeros((2, 4), np.float32)
    for bad in (np.zeros(6, np.uint64), np.zeros((2, 3), np.int64), np.zeros((3, 3), np.uint64), [[1, 2, 3], [4, 5, 6]]):
        with pytest.raises(E.InvalidArgument):
            c.search_mmr(q, bad, 2)
    order, obj, n = G.GpuCorpus.mmr_walk(np.array([1, 3, 2], np.float32), np.zeros((3, 3), np.float32), G.INNER_PRODUCT, 0.5, 2)
    assert n == 2 and order.tolist() == [1, 2]


def test_every_function_of_the_header_has_a_class():
    text = open(os.path.join(ROOT, "include", "mvf_gpu_mmr.h")).read()
    declared = set(re.findall(r"^\s*(?:int|void|uint\d+_t|const char\*)\s+(mvfgpu_\w+)\s*\(", text, re.M))
    assert declared == set(MM.ENTRY_CLASS), declared ^ set(MM.ENTRY_CLASS)
    classes = {S.NO_HANDLE, S.NO_DEVICE_WORK, S.DEVICE_CALL, S.BLOCKS_DEVICE, S.HOST_WAIT}
    assert set(MM.ENTRY_CLASS.values()) <= classes
    assert not set(MM.ENTRY_CLASS) & set(S.ENTRY_CLASS), "include/mvf_gpu.h declares none of them"
    for aid, form in MM.TIMED_FORM_OF.items():
        assert MM.ENTRY_CLASS[aid] == MM.ENTRY_CLASS[form] == S.DEVICE_CALL
    lib = _lib.gpu()
    for name in MM.ENTRY_CLASS:
        assert hasattr(lib, name), name
    assert int(re.search(r"#define MVFGPU_MMR_MAX_CANDIDATES (\d+)u", text).group(1)) == G.MMR_MAX_CANDIDATES
    assert '#include "mvf_gpu.h"' in text
