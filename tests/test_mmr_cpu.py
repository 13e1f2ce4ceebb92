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


# ---- the walk kernel's forms: mvfgpu_selftest_mmr_form, the case table and the references of tests/test_gpu_mmr_forms.py
def test_the_form_table_is_the_rule_and_the_selftest():
    """tests/_mmr.py's FORM_CELLS / FORCED_CELLS, written out by hand, against choose_group's rule restated in Python
    (MM.form_rule) and against the host code the launch itself calls; the rule against the self-test over every dimension up to
    2100 and around the LDS switch; the table holds all six widths of every type, both sides of the switch and the widest
    integer rows"""
    for (dt, dim), cell in MM.FORM_CELLS.items():
        assert MM.form_rule(dt, dim) == cell == tuple(G.mmr_form(MM.DTYPE[dt], dim)), (dt, dim)
    for (dt, dim, width), cell in MM.FORCED_CELLS.items():
        assert MM.form_rule(dt, dim, width) == cell == tuple(G.mmr_form(MM.DTYPE[dt], dim, width)), (dt, dim, width)
        assert MM.form_rule(dt, dim)[0] != width, "a width only MVF_K1_G reaches"
    for dt in MM.DTYPE:
        assert {cell[0] for (t, _), cell in MM.FORM_CELLS.items() if t == dt} == {1, 4, 8, 16, 32, 64}, dt
        for dim in list(range(1, 2101)) + [10239, 10240, 10241, 10248, 20000, 33025]:
            for width in (0, 16):
                assert MM.form_rule(dt, dim, width) == tuple(G.mmr_form(MM.DTYPE[dt], dim, width)), (dt, dim, width)
    for dt, near, far in MM.FORM_SWITCH:
        assert MM.FORM_CELLS[dt, near][2] and not MM.FORM_CELLS[dt, far][2] and far == near + 1
    for dt in ("i8", "u8"):
        assert MM.FORM_CELLS[dt, 33025] == (64, 33, True) and 64 * 33 * 16 == 33792   # the dynamic LDS of the widest rows
    assert [cell for (dt, dim, w), cell in MM.FORCED_CELLS.items() if not cell[2]] == [(16, 161, False), (16, 81, False)]
    # every call of a through-the-cache case keeps all four waves busy over several rewrites of the scratch row
    cases = [(dt, dim, 0) for dt, dim in MM.FORM_CASES] + MM.FORCED_CASES
    for ci, (dt, dim, width) in enumerate(cases):
        qlds = MM.form_rule(dt, dim, width)[2]
        for mi in range(3):
            calls = MM.form_calls(ci, mi, dim, qlds)
            assert all(m <= MM.form_rows(dim) and m in MM.form_ms(dim) for m, _, _, _ in calls)
            assert {k for _, k, _, _ in calls} >= {MM.F64_K} and calls[0][1] == calls[0][0] and {nq for *_, nq in calls} == {1, 3}
            assert qlds or all(m >= 65 and k >= 8 for m, k, _, _ in calls)
    ms = {(dim >= 10240, m) for ci, (dt, dim, width) in enumerate(cases) for mi in range(3) for m, *_ in MM.form_calls(ci, mi, dim, True)}
    assert ms == {(False, 65), (False, 257), (False, 1000), (False, 1024), (True, 65), (True, 257)}


def test_the_form_selftest_refuses_bad_arguments():
    lib = _lib.gpu()
    outs = [C.c_uint32(0) for _ in range(3)]
    ok = [C.byref(o) for o in outs]
    msg = lambda: lib.mvfgpu_last_error_message().decode()  # noqa: E731
    assert lib.mvfgpu_selftest_mmr_form(0, 100, 0, *ok) == 0 and [o.value for o in outs] == [32, 1, 1]
    for i in range(3):
        assert lib.mvfgpu_selftest_mmr_form(0, 100, 0, *[None if j == i else p for j, p in enumerate(ok)]) == INV and msg() == "NULL buffer"
    assert lib.mvfgpu_selftest_mmr_form(9, 100, 0, *ok) == INV and "data type" in msg()
    assert lib.mvfgpu_selftest_mmr_form(0, 0, 0, *ok) == INV and msg() == "dimension must be > 0"
    for dtype in (2, 3):
        assert lib.mvfgpu_selftest_mmr_form(dtype, 33025, 0, *ok) == 0
        assert lib.mvfgpu_selftest_mmr_form(dtype, 33026, 0, *ok) == INV and "33025" in msg()
    assert lib.mvfgpu_selftest_mmr_form(0, 33026, 0, *ok) == 0
    assert lib.mvfgpu_selftest_mmr_form(0, (1 << 28) + 1, 0, *ok) == INV and "1 GiB" in msg()
    for forced in (2, 3, 48, 128):
        assert lib.mvfgpu_selftest_mmr_form(0, 100, forced, *ok) == INV and "forced_g" in msg()
    with pytest.raises(E.InvalidArgument):
        G.mmr_form(2, 40000)


FLOAT_FORMS = [(ci, c) for ci, c in enumerate([(dt, dim, 0) for dt, dim in MM.FORM_CASES] + MM.FORCED_CASES) if not MM.is_int(c[0])]


@pytest.mark.parametrize("ci,case", FLOAT_FORMS, ids=[f"{dt}d{dim}g{w}" for _, (dt, dim, w) in FLOAT_FORMS])
def test_the_float64_walk_s_own_path_is_clear(ci, case):
    """the condition that keeps the band from hiding a failure, from the reference alone: along the float64 walk's own path at
    most 4 of the 32 steps have a second candidate within the band, for every metric and lambda the GPU file uses"""
    from _util import TOL
    dt, dim, _ = case
    rows, qs = MM.form_world(dt, dim)
    sel = np.sort(MM.f64_list(dt, dim, rows.shape[0], MM.f64_m(ci, dim)).astype(np.int64))
    terms = MM.f64_terms(rows[sel], qs[0], TOL)
    for mi, metric in enumerate(METRICS):
        unclear, _ = MM.f64_walk(metric, MM.f64_lambda(ci, mi), terms[metric], MM.F64_K)
        assert unclear <= MM.F64_OWN_UNCLEAR_MAX, f"metric {metric}: {unclear} unclear steps of {MM.F64_K}"


def _f32_scores(x, queries, metric):
    """a kernel's scores as numpy float32 (pairwise sums): [nq, c]"""
    import _wide as W
    return np.stack([W.pairwise_f32_scores(x, q, metric) for q in queries])


@pytest.fixture(scope="module")
def teeth_world():
    """257 Float32 rows of dimension 100 with ten exact copies of row 5 further up the list, their float64 terms and their
    scores in numpy float32"""
    from _util import TOL
    rows, qs = MM.form_world("f32", 100)
    x = rows[:257].copy()
    x[100:110] = x[5]
    return x, qs[0], MM.f64_terms(x, qs[0], TOL), {m: (_f32_scores(x, qs[:1], m)[0], _f32_scores(x, x, m)) for m in METRICS}


@pytest.mark.parametrize("metric", METRICS)
def test_the_float64_check_has_teeth(teeth_world, metric):
    """the contract's walk in numpy float32 passes the float64 check; a walk that ignores red, one that sums the sims, one that
    takes the sim's sign wrongly under L2 and one that breaks ties by descending position do not"""
    x, q, terms, f32 = teeth_world
    rel, sim = f32[metric]
    for lam in (0.3, 0.5):
        order, obj = MM.numpy_walk(metric, rel, sim, lam, MM.F64_K)
        unclear, frac = MM.f64_walk(metric, lam, terms[metric], MM.F64_K, order, obj, rel[order])
        assert frac < 1.0 and unclear <= MM.F64_DEVICE_UNCLEAR_MAX
        models = ["top_k", "sum"] + (["l2_sign"] if metric == G.L2 else [])
        for model in models:
            worder, wobj = MM.wrong_walk(metric, rel, sim, lam, MM.F64_K, model)
            assert worder != order, model
            with pytest.raises(AssertionError):
                MM.f64_walk(metric, lam, terms[metric], MM.F64_K, worder, wobj, rel[worder])
        # ties: the copies of row 5 hold equal objectives until one is picked, which all 257 picks bring about
        order, obj = MM.numpy_walk(metric, rel, sim, lam, 257)
        MM.f64_walk(metric, lam, terms[metric], 257, order, obj, rel[order])
        worder, wobj = MM.wrong_walk(metric, rel, sim, lam, 257, "descending")
        with pytest.raises(AssertionError, match="copy"):
            MM.f64_walk(metric, lam, terms[metric], 257, worder, wobj, rel[worder])
        order, obj = order[:MM.F64_K], obj[:MM.F64_K]
        # the right picks with an objective or a score off by three tolerances
        for name in ("objective", "score"):
            o2, s2 = obj.copy(), rel[order].copy()
            (o2 if name == "objective" else s2)[7] += np.float32(3e-5 * max(1.0, float(np.abs(rel).max()) * float(np.abs(sim).max())))
            with pytest.raises(AssertionError, match=name):
                MM.f64_walk(metric, lam, terms[metric], MM.F64_K, order, o2, s2)


def test_the_ascending_copies_property_has_teeth(teeth_world):
    x, q, terms, f32 = teeth_world
    groups = np.arange(257)
    groups[100:110] = 5
    for metric in METRICS:
        rel, sim = f32[metric]
        assert MM.first_descending_copy(MM.numpy_walk(metric, rel, sim, 0.3, 257)[0], groups) is None
        bad = MM.first_descending_copy(MM.wrong_walk(metric, rel, sim, 0.3, 257, "descending")[0], groups)
        assert bad is not None and bad[0] < bad[1]
    assert MM.first_descending_copy([3, 9, 4, 10], np.array([0] * 5 + [1] * 6)) is None
    assert MM.first_descending_copy([3, 9, 10, 2], np.array([0] * 5 + [1] * 6)) == (0, 3)
    # the ownership edges of D0's block: position i is folded by thread i % 256 of wave (i % 256) / 64
    g = np.arange(1024)
    assert MM.tie_edges(g) == (False, False, False)
    for a, b, want in ((0, 64, (True, False, False)), (0, 1, (False, False, False)), (3, 260, (False, True, False)),
                       (3, 256 + 67, (True, True, False)), (3, 515, (False, True, True))):
        g2 = g.copy()
        g2[b] = g2[a]
        assert MM.tie_edges(g2) == want, (a, b)
    import _dups as D
    for dtype in (0, 1):
        cp = D.corpus_b(MM.DUP_SEED + dtype, MM.DUP_N, MM.DUP_DIM, dtype)
        assert MM.tie_edges(cp.group_of[MM.dup_list().astype(np.int64)]) == (True, True, True)


@pytest.mark.parametrize("metric", METRICS)
def test_a_walk_that_flushes_float16_subnormals_is_rejected(oracle, metric):
    """tests/_edges.py's flush-to-zero model as D0's row_element: the picked row reaches the scoring flushed, the rows scored
    against it and the relevance do not.  On S (every metric) and on R (L2 and Cosine) the model's walk differs from the contract's
    (the recipe check), and from what the twin identities expect -- R's picks from H's under Cosine, S's from H's under L2"""
    import _edges as ED
    case = ED.get_case(oracle, MM.EDGE_SHAPE, ED.F16)
    sel = np.sort(np.unique(MM.edge_lists(case)[0]))
    sel = sel[sel < case.n].astype(np.int64)
    k, lam = MM.EDGE_K, MM.EDGE_LAMBDA

    def walks(kind):
        x16 = case.rows(kind)[sel]
        x = x16.astype(np.float32)
        q = case.queries_for(kind, metric, case.pool[:1])
        rel = _f32_scores(x, q, metric)[0]
        right = MM.numpy_walk(metric, rel, _f32_scores(x, x, metric), lam, k)
        model = MM.numpy_walk(metric, rel, _f32_scores(x, ED.flushed(x16).astype(np.float32), metric), lam, k)
        return right, model

    (h_order, h_obj), (h_model, h_mobj) = walks("H")
    assert h_model == h_order and h_mobj.tobytes() == h_obj.tobytes(), "H holds no subnormal: the model is the contract there"
    for kind in ("S", "R"):
        (order, obj), (model, mobj) = walks(kind)
        if (kind, metric) != ("R", G.INNER_PRODUCT):   # there a subnormal row's sims are too small to move any maximum: S decides
            assert model != order or mobj.tobytes() != obj.tobytes(), f"{kind}: the recipe check tells the model from the contract"
        if (kind, metric) == ("R", G.COSINE):
            assert order == h_order and obj.tobytes() == h_obj.tobytes() and model != h_order
        if (kind, metric) == ("S", G.L2):
            assert order == h_order and obj.tobytes() == np.ldexp(h_obj, ED.SHIFT["S"]).astype(np.float32).tobytes()
            assert model != h_order
