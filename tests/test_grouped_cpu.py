"""Grouped search, CPU tier (DESIGN.md §3 "Grouped search"): the library exports the new entry points and Python names them,
the numpy reference of the walk is the contract's loop, every refusal that needs no handle precedes any device call and names
its cause, G1's tier rule is the pure function the header states, and the layouts (tests/_grouped.py) are what the GPU tests
take them for."""
import ctypes as C
import os

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

import _grouped as GR
import _partitioned as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT


def _msg():
    return _lib.gpu().mvfgpu_last_error_message().decode()


def test_entry_points_and_python_names_exist():
    lib = _lib.gpu()
    for name in ("mvfgpu_search_grouped", "mvfgpu_search_grouped_device", "mvfgpu_column_gather", "mvfgpu_selftest_group_plan",
                 "mvfgpu_selftest_grouped_stage_ms"):
        assert hasattr(lib, name), name
    for name in ("search_grouped", "search_grouped_device"):
        assert hasattr(G.GpuCorpus, name), name
    assert hasattr(G.GpuColumn, "gather") and hasattr(G, "group_plan") and hasattr(G.GpuCorpus, "grouped_stage_ms")
    assert "find_top_k_grouped" in M.__all__ and hasattr(M, "find_top_k_grouped")
    hpp = open(os.path.join(ROOT, "include", "mvf.hpp")).read()
    assert "find_top_k_grouped" in hpp and "mvfgpu_column_gather" in hpp
    header = open(os.path.join(ROOT, "include", "mvf_gpu.h")).read()
    assert "#define MVFGPU_GROUP_MAX_PER_KEY 64u" in header
    assert _lib.gpu().mvfgpu_abi_version() == 3, "an additive change: the ABI version stays"


def test_the_numpy_walk_is_the_contracts_loop():
    rng = np.random.default_rng(11)
    for trial in range(200):
        n = int(rng.integers(1, 400))
        nkeys = int(rng.integers(1, 40))
        col = rng.integers(0, nkeys, n).astype(np.uint64) * np.uint64((1 << 33) + 5)
        ranked = rng.permutation(n)[:int(rng.integers(0, n + 1))]
        per_key = int(rng.choice([1, 2, 3, 63, 64]))
        k = int(rng.choice([1, 10, 100, n + 5]))
        got, want = GR.grouped_walk(ranked, col, per_key, k), GR.walk_by_dict(ranked, col, per_key, k)
        assert got.tolist() == want.tolist(), (trial, n, nkeys, per_key, k)
    # per_key beyond every key's size: the ranking cut at k; every row its own key: the same
    ranked = rng.permutation(50)
    assert GR.grouped_walk(ranked, np.zeros(50, np.uint32), 64, 10).tolist() == list(range(10))
    assert GR.grouped_walk(ranked, np.arange(50, dtype=np.uint32), 1, 10).tolist() == list(range(10))
    assert GR.grouped_walk(ranked, np.zeros(50, np.uint32), 3, 10).tolist() == [0, 1, 2]


def test_refusals_without_a_handle_precede_any_device_call_in_the_searchs_order():
    lib = _lib.gpu()
    one = np.zeros(4, np.uint64)
    p1 = one.ctypes.data_as(C.c_void_p)

    def host(metric=0, q=p1, nq=1, k=1, per_key=1, sc=p1, idx=p1):
        return lib.mvfgpu_search_grouped(None, None, metric, q, 0, 4, nq, k, per_key, sc, idx, None)

    def dev(metric=0, q=p1, nq=1, k=1, per_key=1, sc=p1, idx=p1):
        return lib.mvfgpu_search_grouped_device(None, None, metric, q, 0, 4, nq, k, per_key, sc, idx, None, None)

    for call in (host, dev):
        # everything wrong at once: the metric is named; then nq, k, the buffers, per_key, the partition
        assert call(metric=9, q=None, nq=0, k=0, per_key=0) == INV and "metric" in _msg()
        assert call(q=None, nq=0, k=0, per_key=0) == INV and "nq" in _msg()
        assert call(q=None, k=0, per_key=0) == INV and "k must be" in _msg()
        assert call(q=None, per_key=0) == INV and "NULL buffer" in _msg()
        assert call(sc=None, per_key=0) == INV and "NULL buffer" in _msg()
        assert call(idx=None, per_key=65) == INV and "NULL buffer" in _msg()
        assert call(per_key=0) == INV and "per_key must be in 1..64" in _msg() and "got 0" in _msg()
        assert call(per_key=65) == INV and "per_key must be in 1..64" in _msg() and "got 65" in _msg()
        assert call(per_key=64) == INV and "partition is NULL" in _msg()
        assert call(per_key=1) == INV and "partition is NULL" in _msg()
    assert lib.mvfgpu_column_gather(None, p1, 1, p1) == INV and "column is NULL" in _msg()
    fake = C.c_void_p(16)  # never dereferenced: the NULL argument is found first
    assert lib.mvfgpu_column_gather(fake, None, 1, p1) == INV and "NULL buffer" in _msg()
    assert lib.mvfgpu_column_gather(fake, p1, 1, None) == INV and "NULL buffer" in _msg()
    assert lib.mvfgpu_selftest_group_plan(None, p1, 1, 1, p1) == INV and _msg()
    assert lib.mvfgpu_selftest_group_plan(p1, None, 1, 1, p1) == INV and _msg()
    assert lib.mvfgpu_selftest_group_plan(p1, p1, 1, 1, None) == INV and _msg()


_ONE = np.zeros(4, np.uint64)
_P1 = _ONE.ctypes.data_as(C.c_void_p)
_NAN, _RADII = np.full(1, np.nan, np.float32), np.ones(1, np.float32)
_FAKE = C.c_void_p(16)  # a filter / partition that is never dereferenced: `corpus is NULL` is found first
_BUFFERS = dict(q=_P1, sc=_P1, idx=_P1)
_PER_KEY_0 = "per_key must be in 1..64, got 0"


def _topk_ladder(own):
    """everything wrong at once, then one fix after the other: (the message reported, the fix that follows it)"""
    return [("unsupported distance metric code 9", dict(metric=0)), ("nq must be > 0", dict(nq=1)),
            ("k must be in 1..2^31", dict(k=1)), ("NULL buffer", _BUFFERS)] + own


def _candidates(device):
    fn = getattr(_lib.gpu(), "mvfgpu_search_candidates" + ("_device" if device else ""))
    return (lambda a: fn(None, a["metric"], a["q"], 0, 4, a["nq"], a["cand"], 5, a["k"], a["sc"], a["idx"], None, None, *[None] * device),
            dict(cand=None), _topk_ladder([("NULL buffer (candidates)", dict(cand=_P1))]))


def _filtered(device):
    fn = getattr(_lib.gpu(), "mvfgpu_search_filtered" + ("_device" if device else ""))
    return (lambda a: fn(None, a["flt"], a["metric"], a["q"], 0, 4, a["nq"], a["k"], a["sc"], a["idx"], None, *[None] * device),
            dict(flt=None), _topk_ladder([("filter is NULL", dict(flt=_FAKE))]))


def _partitioned(device):
    fn = getattr(_lib.gpu(), "mvfgpu_search_partitioned" + ("_device" if device else ""))
    return (lambda a: fn(None, a["part"], a["metric"], a["q"], 0, 4, a["nq"], a["keys"], a["k"], a["sc"], a["idx"], None, *[None] * device),
            dict(part=None, keys=None), _topk_ladder([("NULL buffer (keys)", dict(keys=_P1)), ("partition is NULL", dict(part=_FAKE))]))


def _grouped(device):
    fn = getattr(_lib.gpu(), "mvfgpu_search_grouped" + ("_device" if device else ""))
    return (lambda a: fn(None, a["part"], a["metric"], a["q"], 0, 4, a["nq"], a["k"], a["per_key"], a["sc"], a["idx"], None, *[None] * device),
            dict(part=None, per_key=0), _topk_ladder([(_PER_KEY_0, dict(per_key=1)), ("partition is NULL", dict(part=_FAKE))]))


def _radius(device):
    """its three required buffers are the queries, the radii and the counts, and they come before its own range of
    max_per_query (`k` here); the result buffers are required only where entries are asked for"""
    fn = _lib.gpu().mvfgpu_search_radius
    nan, radii = _NAN.ctypes.data_as(C.c_void_p), _RADII.ctypes.data_as(C.c_void_p)
    return (lambda a: fn(None, a["metric"], a["q"], 0, 4, a["nq"], a["radii"], a["k"], a["counts"], a["sc"], a["idx"], None),
            dict(radii=None, counts=None, k=(1 << 31) + 1),
            [("unsupported distance metric code 9", dict(metric=0)), ("nq must be > 0", dict(nq=1)),
             ("NULL buffer", dict(q=_P1, radii=nan, counts=_P1)), ("max_per_query must be in 0..2^31", dict(k=1)),
             ("NULL buffer (out_scores / out_indices are required when max_per_query > 0)", dict(sc=_P1, idx=_P1)),
             ("radius of query 0 is NaN", dict(radii=radii))])


@pytest.mark.parametrize("make,device", [(_candidates, 0), (_candidates, 1), (_filtered, 0), (_filtered, 1), (_partitioned, 0),
                                         (_partitioned, 1), (_grouped, 0), (_grouped, 1), (_radius, 0)],
                         ids=lambda v: v.__name__.strip("_") if callable(v) else ("device" if v else "host"))
def test_refusal_precedence_of_every_list_search_without_a_handle(make, device):
    """corpus = NULL and every other argument bad as well: the metric is named first, then nq, the range of k, the required
    buffers, the call's own argument(s), and `corpus is NULL` only once all of them are valid -- code and message at every
    step.  The radius search names its buffers before its own range, as it always has."""
    call, own, ladder = make(device)
    state = {**dict(metric=9, nq=0, k=0, q=None, sc=None, idx=None), **own}
    for message, fix in ladder:
        assert call(state) == INV and _msg() == message, (message, _msg())
        state = {**state, **fix}
    assert call(state) == INV and _msg() == "corpus is NULL", _msg()


def test_the_tier_rule_at_every_boundary():
    for per_key in GR.PER_KEYS:
        lengths = sorted({1, per_key - 1, per_key, per_key + 1, GR.RANK_MAX - 1, GR.RANK_MAX, GR.RANK_MAX + 1, GR.TILE - 1, GR.TILE} - {0})
        for crossing in (0, 1):
            got = G.group_plan(lengths, [crossing] * len(lengths), per_key).tolist()
            assert got == [GR.run_tier(n, per_key, crossing) for n in lengths], (per_key, crossing)
    assert G.group_plan([1, 2, 3, 128, 129, 1, 1024], [0, 0, 0, 0, 0, 1, 1], 2).tolist() == [0, 0, 1, 1, 2, 2, 2]
    assert G.group_plan([64, 65, 128, 129], [0] * 4, 64).tolist() == [0, 1, 1, 2]
    for bad in (0, 65):
        with pytest.raises(E.InvalidArgument, match="per_key must be in 1..64"):
            G.group_plan([1], [0], bad)
    for bad in (0, GR.TILE + 1):
        with pytest.raises(E.InvalidArgument, match="a run holds 1..1024"):
            G.group_plan([bad], [0], 1)
    with pytest.raises(E.InvalidArgument):
        G.group_plan([1, 2], [0], 1)


@pytest.mark.parametrize("flavour", ["u32", "u64"])
def test_the_cap_layout_holds_every_size_around_every_cap_and_every_tier(flavour):
    lay = GR.caps(flavour)
    _, counts = P.group_by(lay)
    sizes = set(counts.tolist())
    for per_key in GR.PER_KEYS:
        for size in (per_key - 1, per_key, per_key + 1):
            assert size == 0 or size in sizes, (per_key, size)
    for size in (GR.RANK_MAX - 1, GR.RANK_MAX, GR.RANK_MAX + 1, GR.TILE - 1, GR.TILE, GR.TILE + 1):
        assert size in sizes, size
    runs = GR.runs(lay)
    assert sum(n for n, _ in runs) == int((~lay["dead"]).sum())
    for per_key in GR.PER_KEYS:
        tiers = {(GR.run_tier(n, per_key, cr), cr) for n, cr in runs}
        assert {(0, False), (1, False), (2, False), (2, True)} <= tiers, (per_key, tiers)
    assert any(cr and n < 64 for n, cr in runs) and any(cr and n > 64 for n, cr in runs), "short and long runs of crossing keys"


@pytest.mark.parametrize("flavour", ["u32", "u64"])
def test_the_other_layouts(flavour):
    lay = GR.stock(flavour)
    assert sorted(P.group_by(lay)[1].tolist(), reverse=True)[:5] == [3000, 1025, 1024, 1023, 300]
    assert any(cr for _, cr in GR.runs(lay)), "the stock layout's large keys cross tiles"
    lay = GR.own_keys(flavour)
    keys, counts = P.group_by(lay)
    assert keys.size == int((~lay["dead"]).sum()) and (counts == 1).all()
    lay = GR.one_key(flavour)
    assert P.group_by(lay)[1].tolist() == [P.N - 820]
    assert len(GR.runs(lay)) == 8 and all(cr for _, cr in GR.runs(lay)), "one segment over all eight tiles"
    lay = GR.all_dead(flavour)
    assert lay["dead"].all()


def test_the_dominant_key_starves_a_fourfold_over_fetch():
    """k = 100, per_key = 1 on layout (c): the first 4 k rows of the plain ranking hold fewer than k keys, the whole ranking
    holds them -- from a float64 ranking of the rows the GPU test uses"""
    lay = GR.dominant("u32")
    keys, counts = P.group_by(lay)
    assert counts.max() == 6500 and keys.size == 1 + GR.DOMINANT_FURTHER and np.sort(counts)[-2] <= 8
    rows = P.make_rows(P.N, 100, "f32").astype(np.float64)
    live = GR.live_rows(lay)
    for q in P.make_queries(5, 100, "f32").astype(np.float64):
        d = ((rows[live] - q) ** 2).sum(1)
        ranked = live[np.lexsort((live, d))]
        k = 100
        over = GR.grouped_walk(ranked[:4 * k], lay["col"], 1, k)
        assert over.size < k, "a 4x over-fetch must not fill the capped list"
        full = GR.grouped_walk(ranked, lay["col"], 1, k)
        assert full.size == k and full[-1] >= 4 * k
