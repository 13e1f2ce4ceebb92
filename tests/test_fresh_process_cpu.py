"""The table of fresh-process scenarios (tests/_fresh_process.py) without a GPU: every scenario has its expectation, its inputs
are a function of fixed seeds, and the conditions the references of S11 .. S17 rely on hold -- computed from the reference side
alone (layouts, lists, float64 sums), never from an answer of the library."""
import numpy as np

import _fresh_process as F
import _maxsim as MS
import _maxsim_candidates as MC
import _partitioned as P
import test_gpu_fresh_process as T
from _util import TOL


def _same(a, b, what):
    assert type(a) is type(b), what
    if isinstance(a, dict):
        assert list(a) == list(b), what
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    else:
        assert a == b, what


def _builders():
    """name -> a function that builds the scenario family's inputs"""
    out = {"s1": F.s1_inputs, "s6": F.s6_inputs, "s7": F.s7_inputs, "s9": F.s9_inputs, "s16": F.s16_inputs, "s17": F.s17_inputs}
    for dt, dim in F.S2_SHAPES:
        out[f"s2_{dt}d{dim}"] = lambda dt=dt, dim=dim: F.s2_inputs(dt, dim)
        out[f"s3_{dt}d{dim}"] = lambda dt=dt, dim=dim: F.s3_inputs(dt, dim)
    for dt, dim in F.EXACT_FIT:
        out[f"s4_{dt}d{dim}"] = lambda dt=dt, dim=dim: F.s4_inputs(dt, dim)
    for dt in F.S8_SHAPES:
        out[f"s8_{dt}"] = lambda dt=dt: F.s8_inputs(dt)
        out[f"s10_{dt}"] = lambda dt=dt: F.s10_inputs(dt)
    for dt, dim in F.S11_SHAPES:
        out[f"s11_{dt}d{dim}"] = lambda dt=dt, dim=dim: F.s11_inputs(dt, dim)
    for dt, dim in F.S12_SHAPES:
        out[f"s12_{dt}d{dim}"] = lambda dt=dt, dim=dim: F.s12_inputs(dt, dim)
    for dt, dim in F.S13_SHAPES:
        out[f"s13_{dt}d{dim}"] = lambda dt=dt, dim=dim: F.ms_inputs("s13", dt, dim)
    for case, (dt, dim, _) in F.S14_CASES.items():
        out[f"s14_{case}"] = lambda dt=dt, dim=dim: F.ms_inputs("s14", dt, dim)
    for dt, dim in F.S15_SHAPES:
        out[f"s15_{dt}d{dim}"] = lambda dt=dt, dim=dim: F.s15_inputs(dt, dim)
    return out


def test_every_scenario_has_an_expectation():
    names = list(F.scenarios())
    assert len(set(names)) == len(names)
    for name in names:
        assert name.split("_")[0] in T.EXPECT, name
    assert {n.split("_")[0] for n in names} == set(T.EXPECT), "an expectation no scenario uses"
    for fam in ("s11", "s12", "s13", "s14", "s15", "s16", "s17"):
        assert any(n.split("_")[0] == fam for n in names), fam
    assert {"s17_cpp", "s17_mixed"} <= set(names)
    assert all(isinstance(v, bool) for v in F.scenarios().values())


def test_inputs_are_the_same_in_two_constructions():
    for name, build in _builders().items():
        _same(build(), build(), name)
    for calls in (F.s11_calls, F.s12_calls, F.ms_calls):
        assert list(calls()) == list(calls())
        keys = [c[0] for c in calls()]
        assert len(set(keys)) == len(keys), "two calls under one name"


def test_the_layout_holds_every_kind_of_key():
    lay = F.fi_layout()
    keys, counts = P.group_by(lay)
    assert keys.size == len(F.FI_SIZES) + F.FI_FURTHER == 27
    assert [int(counts[keys == np.uint64(g)][0]) for g in lay["keys"]] == list(F.FI_SIZES), "a key of 300 rows .. a key of one"
    assert int(counts.min()) == 1 and int(counts.max()) == 300
    assert (lay["col"] == lay["dead_key"]).any() and P.reference_rows(lay, lay["dead_key"]).size == 0, "a key that is wholly deleted"
    assert not (lay["col"] == lay["absent_key"]).any(), "an absent key"
    assert lay["dead"].sum() > 0 and keys.size == MS.key_order(lay)[3].size


def test_s11_asks_below_and_above_every_keys_rows():
    for dt, dim in F.S11_SHAPES:
        inp = F.s11_inputs(dt, dim)
        held = [P.reference_rows(inp["lay"], key).size for key in inp["keys"]]
        assert held == [300, 1, 0, 0, 2]
        assert min(F.S11_KS) < max(held) < max(F.S11_KS), "k below and above the largest key asked for"
        assert min(F.S11_KS) > 1, "k above the key of one row"


def test_s12_k_above_exceeds_what_the_caps_give():
    _, counts = P.group_by(F.fi_layout())
    for per_key in F.S12_PER_KEYS:
        gives = int(np.minimum(counts, np.uint64(per_key)).sum())
        assert min(F.S12_KS) < gives < max(F.S12_KS), f"per_key {per_key}: {gives} rows at most"
    assert {nq for *_, nq in F.s12_calls()} == {1, F.S12_NQ}


def test_the_multi_vector_cases_ask_below_and_above_the_keys():
    nk = P.group_by(F.fi_layout())[0].size
    assert min(F.MS_KS) < nk < max(F.MS_KS)
    assert F.MS_TS == (3, 33) and 33 % MS.TOKEN_GROUP == 1, "T = 33 ends in a short token group"
    assert set(F.MS_NQS) == {1, 3} and F.MS_POOL == (max(F.MS_NQS), max(F.MS_TS))
    assert {(dt, m) for dt, _, m in F.S14_CASES.values()} == {("f32", F.IP), ("f16", F.COS)}


def _clear_share(inp, metrics, k):
    """the share of (metric, T, set) cases whose float64 k-th and (k + 1)-th sums lie further apart than the contract's band"""
    nq, pool_T, dim = inp["pool"].shape
    f64 = MS.f64_key_bests(inp["rows"], inp["lay"], inp["pool"].reshape(nq * pool_T, dim), TOL)
    clear = total = 0
    for metric in metrics:
        b, tol = f64[metric]
        for T_ in F.MS_TS:
            for j in range(nq):
                sl = slice(j * pool_T, j * pool_T + T_)
                S, t = b[sl].sum(0), tol[sl].sum(0)
                key = np.sort((1.0 if metric == F.L2 else -1.0) * S)
                total += 1
                clear += bool(key[k] - key[k - 1] > 2 * t.max())
    return clear / total


def test_the_float_worlds_decide_their_kth_key():
    """S13, S14: the gap between the k-th and the (k + 1)-th float64 sum exceeds the contract's band (twice the largest
    tolerance) for at least 90 % of the query sets, so the contract pins the keys and not only the sums"""
    k = min(F.MS_KS)
    for dt, dim in F.S13_SHAPES:
        if dt not in T.INT:
            share = _clear_share(F.ms_inputs("s13", dt, dim), F.METRICS, k)
            assert share >= 0.9, f"s13 {dt} x {dim}: {share:.2f}"
    for case, (dt, dim, metric) in F.S14_CASES.items():
        share = _clear_share(F.ms_inputs("s14", dt, dim), (metric,), k)
        assert share >= 0.9, f"s14 {case}: {share:.2f}"


def test_s15_lists_keep_some_keys_and_end_at_the_block_edges():
    for dt, dim in F.S15_SHAPES:
        inp = F.s15_inputs(dt, dim)
        held, mine = T.s15_held(inp)
        counts = dict(zip(held.tolist(), P.group_by(inp["lay"])[1].tolist()))
        assert len(mine) == F.S15_MIXED + 2 == inp["sets"].shape[0] and inp["lists"].shape == (len(mine), F.S15_M)
        for j, m in enumerate(mine):
            assert 1 <= m.size < F.S15_M, f"list {j} keeps {m.size} keys"
            assert max(F.S15_KS) > m.size, "k above exceeds the held count"
        rows = [sum(counts[int(g)] for g in m) for m in mine]
        assert rows[-2:] == [MC.BLOCK, MC.BLOCK + 1], rows
        assert all(m.size >= 2 for m in mine[-2:]), "the edge lists hold several keys"
        lists = inp["lists"]
        assert (lists == F.PAD).any() and (lists == np.uint64(inp["lay"]["dead_key"])).any() and (lists == np.uint64(inp["lay"]["absent_key"])).any()
        assert any(np.unique(l[l != F.PAD]).size < (l != F.PAD).sum() for l in lists), "a repeat"
        assert len({m.size for m in mine[:F.S15_MIXED]}) > 1, "the mixed lists differ in their held counts"


def test_s16_is_the_planted_world_cut_down():
    inp = F.s16_inputs()
    assert inp["rows"].shape == (F.S16_N, F.S16_DIM) and F.S16_N <= 3000 and inp["lists"].shape == (2, F.S16_M) and F.S16_M == 64
    assert inp["copies"].size == 8 and np.isin(inp["copies"], inp["lists"][0]).all()
    assert (inp["rows"][inp["copies"].astype(np.int64)] == inp["rows"][int(inp["copies"][0])]).all(), "the copies are one row"
    second = inp["lists"][1]
    assert (second == F.PAD).any() and (second[second != F.PAD] >= F.S16_N).any(), "pads and rows behind the corpus"
    assert set(F.S16_LAMBDAS) == {0.5, 1.0}


def test_s17_is_the_documents_example():
    inp = F.s17_inputs()
    rng = np.random.default_rng(21)   # tests/test_gpu_maxsim_candidates_cpp.py's lines
    rows = rng.standard_normal((600, 8)).astype(np.float32)
    doc = rng.integers(0, 30, 600).astype(np.uint64) * np.uint64(1000003)
    assert (inp["rows"] == rows).all() and (inp["doc"] == doc).all() and (inp["query"] == rows[:3]).all()
    assert (F.S17_T, F.S17_K) == (3, 6)
    docs, S, tol, held = T.s17_reference()
    assert docs.size == F.S17_DOCS == 30 and held.size == 5, "4, 9, 0, 13, 21 hold rows; 77 and the pad do not"
    assert sorted((held // np.uint64(F.S17_UNIT)).tolist()) == [0, 4, 9, 13, 21]
    assert F.S17_K > held.size and F.S17_DOCS + 2 > docs.size, "k above the candidates, and above the documents"
    assert F.S17_STEPS["cpp"] == ("full", "cand", "empty"), "examples/cpp/rerank_documents.cpp's order"
    assert F.S17_STEPS["mixed"] == ("cand", "perkey", "grouped", "full", "cand")
    key = np.sort(S)   # the float64 sums decide the order of the documents the example prints
    assert (np.diff(key)[:F.S17_K] > 2 * tol.max()).all() and (np.diff(np.sort(S[np.searchsorted(docs, held)])) > 2 * tol.max()).all()
