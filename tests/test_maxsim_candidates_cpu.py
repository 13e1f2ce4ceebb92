"""Candidate multi-vector search, CPU tier (DESIGN.md §3 "Candidate keys"): the library exports the new entry points and Python
names them, every refusal that needs no handle precedes any device call in the stated order, the host plan of one list is the
pure function the header states -- the first occurrence of every held key, slots ascending by key value --, and the filter the
GPU tests compare with (tests/_maxsim_candidates.py) is identity 1 on the contract's dict reference."""
import ctypes as C
import os

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

import _maxsim as MS
import _maxsim_candidates as MC
import _partitioned as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT


def _msg():
    return _lib.gpu().mvfgpu_last_error_message().decode()


def test_entry_points_and_python_names_exist():
    lib = _lib.gpu()
    for name in ("mvfgpu_search_maxsim_candidates", "mvfgpu_search_maxsim_candidates_device", "mvfgpu_selftest_maxsim_candidates_plan",
                 "mvfgpu_selftest_maxsim_candidates_stage_ms"):
        assert hasattr(lib, name), name
    for name in ("search_maxsim_candidates", "search_maxsim_candidates_device", "maxsim_candidates_stage_ms"):
        assert hasattr(G.GpuCorpus, name), name
    assert hasattr(G, "maxsim_candidates_plan")
    assert "rerank_top_k_documents" in M.__all__ and hasattr(M, "rerank_top_k_documents")
    hpp = open(os.path.join(ROOT, "include", "mvf.hpp")).read()
    assert "rerank_top_k_documents" in hpp and "mvfgpu_search_maxsim_candidates" in hpp
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "fn mvfgpu_search_maxsim_candidates(" in rust and "fn mvfgpu_search_maxsim_candidates_device(" in rust
    assert lib.mvfgpu_abi_version() == 3, "an additive change: the ABI version stays"


_ONE = np.zeros(4, np.uint64)
_P1 = _ONE.ctypes.data_as(C.c_void_p)
_FAKE = C.c_void_p(16)  # a partition that is never dereferenced: `corpus is NULL` is found first


@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
def test_refusal_precedence_without_a_handle(device):
    """corpus = NULL and every other argument bad as well: mvfgpu_search_maxsim's ladder up to n_tokens, then the NULL list
    while nq * m > 0, then the partition and `corpus is NULL` -- code and message at every step"""
    fn = getattr(_lib.gpu(), "mvfgpu_search_maxsim_candidates" + ("_device" if device else ""))

    def call(a):
        return fn(None, a["part"], a["metric"], a["q"], 0, 4, a["nq"], a["n_tokens"], a["cand"], a["m"], a["k"], a["sc"], a["keys"], None,
                  *[None] * device)

    state = dict(metric=9, nq=0, k=0, q=None, sc=None, keys=None, n_tokens=0, cand=None, m=3, part=None)
    ladder = [("unsupported distance metric code 9", dict(metric=0)), ("nq must be > 0", dict(nq=1)),
              ("k must be in 1..2^31", dict(k=1)), ("NULL buffer", dict(q=_P1)), ("NULL buffer", dict(sc=_P1)),
              ("NULL buffer", dict(keys=_P1)), ("n_tokens must be in 1..1024, got 0", dict(n_tokens=1025)),
              ("n_tokens must be in 1..1024, got 1025", dict(n_tokens=1024)), ("NULL buffer (candidate_keys)", dict(cand=_P1)),
              ("partition is NULL", dict(part=_FAKE))]
    for message, fix in ladder:
        assert call(state) == INV and _msg() == message, (message, _msg())
        state = {**state, **fix}
    assert call(state) == INV and _msg() == "corpus is NULL", _msg()
    state.update(cand=None, m=0, part=None)
    assert call(state) == INV and _msg() == "partition is NULL", "m = 0: a NULL list is no refusal"


def test_the_stage_timer_and_the_plan_refuse_before_any_device_call():
    lib = _lib.gpu()
    timer = lib.mvfgpu_selftest_maxsim_candidates_stage_ms
    assert timer(None, None, 0, _P1, 0, 4, 1, 1, _P1, 1, 1, _P1, _P1, None, None) == INV and _msg() == "NULL buffer"
    assert timer(None, None, 0, _P1, 0, 4, 1, 0, _P1, 1, 1, _P1, _P1, None, _P1) == INV and "n_tokens" in _msg()
    assert timer(None, None, 0, _P1, 0, 4, 1, 1, None, 1, 1, _P1, _P1, None, _P1) == INV and _msg() == "NULL buffer (candidate_keys)"
    assert timer(None, _FAKE, 0, _P1, 0, 4, 1, 1, _P1, 1, 1, _P1, _P1, None, _P1) == INV and _msg() == "corpus is NULL"
    plan = lib.mvfgpu_selftest_maxsim_candidates_plan
    assert plan(_P1, _P1, 1, _P1, None, _P1) == INV and _msg() == "NULL buffer"
    assert plan(_P1, _P1, 1, _P1, _P1, None) == INV and _msg() == "NULL buffer"
    assert plan(None, _P1, 1, _P1, _P1, _P1) == INV and plan(_P1, None, 1, _P1, _P1, _P1) == INV and plan(_P1, _P1, 1, None, _P1, _P1) == INV
    with pytest.raises(E.InvalidArgument, match="one entry per candidate"):
        G.maxsim_candidates_plan(np.zeros(3, np.uint64), np.zeros(2, np.uint64))


@pytest.mark.parametrize("m", [0, 1, 2, 1000])
def test_the_plan_of_one_list_is_the_first_occurrence_ranked_by_key_value(m):
    for trial in range(6):
        rng = np.random.default_rng(P._seed("cand plan", m, trial))
        pool = rng.integers(0, 1 << 64, max(m // 3, 2), dtype=np.uint64)   # a third as many values: repeats near and far
        pool[0] = MC.PAD
        cand = rng.choice(pool, m) if m else np.zeros(0, np.uint64)
        held_of = {int(v): int(rng.integers(0, 4)) * int(rng.integers(1, 500)) for v in pool}   # a quarter of the values is not held
        if trial == 0:
            held_of = {v: 0 for v in held_of}                              # a list of skipped entries only
        held = np.array([held_of[int(v)] for v in cand], np.uint64)
        slot, distinct, rows = G.maxsim_candidates_plan(cand, held)
        want = MC.plan_reference(cand, held)
        assert (slot == want[0]).all() and (distinct, rows) == want[1:], (m, trial)
        taken = np.nonzero(slot != MC.SKIPPED)[0]
        assert distinct == taken.size == np.unique(cand[held > 0]).size
        assert sorted(slot[taken].tolist()) == list(range(distinct)), "the slots are the ranks 0 .. distinct - 1"
        by_slot = cand[taken][np.argsort(slot[taken])]
        assert (by_slot[1:] > by_slot[:-1]).all(), "ascending slot is ascending key value"
        for i in taken:
            assert not (cand[:i] == cand[i]).any(), "the first occurrence wins"
        assert rows == sum(held_of[int(v)] for v in np.unique(cand)), "every distinct held key's rows once"
    if m == 2:
        slot, distinct, rows = G.maxsim_candidates_plan(np.array([9, 9], np.uint64), np.array([5, 5], np.uint64))
        assert slot.tolist() == [0, int(MC.SKIPPED)] and (distinct, rows) == (1, 5)
        slot, distinct, rows = G.maxsim_candidates_plan(np.array([9, 3], np.uint64), np.array([5, 7], np.uint64))
        assert slot.tolist() == [1, 0] and (distinct, rows) == (2, 12)


def _synthetic(seed, m, n_keys, T):
    rng = np.random.default_rng(seed)
    row_keys = rng.integers(0, n_keys, m).astype(np.uint64) * np.uint64((1 << 33) + 5)
    s = (np.round(rng.standard_normal((T, m)) * 2) / 2).astype(np.float32)   # a coarse grid: many tied sums
    s[rng.random((T, m)) < 0.02] = np.nan
    return s, row_keys


@pytest.mark.parametrize("metric", [0, 1])
def test_identity_1_on_the_dict_reference(metric):
    """the contract's reference over the candidates' rows alone is the filter of its full row: what filter_full states"""
    for trial in range(4):
        s, row_keys = _synthetic(P._seed("cand identity", trial), 500, 40, 5)
        held = np.unique(row_keys)
        full = MS.by_dict(s, row_keys, metric, held.size + 2)
        lists = MC.mixed_lists(held, 3, 25, [7, int(MC.PAD)], trial)
        for k in (1, 10, 25, 30):
            sc, ky, cnt = MC.filter_full(full[0][None].repeat(3, 0), full[1][None].repeat(3, 0), held.size, lists, held, k, metric)
            for q in range(3):
                mine = MC.held_distinct(lists[q], held)
                rows = np.isin(row_keys, mine)
                want = MS.by_dict(s[:, rows], row_keys[rows], metric, k)
                assert cnt[q] == want[2] == min(k, mine.size)
                assert (ky[q] == want[1]).all() and (MS.canonical(sc[q]).view(np.uint32) == want[0].view(np.uint32)).all(), (trial, k, q)
        assert len({MC.held_distinct(l, held).size for l in lists}) == 3, "a different number of held candidates per set"
