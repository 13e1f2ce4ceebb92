"""Candidate search, CPU tier: the C ABI entry points and the Python methods exist, refuse bad arguments before any
device call, the Python layer refuses malformed candidate arrays, and the oracle restatement of the semantics
(tests/_candidates.py) is pinned on hand-made lists -- including that row-range shards given the same global lists merge
into the whole."""
import ctypes as C

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

from _candidates import PAD, candidate_rows, oracle_candidates

INV, BUILD, DIM = 12, 10, 6  # MVF_ERR_INVALID_ARGUMENT, MVF_ERR_BUILD, MVF_ERR_DIMENSION_MISMATCH


def _call(device=False, corpus=None, metric=0, q=True, qdtype=0, qdim=4, nq=1, cand=True, m=3, k=2, sc=True, idx=True):
    qa = np.zeros(qdim * max(nq, 1), np.float32)
    ca = np.zeros(max(nq * m, 1), np.uint64)
    s = np.zeros(max(nq * k, 1), np.float32)
    i = np.zeros(max(nq * k, 1), np.uint64)
    cnt = np.zeros(max(nq, 1), np.uint64)
    p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    if device:
        rc = lib.mvfgpu_search_candidates_device(corpus, metric, p(qa, q), qdtype, qdim, nq, p(ca, cand), m, k, p(s, sc),
                                                 p(i, idx), None, p(cnt, True), None)
    else:
        rc = lib.mvfgpu_search_candidates(corpus, metric, p(qa, q), qdtype, qdim, nq, p(ca, cand), m, k, p(s, sc), p(i, idx),
                                          None, p(cnt, True))
    return rc, lib.mvfgpu_last_error_message().decode()


def test_entry_points_are_exported():
    lib = _lib.gpu()
    assert hasattr(lib, "mvfgpu_search_candidates") and hasattr(lib, "mvfgpu_search_candidates_device")
    assert hasattr(G.GpuCorpus, "search_candidates") and hasattr(G.GpuCorpus, "search_candidates_device")
    assert callable(M.rerank_top_k) and "rerank_top_k" in M.__all__


@pytest.mark.parametrize("device", [False, True])
def test_refusals_precede_any_device_call(device):
    rc, msg = _call(device, corpus=None)
    assert rc == INV and "corpus is NULL" in msg
    rc, msg = _call(device, metric=7)
    assert rc == INV and "metric" in msg
    rc, msg = _call(device, nq=0)
    assert rc == INV and "nq" in msg
    rc, msg = _call(device, k=0)
    assert rc == INV and "k must be" in msg
    rc, msg = _call(device, k=2**31 + 1)
    assert rc == INV and "k must be" in msg
    rc, msg = _call(device, q=False)
    assert rc == INV and "NULL" in msg
    rc, msg = _call(device, sc=False)
    assert rc == INV and "NULL" in msg
    rc, msg = _call(device, idx=False)
    assert rc == INV and "NULL" in msg
    rc, msg = _call(device, cand=False)
    assert rc == INV and "candidates" in msg
    rc, msg = _call(device, cand=False, m=0)  # nothing listed: no list needed -> the handle check refuses next
    assert rc == INV and "corpus is NULL" in msg


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_refusals_on_a_live_handle(device):
    """The arguments that need the handle are checked as mvfgpu_search checks them."""
    rows = np.zeros((8, 4), np.float32)
    with G.GpuCorpus.from_array(rows) as c:
        rc, msg = _call(device, corpus=c._h, qdtype=G.INT8)
        assert rc == BUILD and "query data type" in msg
        rc, msg = _call(device, corpus=c._h, qdim=5)
        assert rc == DIM and "Dimension mismatch" in msg


def test_python_layer_refuses_malformed_candidate_arrays():
    c = G.GpuCorpus(0)  # a NULL handle: nothing may reach the device
    c._h = C.c_void_p(None)
    q = np.zeros((2, 4), np.float32)
    for bad in (np.zeros(6, np.uint64),                       # 1-D
                np.zeros((2, 3), np.int64),                   # signed
                np.zeros((2, 3), np.float64),                 # not integers
                np.zeros((2, 3, 1), np.uint64),               # 3-D
                np.zeros((3, 3), np.uint64),                  # one list per query
                [[1, 2, 3], [4, 5, 6]]):                      # a list of lists
        with pytest.raises(E.InvalidArgument):
            c.search_candidates(q, bad, 2)


def test_candidate_rows_rule():
    n, base = 10, 100
    dead = np.zeros(n, bool)
    dead[4] = True
    ent = np.array([103, 103, PAD, 7, 110, 99, 104, 101, 109, 2**63], np.uint64)
    assert candidate_rows(ent, n, index_base=base, dead=dead).tolist() == [1, 3, 9]
    ids = np.array([50, 51, 52, 51, 54, 55, 56, 57, 58, 59], np.uint64)  # id 51 twice: the first row holds it
    ent = np.array([51, 51, 59, 60, PAD, 54, 3], np.uint64)
    assert candidate_rows(ent, n, ids=ids, dead=dead).tolist() == [1, 9]


@pytest.mark.parametrize("dtype", [G.FLOAT32, G.INT8])
@pytest.mark.parametrize("metric", [G.L2, G.INNER_PRODUCT, G.COSINE])
def test_oracle_restatement_on_hand_made_lists(oracle, dtype, metric):
    n, dim = 12, 5
    rows = oracle.synth_rows(7, 0, n, dim, dtype)
    if dtype == G.FLOAT32:
        rows[6, 2] = np.nan  # a NaN row ranks last among the candidates
    q = oracle.synth_queries(8, 1, dim, dtype)[0]
    sc, keys, raw = oracle.scores(rows, dtype, metric, q)
    dead = np.zeros(n, bool)
    dead[5] = True
    ent = np.array([6, 3, 3, 11, PAD, 5, 40, 0, 3, PAD], np.uint64)
    k = 8  # more than the four distinct live candidates: padding
    cnt, S, I, R = oracle_candidates(oracle, rows, dtype, metric, q, ent, k, dead=dead)
    assert cnt == 4
    live = np.array([0, 3, 6, 11])
    order = live[np.lexsort((live, keys[live]))]
    assert I[:4].tolist() == order.tolist() and (I[4:] == PAD).all()
    assert (S[:4].view(np.uint32) == sc[order].view(np.uint32)).all() and (R[:4] == raw[order]).all()
    assert (S[4:] == (np.inf if metric == G.L2 else -np.inf)).all() and (R[4:] == 0).all()
    if dtype == G.FLOAT32 and metric != G.COSINE:  # (cosine scores a NaN row 0: its denominator is not > 0)
        assert I[3] == 6 and np.isnan(S[3]), "the NaN row ranks last"
    # a list of every row reproduces the oracle's top-k search
    every = np.random.default_rng(1).permutation(n).astype(np.uint64)
    osc, oidx, oraw = oracle.search(rows, dtype, metric, q, k)
    cnt, S, I, R = oracle_candidates(oracle, rows, dtype, metric, q, every, k)
    assert cnt == n and (I == oidx[0]).all() and (R == oraw[0]).all()
    assert (S.view(np.uint32) == osc[0].view(np.uint32)).all()
    # ids: entries are ids, results report ids
    ids = (np.arange(n, dtype=np.uint64) * 3 + 1000)
    cnt, S, I, R = oracle_candidates(oracle, rows, dtype, metric, q, np.array([1000 + 9, 1003, 999, PAD], np.uint64), k, ids=ids)
    assert cnt == 2 and sorted(I[:2].tolist()) == [1003, 1009]


@pytest.mark.parametrize("dtype", [G.FLOAT32, G.UINT8])
@pytest.mark.parametrize("metric", [G.L2, G.COSINE])
def test_shards_given_the_same_lists_merge_into_the_whole(oracle, dtype, metric):
    n, dim, nq, m, k = 30, 6, 4, 25, 7
    rows = oracle.synth_rows(11, 0, n, dim, dtype)
    qs = oracle.synth_queries(12, nq, dim, dtype)
    rng = np.random.default_rng(3)
    lists = rng.integers(0, n + 5, size=(nq, m)).astype(np.uint64)
    lists[:, -3:] = PAD
    lists[1, :] = PAD  # one query with nothing listed
    whole = [oracle_candidates(oracle, rows, dtype, metric, qs[j], lists[j], k) for j in range(nq)]
    cuts = [0, 9, 20, n]
    per = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        per.append([oracle_candidates(oracle, rows[a:b], dtype, metric, qs[j], lists[j], k, index_base=a) for j in range(nq)])
    for j in range(nq):
        assert sum(p[j][0] for p in per) == whole[j][0], "counts add up across shards"
    S = np.array([[p[j][1] for j in range(nq)] for p in per])
    I = np.array([[p[j][2] for j in range(nq)] for p in per])
    R = np.array([[p[j][3] for j in range(nq)] for p in per])
    merged = G.merge_topk_host(S, I, R, metric, dtype)
    for j in range(nq):
        assert (merged.indices[j] == whole[j][2]).all()
        assert (merged.scores[j].view(np.uint32) == whole[j][1].view(np.uint32)).all()
        assert (merged.raw[j] == whole[j][3]).all()
