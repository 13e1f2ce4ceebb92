"""MaxSim alignments, CPU tier (DESIGN.md §3 "Alignments"): the library exports every symbol of include/mvf_gpu_maxsim_align.h
and the layers above name them, every refusal precedes any device call in the stated order and wording, the scratch plan is the
pure function the header states, and the numpy reference the GPU tests lean on (tests/_maxsim_align.py) answers a hand-made
world of three keys as the contract says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import gpu as G

import _maxsim as MS
import _maxsim_align as MA
import _partitioned as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT


def _msg():
    return _lib.gpu().mvfgpu_last_error_message().decode()


def test_every_symbol_of_the_header_is_exported_and_named_by_the_layers_above():
    header = open(os.path.join(ROOT, "include", "mvf_gpu_maxsim_align.h")).read()
    declared = sorted(set(re.findall(r"^int (mvfgpu_\w+)\(", header, re.M)))
    assert declared == ["mvfgpu_maxsim_align", "mvfgpu_maxsim_align_device", "mvfgpu_selftest_maxsim_align_plan",
                        "mvfgpu_selftest_maxsim_align_stage_ms"]
    lib = _lib.gpu()
    for name in declared:
        assert hasattr(lib, name), name
    for name in ("maxsim_align", "maxsim_align_device", "maxsim_align_stage_ms"):
        assert hasattr(G.GpuCorpus, name), name
    assert hasattr(G, "maxsim_align_plan") and hasattr(G, "MaxSimAlignment")
    assert "align_documents" in M.__all__ and hasattr(M, "align_documents")
    hpp = open(os.path.join(ROOT, "include", "mvf.hpp")).read()
    assert "align_documents" in hpp and "mvfgpu_maxsim_align(" in hpp
    assert lib.mvfgpu_abi_version() == 3, "an additive change: the ABI version stays"
    assert "the arg-best rows" not in open(os.path.join(ROOT, "include", "mvf_gpu.h")).read()


_ONE = np.zeros(4, np.uint64)
_P1 = _ONE.ctypes.data_as(C.c_void_p)
_FAKE = C.c_void_p(16)  # a partition that is never dereferenced: `corpus is NULL` is found first


@pytest.mark.parametrize("entry", ["host", "device", "timer"])
def test_refusal_precedence_without_a_handle(entry):
    """corpus = NULL and every other argument bad as well: mvfgpu_search_maxsim_candidates' ladder as with k = 1 -- no k step --,
    the list's message naming `keys` -- code and message at every step"""
    lib = _lib.gpu()
    fn = {"host": lib.mvfgpu_maxsim_align, "device": lib.mvfgpu_maxsim_align_device, "timer": lib.mvfgpu_selftest_maxsim_align_stage_ms}[entry]
    tail = {"host": [], "device": [None], "timer": [None, _P1]}[entry]

    def call(a):
        return fn(None, a["part"], a["metric"], a["q"], 0, 4, a["nq"], a["n_tokens"], a["keys"], a["m"], a["sc"], a["rows"], None, *tail)

    state = dict(metric=9, nq=0, q=None, sc=None, rows=None, n_tokens=0, keys=None, m=3, part=None)
    ladder = [("unsupported distance metric code 9", dict(metric=0)), ("nq must be > 0", dict(nq=1)), ("NULL buffer", dict(q=_P1)),
              ("NULL buffer", dict(sc=_P1)), ("NULL buffer", dict(rows=_P1)), ("n_tokens must be in 1..1024, got 0", dict(n_tokens=1025)),
              ("n_tokens must be in 1..1024, got 1025", dict(n_tokens=1024)), ("NULL buffer (keys)", dict(keys=_P1)),
              ("partition is NULL", dict(part=_FAKE))]
    for message, fix in ladder:
        assert call(state) == INV and _msg() == message, (message, _msg())
        state = {**state, **fix}
    assert call(state) == INV and _msg() == "corpus is NULL", _msg()
    state.update(keys=None, m=0, part=None)
    assert call(state) == INV and _msg() == "partition is NULL", "m = 0: a NULL list is no refusal"
    if entry == "timer":
        assert fn(None, None, 9, None, 0, 4, 0, 0, None, 3, None, None, None, None, None) == INV and _msg() == "NULL buffer", "out_ms first"


def test_the_handle_checks_come_behind_the_partition_and_a_well_formed_call_reaches_the_device():
    """with a handle: the query's type and dimension are refused behind `partition is NULL`; where no GPU is present the handle
    cannot be made and this is the ladder's end"""
    try:
        c = G.GpuCorpus.from_array(P.make_rows(64, 8, "f32"))
    except M.MvfError:
        return  # no device: a handle needs one; the GPU tier runs the well-formed calls
    with c:
        q = P.make_queries(2, 8, "f32")
        sc, rows = np.zeros(8, np.float32), np.zeros(8, np.uint64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = _lib.gpu().mvfgpu_maxsim_align(c._h, None, 0, vp(q), 0, 7, 1, 2, _P1, 1, vp(sc), vp(rows), None)
        assert rc == INV and _msg() == "partition is NULL"


GRID = [(nk, T, nq, tb, budget)
        for nk in (0, 1, 7, 1000, 100_000)
        for T in (1, 3, 4, 5, 32, 33, 1024)
        for nq in (1, 3, 2000)
        for tb in (0, 16, 512, 3072, 40 * 1024, 40 * 1024 + 16)
        for budget in (1, 8 * 4 - 1, 8 * 4 * 1000 - 1, 8 * 4 * 1000, 1 << 20, 512 << 20, 1 << 40)]


def test_the_plan_is_the_headers_rule_over_a_grid():
    small = 0
    for nk, T, nq, tb, budget in GRID:
        got, want = G.maxsim_align_plan(nk, T, nq, tb, budget), MA.plan(nk, T, nq, tb, budget)
        assert got == want, ((nk, T, nq, tb, budget), got, want)
        chunk, window = got
        assert 1 <= chunk <= min(T, MS.CHUNK_MAX) and 1 <= window <= min(nq, MS.WINDOW_MAX)
        if tb and tb <= MS.LDS_TOKEN_BYTES:
            assert chunk * tb <= MS.LDS_TOKEN_BYTES, "the chunk's tokens fit 40 KiB of LDS"
        group = min(T, MS.TOKEN_GROUP, MS.LDS_TOKEN_BYTES // tb if tb and tb <= MS.LDS_TOKEN_BYTES else MS.CHUNK_MAX)
        one_group = max(nk, 1) * group * MA.MIN_BYTES
        if one_group > budget:   # a budget smaller than one token group's scratch: one set, the least chunk, whatever the budget
            small += 1
            assert (chunk, window) == (group, 1)
        else:
            assert window * max(nk, 1) * chunk * MA.MIN_BYTES <= budget, "inside the budget wherever one set with one group fits"
    assert small > 100
    assert G.maxsim_align_plan(1000, 32, 64, 512, 512 << 20) == (32, 64)
    assert G.maxsim_align_plan(1000, 32, 3, 512, 1000 * 8 * 8) == (8, 1) and G.maxsim_align_plan(1000, 32, 3, 512, 2 * 1000 * 8 * 8) == (16, 1)
    lib = _lib.gpu()
    out = C.c_uint32(0)
    assert lib.mvfgpu_selftest_maxsim_align_plan(1, 1, 1, 0, 1, None, C.byref(out)) == INV and _msg() == "NULL buffer"
    assert lib.mvfgpu_selftest_maxsim_align_plan(1, 0, 1, 0, 1, C.byref(out), C.byref(out)) == INV and _msg() == "n_tokens must be in 1..1024, got 0"
    assert lib.mvfgpu_selftest_maxsim_align_plan(1, 1, 0, 0, 1, C.byref(out), C.byref(out)) == INV and _msg() == "empty batch or budget"


def test_the_numpy_reference_on_a_hand_made_world_of_three_keys():
    """rows 0 .. 6 at positions 10 .. 16; key 5: rows 0, 2, 3; key 9: rows 1, 4; key 7: row 5, all NaN; row 6's key 11 is listed
    nowhere.  Two tokens under InnerProduct (larger is better)"""
    nan = np.float32(np.nan)
    row_keys = np.array([5, 9, 5, 5, 9, 7, 11], np.uint64)
    names = np.arange(10, 17).astype(np.uint64)
    s = np.array([[1.0, -0.0, 3.0, 3.0, 0.0, nan, 8.0],     # token 0: key 5 ties at rows 2 and 3; key 9: -0.0 == +0.0, row 1 first
                  [nan, 2.0, -1.0, nan, 2.5, nan, 8.0]], np.float32)   # token 1: a NaN never beats a number
    raw = np.arange(14, dtype=np.int32).reshape(2, 7)
    keys = np.array([9, 5, 4, 7, 5, int(P.PAD)], np.uint64)   # 4 is unknown, 5 is listed twice, then the pad
    rows, sc, rw = MA.by_contract(s, row_keys, names, keys, 1, raw)
    assert rows.tolist() == [[11, 14], [12, 12], [int(P.PAD)] * 2, [15, 15], [12, 12], [int(P.PAD)] * 2]
    assert sc[0].tolist() == [0.0, 2.5] and not np.signbit(sc[0, 0]), "+0.0 stands for +-0.0"
    assert sc[1].tolist() == [3.0, -1.0] and (sc[4].view(np.uint32) == sc[1].view(np.uint32)).all(), "a repeat gets the same answer"
    assert np.isneginf(sc[2]).all() and np.isneginf(sc[5]).all() and (rw[2] == 0).all(), "padding for what is not held"
    assert (sc[3].view(np.uint32) == MS.NAN_BITS).all(), "every row NaN: the lowest position, the results' NaN"
    assert rw.tolist() == [[1, 11], [2, 9], [0, 0], [5, 12], [2, 9], [0, 0]]
    # L2: smaller is better, the padding is +inf
    rows2, sc2, _ = MA.by_contract(np.abs(s), row_keys, names, keys, 0)
    assert rows2[:2].tolist() == [[11, 11], [10, 12]] and np.isposinf(sc2[2]).all()
    # identity 2's sum: plain f32 in token order
    assert MA.token_sum(sc)[:2].tolist() == [2.5, 2.0] and np.isnan(MA.token_sum(sc)[3])
    q, k = MA.partitioned_pairs(np.arange(12, dtype=np.float32).reshape(2, 3, 2), np.array([[1, 2], [3, 4]], np.uint64))
    assert k.tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4] and q[3:6].tolist() == q[:3].tolist() and q[6].tolist() == [6.0, 7.0]
