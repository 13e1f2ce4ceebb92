"""Multi-vector search, CPU tier (DESIGN.md §3 "Multi-vector search"): the library exports the new entry points and Python names
them, every refusal that needs no handle precedes any device call and names its cause in the stated order, the scratch plan is
the pure function the header states, and the numpy reference (tests/_maxsim.py) is the contract's loop: it agrees with its
vectorised form on the GPU tests' layouts and tells three wrong models from the contract."""
import ctypes as C
import os

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

import _grouped as GR
import _maxsim as MS
import _partitioned as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT
LAYOUTS = {"stock": GR.stock, "caps": GR.caps, "dominant": GR.dominant, "own_keys": GR.own_keys, "one_key": GR.one_key,
           "all_dead": GR.all_dead}


def _msg():
    return _lib.gpu().mvfgpu_last_error_message().decode()


def test_entry_points_and_python_names_exist():
    lib = _lib.gpu()
    for name in ("mvfgpu_search_maxsim", "mvfgpu_search_maxsim_device", "mvfgpu_selftest_maxsim_plan", "mvfgpu_selftest_maxsim_stage_ms"):
        assert hasattr(lib, name), name
    for name in ("search_maxsim", "search_maxsim_device", "maxsim_stage_ms"):
        assert hasattr(G.GpuCorpus, name), name
    assert hasattr(G, "maxsim_plan") and hasattr(G, "MaxSimResult")
    assert "find_top_k_documents" in M.__all__ and hasattr(M, "find_top_k_documents") and "MaxSimResult" in M.__all__
    hpp = open(os.path.join(ROOT, "include", "mvf.hpp")).read()
    assert "find_top_k_documents" in hpp and "mvfgpu_search_maxsim" in hpp
    header = open(os.path.join(ROOT, "include", "mvf_gpu.h")).read()
    assert "#define MVFGPU_MAXSIM_MAX_TOKENS 1024u" in header
    assert _lib.gpu().mvfgpu_abi_version() == 3, "an additive change: the ABI version stays"


_ONE = np.zeros(4, np.uint64)
_P1 = _ONE.ctypes.data_as(C.c_void_p)
_FAKE = C.c_void_p(16)  # a partition that is never dereferenced: `corpus is NULL` is found first


@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
def test_refusal_precedence_without_a_handle(device):
    """corpus = NULL and every other argument bad as well: the metric is named first, then nq, the range of k, the required
    buffers, n_tokens, the partition, and `corpus is NULL` only once all of them are valid -- code and message at every step"""
    fn = getattr(_lib.gpu(), "mvfgpu_search_maxsim" + ("_device" if device else ""))

    def call(a):
        return fn(None, a["part"], a["metric"], a["q"], 0, 4, a["nq"], a["n_tokens"], a["k"], a["sc"], a["keys"], None, *[None] * device)

    state = dict(metric=9, nq=0, k=0, q=None, sc=None, keys=None, n_tokens=0, part=None)
    ladder = [("unsupported distance metric code 9", dict(metric=0)), ("nq must be > 0", dict(nq=1)),
              ("k must be in 1..2^31", dict(k=1)), ("NULL buffer", dict(q=_P1)), ("NULL buffer", dict(sc=_P1)),
              ("NULL buffer", dict(keys=_P1)), ("n_tokens must be in 1..1024, got 0", dict(n_tokens=1025)),
              ("n_tokens must be in 1..1024, got 1025", dict(n_tokens=1024)), ("partition is NULL", dict(part=_FAKE))]
    for message, fix in ladder:
        assert call(state) == INV and _msg() == message, (message, _msg())
        state = {**state, **fix}
    assert call(state) == INV and _msg() == "corpus is NULL", _msg()
    state["n_tokens"] = 1
    assert call(state) == INV and _msg() == "corpus is NULL", _msg()


def test_the_stage_timer_and_the_plan_refuse_before_any_device_call():
    lib = _lib.gpu()
    assert lib.mvfgpu_selftest_maxsim_stage_ms(None, None, 0, _P1, 0, 4, 1, 1, 1, _P1, _P1, None, None) == INV and _msg() == "NULL buffer"
    assert lib.mvfgpu_selftest_maxsim_stage_ms(None, None, 0, _P1, 0, 4, 1, 0, 1, _P1, _P1, None, _P1) == INV and "n_tokens" in _msg()
    assert lib.mvfgpu_selftest_maxsim_stage_ms(None, _FAKE, 0, _P1, 0, 4, 1, 1, 1, _P1, _P1, None, _P1) == INV and _msg() == "corpus is NULL"
    assert lib.mvfgpu_selftest_maxsim_plan(1, 1, 1, 16, 1 << 20, None, _P1) == INV and _msg() == "NULL buffer"
    assert lib.mvfgpu_selftest_maxsim_plan(1, 1, 1, 16, 1 << 20, _P1, None) == INV and _msg() == "NULL buffer"
    for bad in (0, 1025):
        with pytest.raises(E.InvalidArgument, match="n_tokens must be in 1..1024"):
            G.maxsim_plan(10, bad, 1, 16, 1 << 20)
    with pytest.raises(E.InvalidArgument):
        G.maxsim_plan(10, 4, 0, 16, 1 << 20)
    with pytest.raises(E.InvalidArgument):
        G.maxsim_plan(10, 4, 1, 16, 0)


def test_the_plan_is_the_headers_rule_and_keeps_its_invariants():
    grid = [(nk, T, nq, tb, budget)
            for nk in (0, 1, 7, 1000, 7372, 10_000_000, (1 << 32) - 1)
            for T in (1, 3, 4, 5, 31, 32, 33, 128, 1024)
            for nq in (1, 3, 1024, 5000)
            for tb in (16, 512, 3072, 10240, 40960, 40976, 200_000)
            for budget in (1, 1000, 36 * 7372, 36 * 7372 - 1, 1 << 20, 512 << 20, 1 << 40)]
    for nk, T, nq, tb, budget in grid:
        chunk, window = G.maxsim_plan(nk, T, nq, tb, budget)
        assert (chunk, window) == MS.plan(nk, T, nq, tb, budget), (nk, T, nq, tb, budget)
        assert 1 <= chunk <= min(T, MS.CHUNK_MAX) and 1 <= window <= min(nq, MS.WINDOW_MAX)
        assert -(-T // chunk) * chunk >= T, "the chunks cover every token"
        if tb <= MS.LDS_TOKEN_BYTES:
            assert chunk * tb <= MS.LDS_TOKEN_BYTES, "the chunk's padded tokens fit their share of LDS"
        group = min(T, MS.TOKEN_GROUP, max(1, MS.LDS_TOKEN_BYTES // tb) if tb <= MS.LDS_TOKEN_BYTES else MS.TOKEN_GROUP)
        assert chunk >= group, "at least one token group"
        if max(nk, 1) * (group * 4 + MS.KEY_BYTES) <= budget:  # a one-group chunk fits: the window's scratch does
            assert window * max(nk, 1) * (chunk * 4 + MS.KEY_BYTES) <= budget, (nk, T, nq, tb, budget)
    # the shapes the GPU tests force: T = 33 in at least 3 chunks, nq = 3 in at least 2 windows
    assert G.maxsim_plan(70, 33, 3, 512, 70 * (8 * 4 + 20)) == (8, 1)
    assert G.maxsim_plan(70, 33, 3, 512, 512 << 20) == (32, 3)
    assert G.maxsim_plan(1000, 32, 1, 3072, 512 << 20) == (13, 1), "768 f32 dimensions: 13 padded tokens in 40 KiB"


def _synthetic(seed, m, n_keys, T, nan_share=0.0, step=None):
    rng = np.random.default_rng(seed)
    row_keys = (rng.integers(0, n_keys, m).astype(np.uint64) * np.uint64((1 << 33) + 5))
    s = rng.standard_normal((T, m)).astype(np.float32)
    if step:
        s = (np.round(s / step) * step).astype(np.float32)
    if nan_share:
        s[rng.random((T, m)) < nan_share] = np.nan
    return s, row_keys


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("flavour", ["u32", "u64"])
def test_the_dict_reference_agrees_with_its_vectorised_form_on_the_layouts(layout, flavour):
    lay = LAYOUTS[layout](flavour)
    live = GR.live_rows(lay)
    rng = np.random.default_rng(P._seed("maxsim", layout, flavour))
    T = 3
    s = rng.standard_normal((T, live.size)).astype(np.float32)
    if live.size:
        s[:, ::7] = np.round(s[:, ::7])        # ties, +-0.0
        s[0, ::13] = np.nan                    # NaN rows
        s[1, ::5] = -0.0
    row_keys = lay["col"][live].astype(np.uint64)
    n_keys = np.unique(row_keys).size
    for metric in (0, 1):
        for k in (1, 10, max(n_keys, 1), n_keys + 3):
            a, b = MS.by_dict(s, row_keys, metric, k), MS.vectorised(s, row_keys, metric, k)
            assert a[2] == b[2] == min(k, n_keys)
            assert (a[1] == b[1]).all() and (a[0].view(np.uint32) == b[0].view(np.uint32)).all(), (layout, flavour, metric, k)
            if layout == "own_keys" and k > 10:
                break  # 7372 keys: the two large k are one check


def test_the_reference_tells_three_wrong_models_from_the_contract():
    """each on at least 90 % of 20 query sets of data that can show it: many tokens of unrounded scores (a float64 sum), NaN
    rows inside keys that also hold real rows (a max that prefers NaN), scores on a coarse grid (ties by descending key)"""
    sets = 20
    cases = [("f64 sum", dict(total="f64"), dict(T=33, nan_share=0.0, step=None)),
             ("NaN first", dict(best="nan_first"), dict(T=5, nan_share=0.05, step=None)),
             ("descending ties", dict(tie="descending"), dict(T=5, nan_share=0.0, step=0.5))]
    for name, wrong, data in cases:
        told = 0
        for i in range(sets):
            s, row_keys = _synthetic(P._seed("wrong", name, i), 600, 40, **data)
            for metric in (0, 1):
                right, other = MS.by_dict(s, row_keys, metric, 43), MS.by_dict(s, row_keys, metric, 43, **wrong)
                vec = MS.vectorised(s, row_keys, metric, 43)
                assert (right[1] == vec[1]).all() and (right[0].view(np.uint32) == vec[0].view(np.uint32)).all()
                if metric == 0:
                    told += int((right[1] != other[1]).any() or (right[0].view(np.uint32) != other[0].view(np.uint32)).any())
        assert told >= 0.9 * sets, f"{name}: told apart on {told} of {sets} query sets"


def test_order_keys_and_scores_round_trip():
    s = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 1e-45, -1e-45], np.float32)
    for metric in (0, 1, 2):
        key = MS.order_key(s, metric)
        assert key[0] == key[1] and key[6] == MS.NAN_KEY and (key[:6] < MS.NAN_KEY).all()
        back = MS.score_of_key(key, metric)
        assert (back[[2, 3, 4, 5, 7, 8]] == s[[2, 3, 4, 5, 7, 8]]).all() and np.isnan(back[6])
        assert back[:2].view(np.uint32).tolist() == [0, 0], "+0.0 stands for +-0.0"
        best_first = np.argsort(key[:6], kind="stable")
        want = np.argsort(s[:6] if metric == 0 else -s[:6], kind="stable")
        assert s[best_first].tolist() == s[want].tolist()
