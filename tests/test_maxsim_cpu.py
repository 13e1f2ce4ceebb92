"""Multi-vector search, CPU tier (DESIGN.md §3 "Multi-vector search"): the library exports the new entry points and Python names
them, every refusal that needs no handle precedes any device call and names its cause in the stated order, the scratch plan is
the pure function the header states, and the numpy reference (tests/_maxsim.py) is the contract's loop: it agrees with its
vectorised form on the GPU tests' layouts and tells three wrong models from the contract.  The scoring kernel's forms
(DESIGN.md §5 "M0 / M1"): mvfgpu_selftest_maxsim_form reaches exactly the cells of tests/_maxsim.py's table, the table holds
both sides of every switch, the forced widths, the self-test's refusals, the saturated world's values next to 2^31, and the
exact integer reference tells two wrong kernels from the right one."""
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
    for name in ("mvfgpu_search_maxsim", "mvfgpu_search_maxsim_device", "mvfgpu_selftest_maxsim_plan", "mvfgpu_selftest_maxsim_stage_ms",
                 "mvfgpu_selftest_maxsim_form"):
        assert hasattr(lib, name), name
    for name in ("search_maxsim", "search_maxsim_device", "maxsim_stage_ms"):
        assert hasattr(G.GpuCorpus, name), name
    assert hasattr(G, "maxsim_plan") and hasattr(G, "MaxSimResult") and hasattr(G, "maxsim_form") and hasattr(G, "MaxSimForm")
    assert "find_top_k_documents" in M.__all__ and hasattr(M, "find_top_k_documents") and "MaxSimResult" in M.__all__
    hpp = open(os.path.join(ROOT, "include", "mvf.hpp")).read()
    assert "find_top_k_documents" in hpp and "mvfgpu_search_maxsim" in hpp
    header = open(os.path.join(ROOT, "include", "mvf_gpu.h")).read()
    assert "#define MVFGPU_MAXSIM_MAX_TOKENS 1024u" in header and "int mvfgpu_selftest_maxsim_form(" in header
    assert "fn mvfgpu_selftest_maxsim_form(" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
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


# ---- the scoring kernel's forms: mvfgpu_selftest_maxsim_form and the case table of tests/test_gpu_maxsim_forms.py
FLOAT_MAX_DIM, INT_MAX_DIM = 12288, 33025


def _form(dt, dim, forced=0):
    return G.maxsim_form(MS.DTYPE[dt], dim, forced)


def test_every_reachable_cell_is_in_the_table_and_every_case_is_in_its_cell():
    """every dimension a float search of up to 12288 and an integer search of up to 33025 dimensions can have: the (type, lanes
    per row, form) triples the launch can reach are exactly the table's -- 9 per float type, 8 per integer type"""
    reachable = set()
    for dt in MS.DTYPE:
        for dim in range(1, (INT_MAX_DIM if dt in ("i8", "u8") else FLOAT_MAX_DIM) + 1):
            f = _form(dt, dim)
            reachable.add((dt, f.G, f.form))
    table = set()
    for (dt, dim), cell in MS.FORM_CELLS.items():
        f = _form(dt, dim)
        assert (f.G, f.J, f.form) == cell, f"{dt} x {dim}: listed as {cell}, the library says {f}"
        assert (f.form == MS.REG) == (f.J <= MS.REG_STEPS) and (f.form == MS.CACHE) == (f.token_bytes > MS.LDS_TOKEN_BYTES)
        assert f.token_bytes == f.G * f.J * (32 if dt == "f16" else 16)
        assert f.lds_chunk_cap == MS.plan(1, 1024, 1, f.token_bytes, 1 << 62)[0]
        table.add((dt, f.G, f.form))
    assert table == reachable, f"not in the table: {sorted(reachable - table)}; not reachable: {sorted(table - reachable)}"
    assert len(reachable) == 34 and [sum(c[0] == dt for c in reachable) for dt in ("f32", "f16", "i8", "u8")] == [9, 9, 8, 8]
    assert MS.FORM_CASES == list(MS.FORM_CELLS) and len(MS.FORM_CASES) == 45
    assert _form("i8", 33025).lds_chunk_cap == 1 and _form("u8", 33025).lds_chunk_cap == 1


def test_the_table_holds_both_sides_of_each_switch():
    """per switch and type that has it: the near case is the last dimension of its side, the far case lies in the first 16-byte
    step of the other side -- the same lanes per row, J 4 | 5 (registers | re-read) or a token of 40 KiB | beyond (LDS with a
    chunk of one token | the cache with 32)"""
    for name, pairs in MS.FORM_SWITCHES.items():
        for dt, near, far in pairs:
            assert (dt, near) in MS.FORM_CELLS and (dt, far) in MS.FORM_CELLS, (name, dt)
            a, b = _form(dt, near), _form(dt, far)
            assert a.G == b.G, (name, dt)
            if name == "LDS to cache":
                assert (a.form, a.lds_chunk_cap, b.form, b.lds_chunk_cap) == (MS.REREAD, 1, MS.CACHE, 32), (name, dt, a, b)
                assert a.token_bytes == MS.LDS_TOKEN_BYTES < b.token_bytes and b.J == a.J + 1
                other_side = lambda f: f.form == MS.CACHE
            else:
                assert (a.J, a.form, b.J, b.form) == (MS.REG_STEPS, MS.REG, MS.REG_STEPS + 1, MS.REREAD), (name, dt, a, b)
                other_side = lambda f: f.G == a.G and f.form == MS.REREAD
            nxt = _form(dt, near + 1)
            assert (nxt.G, nxt.J, nxt.form) != (a.G, a.J, a.form), f"{name}, {dt}: {near} is not the last dimension of its side"
            first = next(d for d in range(near + 1, far + 1) if other_side(_form(dt, d)))
            assert _form(dt, first) == b, f"{name}, {dt}: {far} is not in the first step of the other side ({first} is)"


def test_the_forced_widths_are_classified():
    """MVF_K1_G at V = 50 vectors per row: 1, 4 and 8 lanes take 50, 13 and 7 steps (rows re-read: the only way to the kernel's
    G 1 / 4 / 8 re-read instantiations), 16, 32 and 64 lanes 4, 2 and 1 (registers)"""
    for dt, dim in MS.FORCED_SHAPES:
        got = [_form(dt, dim, g) for g in MS.FORCED_WIDTHS]
        assert [(f.G, f.J, f.form) for f in got] == [(1, 50, MS.REREAD), (4, 13, MS.REREAD), (8, 7, MS.REREAD), (16, 4, MS.REG),
                                                     (32, 2, MS.REG), (64, 1, MS.REG)], (dt, got)
        own = _form(dt, dim)
        assert (own.G, own.form) == (64, MS.REG) and own == _form(dt, dim, 64), "V = 50: the library's own rule takes 64 lanes"


def test_the_form_self_test_refuses_what_it_cannot_answer():
    lib = _lib.gpu()
    outs = [C.c_uint32(7) for _ in range(5)]
    ok = [C.byref(o) for o in outs]
    assert lib.mvfgpu_selftest_maxsim_form(0, 100, 0, *ok) == 0
    for i in range(5):
        assert lib.mvfgpu_selftest_maxsim_form(0, 100, 0, *[None if j == i else p for j, p in enumerate(ok)]) == INV and _msg() == "NULL buffer"
    for dtype in (4, 5, 6, 255):
        assert lib.mvfgpu_selftest_maxsim_form(dtype, 100, 0, *ok) == INV and "data type" in _msg()
    for dtype in range(4):
        assert lib.mvfgpu_selftest_maxsim_form(dtype, 0, 0, *ok) == INV and _msg() == "dimension must be > 0"
    for dtype in (2, 3):
        assert lib.mvfgpu_selftest_maxsim_form(dtype, 33025, 0, *ok) == 0
        assert lib.mvfgpu_selftest_maxsim_form(dtype, 33026, 0, *ok) == INV and "33025" in _msg()
    assert lib.mvfgpu_selftest_maxsim_form(0, 33026, 0, *ok) == 0 and lib.mvfgpu_selftest_maxsim_form(1, 33026, 0, *ok) == 0
    for forced in (2, 3, 5, 24, 128):
        assert lib.mvfgpu_selftest_maxsim_form(0, 100, forced, *ok) == INV and "forced_g" in _msg()
    with pytest.raises(E.InvalidArgument):
        G.maxsim_form(2, 40000)


def test_the_saturated_world_is_near_the_i32_limit():
    """UInt8 x 33025: the all-max row against the all-max token is 65025 x 33025 = INT32_MAX - 33022 under InnerProduct, the
    all-min row against it the same value under L2; both rows hold a key of their own, so these are per-key bests; and the two
    equal rows under different keys give bit-equal sums"""
    import _wide as W
    dt, dim = "u8", 33025
    rows, lay, pos = MS.saturated_world(dt, dim)
    sets = MS.saturated_sets(dt, dim)
    assert rows.shape == (1024, dim) and MS.spans_block_edge(lay) and sets.shape == (2, 5, dim)
    _, keys, starts, key_values = MS.key_order(lay)
    assert all((keys == np.uint64(MS.SAT_OWN_KEY0 + i)).sum() == 1 for i in range(10)) and (keys == np.uint64(MS.SAT_TIE_KEY)).sum() == 3
    tokens = sets.reshape(10, dim)
    for metric, floor in ((W.IP, W.L2_RAW_MAX), (W.L2, 1 << 30)):
        sc, raw, _ = MS.int_row_scores(rows, lay, tokens, metric)
        best = np.maximum.reduceat(raw.astype(np.int64), starts, axis=1) if metric == W.IP else np.minimum.reduceat(raw.astype(np.int64), starts, axis=1)
        assert best.max() >= floor and raw.max() == W.L2_RAW_MAX, f"metric {metric}: the per-key bests reach {best.max()}"
        if metric == W.IP:
            assert (best == W.L2_RAW_MAX).any()
    for metric in (W.L2, W.IP, W.COS):
        scores, got_keys, counts = MS.int_reference(rows, lay, sets, metric, key_values.size)
        assert (counts == key_values.size).all()
        for j in range(2):
            at = {int(g): i for i, g in enumerate(got_keys[j])}
            a, b = at[MS.SAT_OWN_KEY0 + 4], at[MS.SAT_OWN_KEY0 + 5]
            assert scores[j].view(np.uint32)[a] == scores[j].view(np.uint32)[b] and b == a + 1, "equal rows: equal sums, ranked by key value"


@pytest.mark.parametrize("dt,dim", [("i8", 768), ("u8", 2048), ("i8", 4112)])
def test_the_integer_reference_tells_two_wrong_kernels_from_the_right_one(dt, dim):
    """a kernel that never runs a row's last step, and one that takes row u of a step for row u ^ 1: each gives other bytes
    than the exact reference on the form cases' world, under every metric"""
    f = _form(dt, dim)
    assert f.J > 1
    lay = MS.form_layout(1024)
    rows, sets = P.make_rows(1024, dim, dt), MS.token_pool(dt, dim)[:2, :5]
    _, _, _, key_values = MS.key_order(lay)
    for metric in (0, 1, 2):
        right = MS.int_reference(rows, lay, sets, metric, key_values.size)
        short_rows, short_tokens = MS.model_drops_last_step(rows, sets.reshape(10, dim), f.G, f.J)
        dropped = MS.int_reference(short_rows, lay, short_tokens.reshape(sets.shape), metric, key_values.size)
        assert (right[0].view(np.uint32) != dropped[0].view(np.uint32)).any(), f"metric {metric}: the last step does not show"
        for j in range(2):
            sc, _, keys = MS.int_row_scores(rows, lay, sets[j], metric)
            swapped = MS.vectorised(sc[:, MS.model_swaps_row_pairs(keys.size, f.G)], keys, metric, key_values.size)
            assert (swapped[1] != right[1][j]).any() or (swapped[0].view(np.uint32) != right[0][j].view(np.uint32)).any(), \
                f"metric {metric}, set {j}: swapped rows do not show"
