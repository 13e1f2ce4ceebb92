"""-m gpu tests of the candidate multi-vector search (DESIGN.md §3 "Candidate keys").  The yardstick is identity 1: the full
search (search_maxsim at k = n_keys, whose own tests check it against the recipe of grouped searches) with every entry whose key
is no candidate of the set removed in numpy, cut at k and padded -- search_maxsim_candidates must return exactly those score
bits, keys and counts.  Beside it: identity 2 (every key listed reproduces search_maxsim), identity 3 (b(t, g) from
search_partitioned at k = 1), lists whose rows end around the 128 positions of a block, skipped entries, chunks and windows
under a small scratch budget, wide rows, duplicate rows and edge tokens, the float64 contract reference, the device call and the
stage timer, the refusals and a fresh process.  8192 rows and the layouts of tests/_grouped.py unless stated."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _dups as D
import _grouped as GR
import _maxsim as MS
import _maxsim_candidates as MC
import _partitioned as P
from _children import RUNNER
from _util import PAD, TOL
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
L2, IP, COS = 0, 1, 2
METRICS = (L2, IP, COS)
SHAPES = [("f32", 100), ("f32", 768), ("f16", 776), ("i8", 64), ("u8", 64)]
TOKENS = (1, 3, 4, 5, 33)
NQS = (1, 3)
LAYOUTS = {"stock": GR.stock, "caps": GR.caps, "dominant": GR.dominant, "own_keys": GR.own_keys, "one_key": GR.one_key}


class World:
    """one corpus with its column and partition index; the full search's rows are computed once per (sets, metric)"""

    def __init__(self, dt, dim, lay, rows=None):
        self.dt, self.dim, self.lay = dt, dim, lay
        self.rows = P.make_rows(len(lay["col"]), dim, dt) if rows is None else rows
        self.c = G.GpuCorpus.from_array(self.rows)
        self.c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        self.col = self.c.attach_column(lay["col"])
        self.part = self.c.make_partition(self.col)
        self.live = GR.live_rows(lay)
        self.keys, self.key_rows = self.part.keys()
        self.nk = int(self.keys.size)
        self._full = {}
        held = set(self.keys.tolist())
        self.unheld = [v for v in (lay.get("absent_key", 1), lay.get("dead_key", 2), 1, 2, 5) if v not in held][:2]  # two values no live row carries

    def full(self, sets, metric):
        key = (sets.tobytes(), sets.shape, metric)
        if key not in self._full:
            self._full[key] = self.c.search_maxsim(sets, self.nk + 1, metric, self.part)  # + 1: a padding entry behind the keys
            assert (self._full[key].counts == self.nk).all()
        return self._full[key]

    def close(self):
        self.part.close()
        self.col.close()
        self.c.close()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(dt, dim, layout, flavour):
        if (dt, dim, layout, flavour) not in made:
            made[dt, dim, layout, flavour] = World(dt, dim, LAYOUTS[layout](flavour))
        return made[dt, dim, layout, flavour]
    yield get
    for w in made.values():
        w.close()


def same_bytes(got, want, what):
    assert got.scores.shape == want.scores.shape and got.keys.shape == want.keys.shape, what
    assert (got.counts == want.counts).all(), f"{what}: counts {got.counts} != {want.counts}"
    assert (got.keys == want.keys).all(), f"{what}: keys"
    assert (got.scores.view(np.uint32) == want.scores.view(np.uint32)).all(), f"{what}: score bits"


def filtered(w, sets, lists, metric, k):
    """identity 1's right-hand side"""
    full = w.full(sets, metric)
    return G.MaxSimResult(*MC.filter_full(full.scores, full.keys, w.nk, lists, w.keys, k, metric))


def distinct_counts(w, lists):
    return [int(MC.held_distinct(l, w.keys).size) for l in lists]


def check(w, sets, lists, metric, what, ks=None):
    """search_maxsim_candidates at every k against the filtered full search"""
    lists = np.asarray(lists, np.uint64).reshape(sets.shape[0], -1)
    d = distinct_counts(w, lists)
    for k in ks or sorted({1, 10, max(min(d), 1), max(max(d), 1), max(d) + 3}):
        got = w.c.search_maxsim_candidates(sets, lists, k, metric, w.part)
        same_bytes(got, filtered(w, sets, lists, metric, k), f"{what}, k {k}")
        assert (got.counts == np.minimum(k, d)).all(), f"{what}, k {k}: counts are min(k, distinct held candidates)"


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=[f"{dt}d{dim}" for dt, dim in SHAPES])
def test_every_row_is_the_full_searchs_row_without_the_other_keys(worlds, case):
    """identity 1 over the matrix; every set has its own list and its own number of held candidates, some entries are skipped"""
    dt, dim = SHAPES[case]
    flavour = "u64" if case % 2 else "u32"
    w = worlds(dt, dim, "stock", flavour)
    for metric in METRICS:
        for T in TOKENS:
            for nq in NQS:
                lists = MC.mixed_lists(w.keys, nq, 40, w.unheld + [int(PAD)], (case, metric, T))
                assert len(set(distinct_counts(w, lists))) == nq
                check(w, MS.make_sets(nq, T, dim, dt), lists, metric, f"{dt} x {dim}, metric {metric}, T {T}, nq {nq}")


def _block_cut_lists(w):
    """name -> list: row totals of 127, 128, 129, 256 and 3 * 128 + 1 where the layout's key sizes can make them, a single key
    of one row, the largest key alone, the first and the last key of the table, every key"""
    rng = np.random.default_rng(P._seed("block cuts", w.nk))
    out = {}
    for target in (127, 128, 129, 256, 385):
        got = MC.rows_ending_at(w.keys, w.key_rows, target, rng)
        if got is not None:
            out[f"{target} rows"] = got
    ones = w.keys[w.key_rows == 1]
    if ones.size:
        out["one key of one row"] = ones[:1]
    out["the largest key alone"] = w.keys[np.argmax(w.key_rows)][None]
    out["the first and the last key"] = w.keys[[0, -1]]
    out["every key"] = w.keys[rng.permutation(w.nk)]
    return out


@pytest.mark.parametrize("flavour", ["u32", "u64"])
@pytest.mark.parametrize("layout", ["caps", "dominant", "own_keys", "one_key"])
def test_lists_that_end_around_a_block_of_128_positions(worlds, layout, flavour):
    for dt, dim, metric in (("f32", 100, COS), ("i8", 64, L2)):
        w = worlds(dt, dim, layout, flavour)
        named = _block_cut_lists(w)
        if layout in ("caps", "own_keys"):
            assert {"127 rows", "128 rows", "129 rows", "256 rows", "385 rows", "one key of one row"} <= set(named)
        if layout == "dominant":
            assert int(w.key_rows.max()) > 40 * MC.BLOCK, "one slot runs over many blocks"
        T = 3
        one = MS.make_sets(1, T, dim, dt)
        for name, lst in named.items():
            check(w, one, lst[None], metric, f"layout {layout} {flavour}, {dt}: {name}", ks=(1, 10, lst.size + 3))
        # identity 2, against search_maxsim directly
        for k in (10, w.nk + 3) if layout != "own_keys" else (10,):
            same_bytes(w.c.search_maxsim_candidates(one, named["every key"], k, metric, w.part), w.c.search_maxsim(one, k, metric, w.part),
                       f"layout {layout} {flavour}, {dt}: every key listed is search_maxsim, k {k}")
        # all of them as the sets of ONE call: no block spans two sets, the sets' ends fall on and around block edges
        short = {n: l for n, l in named.items() if l.size <= 400}
        m = max(l.size for l in short.values())
        lists = np.stack([np.concatenate([l, np.full(m - l.size, w.unheld[0], np.uint64)]) for l in short.values()])
        check(w, MS.make_sets(len(short), T, dim, dt), lists, metric, f"layout {layout} {flavour}, {dt}: {list(short)} in one call", ks=(1, 10, m + 3))


@pytest.mark.parametrize("flavour", ["u32", "u64"])
def test_entries_the_partition_does_not_hold_are_skipped_and_repeats_count_once(worlds, flavour):
    w = worlds("f32", 100, "stock", flavour)
    lay = w.lay
    T, metric, k = 4, IP, 12
    sets = MS.make_sets(3, T, 100, "f32")
    a, b, c = (np.uint64(x) for x in lay["keys"][3:6])
    unknown, dead = np.uint64(lay["absent_key"]), np.uint64(lay["dead_key"])
    lists = np.array([[a, a, unknown, b, PAD, dead, c, PAD, unknown, a, b, PAD],          # repeats side by side and far apart
                      [unknown, dead, PAD, PAD, unknown, dead, dead, unknown, PAD, PAD, PAD, PAD],  # skipped entries only (u32)
                      [c, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, PAD, c]], np.uint64)
    holds_pad = bool((w.keys == PAD).any())
    assert holds_pad == (flavour == "u64"), "the u64 layout really holds UINT64_MAX as a key"
    want_counts = [3 + holds_pad, int(holds_pad), 1 + holds_pad]
    assert distinct_counts(w, lists) == want_counts
    got = w.c.search_maxsim_candidates(sets, lists, k, metric, w.part)
    assert got.counts.tolist() == want_counts
    same_bytes(got, filtered(w, sets, lists, metric, k), f"skipping, {flavour}")
    for q in range(3):
        n = want_counts[q]
        assert (got.keys[q, n:] == PAD).all() and np.isneginf(got.scores[q, n:]).all(), "padding behind the counts"
        assert ((got.keys[q, :n] == PAD).sum() == int(holds_pad)) and np.isfinite(got.scores[q, :n]).all(), \
            "a real key UINT64_MAX is a candidate with a score: the counts tell it from padding"
    # m = 0: no list at all, and a [nq, 0] one
    for none in (None, np.zeros((3, 0), np.uint64)):
        res = w.c.search_maxsim_candidates(sets, none, k, L2, w.part)
        assert (res.counts == 0).all() and (res.keys == PAD).all() and np.isposinf(res.scores).all()
    # one list for every set
    shared = w.c.search_maxsim_candidates(sets, lists[0], k, metric, w.part)
    same_bytes(shared, filtered(w, sets, np.broadcast_to(lists[0], (3, 12)), metric, k), "one list shared by the sets")


@pytest.mark.parametrize("dt,dim,metric", [("f32", 100, COS), ("i8", 64, L2), ("f32", 100, L2), ("i8", 64, IP)])
def test_the_per_token_best_is_the_partitioned_searchs_score(worlds, dt, dim, metric):
    """identity 3: b(t, g) = the score search_partitioned reports for (token t, key g, k = 1), summed in numpy f32 in token order
    and ranked by (order key, key value)"""
    w = worlds(dt, dim, "stock", "u32")
    T, nq = 5, 2
    sets = MS.make_sets(nq, T, dim, dt)
    lists = MC.mixed_lists(w.keys, nq, 30, w.unheld, "identity 3")
    for q in range(nq):
        cand = MC.held_distinct(lists[q], w.keys)
        queries = np.ascontiguousarray(np.repeat(sets[q], cand.size, axis=0))          # token-major: token t against every candidate
        res = w.c.search_partitioned(queries, np.tile(cand, T), 1, metric, w.part)
        best = res.scores[:, 0].reshape(T, cand.size)
        for k in (1, 10, cand.size + 3):
            want = MS.rank_keys(best, cand, metric, k)
            got = w.c.search_maxsim_candidates(sets[q], lists[q], k, metric, w.part)
            assert got.counts[0] == want[2] and (got.keys[0] == want[1]).all() and \
                (got.scores[0].view(np.uint32) == want[0].view(np.uint32)).all(), f"{dt}, metric {metric}, set {q}, k {k}"


def test_chunks_and_windows_give_the_unchunked_bytes(worlds, monkeypatch):
    """MVF_MAXSIM_SCRATCH_BYTES, read when the handle is created.  First so small that one set's list and an 8-token chunk just
    fit: T = 33 takes at least 3 chunks and nq = 3 at least 2 windows.  Then below even the shortest set's list, whose share
    leaves nothing: one set per window, whatever the budget, and the least chunk."""
    for dt, dim, metric in (("f32", 100, COS), ("f16", 776, L2), ("i8", 64, IP)):
        w = worlds(dt, dim, "stock", "u32")
        sets = MS.make_sets(3, 33, dim, dt)
        lists = MC.mixed_lists(w.keys, 3, 40, w.unheld, "chunks")
        d = distinct_counts(w, lists)
        rows = [int(w.key_rows[np.isin(w.keys, MC.held_distinct(l, w.keys))].sum()) for l in lists]
        positions = [-(-r // MC.BLOCK) * MC.BLOCK for r in rows]
        per_set = [dq * (8 * 4 + MS.KEY_BYTES) + 8 * p for dq, p in zip(d, positions)]
        tight, at = max(per_set), int(np.argmax(per_set))
        assert tight < per_set[0] + per_set[1], "the first two sets do not fit one window: at least 2 windows"
        chunk, _ = G.maxsim_plan(d[at], 33, 1, 16, tight - 8 * positions[at])
        assert -(-33 // chunk) >= 3, "the LDS share can only shorten the chunk further"
        lists_only = 8 * min(positions) - 1
        whole = {k: w.c.search_maxsim_candidates(sets, lists, k, metric, w.part) for k in (1, 10, max(d) + 3)}
        for budget in (tight, lists_only):
            monkeypatch.setenv("MVF_MAXSIM_SCRATCH_BYTES", str(budget))
            small = World(dt, dim, w.lay)
            monkeypatch.delenv("MVF_MAXSIM_SCRATCH_BYTES")
            try:
                for k, want in whole.items():
                    cut = small.c.search_maxsim_candidates(sets, lists, k, metric, small.part)
                    same_bytes(cut, want, f"{dt}, budget {budget}, k {k}: chunked against unchunked")
                    same_bytes(cut, filtered(w, sets, lists, metric, k), f"{dt}, budget {budget}, k {k}: chunked against the filter")
            finally:
                small.close()


@pytest.mark.parametrize("dim", [4100, 12000])
def test_wide_rows(dim):
    """2048 Float32 rows: 4100 dimensions are 17 steps per lane -- beyond the registers, the rows are read again per token
    group --, 12000 dimensions are a padded token of 47 KiB that is read through the cache"""
    lay = P.layout("u32", 2048, (300, 129, 128, 127, 64, 2, 1), 20)
    w = World("f32", dim, lay)
    try:
        lists = MC.mixed_lists(w.keys, 2, 12, w.unheld, ("wide", dim))
        lists[0, :4] = [np.uint64(v) for v in lay["keys"][:4]]   # 300 + 129 + 128 + 127 rows among set 0's
        for metric in (L2, COS):
            check(w, MS.make_sets(2, 5, dim, "f32"), lists, metric, f"f32 x {dim}, metric {metric}", ks=(10, 15))
    finally:
        w.close()


@pytest.mark.parametrize("dtype,metric", [(0, L2), (1, IP)])
def test_duplicated_rows_tie_bit_for_bit_and_rank_by_key_value(dtype, metric):
    """tests/_dups.py's corpus of 24 distinct vectors: every key of position % 50 holds copies of nearly all of them, so most
    candidates carry identical sums and their order is the key values'"""
    dim = 48
    cp = D.corpus_b(P._seed("maxsim dups", dtype), P.N, dim, dtype)
    dead = D.tombstones(5, P.N)
    col = (np.arange(P.N) % 50).astype(np.uint32) * np.uint32(9)
    w = World("f16" if dtype else "f32", dim, dict(col=col, dead=dead), rows=cp.rows)
    try:
        sets = D.gaussian_queries(77, 3 * 5, dim).reshape(3, 5, dim)
        lists = MC.mixed_lists(w.keys, 3, 45, [1, 2], "dups")
        check(w, sets, lists, metric, f"duplicates, dtype {dtype}")
        got = w.c.search_maxsim_candidates(sets, lists, 45, metric, w.part)
        n = int(got.counts[0])
        assert n >= 40 and np.unique(got.scores[0, :n].view(np.uint32)).size <= n // 2, "many candidates tie bit for bit"
        tied = got.scores[0, 1:n].view(np.uint32) == got.scores[0, :n - 1].view(np.uint32)
        assert tied.any() and (got.keys[0, 1:n][tied] > got.keys[0, :n - 1][tied]).all(), "ties rank by ascending key value"
    finally:
        w.close()


@pytest.mark.parametrize("metric", METRICS)
def test_edge_tokens(worlds, metric):
    """§3 "Values at the edges": a NaN token (L2 / InnerProduct: every sum NaN; Cosine: 0 for every row), a +Inf element (L2 +inf,
    InnerProduct +-inf, Cosine NaN for every row) and, under Cosine, a zero token.  Against the filtered full search; where
    every sum is NaN the candidates come in ascending key value, ahead of the padding -- also in the set that holds fewer
    candidates than the window's widest, whose filler entries sort behind its NaN sums"""
    w = worlds("f32", 100, "stock", "u32")
    T = 4
    base = MS.make_sets(2, T, 100, "f32")
    lists = MC.mixed_lists(w.keys, 2, 30, w.unheld + [int(PAD)], "edges")
    d = distinct_counts(w, lists)
    assert d[1] < d[0]
    edges = {"nan": np.full(100, np.nan, np.float32), "inf": base[0, 2].copy()}
    edges["inf"][0] = np.inf
    if metric == COS:
        edges["zero"] = np.zeros(100, np.float32)
    for name, token in edges.items():
        for at in (0, 2, T - 1):
            sets = base.copy()
            sets[:, at] = token
            check(w, sets, lists, metric, f"{name} token at {at}, metric {metric}", ks=(10, max(d) + 3))
            if (name == "nan" and metric != COS) or (name == "inf" and metric == COS):
                got = w.c.search_maxsim_candidates(sets, lists, max(d) + 3, metric, w.part)
                for q in range(2):
                    assert got.counts[q] == d[q] and np.isnan(got.scores[q, :d[q]]).all(), "NaN sums are results"
                    assert (got.keys[q, :d[q]] == MC.held_distinct(lists[q], w.keys)).all(), "NaN sums in ascending key value"
                    assert (got.keys[q, d[q]:] == PAD).all() and np.isinf(got.scores[q, d[q]:]).all(), "then the padding"


def _f64_row_scores(rows, q, metric):
    x, q = rows.astype(np.float64), q.astype(np.float64)
    with np.errstate(all="ignore"):
        if metric == L2:
            return np.sqrt(((x - q) ** 2).sum(1))
        dot = (x * q).sum(1)
        if metric == IP:
            return dot
        den = np.sqrt((q * q).sum()) * np.sqrt((x * x).sum(1))
        return np.where(den > 0, dot / den, 0.0)


@pytest.mark.parametrize("metric", METRICS)
def test_the_float64_contract_reference_within_the_tolerance_scaled_by_the_tokens(worlds, metric):
    """independent of every kernel, restricted to the candidates: b(t, g) and S in float64; every returned sum within the sum
    over tokens of §3's tolerance of a row score, the list in (order key, key value) order, and the set of keys right up to sums
    within two such tolerances of the k-th -- boundary ties only at the k-th rank"""
    w = worlds("f32", 100, "stock", "u32")
    T, nq = 5, 3
    sets = MS.make_sets(nq, T, 100, "f32")
    lists = MC.mixed_lists(w.keys, nq, 40, w.unheld + [int(PAD)], "f64")
    col = w.lay["col"].astype(np.uint64)
    sign = 1.0 if metric == L2 else -1.0
    for j in range(nq):
        cand = MC.held_distinct(lists[j], w.keys)
        live = w.live[np.isin(col[w.live], cand)]
        x = w.rows[live]
        xn = np.sqrt((x.astype(np.float64) ** 2).sum(1))
        by_key = np.argsort(col[live], kind="stable")
        starts = np.nonzero(np.concatenate([[True], np.diff(col[live][by_key]) != 0]))[0]
        assert (col[live][by_key][starts] == cand).all()
        S, tol = np.zeros(cand.size), np.zeros(cand.size)
        for t in range(T):
            s = _f64_row_scores(x, sets[j, t], metric)
            b = sign * np.minimum.reduceat((sign * s)[by_key], starts)
            S += b
            qn = float(np.linalg.norm(sets[j, t].astype(np.float64)))
            tol += TOL * np.abs(b) if metric == L2 else TOL if metric == COS else TOL * np.maximum.reduceat(xn[by_key], starts) * qn
        for k in (1, 10, cand.size):
            got = w.c.search_maxsim_candidates(sets[j], lists[j], k, metric, w.part)
            assert got.counts[0] == k
            MS.assert_f64_contract(got.scores[0], got.keys[0], cand, S, tol, metric, k)   # "keys of the partition": the set's candidates


def test_device_call_equals_the_host_call_and_the_stage_timer_is_the_device_call(worlds):
    import torch
    w = worlds("f32", 100, "stock", "u64")
    nq, T = 3, 33
    sets = MS.make_sets(nq, T, 100, "f32")
    lists = MC.mixed_lists(w.keys, nq, 40, w.unheld, "device")
    for k in (10, 43):
        host = w.c.search_maxsim_candidates(sets, lists, k, COS, w.part)
        same_bytes(host, filtered(w, sets, lists, COS, k), f"host call, k {k}")
        dq = torch.from_numpy(sets).cuda()
        ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        dk = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        dc = torch.empty((nq,), dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        w.c.search_maxsim_candidates_device(w.part, dq.data_ptr(), 0, 100, nq, T, lists, k, COS, ds.data_ptr(), dk.data_ptr(), dc.data_ptr(), stream)
        torch.cuda.synchronize()
        dev = G.MaxSimResult(ds.cpu().numpy(), dk.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint32))
        same_bytes(dev, host, f"device call, k {k}")
        ds.zero_(), dk.zero_()
        ms = w.c.maxsim_candidates_stage_ms(w.part, dq.data_ptr(), 0, 100, nq, T, lists, k, COS, ds.data_ptr(), dk.data_ptr(), stream)
        assert len(ms) == 4 and all(0.0 <= x < 1000.0 for x in ms) and ms[0] > 0.0 and ms[1] > 0.0
        assert (dk.cpu().numpy().view(np.uint64) == host.keys).all() and (ds.cpu().numpy().view(np.uint32) == host.scores.view(np.uint32)).all()
        # two calls back to back on one stream: the second plan waits for the first to have left the pinned buffer
        ds2, dk2 = torch.empty_like(ds), torch.empty_like(dk)
        w.c.search_maxsim_candidates_device(w.part, dq.data_ptr(), 0, 100, nq, T, lists, k, COS, ds.data_ptr(), dk.data_ptr(), 0, stream)
        w.c.search_maxsim_candidates_device(w.part, dq.data_ptr(), 0, 100, nq, T, lists[::-1].copy(), k, COS, ds2.data_ptr(), dk2.data_ptr(), 0, stream)
        torch.cuda.synchronize()
        assert (dk.cpu().numpy().view(np.uint64) == host.keys).all()
        back = w.c.search_maxsim_candidates(sets, lists[::-1].copy(), k, COS, w.part)
        assert (dk2.cpu().numpy().view(np.uint64) == back.keys).all() and (ds2.cpu().numpy().view(np.uint32) == back.scores.view(np.uint32)).all()


def _no_device_error():
    import torch
    hip = P._hip_runtime()
    hip.hipGetLastError.restype = C.c_int
    assert hip.hipGetLastError() == 0, "a refusal left a device error behind"
    torch.cuda.synchronize()


def test_refusals_their_order_and_the_handles_other_searches():
    lay = GR.stock("u32")
    rows = P.make_rows(P.N, 64, "i8")
    q, q64 = P.make_queries(4, 64, "i8"), P.make_queries(64, 64, "i8")
    sets = MS.make_sets(2, 5, 64, "i8")
    lists = MC.mixed_lists(P.group_by(lay)[0], 2, 20, [lay["absent_key"]], "refusals")
    lib = _lib.gpu()
    INV = 12
    with G.GpuCorpus.from_array(rows) as c, G.GpuCorpus.from_array(rows[:100]) as other:
        c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        before, before64 = c.search(q, 10, L2), c.search(q64, 10, L2)
        state = c.info().selection_state
        with c.attach_column(lay["col"]) as col, other.attach_column(lay["col"][:100].copy()) as ocol:
            part, opart = c.make_partition(col), other.make_partition(ocol)
            first = c.search_maxsim_candidates(sets, lists, 10, L2, part)
            # the ladder with a real handle, everything wrong at once: code and message at every step
            sc, ky = np.zeros(20, np.float32), np.zeros(20, np.uint64)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
            arg = dict(part=None, metric=9, q=None, dim=63, nq=0, T=0, cand=None, m=20, k=0, sc=None, ky=None)
            ladder = [("unsupported distance metric code 9", dict(metric=0)), ("nq must be > 0", dict(nq=2)), ("k must be in 1..2^31", dict(k=10)),
                      ("NULL buffer", dict(q=vp(sets))), ("NULL buffer", dict(sc=vp(sc))), ("NULL buffer", dict(ky=vp(ky))),
                      ("n_tokens must be in 1..1024, got 0", dict(T=1025)), ("n_tokens must be in 1..1024, got 1025", dict(T=5)),
                      ("NULL buffer (candidate_keys)", dict(cand=vp(lists))), ("partition is NULL", dict(part=opart._h))]
            for device in (0, 1):
                fn = lib.mvfgpu_search_maxsim_candidates_device if device else lib.mvfgpu_search_maxsim_candidates
                a = dict(arg)
                for message, fix in ladder:
                    rc = fn(c._h, a["part"], a["metric"], a["q"], 2, a["dim"], a["nq"], a["T"], a["cand"], a["m"], a["k"], a["sc"], a["ky"], None,
                            *[None] * device)
                    assert rc == INV and lib.mvfgpu_last_error_message().decode() == message, (device, message)
                    a.update(fix)
                _no_device_error()
            with pytest.raises(E.DimensionMismatch):
                c.search_maxsim_candidates(sets[:, :, :63], lists, 10, L2, opart)   # the handle checks precede the partition's
            with pytest.raises(E.BuildError):
                c.search_maxsim_candidates(sets.astype(np.float32), lists, 10, L2, opart)
            with pytest.raises(E.InvalidArgument, match="another corpus handle"):
                c.search_maxsim_candidates(sets, lists, 10, L2, opart)
            with pytest.raises(E.InvalidArgument, match=r"candidate_keys must be \[m\] or \[2, m\]"):
                c.search_maxsim_candidates(sets, np.zeros((3, 4), np.uint64), 10, L2, part)
            _no_device_error()
            for a, b, what in ((before, c.search(q, 10, L2), "a plain search"), (before64, c.search(q64, 10, L2), "a batched plain search")):
                assert (a.indices == b.indices).all() and (a.raw == b.raw).all() and (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), what
            assert c.info().selection_state == state
            # new tombstones: the old index is stale; a new one skips the deleted key
            gone = int(first.keys[0][0])
            dead2 = lay["dead"] | (lay["col"].astype(np.uint64) == np.uint64(gone))
            c.set_tombstones(np.packbits(dead2, bitorder="little"))
            with pytest.raises(E.InvalidArgument, match="stale partition: mvfgpu_corpus_set_tombstones changed the handle's tombstones"):
                c.search_maxsim_candidates(sets, lists, 10, L2, part)
            _no_device_error()
            with c.make_partition(col) as part2:
                second = c.search_maxsim_candidates(sets, lists, 10, L2, part2)
                held2 = P.group_by(dict(col=lay["col"], dead=dead2))[0]
                assert not (second.keys == np.uint64(gone)).any() and not (held2 == np.uint64(gone)).any()
                assert second.counts.tolist() == [min(10, MC.held_distinct(l, held2).size) for l in lists]
            part.close()
            opart.close()


def test_a_fresh_process_gives_the_checked_answer_whatever_its_allocations_held(worlds, tmp_path):
    """the scenario of tests/_maxsim_candidates.py with the candidate search as a child's first device work, every allocation of
    the library filled with 0xFF: one child, none after a fault"""
    inp = MC.fresh_inputs()
    w = worlds("f32", MC.FP_DIM, "stock", "u32")
    assert (w.rows == inp["rows"]).all() and (w.lay["col"] == inp["lay"]["col"]).all()
    want = w.c.search_maxsim_candidates(inp["queries"], inp["lists"], MC.FP_K, MC.FP_METRIC, w.part)
    same_bytes(want, filtered(w, inp["queries"], inp["lists"], MC.FP_METRIC, MC.FP_K), "fresh process, in this process")
    env = {k: v for k, v in os.environ.items() if k not in ("MVF_DEBUG_POISON", "MVF_MAXSIM_SCRATCH_BYTES")}
    env["MVF_DEBUG_POISON"] = "255"
    path = str(tmp_path / "poisonFF.npz")
    out = RUNNER.run([sys.executable, os.path.join(HERE, "_maxsim_candidates.py"), path], env=env)
    assert out.returncode == 0, f"exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
    with np.load(path) as z:
        assert z["poison"].tolist() == [255], "the child's poison byte"
        for call in ("host", "device"):
            got = G.MaxSimResult(z[call + ".scores"], z[call + ".keys"], z[call + ".counts"])
            same_bytes(got, want, f"the {call} call")
            assert P.digest(got.scores, got.keys, got.counts) == P.digest(want.scores, want.keys, want.counts)


def test_rerank_top_k_documents_reads_the_files_column(tmp_path, oracle):
    import metrovector_amd as M
    n, dim, T = 700, 12, 4
    rng = np.random.default_rng(10)
    rows = oracle.synth_rows(91, 0, n, dim, 0)
    q = oracle.synth_queries(92, 2 * T, dim, 0).reshape(2, T, dim)
    doc = rng.integers(0, 40, n).astype(np.uint64) << np.uint64(31)
    dead = rng.random(n) < 0.2
    b = M.MvfBuilder()
    b.add_vector_space("s", dim, 0, 0, 0)
    b.add_vectors("s", rows)
    b.set_tombstones("s", 1, np.packbits(dead, bitorder="little").tobytes() + b"\0", int(dead.sum()))
    b.add_metadata_column("doc", 5, doc.astype("<u8").tobytes())
    b.add_metadata_column("few", 4, np.zeros(n - 1, "<u4").tobytes())
    path = str(tmp_path / "documents.mvf")
    b.build().save(path)
    cand = np.array([[3, 7, 7, 99, 12, 0], [39, 3, 41, 5, 5, 5]], np.uint64) << np.uint64(31)
    with M.MvfReader.open(path) as r:
        space = r.vector_space("s")
        full = M.find_top_k_documents(space, q, 45, column="doc")
        got = M.rerank_top_k_documents(space, q, cand, 5, column="doc")
        one = M.rerank_top_k_documents(space, q[1], cand[1], 5, column="doc")
        assert got.scores.shape == got.keys.shape == (2, 5) and got.counts.tolist() == [4, 3]
        assert (one.keys[0] == got.keys[1]).all() and (one.scores[0].view(np.uint32) == got.scores[1].view(np.uint32)).all()
        want = MC.filter_full(full.scores, full.keys, 40, cand, np.unique(doc[~dead]), 5, L2)
        same_bytes(got, G.MaxSimResult(*want), "rerank_top_k_documents against find_top_k_documents")
        with pytest.raises(E.BuildError, match="holds 699 values"):
            M.rerank_top_k_documents(space, q, cand, 3, column="few")
