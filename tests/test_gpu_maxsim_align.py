"""-m gpu tests of the MaxSim alignments (DESIGN.md §3 "Alignments"; include/mvf_gpu_maxsim_align.h).  The yardstick is
identity 1: element (q, i, t) of maxsim_align is the single result of search_partitioned for the one query "token t of set q"
with the key keys[q][i] and k = 1 -- rows, score bits and raw, skipped and repeated entries included.  One partitioned batch of
nq m T queries answers a whole call.  Beside it: identity 2 (the f32 sum of a key's scores in token order is
search_maxsim_candidates' score), duplicate rows and special values, every form of the scoring kernel, windows and chunks under
a small scratch budget, the edges, the device call, a fresh process, the layers above and a float64 check.  The smallest shapes
at which the kernel can still go wrong: 8192 rows and the stock layout of tests/_grouped.py unless stated."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _grouped as GR
import _maxsim as MS
import _maxsim_align as MA
import _maxsim_candidates as MC
import _partitioned as P
from _children import RUNNER
from _util import PAD, TOL
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L2, IP, COS = 0, 1, 2
METRICS = (L2, IP, COS)
SHAPES = [("f32", 100), ("f16", 200), ("i8", 400), ("u8", 300)]
NQ, T, M_LIST = 3, 5, 40


class World:
    """one corpus with its column and partition index"""

    def __init__(self, dt, dim, lay, rows=None, index_base=0, ids=None):
        self.dt, self.dim, self.lay = dt, dim, lay
        self.rows = P.make_rows(len(lay["col"]), dim, dt) if rows is None else rows
        self.c = G.GpuCorpus.from_array(self.rows, index_base=index_base)
        self.c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        if ids is not None:
            self.c.set_vector_ids(ids)
        self.col = self.c.attach_column(lay["col"])
        self.part = self.c.make_partition(self.col)
        self.keys, self.key_rows = self.part.keys()
        self.nk = int(self.keys.size)
        held = set(self.keys.tolist())
        self.unheld = [v for v in (lay.get("absent_key", 1), lay.get("dead_key", 2), 1, 2, 5) if v not in held][:2]

    def close(self):
        self.part.close()
        self.col.close()
        self.c.close()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(dt, dim):
        if (dt, dim) not in made:
            made[dt, dim] = World(dt, dim, GR.stock("u32"))
        return made[dt, dim]
    yield get
    for w in made.values():
        w.close()


def partitioned(w, sets, lists, metric):
    """identity 1's right-hand side: (rows, scores, raw) [nq, m, T] from ONE partitioned search at k = 1"""
    nq, n_tokens, _ = sets.shape
    lists = np.asarray(lists, np.uint64).reshape(nq, -1)
    queries, keys = MA.partitioned_pairs(sets, lists)
    res = w.c.search_partitioned(queries, keys, 1, metric, w.part)
    shape = (nq, lists.shape[1], n_tokens)
    return res.indices.reshape(shape), res.scores.reshape(shape), res.raw.reshape(shape)


def same_bytes(got, want, what):
    rows, scores, raw = want
    assert got.rows.shape == rows.shape and got.scores.shape == scores.shape and got.raw.shape == raw.shape, what
    assert (got.rows == rows).all(), f"{what}: rows differ at {np.argwhere(got.rows != rows)[:5].tolist()}"
    assert (got.scores.view(np.uint32) == scores.view(np.uint32)).all(), f"{what}: score bits"
    assert (got.raw == raw).all(), f"{what}: raw"


def check(w, sets, lists, metric, what):
    """maxsim_align against the partitioned searches; -> the alignment"""
    got = w.c.maxsim_align(sets, lists, metric, w.part)
    same_bytes(got, partitioned(w, sets, lists, metric), what)
    return got


def stock_lists(w, seed):
    lists = MC.mixed_lists(w.keys, NQ, M_LIST, w.unheld + [int(PAD)], ("align", seed))
    for v in w.unheld + [int(PAD)]:
        assert (lists == np.uint64(v)).any(), "the absent key, the dead key and the pad are listed"
    assert any(np.unique(l[np.isin(l, w.keys)]).size < np.count_nonzero(np.isin(l, w.keys)) for l in lists), "repeats are listed"
    return lists


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=[f"{dt}d{dim}" for dt, dim in SHAPES])
def test_every_element_is_the_partitioned_searchs_single_result(worlds, case):
    """1. identity 1 on the stock world: held keys, repeats, the absent key, the dead key and the pad; T = 5 is a short last
    token group.  2. identity 2 on the same calls"""
    dt, dim = SHAPES[case]
    w = worlds(dt, dim)
    assert (w.lay["dead_key"] not in w.keys.tolist()) and (w.lay["absent_key"] not in w.keys.tolist())
    sets = MS.make_sets(NQ, T, dim, dt)
    lists = stock_lists(w, case)
    for metric in METRICS:
        what = f"{dt} x {dim}, metric {metric}"
        got = check(w, sets, lists, metric, what)
        held = np.isin(lists, w.keys)
        assert (got.rows[~held] == PAD).all() and (got.rows[held] != PAD).all(), what
        assert (got.scores[~held] == (np.inf if metric == L2 else -np.inf)).all() and (got.raw[~held] == 0).all(), what
        assert not w.lay["dead"][got.rows[held].astype(np.int64)].any(), "a deleted row is never the arg"
        assert (w.lay["col"][got.rows[held].astype(np.int64)] == np.broadcast_to(lists[:, :, None], got.rows.shape)[held]).all(), "a row of the entry's key"
        if dt in ("i8", "u8") and metric != COS:
            assert (got.raw[held] != 0).any()
        else:
            assert (got.raw == 0).all()
        # identity 2: the f32 sum in token order is the candidate search's score of the key
        cand = w.c.search_maxsim_candidates(sets, lists, M_LIST, metric, w.part)
        sums = MA.token_sum(got.scores)
        for q in range(NQ):
            n = int(cand.counts[q])
            score_of = dict(zip(cand.keys[q, :n].tolist(), MS.canonical(cand.scores[q, :n]).view(np.uint32).tolist()))
            assert n == np.unique(lists[q][held[q]]).size
            for i in np.nonzero(held[q])[0]:
                assert int(sums[q, i].view(np.uint32)) == score_of[int(lists[q, i])], f"{what}: set {q}, entry {i}: the sum of the scores"


@pytest.mark.parametrize("dt,dim", [("f32", 100), ("f16", 200)])
def test_the_returned_rows_float64_score_is_within_the_tolerance_of_the_keys_float64_best(worlds, dt, dim):
    """no exclusions: for every held entry and token, the float64 score of the returned row lies within §3's tolerance of a row
    score of the float64 best among the key's live rows"""
    import _wide as W
    w = worlds(dt, dim)
    sets = MS.make_sets(NQ, T, dim, dt)
    lists = stock_lists(w, SHAPES.index((dt, dim)))
    key_values = MS.key_order(w.lay)[3]
    assert (key_values == w.keys).all()
    for q in range(NQ):
        f64 = MS.f64_key_bests(w.rows, w.lay, sets[q], TOL)
        held = np.nonzero(np.isin(lists[q], w.keys))[0]
        slot = np.searchsorted(w.keys, lists[q][held])
        for metric in METRICS:
            got = w.c.maxsim_align(sets[q], lists[q], metric, w.part)
            b, tol = f64[metric]
            for t in range(T):
                mine = W.f64_scores_all(w.rows[got.rows[0, held, t].astype(np.int64)], sets[q, t])[metric][0]
                assert (np.abs(mine - b[t, slot]) <= tol[t, slot]).all(), f"{dt}, metric {metric}, set {q}, token {t}"
                assert (np.abs(got.scores[0, held, t].astype(np.float64) - mine) <= tol[t, slot]).all(), "and the reported score is that row's"


def _doubled_world(dt, dim):
    """2048 rows: rows 1024 .. 2047 repeat rows 0 .. 1023 with their keys and deletions, so that every row of a key has an
    exact duplicate at a higher position"""
    half = P.layout("u32", 1024, (300, 129, 70, 64, 2, 1), 12)
    lay = dict(half, col=np.concatenate([half["col"], half["col"]]), dead=np.concatenate([half["dead"], half["dead"]]))
    rows = P.make_rows(1024, dim, dt)
    return lay, np.concatenate([rows, rows])


@pytest.mark.parametrize("dt", ["f32", "i8"])
def test_ties_and_special_values(dt):
    """3. duplicates: the arg is the lower position everywhere, also for a pair on both sides of a 128-position block edge; a
    zero token under InnerProduct: every row scores +-0.0 and the key's first row wins; a key whose rows all hold a NaN: its
    lowest position and the results' NaN; a key with one NaN row among finite ones never returns that row (L2 and InnerProduct:
    under Cosine a NaN row's denominator is not > 0 and its score is 0 by §3, a tie with its copies)"""
    dim = 64
    lay, rows = _doubled_world(dt, dim)
    assert MS.spans_block_edge(lay), "with every key listed a key's rows lie on both sides of a block edge of the set's list"
    live, lkeys, starts, key_values = MS.key_order(lay)
    ends = np.concatenate([starts[1:], [lkeys.size]])
    crossing = [g for g in range(key_values.size) if starts[g] // 128 != (ends[g] - 1) // 128]
    pairs_split = 0
    for g in crossing:   # the pair (row, row + 1024) of a key of n live rows lies n / 2 list positions apart
        n = ends[g] - starts[g]
        at = np.arange(starts[g], starts[g] + n // 2)
        pairs_split += int(((at // 128) != ((at + n // 2) // 128)).sum())
    assert pairs_split > 0, "a duplicate pair lies on both sides of a block edge"
    first_row = {int(key_values[g]): int(live[starts[g]]) for g in range(key_values.size)}
    all_nan, one_nan = int(lay["keys"][2]), int(lay["keys"][3])
    nan_row = first_row[one_nan]
    if dt == "f32":
        rows[lay["col"] == np.uint32(all_nan), 7] = np.nan
        rows[[nan_row, nan_row + 1024], 3] = np.nan     # the key's lowest position and its duplicate
    w = World(dt, dim, lay, rows=rows)
    try:
        sets = MS.make_sets(2, T, dim, dt)
        sets[1, 2] = 0                                   # a zero token
        lists = np.stack([w.keys, w.keys[::-1]])         # every key: the set's list is the index's whole order
        for metric in METRICS:
            got = check(w, sets, lists, metric, f"duplicates, {dt}, metric {metric}")
            assert (got.rows < 1024).all(), "of two equal rows the lower position is the arg"
            if metric == IP:
                want = np.array([first_row[int(k)] for k in lists[1]], np.uint64)
                plain = np.ones(w.nk, bool) if dt != "f32" else ~np.isin(lists[1], [all_nan, one_nan])
                assert (got.rows[1, plain, 2] == want[plain]).all(), "a zero token: every row scores +-0.0, the key's first row wins"
                assert (got.scores[1, plain, 2].view(np.uint32) == 0).all(), "+0.0 stands for +-0.0"
            if dt == "f32":
                for q in range(2):
                    i_all, i_one = int(np.nonzero(lists[q] == all_nan)[0][0]), int(np.nonzero(lists[q] == one_nan)[0][0])
                    assert (got.rows[q, i_all] == first_row[all_nan]).all(), "every row NaN: the key's lowest position"
                    if metric == COS:   # §3: a Cosine whose denominator is not > 0 is 0, so a NaN row scores 0 and ties with its copies
                        assert (got.scores[q, i_all].view(np.uint32) == 0).all(), "Cosine of a NaN row is +0.0"
                        continue
                    assert (got.scores[q, i_all].view(np.uint32) == MS.NAN_BITS).all(), "and the NaN every result carries"
                    assert (got.rows[q, i_one] != nan_row).all() and not np.isnan(got.scores[q, i_one]).any(), "a NaN row among finite ones never wins"
    finally:
        w.close()


def _form_world(dt, dim, rows=None):
    return World(dt, dim, MS.form_layout(MS.form_rows(dim)), rows=rows)


def _form_check(w, dt, dim, nq, n_tokens, metric, what):
    assert MS.spans_block_edge(w.lay)
    sets = np.ascontiguousarray(MS.token_pool(dt, dim, 2, 33)[:nq, :n_tokens])
    rng = np.random.default_rng(P._seed("form lists", dt, dim))
    lists = np.stack([w.keys[rng.permutation(w.nk)] for _ in range(nq)])   # all keys: a key crosses a block edge
    check(w, sets, lists, metric, what)


LONG_CELLS = {("f32", 100): MS.REG, ("f32", 288): MS.REREAD, ("f32", 10241): MS.CACHE}   # one cell per form with T = 33 as well


@pytest.mark.parametrize("case", range(len(MS.FORM_CASES)), ids=[f"{dt}d{dim}" for dt, dim in MS.FORM_CASES])
def test_every_form_of_the_scoring_kernel(case):
    """4. identity 1 on every (type, dimension) cell of tests/_maxsim.py, one metric per case in rotation; T = 33 -- two chunks --
    on one cell per form"""
    dt, dim = MS.FORM_CASES[case]
    f = G.maxsim_form(MS.DTYPE[dt], dim)
    assert (f.G, f.J, f.form) == MS.FORM_CELLS[dt, dim], f"{dt} x {dim}: listed as {MS.FORM_CELLS[dt, dim]}, the library says {f}"
    metric = METRICS[case % 3]
    w = _form_world(dt, dim)
    try:
        _form_check(w, dt, dim, 2, 5, metric, f"{dt} x {dim}, form {f.form}, metric {metric}")
        if (dt, dim) in LONG_CELLS:
            assert f.form == LONG_CELLS[dt, dim]
            chunk = G.maxsim_align_plan(w.nk, 33, 1, f.token_bytes, 512 << 20)[0]
            assert -(-33 // chunk) == 2, "two chunks"
            _form_check(w, dt, dim, 1 if f.form == MS.CACHE else 2, 33, metric, f"{dt} x {dim}, form {f.form}, T 33")
    finally:
        w.close()


FORCED_CELLS = {1: (1, 50, MS.REREAD), 4: (4, 13, MS.REREAD), 8: (8, 7, MS.REREAD), 16: (16, 4, MS.REG), 32: (32, 2, MS.REG),
                64: (64, 1, MS.REG)}


@pytest.mark.parametrize("dt,dim", MS.FORCED_SHAPES, ids=[f"{dt}d{dim}" for dt, dim in MS.FORCED_SHAPES])
def test_forced_widths(dt, dim, monkeypatch):
    """4, continued: MVF_K1_G, read when the handle is created: rows of 50 vectors under each of the six widths"""
    rows = None
    for at, width in enumerate(MS.FORCED_WIDTHS):
        f = G.maxsim_form(MS.DTYPE[dt], dim, width)
        assert (f.G, f.J, f.form) == FORCED_CELLS[width]
        monkeypatch.setenv("MVF_K1_G", str(width))
        w = _form_world(dt, dim, rows)
        monkeypatch.delenv("MVF_K1_G")
        rows = w.rows
        try:
            _form_check(w, dt, dim, 2, 5, METRICS[at % 3], f"{dt} x {dim}, {width} lanes")
        finally:
            w.close()


def test_windows_and_chunks_give_the_default_budgets_bytes(worlds, monkeypatch):
    """5. MVF_MAXSIM_SCRATCH_BYTES, read when the handle is created, so small that the set with the most keys fits alone with a
    chunk of four tokens: at least 2 windows and a chunk below T = 9"""
    nq, n_tokens, m = 5, 9, 16
    for dt, dim, metric in (("f32", 100, COS), ("i8", 400, L2)):
        w = worlds(dt, dim)
        sets = MS.make_sets(nq, n_tokens, dim, dt)
        counts = [12, 3, 7, 1, 9]
        lists = MA.varied_lists(w.keys, counts, m, w.unheld + [int(PAD)], (dt, "windows"))
        d = [int(MC.held_distinct(l, w.keys).size) for l in lists]
        assert d == counts, "a different number of held keys per set"
        positions = [-(-int(w.key_rows[np.isin(w.keys, MC.held_distinct(l, w.keys))].sum()) // MC.BLOCK) * MC.BLOCK for l in lists]
        per_set = [8 * p + 4 * m + dq * MS.TOKEN_GROUP * MA.MIN_BYTES for dq, p in zip(d, positions)]
        tight, at = max(per_set), int(np.argmax(per_set))
        token_bytes = G.maxsim_form(MS.DTYPE[dt], dim).token_bytes
        chunk, window = G.maxsim_align_plan(d[at], n_tokens, 1, token_bytes, tight - 8 * positions[at] - 4 * m)
        assert (chunk, window) == (MS.TOKEN_GROUP, 1) and chunk < n_tokens, "the plan self-test: a chunk below T"
        other = 1 if at == 0 else 0
        assert 8 * (positions[at] + positions[other]) + 2 * 4 * m + 2 * max(d[at], d[other]) * MS.TOKEN_GROUP * MA.MIN_BYTES > tight, \
            "no second set fits beside the largest: at least 2 windows"
        whole = check(w, sets, lists, metric, f"{dt}: the default budget")
        monkeypatch.setenv("MVF_MAXSIM_SCRATCH_BYTES", str(tight))
        small = World(dt, dim, w.lay)
        monkeypatch.delenv("MVF_MAXSIM_SCRATCH_BYTES")
        try:
            cut = small.c.maxsim_align(sets, lists, metric, small.part)
            same_bytes(cut, (whole.rows, whole.scores, whole.raw), f"{dt}, budget {tight}: windows and chunks against the default budget")
        finally:
            small.close()


def test_edges(worlds):
    """6. one key of one row with nq = m = T = 1; a list of skipped entries only beside a set with candidates; m = 0; a stale
    partition"""
    w = worlds("f32", 100)
    lay = w.lay
    ones = w.keys[w.key_rows == 1]
    assert ones.size
    one = MS.make_sets(1, 1, 100, "f32")
    for metric in METRICS:
        got = check(w, one, ones[:1][None], metric, "nq = m = T = 1")
        assert got.rows.shape == (1, 1, 1) and got.rows[0, 0, 0] == P.reference_rows(lay, ones[0])[0]
    sets = MS.make_sets(2, 3, 100, "f32")
    lists = np.array([[lay["absent_key"], int(PAD), lay["dead_key"], int(PAD)], [lay["keys"][3], int(PAD), lay["keys"][5], lay["keys"][3]]], np.uint64)
    got = check(w, sets, lists, IP, "a set of skipped entries only")
    assert (got.rows[0] == PAD).all() and np.isneginf(got.scores[0]).all() and (got.rows[1, [0, 2, 3]] != PAD).all()
    assert (got.rows[1, 0] == got.rows[1, 3]).all(), "a key listed twice gets the same answer at both entries"
    only = check(w, sets, np.broadcast_to(lists[0], (2, 4)), L2, "no set holds a candidate")
    assert (only.rows == PAD).all() and np.isposinf(only.scores).all() and (only.raw == 0).all()
    shared = w.c.maxsim_align(sets, lists[1], COS, w.part)   # one list for every set
    same_bytes(shared, partitioned(w, sets, np.broadcast_to(lists[1], (2, 4)), COS), "a 1-D list serves every set")
    for none in (None, np.zeros((2, 0), np.uint64)):
        empty = w.c.maxsim_align(sets, none, L2, w.part)
        assert empty.rows.shape == empty.scores.shape == empty.raw.shape == (2, 0, 3)


def test_index_base_vector_ids_and_a_stale_partition():
    """6, continued: rows come back as index_base + row, or as the vector id -- duplicate ids included --, and new tombstones
    make the partition stale, with the candidate call's message"""
    lay = P.layout("u32", 2048, (300, 129, 128, 127, 64, 2, 1), 20)
    sets = MS.make_sets(2, T, 100, "f32")
    plain = World("f32", 100, lay)
    based = World("f32", 100, lay, rows=plain.rows, index_base=5000)
    ids = (np.arange(2048, dtype=np.uint64) // np.uint64(2)) * np.uint64(1 << 33) + np.uint64(9)   # every id twice
    named = World("f32", 100, lay, rows=plain.rows, ids=ids)
    try:
        lists = MC.mixed_lists(plain.keys, 2, 20, plain.unheld + [int(PAD)], "bases")
        want = check(plain, sets, lists, COS, "index_base 0")
        held = want.rows != PAD
        got = check(based, sets, lists, COS, "index_base 5000")
        assert (got.rows[held] == want.rows[held] + np.uint64(5000)).all() and (got.rows[~held] == PAD).all()
        got = check(named, sets, lists, COS, "vector ids attached")
        assert (got.rows[held] == ids[want.rows[held].astype(np.int64)]).all() and (got.rows[~held] == PAD).all()
        assert (got.scores.view(np.uint32) == want.scores.view(np.uint32)).all()
        plain.c.set_tombstones(np.packbits(lay["dead"] | (np.arange(2048) % 7 == 0), bitorder="little"))
        with pytest.raises(E.InvalidArgument, match="stale partition: mvfgpu_corpus_set_tombstones changed the handle's tombstones"):
            plain.c.maxsim_align(sets, lists, COS, plain.part)
    finally:
        for w in (plain, based, named):
            w.close()


def test_device_call_writes_every_byte_and_two_calls_queue_on_one_stream(worlds):
    """7. outputs pre-filled with 0xA5 on a non-null stream: every byte is the host call's; a second call queued behind it on the
    same stream, with other lists, is right without a host wait in between; the stage timer is the device call"""
    import torch
    for dt, dim, metric in (("f32", 100, COS), ("i8", 400, L2)):
        w = worlds(dt, dim)
        sets = MS.make_sets(NQ, T, dim, dt)
        lists = stock_lists(w, "device")
        other = np.ascontiguousarray(lists[::-1, ::-1])
        host, host2 = check(w, sets, lists, metric, "host call"), check(w, sets, other, metric, "host call, other lists")
        stream = torch.cuda.Stream()
        dq = torch.from_numpy(sets).cuda()
        n = NQ * M_LIST * T
        bufs = [[torch.full((n * size,), 0xA5, dtype=torch.uint8, device="cuda") for size in (4, 8, 4)] for _ in range(2)]
        torch.cuda.synchronize()
        qcode = 0 if dt == "f32" else 2
        for b, l in zip(bufs, (lists, other)):   # back to back: the second plan waits only for the first to have left the pinned buffer
            w.c.maxsim_align_device(w.part, dq.data_ptr(), qcode, dim, NQ, T, l, metric, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(),
                                    stream.cuda_stream)
        stream.synchronize()
        for b, want, what in ((bufs[0], host, "device call"), (bufs[1], host2, "the call queued behind it")):
            sc, rows, raw = (t.cpu().numpy().view(ty).reshape(NQ, M_LIST, T) for t, ty in zip(b, (np.float32, np.uint64, np.int32)))
            same_bytes(G.MaxSimAlignment(rows, sc, raw), (want.rows, want.scores, want.raw), f"{dt}: {what}")
        for t in bufs[0]:
            t.fill_(0xA5)
        ms = w.c.maxsim_align_stage_ms(w.part, dq.data_ptr(), qcode, dim, NQ, T, lists, metric, bufs[0][0].data_ptr(), bufs[0][1].data_ptr(),
                                       bufs[0][2].data_ptr(), stream.cuda_stream)
        assert len(ms) == 3 and all(0.0 < x < 1000.0 for x in ms)
        sc, rows, raw = (t.cpu().numpy().view(ty).reshape(NQ, M_LIST, T) for t, ty in zip(bufs[0], (np.float32, np.uint64, np.int32)))
        same_bytes(G.MaxSimAlignment(rows, sc, raw), (host.rows, host.scores, host.raw), f"{dt}: the stage timer's answer")
        # without out_raw nothing else changes
        w.c.maxsim_align_device(w.part, dq.data_ptr(), qcode, dim, NQ, T, lists, metric, bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), 0,
                                stream.cuda_stream)
        stream.synchronize()
        assert (bufs[1][1].cpu().numpy().view(np.uint64) == host.rows.reshape(-1)).all()


def test_a_fresh_process_gives_the_checked_answer_whatever_its_allocations_held(worlds, tmp_path):
    """8. the scenario of tests/_maxsim_align.py with the alignment as a child's first device work, every allocation of the
    library filled with 0xFF: one child, none after a fault"""
    inp = MC.fresh_inputs()
    w = worlds("f32", MA.FP_DIM)
    assert (w.rows == inp["rows"]).all() and (w.lay["col"] == inp["lay"]["col"]).all()
    want = check(w, inp["queries"], inp["lists"], MA.FP_METRIC, "fresh process, in this process")
    env = {k: v for k, v in os.environ.items() if k not in ("MVF_DEBUG_POISON", "MVF_MAXSIM_SCRATCH_BYTES", "MVF_K1_G")}
    env["MVF_DEBUG_POISON"] = "255"
    path = str(tmp_path / "poisonFF.npz")
    out = RUNNER.run([sys.executable, os.path.join(HERE, "_maxsim_align.py"), path], env=env)
    assert out.returncode == 0, f"exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
    with np.load(path) as z:
        assert z["poison"].tolist() == [255], "the child's poison byte"
        for call in ("host", "device"):
            got = G.MaxSimAlignment(z[call + ".rows"], z[call + ".scores"], z[call + ".raw"])
            same_bytes(got, (want.rows, want.scores, want.raw), f"the {call} call")


def _documents_file(tmp_path, oracle, name, tombstones):
    import metrovector_amd as M
    n, dim = 700, 12
    rng = np.random.default_rng(10)
    rows = oracle.synth_rows(91, 0, n, dim, 0)
    doc = rng.integers(0, 40, n).astype(np.uint64) << np.uint64(31)
    dead = (rng.random(n) < 0.2) & tombstones
    b = M.MvfBuilder()
    b.add_vector_space("s", dim, 0, 0, 0)
    b.add_vectors("s", rows)
    if tombstones:
        b.set_tombstones("s", 1, np.packbits(dead, bitorder="little").tobytes() + b"\0", int(dead.sum()))
    b.add_metadata_column("doc", 5, doc.astype("<u8").tobytes())
    b.add_metadata_column("few", 4, np.zeros(n - 1, "<u4").tobytes())
    path = str(tmp_path / name)
    b.build().save(path)
    return path, rows, doc, dead


def test_align_documents_reads_the_files_column_and_the_cpp_helper_agrees(tmp_path, oracle):
    """9. align_documents from a file with a metadata column equals GpuCorpus.maxsim_align, and a program over include/mvf.hpp
    (examples/cpp/align_documents.cpp, compiled with -Wall -Wextra -Werror against the built libraries) prints the same bytes"""
    import metrovector_amd as M
    path, rows, doc, dead = _documents_file(tmp_path, oracle, "documents.mvf", True)
    whole_path = _documents_file(tmp_path, oracle, "whole.mvf", False)[0]   # the C++ helper uploads a space without its deletions
    n_tokens, dim = 4, rows.shape[1]
    q = oracle.synth_queries(92, 2 * n_tokens, dim, 0).reshape(2, n_tokens, dim)
    keys = np.array([[3, 7, 7, 99, 12, 0], [39, 3, 41, 5, 5, 5]], np.uint64) << np.uint64(31)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        with c.attach_column(doc) as col, c.make_partition(col) as part:
            want = c.maxsim_align(q, keys, L2, part)
            sums = c.search_maxsim_candidates(q, keys, 6, L2, part)
    with G.GpuCorpus.from_array(rows) as c, c.attach_column(doc) as col, c.make_partition(col) as part:
        first = c.maxsim_align(rows[:n_tokens], keys[0], L2, part)
    with M.MvfReader.open(path) as r:
        space = r.vector_space("s")
        got = M.align_documents(space, q, keys, column="doc")
        same_bytes(got, (want.rows, want.scores, want.raw), "align_documents against GpuCorpus.maxsim_align")
        assert got.rows.shape == (2, 6, n_tokens) and (got.rows[0, 3] == PAD).all() and (got.rows[0, 1] == got.rows[0, 2]).all()
        one = M.align_documents(space, q[1], keys[1], column="doc")
        same_bytes(one, (want.rows[1:], want.scores[1:], want.raw[1:]), "one query set")
        for qi in range(2):   # the recipe: the scores of a returned document add up to its re-ranking score
            for g, s in zip(sums.keys[qi, :sums.counts[qi]], sums.scores[qi, :sums.counts[qi]]):
                i = int(np.nonzero(keys[qi] == g)[0][0])
                assert MA.token_sum(got.scores[qi, i:i + 1])[0].view(np.uint32) == s.view(np.uint32)
        with pytest.raises(E.BuildError, match="holds 699 values"):
            M.align_documents(space, q, keys, column="few")
    exe = str(tmp_path / "align_documents_cpp")
    libdir = os.path.join(ROOT, "metrovector_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "cpp", "align_documents.cpp"), "-L", libdir, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{libdir}", "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    out = RUNNER.run([exe, whole_path, "s", "doc", str(n_tokens)] + [str(int(k)) for k in keys[0]])
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == keys.shape[1], out.stdout
    for i, line in enumerate(lines):
        key, rest = line.split(":", 1)
        pairs = [p.split(":") for p in rest.split()]
        assert int(key) == int(keys[0, i]) and len(pairs) == n_tokens
        assert [int(p[0]) for p in pairs] == first.rows[0, i].tolist(), f"the C++ helper's rows, entry {i}"
        assert [int(p[1], 16) for p in pairs] == first.scores[0, i].view(np.uint32).tolist(), f"the C++ helper's score bits, entry {i}"
