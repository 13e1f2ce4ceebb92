"""-m gpu tests of the grouped search (DESIGN.md §3 "Grouped search"): every batch against identity 1 of the contract -- byte
for byte the walk (tests/_grouped.py) over the candidate search's ranking of ALL rows the partition holds --, identity 2 where
a cap of 64 reaches the largest key, identity 3 for three keys per batch, and the integer worlds against the walk over the
CPU oracle's full ranking.  8192 rows throughout; the layouts are tests/_grouped.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _grouped as GR
import _partitioned as P
from _candidates import oracle_candidates
from _children import RUNNER
from _dups import positions_of_ids
from _util import PAD
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "metrovector_amd")
L2, IP, COS = 0, 1, 2
CODE = {"f32": 0, "f16": 1, "i8": 2, "u8": 3}
INT = ("i8", "u8")

# (rows' type, dimension, metric): one query's lane groups of 1 (dim 4), 32 (100) and 64 (768) lanes, every type and metric
SHAPES = [("f32", 4, L2), ("f32", 100, COS), ("f32", 768, IP), ("f16", 128, IP), ("i8", 64, L2), ("u8", 200, COS)]
NQS = (1, 4, 5, 64)
LIVE5 = -1  # k = live + 5
# (k, per_key): every k and every cap of the contract's list
COMBOS = [(1, 1), (10, 1), (10, 3), (100, 2), (100, 63), (1024, 64), (1025, 3), (LIVE5, 1), (LIVE5, 64), (1024, 2)]
LAYOUTS = {"stock": GR.stock, "caps": GR.caps, "dominant": GR.dominant, "own": GR.own_keys, "one": GR.one_key}


class Ranking:
    """every query's full ranking of the held rows: scores / indices / raw [nq, live] and the local rows"""

    def __init__(self, scores, indices, raw, local):
        self.scores, self.indices, self.raw, self.local = scores, indices, raw, local


class World:
    """one corpus with its column and index, and the rankings the checks share"""

    def __init__(self, dt, dim, lay, index_base=0, ids=None, rows=None):
        self.dt, self.dim, self.base, self.ids, self.lay = dt, dim, index_base, ids, lay
        self.rows = P.make_rows(P.N, dim, dt) if rows is None else rows
        self.c = G.GpuCorpus.from_array(self.rows, index_base=index_base)
        self.c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        if ids is not None:
            self.c.set_vector_ids(ids)
        self.col = self.c.attach_column(lay["col"])
        self.part = self.c.make_partition(self.col)
        self.live = GR.live_rows(lay)
        self._rank, self._orank = {}, {}

    def entries(self, rows):
        return self.ids[rows] if self.ids is not None else rows.astype(np.uint64) + np.uint64(self.base)

    def local(self, idx):
        """local rows of reported entries; padding stays PAD"""
        idx = np.asarray(idx, np.uint64)
        if self.ids is not None:
            return positions_of_ids(self.ids, idx)
        return np.where(idx == PAD, PAD, idx - np.uint64(self.base))

    def rank(self, q, metric):
        """identity 1's C: the candidate search over the list of all held rows, k = their count"""
        memo = (q.tobytes(), metric)
        if memo not in self._rank:
            cand = np.ascontiguousarray(np.broadcast_to(self.entries(self.live), (q.shape[0], self.live.size)))
            c = self.c.search_candidates(q, cand, self.live.size, metric)
            assert (c.indices != PAD).all(), "every held row is ranked"
            self._rank[memo] = Ranking(c.scores, c.indices, c.raw, self.local(c.indices).astype(np.int64))
        return self._rank[memo]

    def oracle_rank(self, oracle, q, metric):
        """the CPU oracle's full ranking (integer types: bit-exact)"""
        memo = (q.tobytes(), metric)
        if memo not in self._orank:
            n = self.live.size
            out = [oracle_candidates(oracle, self.rows, CODE[self.dt], metric, qq, self.entries(self.live), n, index_base=self.base,
                                     ids=self.ids) for qq in q]
            ind = np.stack([o[2] for o in out])
            self._orank[memo] = Ranking(np.stack([o[1] for o in out]), ind, np.stack([o[3] for o in out]), self.local(ind).astype(np.int64))
        return self._orank[memo]

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


def same_bytes(a, b, what):
    assert (a.indices == b.indices).all(), f"{what}: indices"
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), f"{what}: score bits"
    assert (a.raw == b.raw).all(), f"{what}: raw"


def walk_result(rk, col, k, per_key, metric):
    """the contract's result rows from a ranking"""
    nq = rk.local.shape[0]
    s, i, r = np.empty((nq, k), np.float32), np.empty((nq, k), np.uint64), np.empty((nq, k), np.int32)
    for j in range(nq):
        places = GR.grouped_walk(rk.local[j], col, per_key, k)
        s[j], i[j], r[j] = GR.expected(rk.scores[j], rk.indices[j], rk.raw[j], places, k, metric)
    return G.SearchResult(s, i, r)


def check_batch(w, q, k, per_key, metric, what, oracle=None):
    """one grouped search against identity 1 and, for the integer types, the oracle's ranking"""
    if k == LIVE5:
        k = w.live.size + 5
    res = w.c.search_grouped(q, k, per_key, metric, w.part)
    assert res.scores.shape == res.indices.shape == res.raw.shape == (q.shape[0], k)
    what = f"{what}, k {k}, per_key {per_key}"
    same_bytes(res, walk_result(w.rank(q, metric), w.lay["col"], k, per_key, metric), f"{what}: identity 1")
    if oracle is not None and w.dt in INT:
        same_bytes(res, walk_result(w.oracle_rank(oracle, q, metric), w.lay["col"], k, per_key, metric), f"{what}: the oracle's ranking")
    return res


def check_identity_2(w, q, k, metric, what):
    """a cap no key reaches: the candidate search cut at k"""
    assert w.part.info().largest <= 64
    rk = w.rank(q, metric)
    res = w.c.search_grouped(q, k, 64, metric, w.part)
    cut = min(k, w.live.size)
    assert (res.indices[:, :cut] == rk.indices[:, :cut]).all() and (res.raw[:, :cut] == rk.raw[:, :cut]).all() and \
        (res.scores[:, :cut].view(np.uint32) == rk.scores[:, :cut].view(np.uint32)).all(), f"{what}: identity 2"
    assert (res.indices[:, cut:] == PAD).all()


def check_identity_3(w, q, per_key, metric, keys, what):
    """k >= per_key x n_keys: the entries carrying key g, in order, are the partitioned search's row for g, minus its padding"""
    nq = q.shape[0]
    k = per_key * int(w.part.info().n_keys)
    res = w.c.search_grouped(q, k, per_key, metric, w.part)
    loc = w.local(res.indices)
    hit_keys = np.where(res.indices == PAD, np.uint64(0), w.lay["col"].astype(np.uint64)[np.where(res.indices == PAD, 0, loc).astype(np.int64)])
    for g in keys:
        part = w.c.search_partitioned(q, [g] * nq, per_key, metric, w.part)
        for j in range(nq):
            sel = (res.indices[j] != PAD) & (hit_keys[j] == np.uint64(g))
            real = part.indices[j] != PAD
            assert int(sel.sum()) == int(real.sum()) == min(per_key, int(w.part.lookup([g])[0])), f"{what}: identity 3, key {g:#x}, query {j}"
            assert (res.indices[j][sel] == part.indices[j][real]).all() and (res.raw[j][sel] == part.raw[j][real]).all() and \
                (res.scores[j][sel].view(np.uint32) == part.scores[j][real].view(np.uint32)).all(), f"{what}: identity 3, key {g:#x}, query {j}"


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=[f"{dt}d{dim}m{m}" for dt, dim, m in SHAPES])
def test_every_batch_is_the_walk_over_the_candidate_searchs_ranking(oracle, worlds, case):
    dt, dim, metric = SHAPES[case]
    w = worlds(dt, dim, "stock", "u64" if case % 2 else "u32")
    lay = w.lay
    for nq in NQS:
        q = P.make_queries(nq, dim, dt)
        what = f"{dt} x {dim}, metric {metric}, nq {nq}"
        for k, per_key in COMBOS:
            check_batch(w, q, k, per_key, metric, what, oracle if nq <= 5 else None)
        # three keys per batch: the largest (it crosses tiles), one of 64 rows and one of 2
        check_identity_3(w, q, 3 if nq != 4 else 63, metric, [lay["keys"][0], lay["keys"][5], lay["keys"][6]], what)


@pytest.mark.parametrize("layout", ["caps", "dominant", "own", "one"])
def test_the_layouts(oracle, worlds, layout):
    """(b) sizes around the caps, the wave and G1's tier and tile boundaries; (c) a dominant key; (d) every row its own key;
    (e) one key for all rows"""
    for dt, dim, metric, flavour in (("f32", 100, COS, "u32"), ("i8", 64, L2, "u64")):
        w = worlds(dt, dim, layout, flavour)
        q = P.make_queries(5, dim, dt)
        what = f"layout {layout}, {dt} x {dim}"
        for per_key in GR.PER_KEYS:
            for k in (10, 100, LIVE5):
                res = check_batch(w, q, k, per_key, metric, what, oracle)
                real = (res.indices != PAD).sum(1)
                if layout == "one":
                    assert (real == min(len(res.indices[0]), per_key)).all(), "top-min(k, per_key), then padding"
                if layout == "own":
                    assert (real == min(len(res.indices[0]), w.live.size)).all()
        if layout == "own":  # the candidate search's result for any cap
            for k in (10, 1025, LIVE5):
                check_identity_2(w, q, w.live.size + 5 if k == LIVE5 else k, metric, what)
            rk = w.rank(q, metric)
            res = w.c.search_grouped(q, 100, 1, metric, w.part)
            assert (res.indices == rk.indices[:, :100]).all()
        if layout == "dominant":  # a 4x over-fetch at k = 100, per_key = 1 would not have filled these rows
            rk = w.rank(q, metric)
            for j in range(5):
                assert GR.grouped_walk(rk.local[j][:400], w.lay["col"], 1, 100).size < 100
            res = w.c.search_grouped(q, 100, 1, metric, w.part)
            assert (res.indices != PAD).all()
        keys, counts = w.part.keys()
        pick = [int(keys[int(np.argmax(counts))]), int(keys[0]), int(keys[-1])]
        check_identity_3(w, q, 2, metric, pick, what)


def test_all_rows_deleted_and_empty_indexes_give_padding():
    for flavour in ("u32", "u64"):
        lay = GR.all_dead(flavour)
        rows = P.make_rows(P.N, 16, "i8")
        with G.GpuCorpus.from_array(rows) as c:
            c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
            with c.attach_column(lay["col"]) as col, c.make_partition(col) as part:
                assert part.info().live_rows == 0
                for metric, pad in ((L2, np.inf), (IP, -np.inf)):
                    res = c.search_grouped(P.make_queries(3, 16, "i8"), 5, 2, metric, part)
                    assert (res.indices == PAD).all() and (res.scores == pad).all() and (res.raw == 0).all()
                assert (col.gather(res.indices) == 0).all()


def _dup_world(dt, dim):
    """every vector four times: half of the vectors with all copies in one key, the other half with every copy in another"""
    nv = P.N // 4
    rng = np.random.default_rng(P._seed("dups", dt, dim))
    group_of = np.repeat(np.arange(nv), 4)[rng.permutation(P.N)]   # scattered over all positions
    rows = np.ascontiguousarray(P.make_rows(nv, dim, dt)[group_of])
    copy = np.empty(P.N, np.int64)
    copy[np.argsort(group_of, kind="stable")] = np.arange(P.N) % 4  # 0 .. 3 in ascending position
    col = np.where(group_of < nv // 2, group_of % 40, 1000 + (group_of % 10) * 4 + copy).astype(np.uint32)
    dead = np.zeros(P.N, bool)
    dead[::10] = True
    return World(dt, dim, dict(col=col, dead=dead), rows=rows), group_of


@pytest.mark.parametrize("dt,dim,metric", [("f32", 100, L2), ("i8", 64, IP)])
def test_duplicated_rows_keep_their_lowest_positions(oracle, dt, dim, metric):
    w, group_of = _dup_world(dt, dim)
    try:
        q = P.make_queries(5, dim, dt)
        col, dead = w.lay["col"], w.lay["dead"]
        for per_key in (1, 2):
            for k in (10, 100, LIVE5):
                res = check_batch(w, q, k, per_key, metric, f"duplicates, {dt}", oracle)
                if k != 100:
                    continue
                for j in range(5):
                    hits = w.local(res.indices[j][res.indices[j] != PAD]).astype(np.int64)
                    assert hits.size == min(100, per_key * 80), "40 keys of whole vectors and 40 of single copies"
                    for r in hits.tolist():  # a copy in the same key at a lower position ranks in front of r: it was taken too
                        lower = np.nonzero((group_of[:r] == group_of[r]) & (col[:r] == col[r]) & ~dead[:r])[0]
                        assert np.isin(lower, hits).all(), f"query {j}: row {r} was kept, its lower copy was not"
    finally:
        w.close()


def test_nan_rows_come_last_and_count_towards_the_cap():
    lay = GR.stock("u32")
    rows = P.make_rows(P.N, 8, "f32")
    two, big = P.reference_rows(lay, lay["keys"][6]), P.reference_rows(lay, lay["keys"][5])  # keys of 2 and of 64 live rows
    rows[two] = np.nan                 # a key of NaN rows only
    rows[big[2:], 3] = np.nan          # a key with two real rows and 62 NaN rows
    w = World("f32", 8, lay, rows=rows)
    try:
        q = P.make_queries(5, 8, "f32")
        for per_key, nan_hits in ((1, 1), (2, 2), (3, 3), (64, 64)):
            res = check_batch(w, q, LIVE5, per_key, L2, "NaN rows")
            for j in range(5):
                real = res.indices[j] != PAD
                isnan = np.isnan(res.scores[j])
                assert int(isnan.sum()) == nan_hits and isnan[real][-nan_hits:].all(), "NaN last, in front of the padding"
                loc = w.local(res.indices[j][isnan]).astype(np.int64)
                want = list(two[:per_key]) + list(big[2:][:max(per_key - 2, 0)])  # the cap counts the key's two real rows
                assert sorted(loc.tolist()) == sorted(int(x) for x in want)
        check_batch(w, q, 10, 2, L2, "NaN rows")
    finally:
        w.close()


def test_vector_ids_index_base_and_the_keys_of_the_hits(oracle):
    ids = (np.random.default_rng(3).permutation(P.N).astype(np.uint64) * np.uint64(7) + np.uint64(5))
    w = World("i8", 64, GR.stock("u64"), index_base=1000, ids=ids)
    try:
        q = P.make_queries(5, 64, "i8")
        for k, per_key in ((10, 1), (100, 3), (LIVE5, 2)):
            res = check_batch(w, q, k, per_key, L2, "ids", oracle)
            real = res.indices != PAD
            assert np.isin(res.indices[real], ids).all(), "results carry vector ids"
            keys = w.col.gather(res.indices)
            assert keys.shape == res.indices.shape and keys.dtype == np.uint64
            assert (keys[real] == w.lay["col"][w.local(res.indices)[real].astype(np.int64)]).all() and (keys[~real] == 0).all()
            for j in range(5):  # at most per_key hits of any key
                assert np.unique(keys[j][real[j]], return_counts=True)[1].max() <= per_key
        with pytest.raises(E.IndexOutOfBounds, match="vector id 3 is not in this shard"):
            w.col.gather([ids[0], 3])
    finally:
        w.close()
    w = World("f32", 100, GR.stock("u32"), index_base=1000)
    try:
        res = check_batch(w, P.make_queries(5, 100, "f32"), 100, 2, COS, "index_base")
        real = res.indices != PAD
        assert res.indices[real].min() >= 1000 and res.indices[real].max() < 1000 + P.N
        assert (w.col.gather(res.indices)[real] == w.lay["col"][(res.indices[real] - np.uint64(1000)).astype(np.int64)]).all()
        assert w.col.gather(np.array([PAD, 1000, 1000 + P.N - 1], np.uint64)).tolist() == [0, int(w.lay["col"][0]), int(w.lay["col"][-1])]
        for foreign in (5, 999, 1000 + P.N):
            with pytest.raises(E.IndexOutOfBounds):
                w.col.gather([1000, foreign])
        assert w.col.gather(np.zeros((0,), np.uint64)).size == 0
    finally:
        w.close()


def test_device_call_equals_the_host_call(worlds):
    import torch
    w = worlds("f32", 100, "stock", "u64")
    q = P.make_queries(64, 100, "f32")
    for k, per_key in ((10, 1), (1025, 3)):
        host = w.c.search_grouped(q, k, per_key, COS, w.part)
        dq = torch.from_numpy(q).cuda()
        ds = torch.empty((64, k), dtype=torch.float32, device="cuda")
        di = torch.empty((64, k), dtype=torch.int64, device="cuda")
        dr = torch.empty((64, k), dtype=torch.int32, device="cuda")
        w.c.search_grouped_device(w.part, dq.data_ptr(), 0, 100, 64, k, per_key, COS, ds.data_ptr(), di.data_ptr(), dr.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        same_bytes(host, G.SearchResult(ds.cpu().numpy(), di.cpu().numpy().view(np.uint64), dr.cpu().numpy()), f"device call, k {k}")
        # the stage timer is the device call with events between its stages
        ds.zero_(), di.zero_()
        ms = w.c.grouped_stage_ms(w.part, dq.data_ptr(), 0, 100, 64, k, per_key, COS, ds.data_ptr(), di.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        assert len(ms) == 4 and all(0.0 <= x < 1000.0 for x in ms) and ms[1] > 0.0
        assert (di.cpu().numpy().view(np.uint64) == host.indices).all() and (ds.cpu().numpy().view(np.uint32) == host.scores.view(np.uint32)).all()


def test_staleness_ownership_and_the_handles_other_searches():
    import torch
    lay = GR.stock("u32")
    rows = P.make_rows(P.N, 64, "i8")
    q = P.make_queries(4, 64, "i8")
    q64 = P.make_queries(64, 64, "i8")
    with G.GpuCorpus.from_array(rows) as c, G.GpuCorpus.from_array(rows[:100]) as other:
        c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        before, before64 = c.search(q, 10, L2), c.search(q64, 10, L2)
        state = c.info().selection_state
        with c.attach_column(lay["col"]) as col, other.attach_column(lay["col"][:100].copy()) as ocol:
            part = c.make_partition(col)
            opart = other.make_partition(ocol)
            first = c.search_grouped(q, 10, 2, L2, part)
            c.search_grouped(q64, 100, 1, L2, part)
            with pytest.raises(E.InvalidArgument, match="another corpus handle"):
                c.search_grouped(q, 10, 2, L2, opart)
            with pytest.raises(E.InvalidArgument, match="per_key must be in 1..64, got 65"):
                c.search_grouped(q, 10, 65, L2, part)
            with pytest.raises(E.InvalidArgument, match="per_key must be in 1..64, got 0"):
                c.search_grouped(q, 10, 0, L2, part)
            with pytest.raises(E.DimensionMismatch):
                c.search_grouped(q[:, :63], 10, 2, L2, part)
            with pytest.raises(E.BuildError):
                c.search_grouped(q.astype(np.float32), 10, 2, L2, part)
            # the handle's plain searches answer as before and its state is what it was
            same_bytes(before, c.search(q, 10, L2), "a plain search after grouped ones")
            same_bytes(before64, c.search(q64, 10, L2), "a batched plain search after grouped ones")
            assert c.info().selection_state == state
            # new tombstones: the old index is stale, a new one leaves the newly deleted rows out
            gone = (first.indices[0][:3]).astype(np.int64)
            dead2 = lay["dead"].copy()
            dead2[gone] = True
            c.set_tombstones(np.packbits(dead2, bitorder="little"))
            with pytest.raises(E.InvalidArgument, match="stale partition: mvfgpu_corpus_set_tombstones changed the handle's tombstones"):
                c.search_grouped(q, 10, 2, L2, part)
            torch.cuda.synchronize()  # the refusals left no device error behind
            with c.make_partition(col) as part2:
                second = c.search_grouped(q, 10, 2, L2, part2)
                assert not np.isin(second.indices, gone.astype(np.uint64)).any() and (second.indices != PAD).all()
            part.close()
            opart.close()


def test_more_queries_than_one_window(worlds):
    """1100 queries: two windows of the device work (1024 queries at most each); a query's row does not depend on its batch"""
    w = worlds("f32", 4, "stock", "u32")
    q = P.make_queries(1100, 4, "f32")
    res = w.c.search_grouped(q, 10, 2, L2, w.part)
    for j0 in (0, 1020, 1095):
        part = check_batch(w, q[j0:j0 + 5], 10, 2, L2, f"queries {j0} .. {j0 + 5} of 1100")
        same_bytes(G.SearchResult(res.scores[j0:j0 + 5], res.indices[j0:j0 + 5], res.raw[j0:j0 + 5]), part, f"queries from {j0} of 1100")
    for j0 in range(0, 1100, 100):
        part = w.c.search_grouped(q[j0:j0 + 100], 10, 2, L2, w.part)
        same_bytes(G.SearchResult(res.scores[j0:j0 + 100], res.indices[j0:j0 + 100], res.raw[j0:j0 + 100]), part, f"queries from {j0} of 1100")


def test_a_host_window_beyond_the_pinned_mirrors_equals_its_pinned_slices(worlds):
    """256 queries at k = 300 are 256 x 300 x 16 B = 1.17 MiB of results: over the 1 MiB up to which a host window travels
    through the handle's pinned mirrors, so the call copies from and to the caller's buffers.  Slices of 32 queries (150 KiB)
    take the mirrors; a query's row does not depend on its batch, so every byte is the same."""
    w = worlds("f32", 8, "stock", "u32")
    nq, k, per_key = 256, 300, 3
    assert nq * k * 16 > 1 << 20 >= 32 * (k * 16 + 8 * 4)
    q = P.make_queries(nq, 8, "f32")
    whole = w.c.search_grouped(q, k, per_key, L2, w.part)
    for j0 in range(0, nq, 32):
        part = w.c.search_grouped(q[j0:j0 + 32], k, per_key, L2, w.part)
        for name in ("scores", "indices", "raw"):
            assert getattr(whole, name)[j0:j0 + 32].tobytes() == getattr(part, name).tobytes(), f"{name} of queries from {j0}"


def test_a_fresh_process_gives_the_checked_answer_whatever_its_allocations_held(worlds, tmp_path):
    """the scenario of tests/_grouped.py with the grouped search as a child's first device work: plain, then with every
    allocation of the library filled with 0x00 and with 0xFF; one child at a time, none after a fault"""
    inp = GR.fresh_inputs()
    w = worlds("f32", GR.FP_DIM, "stock", "u32")
    assert (w.rows == inp["rows"]).all() and (w.lay["col"] == inp["lay"]["col"]).all()
    res = check_batch(w, inp["queries"], GR.FP_K, GR.FP_PER_KEY, GR.FP_METRIC, "fresh process, in this process")
    want = P.digest(res.scores, res.indices, res.raw)
    want_keys = w.col.gather(res.indices)
    for tag, poison in (("plain", None), ("poison00", 0), ("poisonFF", 255)):
        env = {k: v for k, v in os.environ.items() if k not in ("MVF_DEBUG_POISON", "MVF_FILTER_ROUTE", "MVF_LARGE_K")}
        if poison is not None:
            env["MVF_DEBUG_POISON"] = str(poison)
        path = str(tmp_path / f"{tag}.npz")
        out = RUNNER.run([sys.executable, os.path.join(HERE, "_grouped.py"), path], env=env)
        assert out.returncode == 0, f"{tag}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
        with np.load(path) as z:
            assert z["poison"].tolist() == [-1 if poison is None else poison], f"{tag}: the child's poison byte"
            for call in ("host", "device"):
                got = P.digest(z[call + ".scores"], z[call + ".indices"], z[call + ".raw"])
                assert got == want, f"{tag}: the {call} call's answer differs from the checked one"
            assert (z["host.keys"] == want_keys).all(), f"{tag}: the hits' keys"


_CPP = r"""
#include "mvf.hpp"
#include <cstdio>
int main(int argc, char** argv) {
    using namespace mvf;
    if (argc < 2) return 2;
    try {
        std::vector<std::vector<float>> rows;
        std::vector<uint32_t> doc;
        for (int i = 0; i < 60; i++) {
            rows.push_back({(float)i, 1.0f, 0.0f, 0.0f});
            doc.push_back((uint32_t)(i / 10));   // documents of ten passages
        }
        MvfBuilder b;
        b.add_vector_space("s", 4, VectorType::Dense, DistanceMetric::L2, DataType::Float32);
        b.add_vectors("s", rows);
        b.add_metadata_column("doc", doc);
        b.add_metadata_column("short", std::vector<uint32_t>(59, 0));
        b.build().save(argv[1]);
        MvfReader r = MvfReader::open(argv[1]);
        const GpuVectorSpace resident(r.vector_space("s"));
        const std::vector<float> queries = {21.0f, 1.0f, 0.0f, 0.0f, 3.0f, 1.0f, 0.0f, 0.0f};
        std::vector<std::vector<uint64_t>> keys;
        const auto hits = resident.find_top_k_grouped(queries, 4, 1, r.metadata_column("doc"), &keys);
        for (size_t q = 0; q < hits.size(); q++) {
            for (size_t i = 0; i < hits[q].size(); i++)
                std::printf("%llu:%.1f:%llu ", (unsigned long long)hits[q][i].index, hits[q][i].score, (unsigned long long)keys[q][i]);
            std::printf("|\n");
        }
        const auto two = resident.find_top_k_grouped(queries, 5, 2, r.metadata_column("doc"));
        for (const ScoredVector& v : two[0]) std::printf("%llu ", (unsigned long long)v.index);
        std::printf("|\n%zu\n", resident.find_top_k_grouped(queries, 40, 3, r.metadata_column("doc"))[1].size());
        try { resident.find_top_k_grouped(queries, 4, 1, r.metadata_column("short")); } catch (const MvfError&) { std::printf("short column refused\n"); }
        try { resident.find_top_k_grouped(queries, 4, 65, r.metadata_column("doc")); } catch (const MvfError&) { std::printf("per_key 65 refused\n"); }
    } catch (const MvfError& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
"""


def test_cpp_find_top_k_grouped(tmp_path):
    src, exe = tmp_path / "grouped.cpp", str(tmp_path / "grouped_cpp")
    src.write_text(_CPP)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", LIBDIR, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = RUNNER.run([exe, str(tmp_path / "grouped.mvf")])
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ["21:0.0:2", "19:2.0:1", "30:9.0:3", "9:12.0:0", "|"]
    assert lines[1].split() == ["3:0.0:0", "10:7.0:1", "20:17.0:2", "30:27.0:3", "|"]
    assert lines[2].split() == ["21", "20", "19", "18", "30", "|"], "two passages per document; 20 before 22 on the tie"
    assert lines[3] == "18", "six documents, three passages each"
    assert lines[4] == "short column refused" and lines[5] == "per_key 65 refused"


def test_find_top_k_grouped_reads_the_files_column(tmp_path, oracle):
    import metrovector_amd as M
    n, dim = 700, 12
    rng = np.random.default_rng(10)
    rows = oracle.synth_rows(91, 0, n, dim, 0)
    q = oracle.synth_queries(92, 6, dim, 0)
    doc = rng.integers(0, 40, n).astype(np.uint64) << np.uint64(31)
    dead = rng.random(n) < 0.2
    b = M.MvfBuilder()
    b.add_vector_space("s", dim, 0, 0, 0)
    b.add_vectors("s", rows)
    b.set_tombstones("s", 1, np.packbits(dead, bitorder="little").tobytes() + b"\0", int(dead.sum()))  # an odd block in front of the column
    b.add_metadata_column("doc", 5, doc.astype("<u8").tobytes())
    b.add_metadata_column("few", 4, np.zeros(n - 1, "<u4").tobytes())
    b.add_metadata_column("label", 6, b"x" * (4 * n))
    path = str(tmp_path / "grouped.mvf")
    b.build().save(path)
    with M.MvfReader.open(path) as r:
        space = r.vector_space("s")
        for k, per_key in ((10, 1), (50, 2), (200, 3)):
            got, keys = M.find_top_k_grouped(space, q, k, column="doc", per_key=per_key)
            assert got.indices.shape == keys.shape == (6, k)
            for j in range(6):
                real = got.indices[j] != PAD
                assert (keys[j][real] == doc[got.indices[j][real].astype(np.int64)]).all() and (keys[j][~real] == 0).all()
                assert not dead[got.indices[j][real].astype(np.int64)].any()
                assert int(real.sum()) == min(k, per_key * 40)
                d = ((rows[~dead].astype(np.float64) - q[j].astype(np.float64)) ** 2).sum(1)
                live = np.nonzero(~dead)[0]
                ranked = live[np.lexsort((live, d))]
                places = GR.grouped_walk(ranked, doc, per_key, k)
                assert set(got.indices[j][real].tolist()) == set(ranked[places].tolist()), (k, per_key, j)
        with M.upload_space(space, first=300, count=250) as c:  # a corpus that holds a row range reads its own part
            got, keys = M.find_top_k_grouped(space, q[:2], 9, column="doc", per_key=1, corpus=c)
            real = got.indices != PAD
            assert real.all() and (got.indices >= 300).all() and (got.indices < 550).all()
            assert (keys == doc[got.indices.astype(np.int64)]).all()
        with pytest.raises(E.BuildError, match="holds 699 values"):
            M.find_top_k_grouped(space, q, 3, column="few")
        with pytest.raises(E.BuildError, match="Unsupported metadata column data type"):
            M.find_top_k_grouped(space, q, 3, column="label")
        with pytest.raises(E.VectorSpaceNotFound, match="Metadata column not found"):
            M.find_top_k_grouped(space, q, 3, column="nope")
