"""-m gpu tests of the multi-vector search (DESIGN.md §3 "Multi-vector search").  The yardstick is the recipe the call replaces,
built from the existing API: every token through search_grouped(per_key = 1, k = n_keys), the hits' keys from GpuColumn.gather,
the per-key sum in numpy f32 in token order, the keys ordered by (order key, key value) -- search_maxsim must return exactly
those score bits, keys and counts.  Beside it: the float64 contract reference within §3's tolerance scaled by the tokens, the
chunked and windowed call against the unchunked one, wide rows on the kernel's two other forms, edge tokens, the device call,
the generation rules and a fresh process.  8192 rows and the layouts of tests/_grouped.py unless stated.
Run time on an MI355X: the 29 tests take 6 s together, the slowest 2 s (it also pays the first use of the device)."""
import os
import sys

import numpy as np
import pytest

import _dups as D
import _grouped as GR
import _maxsim as MS
import _partitioned as P
from _children import RUNNER
from _maxsim_world import World, check_sets, expected, ks_of, same_bytes
from _util import PAD, TOL
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


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=[f"{dt}d{dim}" for dt, dim in SHAPES])
def test_every_call_is_the_recipe_of_grouped_searches(worlds, case):
    dt, dim = SHAPES[case]
    w = worlds(dt, dim, "stock", "u64" if case % 2 else "u32")
    for metric in METRICS:
        for T in TOKENS:
            for nq in NQS:
                check_sets(w, MS.make_sets(nq, T, dim, dt), metric, f"{dt} x {dim}, metric {metric}, T {T}, nq {nq}")


@pytest.mark.parametrize("flavour", ["u32", "u64"])
@pytest.mark.parametrize("layout", ["caps", "dominant", "own_keys", "one_key"])
def test_the_layouts(worlds, layout, flavour):
    """sizes around the wave, 128 and the 1024-tile, each +-1; a dominant key; every row its own key; one key for all rows"""
    for dt, dim, metric in (("f32", 100, COS), ("i8", 64, L2)):
        w = worlds(dt, dim, layout, flavour)
        for T, nq in ((3, 3), (33, 1)):
            if layout == "own_keys" and T == 33:
                T = 5  # 7372 keys: the recipe's lists are n_keys long per token
            check_sets(w, MS.make_sets(nq, T, dim, dt), metric, f"layout {layout} {flavour}, {dt} x {dim}, T {T}")


def test_all_rows_deleted_gives_padding_and_counts_of_zero():
    for flavour in ("u32", "u64"):
        lay = GR.all_dead(flavour)
        w = World("i8", 16, lay)
        try:
            assert w.part.info().live_rows == 0
            for metric, pad in ((L2, np.inf), (IP, -np.inf)):
                res = w.c.search_maxsim(MS.make_sets(3, 5, 16, "i8"), 7, metric, w.part)
                assert (res.keys == PAD).all() and (res.scores == pad).all() and (res.counts == 0).all()
        finally:
            w.close()


@pytest.mark.parametrize("dtype,metric", [(0, L2), (1, IP)])
def test_duplicated_rows_tie_bit_for_bit_and_rank_by_key_value(dtype, metric):
    """tests/_dups.py's corpus of 24 distinct vectors: every key of position % 50 holds copies of nearly all of them, so most
    keys carry identical sums"""
    dim = 48
    cp = D.corpus_b(P._seed("maxsim dups", dtype), P.N, dim, dtype)
    dead = D.tombstones(5, P.N)
    col = (np.arange(P.N) % 50).astype(np.uint32) * np.uint32(9)
    w = World("f16" if dtype else "f32", dim, dict(col=col, dead=dead), rows=cp.rows)
    try:
        sets = D.gaussian_queries(77, 3 * 5, dim).reshape(3, 5, dim)
        best = check_sets(w, sets, metric, f"duplicates, dtype {dtype}")
        S = MS.rank_keys(best[0], w.keys, metric, w.nk)[0]
        assert np.unique(S.view(np.uint32)).size <= w.nk // 2, "many keys tie bit for bit"
    finally:
        w.close()


def test_chunks_and_windows_give_the_unchunked_bytes(worlds, monkeypatch):
    """MVF_MAXSIM_SCRATCH_BYTES, read when the handle is created, so small that T = 33 takes at least 3 chunks and nq = 3 at
    least 2 windows"""
    for dt, dim, metric in (("f32", 100, COS), ("f16", 776, L2), ("i8", 64, IP)):
        w = worlds(dt, dim, "stock", "u32")
        budget = w.nk * (8 * 4 + MS.KEY_BYTES)
        chunk, window = G.maxsim_plan(w.nk, 33, 3, 16, budget)
        assert -(-33 // chunk) >= 3 and -(-3 // window) >= 2, "the LDS share can only shorten the chunk further"
        monkeypatch.setenv("MVF_MAXSIM_SCRATCH_BYTES", str(budget))
        small = World(dt, dim, w.lay)
        monkeypatch.delenv("MVF_MAXSIM_SCRATCH_BYTES")
        try:
            sets = MS.make_sets(3, 33, dim, dt)
            best = check_sets(w, sets, metric, f"{dt}: one chunk per 32 tokens")
            for k in ks_of(w):
                whole, cut = w.c.search_maxsim(sets, k, metric, w.part), small.c.search_maxsim(sets, k, metric, small.part)
                same_bytes(cut, whole, f"{dt}, k {k}: chunked against unchunked")
                same_bytes(cut, expected(w, best, metric, k), f"{dt}, k {k}: chunked against the recipe")
        finally:
            small.close()


@pytest.mark.parametrize("dim", [4100, 12000])
def test_wide_rows(dim):
    """2048 Float32 rows: 4100 dimensions are 17 steps per lane -- beyond the registers, the rows are read again per token
    group, two padded tokens fill the LDS share --, 12000 dimensions are a padded token of 47 KiB that is read through the cache"""
    lay = P.layout("u32", 2048, (300, 129, 128, 127, 64, 2, 1), 20)
    w = World("f32", dim, lay)
    try:
        for metric in (L2, COS):
            check_sets(w, MS.make_sets(2, 5, dim, "f32"), metric, f"f32 x {dim}, metric {metric}", ks=(10, w.nk + 3))
    finally:
        w.close()


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
    """independent of every kernel: b(t, g) and S in float64; every returned sum within the sum over tokens of §3's tolerance
    of a row score, the list in (order key, key value) order, and the set of keys right up to sums within two such tolerances
    of the k-th -- boundary ties only at the k-th rank"""
    w = worlds("f32", 100, "stock", "u32")
    T, nq = 5, 3
    sets = MS.make_sets(nq, T, 100, "f32")
    b, tol = MS.f64_key_bests(w.rows, w.lay, sets.reshape(nq * T, 100), TOL)[metric]
    for k in (1, 10, w.nk):
        got = w.c.search_maxsim(sets, k, metric, w.part)
        for j in range(nq):
            MS.assert_f64_contract(got.scores[j], got.keys[j], w.keys, b[j * T:(j + 1) * T].sum(0), tol[j * T:(j + 1) * T].sum(0), metric, k)


def _library_row_scores(w, q, metric):
    """f32 [nq, live]: the score a search reports for every (query, held row), in the held rows' order"""
    cand = np.ascontiguousarray(np.broadcast_to(w.live.astype(np.uint64), (q.shape[0], w.live.size)))
    c = w.c.search_candidates(q, cand, w.live.size, metric)
    out = np.empty((q.shape[0], w.live.size), np.float32)
    np.put_along_axis(out, np.searchsorted(w.live, c.indices.astype(np.int64)), c.scores, 1)
    return out


@pytest.mark.parametrize("metric", METRICS)
def test_edge_tokens(worlds, metric):
    """§3 "Values at the edges": a NaN token (L2 / InnerProduct: every row and so every key's sum NaN, the keys in ascending
    value; Cosine: 0 for every row), a +Inf element (L2 +inf, InnerProduct +-inf, Cosine NaN for every row) and, under Cosine, a
    zero token (0 for every row: adds +0.0).  Expected: the contract reference over
    row scores that are the library's for the ordinary tokens and IEEE's for the edge token, whose class is asserted"""
    w = worlds("f32", 100, "stock", "u32")
    T = 4
    base = MS.make_sets(1, T, 100, "f32")[0]
    row_keys = w.lay["col"][w.live].astype(np.uint64)
    ordinary = _library_row_scores(w, base, metric)
    edges = {"nan": np.full(100, np.nan, np.float32), "inf": base[2].copy()}
    edges["inf"][0] = np.inf
    if metric == COS:
        edges["zero"] = np.zeros(100, np.float32)
    for name, token in edges.items():
        for at in (0, 2, T - 1):
            sets = base.copy()[None]
            sets[0, at] = token
            s = ordinary.copy()
            s[at] = _f64_row_scores(w.rows[w.live], token, metric).astype(np.float32)
            if (name == "nan" and metric != COS) or (name == "inf" and metric == COS):
                assert np.isnan(s[at]).all()
            elif name == "inf":
                assert np.isinf(s[at]).all() and (metric == IP or (s[at] > 0).all())
            else:
                assert (s[at] == 0).all()
            for k in (10, w.nk + 3):
                want = MS.vectorised(s, row_keys, metric, k)
                got = w.c.search_maxsim(sets, k, metric, w.part)
                assert (got.keys[0] == want[1]).all() and (got.scores[0].view(np.uint32) == want[0].view(np.uint32)).all() and \
                    got.counts[0] == want[2], f"{name} token at {at}, metric {metric}, k {k}"
            if np.isnan(s[at]).all():
                assert np.isnan(got.scores[0][:w.nk]).all() and (got.keys[0][:w.nk] == w.keys).all()
            check_sets(w, sets, metric, f"{name} token at {at}: the recipe", ks=(10,))


def test_device_call_equals_the_host_call_and_the_stage_timer_is_the_device_call(worlds):
    import torch
    w = worlds("f32", 100, "stock", "u64")
    nq, T = 3, 33
    sets = MS.make_sets(nq, T, 100, "f32")
    for k in (10, w.nk + 3):
        host = w.c.search_maxsim(sets, k, COS, w.part)
        dq = torch.from_numpy(sets).cuda()
        ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        dk = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        dc = torch.empty((nq,), dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        w.c.search_maxsim_device(w.part, dq.data_ptr(), 0, 100, nq, T, k, COS, ds.data_ptr(), dk.data_ptr(), dc.data_ptr(), stream)
        torch.cuda.synchronize()
        dev = G.MaxSimResult(ds.cpu().numpy(), dk.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint32))
        same_bytes(dev, host, f"device call, k {k}")
        ds.zero_(), dk.zero_()
        w.c.search_maxsim_device(w.part, dq.data_ptr(), 0, 100, nq, T, k, COS, ds.data_ptr(), dk.data_ptr(), 0, stream)  # no counts
        ms = w.c.maxsim_stage_ms(w.part, dq.data_ptr(), 0, 100, nq, T, k, COS, ds.data_ptr(), dk.data_ptr(), stream)
        assert len(ms) == 4 and all(0.0 <= x < 1000.0 for x in ms) and ms[1] > 0.0
        assert (dk.cpu().numpy().view(np.uint64) == host.keys).all() and (ds.cpu().numpy().view(np.uint32) == host.scores.view(np.uint32)).all()


def test_staleness_ownership_and_the_handles_other_searches():
    import torch
    lay = GR.stock("u32")
    rows = P.make_rows(P.N, 64, "i8")
    q, q64 = P.make_queries(4, 64, "i8"), P.make_queries(64, 64, "i8")
    sets = MS.make_sets(2, 5, 64, "i8")
    with G.GpuCorpus.from_array(rows) as c, G.GpuCorpus.from_array(rows[:100]) as other:
        c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        before, before64 = c.search(q, 10, L2), c.search(q64, 10, L2)
        state = c.info().selection_state
        with c.attach_column(lay["col"]) as col, other.attach_column(lay["col"][:100].copy()) as ocol:
            part, opart = c.make_partition(col), other.make_partition(ocol)
            first = c.search_maxsim(sets, 10, L2, part)
            with pytest.raises(E.InvalidArgument, match="another corpus handle"):
                c.search_maxsim(sets, 10, L2, opart)
            with pytest.raises(E.InvalidArgument, match="n_tokens must be in 1..1024, got 1025"):
                c.search_maxsim(np.zeros((1, 1025, 64), np.int8), 10, L2, part)
            with pytest.raises(E.InvalidArgument, match="n_tokens must be in 1..1024, got 0"):
                c.search_maxsim(np.zeros((1, 0, 64), np.int8), 10, L2, part)
            with pytest.raises(E.DimensionMismatch):
                c.search_maxsim(sets[:, :, :63], 10, L2, part)
            with pytest.raises(E.BuildError):
                c.search_maxsim(sets.astype(np.float32), 10, L2, part)
            for a, b, what in ((before, c.search(q, 10, L2), "a plain search"), (before64, c.search(q64, 10, L2), "a batched plain search")):
                assert (a.indices == b.indices).all() and (a.raw == b.raw).all() and (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), what
            assert c.info().selection_state == state
            # new tombstones: the old index is stale; a new one answers without the deleted key
            gone = int(first.keys[0][0])
            dead2 = lay["dead"] | (lay["col"].astype(np.uint64) == np.uint64(gone))
            c.set_tombstones(np.packbits(dead2, bitorder="little"))
            with pytest.raises(E.InvalidArgument, match="stale partition: mvfgpu_corpus_set_tombstones changed the handle's tombstones"):
                c.search_maxsim(sets, 10, L2, part)
            torch.cuda.synchronize()  # the refusals left no device error behind
            with c.make_partition(col) as part2:
                second = c.search_maxsim(sets, 10, L2, part2)
                assert not (second.keys == np.uint64(gone)).any() and (second.counts == 10).all()
            part.close()
            opart.close()


def test_a_fresh_process_gives_the_checked_answer_whatever_its_allocations_held(worlds, tmp_path):
    """the scenario of tests/_maxsim.py with the multi-vector search as a child's first device work: plain, then with every
    allocation of the library filled with 0x00 and with 0xFF; one child at a time, none after a fault"""
    inp = MS.fresh_inputs()
    w = worlds("f32", MS.FP_DIM, "stock", "u32")
    assert (w.rows == inp["rows"]).all() and (w.lay["col"] == inp["lay"]["col"]).all()
    best = check_sets(w, inp["queries"], MS.FP_METRIC, "fresh process, in this process", ks=(MS.FP_K,))
    want = expected(w, best, MS.FP_METRIC, MS.FP_K)
    for tag, poison in (("plain", None), ("poison00", 0), ("poisonFF", 255)):
        env = {k: v for k, v in os.environ.items() if k not in ("MVF_DEBUG_POISON", "MVF_MAXSIM_SCRATCH_BYTES")}
        if poison is not None:
            env["MVF_DEBUG_POISON"] = str(poison)
        path = str(tmp_path / f"{tag}.npz")
        out = RUNNER.run([sys.executable, os.path.join(HERE, "_maxsim.py"), path], env=env)
        assert out.returncode == 0, f"{tag}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
        with np.load(path) as z:
            assert z["poison"].tolist() == [-1 if poison is None else poison], f"{tag}: the child's poison byte"
            for call in ("host", "device"):
                same_bytes(G.MaxSimResult(z[call + ".scores"], z[call + ".keys"], z[call + ".counts"]), want, f"{tag}: the {call} call")


def test_find_top_k_documents_reads_the_files_column(tmp_path, oracle):
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
    with M.MvfReader.open(path) as r:
        space = r.vector_space("s")
        got = M.find_top_k_documents(space, q, 45, column="doc")
        one = M.find_top_k_documents(space, q[1], 45, column="doc")
        assert got.scores.shape == got.keys.shape == (2, 45) and (got.counts == 40).all()
        assert (one.keys[0] == got.keys[1]).all() and (one.scores[0].view(np.uint32) == got.scores[1].view(np.uint32)).all()
        live = np.nonzero(~dead)[0]
        for j in range(2):
            s = np.stack([_f64_row_scores(rows[live], q[j, t], L2) for t in range(T)])
            want = MS.vectorised(s.astype(np.float32), doc[live], L2, 45)
            ref = dict(zip(want[1][:40].tolist(), want[0][:40].tolist()))
            assert sorted(got.keys[j][:40].tolist()) == sorted(ref) and (np.diff(got.scores[j][:40]) >= 0).all()
            assert np.allclose(got.scores[j][:40], [ref[g] for g in got.keys[j][:40].tolist()], rtol=1e-4)
            assert (got.keys[j][40:] == PAD).all() and np.isposinf(got.scores[j][40:]).all()
        with pytest.raises(E.BuildError, match="holds 699 values"):
            M.find_top_k_documents(space, q, 3, column="few")
