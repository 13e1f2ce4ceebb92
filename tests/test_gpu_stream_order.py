"""Cross-stream ordering of one handle's calls behind a STALLED stream (DESIGN.md §3 "Stream discipline", §8).

State flags of a handle (the norms, the shadows, a scratch buffer's pointer) are set when a build is enqueued, not when it has
run: the only thing between a second stream and half-built state is the event chain of corpus_device_call.  Every scenario here
puts the producer behind a stall on one stream and issues the consumer at once -- and asserts that the stall was still pending
then, else it has tested nothing.  Before it, a decoy handle of other rows leaves plausible but wrong state in the memory the
fresh handle recycles; after it, a third handle gives the reference with a full synchronise between the two calls.  Both calls'
bytes must equal the reference's, and the reference is checked against the oracle."""
import os
import sys
import time

import numpy as np
import pytest

from metrovector_amd import gpu as G

import _columns
import _stream_scenarios as SC
import _streams as S
from _children import RUNNER
from _radius import assert_float_radius, oracle_radius
from _util import assert_exact, assert_float_topk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, IP, COS = 0, 1, 2
F32, F16, I8 = 0, 1, 2
N, DIM, K = SC.N, SC.DIM[F32], SC.K
REFERENCE = {}  # scenario id -> the digest of its in-process reference


@pytest.fixture(scope="module")
def streams(oracle):
    """(s1, s2) for which both controls hold -- run before any scenario of this module"""
    rows = np.ascontiguousarray(oracle.synth_rows(7, 0, 4000, DIM, F32))
    q = np.ascontiguousarray(oracle.synth_queries(8, 1, DIM, F32))
    try:
        return S.pick_streams(lambda: G.GpuCorpus.from_array(rows), q)
    except S.ControlFailed as e:
        pytest.skip(str(e))


def _same(got, ref, what):
    assert sorted(got) == sorted(ref)
    wrong = []
    for name in ref:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(ref[name])
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {name}"
        if a.tobytes() != b.tobytes():
            diff = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
            wrong.append(f"{name} in {diff.size} of {a.shape[0]} rows (first {diff[:5].tolist()}: got {a[diff[0]].ravel()[:4]}, "
                         f"reference {b[diff[0]].ravel()[:4]})")
    assert not wrong, f"{what} differs from the reference: " + "; ".join(wrong)


def _oracle_check(oracle, sc, call, got):
    """the reference is more than the code under test: plain searches and radius searches of the handle against the oracle"""
    rows, dtype = sc.rows, sc.dtype
    if type(call) in (SC.SearchDev, SC.SearchHost):
        if dtype == I8:
            res = G.SearchResult(got["scores"].view(np.float32), got["indices"], got["raw"])
            assert_exact(res, *oracle.search(rows, dtype, call.metric, call.q, call.k))
        else:
            rows_f32 = rows.astype(np.float32)
            for j, q in enumerate(call.q):
                all_s = oracle.scores(rows, dtype, call.metric, q)[0]
                assert_float_topk(call.metric, got["scores"][j].view(np.float32), got["indices"][j], all_s, rows_f32, q, call.k)
    elif type(call) is SC.RadiusHost:
        rows_f32 = rows.astype(np.float32)
        for j, q in enumerate(call.q):
            if dtype == I8 and call.metric != COS:
                c, sco, idx, raw = oracle_radius(oracle, rows, dtype, call.metric, q, call.radii[j], call.m)
                assert int(got["counts"][j]) == c, f"query {j}: count {got['counts'][j]} != {c}"
                assert (got["indices"][j] == idx).all() and (got["raw"][j] == raw).all()
                assert (got["scores"][j] == sco.view(np.uint32)).all()
            else:
                all_s = oracle.scores(rows, dtype, call.metric, q)[0]
                assert_float_radius(call.metric, int(got["counts"][j]), got["scores"][j].view(np.float32), got["indices"][j], all_s,
                                    rows_f32, np.asarray(q, np.float32), float(call.radii[j]), call.m)


def test_the_table_names_this_module_s_tests():
    for name in S.CUSTOM:
        assert callable(globals().get(name)), f"tests/_streams.py CUSTOM names {name}, which is no test of this module"


def test_both_controls_hold(oracle, streams):
    """the harness sees a missing dependency: on the chosen streams, and on a handle's own stream"""
    s1, s2 = streams
    assert S.stream_control(s1, s2), "a clone on s1 saw the fill enqueued behind the stall on s2, or the stall had ended"
    rows = np.ascontiguousarray(oracle.synth_rows(9, 0, 4000, DIM, F32))
    # per handle (each has a stream of its own): raises where none of eight fresh handles searches past the stall

    def attempt():
        c = G.GpuCorpus.from_array(rows)
        return None, c, c.close

    S.on_an_independent_handle(attempt, rows[:1], s2)


@pytest.mark.parametrize("sid", list(S.SCENARIOS))
def test_pair(oracle, streams, sid):
    sc = SC.build(sid, oracle)
    assert (sc.producer.entry, sc.consumer.entry) == S.SCENARIOS[sid], "tests/_streams.py SCENARIOS names other entries"
    gp, gc, rp, rc = SC.run(sc, streams)
    REFERENCE[sid] = SC.digest(rp, rc)
    _same(gp, rp, f"{sid}: the producer ({sc.producer.entry}) behind the stall")
    _same(gc, rc, f"{sid}: the consumer ({sc.consumer.entry})")
    _oracle_check(oracle, sc, sc.producer, rp)
    _oracle_check(oracle, sc, sc.consumer, rc)


def test_three_device_searches_on_three_streams(oracle, streams):
    """Three int8-selected batches of one handle on three streams: the third enqueue consumes the first one's repair feedback
    (include/mvf_gpu.h: two in flight), so it may wait on the host -- the first two must not."""
    import torch
    s1, s2 = streams
    s3 = torch.cuda.Stream()
    sc = SC.build("scratch:f32:5", oracle)
    qs = [sc.producer.q, sc.consumer.q, np.ascontiguousarray(oracle.synth_queries(sc.seed + 3, 40, DIM, F32))]

    def go(rows, on):
        calls = [SC.SearchDev(q, K, L2, 5, SC.KERNEL[(5, F32)]) for q in qs]
        ctx = sc.make_ctx(rows)
        try:
            for call in calls:
                call.prepare(ctx)
            calls[0].force(ctx)
            torch.cuda.synchronize()
            got = []
            if on is None:
                for call in calls:
                    got.append(call.issue(ctx, None))
                    torch.cuda.synchronize()
                    call.after(ctx)
            else:
                ev = S.stall(s2)
                got.append(calls[0].issue(ctx, s2))
                got.append(calls[1].issue(ctx, s1))
                S.require_pending(ev, "when the second search had returned")
                got.append(calls[2].issue(ctx, s3))
                torch.cuda.synchronize()
                calls[2].after(ctx)
            return [g() for g in got]
        finally:
            ctx.close()

    go(SC.decoy_of(sc.rows), None)
    got = go(sc.rows, True)
    ref = go(sc.rows, None)
    for i, (a, b) in enumerate(zip(got, ref)):
        _same(a, b, f"search {i} of three")
        _oracle_check(oracle, sc, SC.SearchDev(qs[i], K, L2), b)


def test_column_created_on_the_stalled_stream(oracle, streams):
    inp = SC.column_inputs(oracle)
    got = SC.column_scenario(oracle, streams)
    REFERENCE["column"] = SC.digest(got)
    values = inp["values"]
    assert int(got["admitted"][0]) == int(_columns.where_mask([(values,) + SC.COLUMN_CLAUSE]).sum())
    keys, counts = np.unique(values.astype(np.uint64), return_counts=True)  # tests/_partitioned.py group_by, no row deleted
    assert (got["keys"] == keys).all() and (got["counts"] == counts.astype(np.uint64)).all()
    assert (got["gathered"] == values[inp["positions"].astype(np.int64)].astype(np.uint64)).all()


def _pending_search(oracle, seed, rows=None, nq=32, path=2, metric=COS, k=K):
    """(rows, a batched search_device that builds the norms lazily)"""
    if rows is None:
        rows = np.ascontiguousarray(oracle.synth_rows(seed, 0, N, DIM, F32))
    q = np.ascontiguousarray(oracle.synth_queries(seed + 1, nq, DIM, F32))
    return rows, SC.SearchDev(q, k, metric, path, SC.KERNEL[(path, F32)])


def _behind_a_pending_search(oracle, streams, seed, body, setup=None, **search):
    """decoy, stalled run, reference of: a lazy batched search_device on the stalled stream, then body(ctx) on the host at once
    -> (stalled producer, stalled body, reference producer, reference body)"""
    import torch
    rows, prod = _pending_search(oracle, seed, **search)
    probe = np.ascontiguousarray(oracle.synth_queries(seed + 2, 1, DIM, F32))

    def make(r):
        ctx = SC.Ctx(G.GpuCorpus.from_array(r), r)
        if setup:
            setup(ctx)
        return ctx

    def go(r, stalled):
        ctx = make(r)
        try:
            prod.prepare(ctx)
            prod.force(ctx)
            torch.cuda.synchronize()
            if stalled:
                ev = S.stall(streams[1])
                got = prod.issue(ctx, streams[1])
                S.require_pending(ev, "when the producer had returned and the host call was issued")
            else:
                got = prod.issue(ctx, None)
                torch.cuda.synchronize()
            out = body(ctx)
            torch.cuda.synchronize()
            return (got(), out), ctx.c, ctx.close
        except BaseException:
            ctx.close()
            raise

    def once(r):
        result, _, close = go(r, False)
        close()
        return result

    once(SC.decoy_of(rows))
    gp, gb = S.on_an_independent_handle(lambda: go(rows, True), probe, streams[1])
    rp, rb = once(rows)
    return rows, prod, gp, gb, rp, rb


HOST_CALLS = ["gather_rows", "read_rows", "search_fetch", "set_tombstones", "set_vector_ids", "column_and_filter_create"]


@pytest.mark.parametrize("what", HOST_CALLS)
def test_host_calls_behind_pending_device_work(oracle, streams, what):
    seed = SC._seed_of("host:" + what)
    idx = np.random.default_rng(seed).integers(0, N, 100).astype(np.uint64)
    dead = np.zeros(N, bool)
    dead[::2] = True
    ids = (np.arange(N, dtype=np.uint64) * np.uint64(7919) + np.uint64(1 << 40))
    q2 = np.ascontiguousarray(oracle.synth_queries(seed + 5, 3, DIM, F32))
    values = SC.column_values(N)

    def body(ctx):
        c = ctx.c
        if what == "gather_rows":
            return dict(rows=c.gather_rows(idx))
        if what == "read_rows":
            return dict(rows=c.read_rows(123, 500))
        if what == "search_fetch":
            c.set_scan_path(0)
            r, vec = c.search_fetch(q2, K, COS)
            return dict(SC._res(r), vectors=vec)
        if what == "set_tombstones":
            c.set_tombstones(np.packbits(dead, bitorder="little"))
            return SC._res(c.search(q2, K, COS))
        if what == "set_vector_ids":
            c.set_vector_ids(ids)
            return SC._res(c.search(q2, K, COS))
        col = ctx.own(c.attach_column(values))
        flt = ctx.own(c.make_filter(SC.allow_mask(N)))
        both = ctx.own(c.make_filter_where([(col,) + SC.COLUMN_CLAUSE], base=flt))
        return dict(admitted=np.array([flt.admitted, both.admitted], np.uint64), **SC._res(c.search_filtered(q2, K, COS, both)))

    rows, prod, gp, gb, rp, rb = _behind_a_pending_search(oracle, streams, seed, body)
    _same(gp, rp, f"{what}: the pending search")
    _same(gb, rb, f"{what}: the host call")
    sc = type("Rows", (), dict(rows=rows, dtype=F32))
    _oracle_check(oracle, sc, prod, rp)
    if what == "gather_rows":
        assert gb["rows"].tobytes() == rows[idx.astype(np.int64)].tobytes()
    elif what == "read_rows":
        assert gb["rows"].tobytes() == rows[123:623].tobytes()
    elif what == "search_fetch":
        assert gb["vectors"].tobytes() == rows[gb["indices"].astype(np.int64)].tobytes()
    elif what == "set_tombstones":  # the producer's answer is that of the old bitmap, the consumer's that of the new one
        assert dead[gp["indices"].astype(np.int64)].any() and not dead[gb["indices"].astype(np.int64)].any()
    elif what == "set_vector_ids":
        assert (gp["indices"] < N).all() and (gb["indices"] >= np.uint64(1 << 40)).all()
        with G.GpuCorpus.from_array(rows) as c:
            assert (ids[c.search(q2, K, COS).indices.astype(np.int64)] == gb["indices"]).all()
    else:
        allow = SC.allow_mask(N)
        assert gb["admitted"].tolist() == [int(allow.sum()), int(_columns.where_mask([(values,) + SC.COLUMN_CLAUSE], base=allow).sum())]


def test_last_timing_behind_a_stalled_k1_search(oracle, streams):
    import torch
    rows, prod = _pending_search(oracle, 4242, nq=1, path=1, metric=L2)
    probe = np.ascontiguousarray(oracle.synth_queries(4243, 1, DIM, F32))

    def attempt():
        ctx = SC.Ctx(G.GpuCorpus.from_array(rows), rows)
        try:
            ctx.c.set_profiling(True)
            prod.prepare(ctx)
            prod.force(ctx)
            torch.cuda.synchronize()
            ev = S.stall(streams[1])
            t0 = time.perf_counter()
            got = prod.issue(ctx, streams[1])
            S.require_pending(ev, f"when the search had returned, {(time.perf_counter() - t0) * 1e3:.1f} ms after it was issued, and "
                                  f"mvfgpu_last_timing was issued")
            t = ctx.c.last_timing()  # waits for the search
            assert not S.pending(ev), "mvfgpu_last_timing returned before the search it reports had run"
            assert t.samples == 1 and t.scan_kernel == 1
            times = [t.scan_ms, t.select_ms, t.total_ms, t.scan_ms_avg, t.select_ms_avg, t.search_ms, t.search_ms_avg]
            assert all(x >= 0 for x in times) and t.scan_ms > 0 and t.total_ms < S.STALL_MS, times
            torch.cuda.synchronize()
            ctx.c.set_profiling(False)
            return got(), ctx.c, ctx.close
        except BaseException:
            ctx.close()
            raise

    res = S.on_an_independent_handle(attempt, probe, streams[1])
    _oracle_check(oracle, type("Rows", (), dict(rows=rows, dtype=F32)), prod, res)


def test_filter_created_on_the_stalled_stream(oracle, streams):
    """mvfgpu_filter_create_device reads words that are written behind the stall; it waits for its admitted count itself."""
    import torch
    from _filtered import device_words
    seed = SC._seed_of("filter")
    rows = np.ascontiguousarray(oracle.synth_rows(seed, 0, N, DIM, F32))
    q = np.ascontiguousarray(oracle.synth_queries(seed + 1, 5, DIM, F32))
    allow = SC.allow_mask(N, 7)
    words = np.ascontiguousarray(device_words(allow), np.uint32)

    def go(r, mask_words, stalled):
        c = G.GpuCorpus.from_array(r)
        try:
            src = SC._dev(mask_words)
            dw = torch.zeros_like(src)
            torch.cuda.synchronize()
            if stalled:
                s2 = streams[1]
                ev = S.stall(s2)
                with torch.cuda.stream(s2):
                    dw.copy_(src)
                S.require_pending(ev, "when mvfgpu_filter_create_device was issued")
                flt = c.make_filter_device(dw.data_ptr(), stream=s2.cuda_stream)
            else:
                dw.copy_(src)
                torch.cuda.synchronize()
                flt = c.make_filter_device(dw.data_ptr())
            try:
                return flt.admitted, SC._res(c.search_filtered(q, K, IP, flt))
            finally:
                flt.close()
        finally:
            c.close()

    go(SC.decoy_of(rows), ~words, False)
    admitted, got = go(rows, words, True)
    assert admitted == int(allow.sum()), "the filter was built from words that were not written yet"
    with G.GpuCorpus.from_array(rows) as c, c.make_filter(allow) as flt:  # the reference: the host form of the same mask
        ref = SC._res(c.search_filtered(q, K, IP, flt))
    _same(got, ref, "the filtered search")
    assert allow[got["indices"].astype(np.int64)].all()


def test_shardset_search_with_one_shard_pending(oracle, streams):
    import torch
    seed = SC._seed_of("shardset")
    rows = np.ascontiguousarray(oracle.synth_rows(seed, 0, N, DIM, F32))
    q = np.ascontiguousarray(oracle.synth_queries(seed + 1, 32, DIM, F32))
    cuts = [0, 6_001, 13_000, N]
    _, prod = _pending_search(oracle, seed + 10, rows=rows[cuts[1]:cuts[2]])

    def go(r, stalled):
        shards = [G.GpuCorpus.from_array(np.ascontiguousarray(r[a:b]), index_base=a) for a, b in zip(cuts[:-1], cuts[1:])]
        ctx = SC.Ctx(shards[1], r)
        try:
            with G.ShardSet(shards) as ss:
                prod.prepare(ctx)
                prod.force(ctx)
                torch.cuda.synchronize()
                if stalled:
                    ev = S.stall(streams[1])
                    got = prod.issue(ctx, streams[1])
                    S.require_pending(ev, "when the shard's search had returned and mvfgpu_shardset_search was issued")
                else:
                    got = prod.issue(ctx, None)
                    torch.cuda.synchronize()
                shards[1].set_scan_path(0)
                res = SC._res(ss.search(q, K, COS))
                torch.cuda.synchronize()
                return got(), res
        finally:
            for s in shards:
                s.close()

    go(SC.decoy_of(rows), False)
    gp, gs = go(rows, True)
    rp, rs = go(rows, False)
    _same(gp, rp, "the pending search of the middle shard")
    _same(gs, rs, "the set's search")
    rows_f32 = rows.astype(np.float32)
    for j, v in enumerate(q):
        assert_float_topk(COS, rs["scores"][j].view(np.float32), rs["indices"][j], oracle.scores(rows, F32, COS, v)[0], rows_f32, v, K)


def test_destroy_behind_pending_work(oracle, streams):
    """Filter, partition index, column and handle are destroyed at once behind searches and a column copy that are still queued:
    every destroy path waits (corpus_wait_newest; mvfgpu_corpus_destroy synchronises the device), so the searches read live memory."""
    import torch
    seed = SC._seed_of("destroy")
    rows = np.ascontiguousarray(oracle.synth_rows(seed, 0, N, DIM, F32))
    q = np.ascontiguousarray(oracle.synth_queries(seed + 1, 32, DIM, F32))
    values = SC.column_values(N)
    keys = values[np.random.default_rng(seed).integers(0, N, 32)].astype(np.uint64)
    sc = SC.Scenario("destroy", F32, seed, None, None, needs=("filter", "partition"), rows=rows)

    def go(r, stalled):
        calls = [SC.FilteredDev(q, K, COS, 2), SC.PartDev(q, keys, K, COS)]
        ctx = sc.make_ctx(r)
        try:
            for call in calls:
                call.prepare(ctx)
            calls[0].force(ctx)
            src = SC._dev(values)
            dv = torch.zeros_like(src)
            torch.cuda.synchronize()
            stream = streams[1] if stalled else torch.cuda.current_stream()
            if stalled:
                ev = S.stall(stream)
            got = [call.issue(ctx, stream) for call in calls]
            with torch.cuda.stream(stream):
                dv.copy_(src)
            col2 = ctx.c.attach_column_device(dv.data_ptr(), G.UINT32, stream=stream.cuda_stream)
            if stalled:
                S.require_pending(ev, "when the two searches and the column's creation had returned and the destroys were issued")
            ctx.flt.close(), ctx.part.close(), col2.close(), ctx.col.close()
            ctx.owned = []
            ctx.c.close()
            over = torch.full((r.nbytes // 4,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")  # the freed rows' size, overwritten
            torch.cuda.synchronize()
            del over
            return [g() for g in got]
        finally:
            ctx.close()

    go(SC.decoy_of(rows), False)
    got = go(rows, True)
    ref = go(rows, False)
    for a, b, what in zip(got, ref, ("filtered", "partitioned")):
        _same(a, b, f"the {what} search behind which everything was destroyed")


@pytest.mark.parametrize("poison", ["0", "255"])
def test_under_poison_in_a_child_process(oracle, streams, poison):
    """The lazy-state scenarios and the column scenario once more in a fresh process whose library fills every allocation with
    0x00 / 0xFF first: one child at a time, none after a fault; its digests are the in-process reference's."""
    import torch
    ids = list(S.LAZY) + ["column"]
    for sid in ids:
        if sid not in REFERENCE:  # this test runs alone: the reference, taken here
            if sid == "column":
                REFERENCE[sid] = SC.digest(SC.column_scenario(oracle, streams))
            else:
                sc = SC.build(sid, oracle)
                rp, rc = S.run_pair(lambda: sc.make_ctx(sc.rows), sc.producer, sc.consumer, None)
                REFERENCE[sid] = SC.digest(rp, rc)
    torch.cuda.synchronize()
    env = dict(os.environ, MVF_DEBUG_POISON=poison)
    out = RUNNER.run([sys.executable, os.path.join(ROOT, "tests", "_stream_scenarios.py")] + ids, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    lines = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    assert lines.get("poison") == poison, f"the child's library does not poison with {poison}: {lines.get('poison')}"
    wrong = [sid for sid in ids if lines.get(sid) != REFERENCE[sid]]
    assert not wrong, f"under MVF_DEBUG_POISON={poison} these scenarios differ from the in-process reference: {wrong}"
