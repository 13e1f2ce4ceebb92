"""The fixed cost around the single-query shadow scan was trimmed (round 7): the query preparation moved into K1's
prologue, the flag compaction into the final select, the repair feedback rides on the end-of-call event.  None of it may
change an answer: "identical" below means identical indices, raw values and score bits (test_gpu_stream_i8_default.py)."""
import ctypes as C

import numpy as np
import pytest

from metrovector_amd import _lib
from metrovector_amd import gpu as G

SEED = 0x4D564631
L2, IP, COS = 0, 1, 2
F32, F16 = 0, 1
STREAM_MAX_K = 204  # api.hip kQsStreamMaxK

# kernel launches of one search, counted by the library on the host (mvfgpu_timing::search_launches)
LAUNCHES_SHADOW_STREAM = 6  # K1 over the shadow (prepares the query itself), margin select, K1-order re-score, final select
                            # (compacts the flags itself), the repair pair (K1 + select: both exit when nothing is flagged)
LAUNCHES_K1 = 2             # K1 over the stored rows, select


def _same(a, b, what):
    assert (a.indices == b.indices).all(), f"{what}: indices differ"
    assert (a.raw == b.raw).all(), f"{what}: raw values differ"
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), f"{what}: score bits differ"


# ---- CPU tier ----------------------------------------------------------------------------------------------------------

def test_timing_struct_keeps_its_size_and_the_launch_count_sits_where_reserved_sat():
    assert C.sizeof(_lib.Timing) == 80  # the parent commit's
    assert _lib.Timing.search_launches.offset == 76 and _lib.Timing.search_launches.size == 4
    assert _lib.Timing.repaired_queries.offset == 72


# ---- GPU tier ------------------------------------------------------------------------------------------------------------

MID_ROWS, MID_DIM = 400_000, 768  # 1.2 GB of Float32 rows: the default route of one query is the shadow stream


@pytest.fixture(scope="module")
def mid(oracle):
    rows = np.ascontiguousarray(oracle.synth_rows(SEED, 0, MID_ROWS, MID_DIM, F32))
    c = G.GpuCorpus.from_array(rows)
    yield c, rows
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_default_route_is_identical_to_k1_and_counts_its_launches(oracle, mid, metric):
    c, rows = mid
    # (sixteen queries: the zero query is flagged and repaired under InnerProduct and Cosine, and more than one repaired
    # search in eight would send the handle back to its stored rows: feedback_consume)
    q = oracle.synth_queries(SEED + 1, 16, MID_DIM, F32).copy()
    q[0] = rows[321_987]  # a stored row
    q[1] = 0.0            # a zero query
    c.set_profiling(True)
    try:
        for k in (1, 100, STREAM_MAX_K):
            for i in range(q.shape[0]):
                c.set_scan_path(0)
                got = c.search(q[i:i + 1], k, metric)
                t = c.last_timing()
                assert t.scan_kernel == 7
                assert t.search_launches == LAUNCHES_SHADOW_STREAM
                c.set_scan_path(1)
                want = c.search(q[i:i + 1], k, metric)
                t = c.last_timing()
                assert t.scan_kernel == 1
                assert t.search_launches == LAUNCHES_K1
                _same(got, want, f"metric {metric} k {k} query {i}")
    finally:
        c.set_scan_path(0)
        c.set_profiling(False)


# dims whose one-query lane width (api.hip choose_group) is 1, 4, 8, 16, 32 and 64
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("dim", [3, 13, 30, 128, 100, 200])
def test_path6_one_to_four_queries_identical_to_k1(oracle, dim, dtype):
    n = 40_000
    rows = np.ascontiguousarray(oracle.synth_rows(SEED, 0, n, dim, dtype))
    q = oracle.synth_queries(SEED + 2, 4, dim, dtype).copy()
    q[0] = rows[1234].astype(np.float32)
    for metric in (L2, IP, COS):
        with G.GpuCorpus.from_array(rows) as c:
            c.set_profiling(True)
            for k in (10, 100):
                for nq in (1, 2, 3, 4):
                    c.set_scan_path(6)
                    got = c.search(q[:nq], k, metric)
                    assert c.last_timing().scan_kernel == 7  # (path 6 builds the shadow: no quiet way back to K1)
                    c.set_scan_path(1)
                    want = c.search(q[:nq], k, metric)
                    for i in range(nq):
                        for a, b, what in ((got.indices, want.indices, "indices"), (got.raw, want.raw, "raw values"),
                                           (got.scores.view(np.uint32), want.scores.view(np.uint32), "score bits")):
                            assert (a[i] == b[i]).all(), f"dtype {dtype} dim {dim} metric {metric} k {k}: query {i} of {nq}: {what} differ"


@pytest.mark.gpu
def test_repaired_queries_are_identical_through_the_folded_compaction(oracle):
    """A dense cluster of near-duplicates (test_gpu_stream_i8_default.py): every query is flagged and redone by K1."""
    n, dim = 40_000, 64
    rng = np.random.default_rng(11)
    base = rng.standard_normal(dim).astype(np.float32)
    rows = (base[None, :] + rng.standard_normal((n, dim)).astype(np.float32) * 1e-4).astype(np.float32)
    rows[::97] = base  # exact duplicates: ties
    q = np.stack([base + rng.standard_normal(dim).astype(np.float32) * 1e-3 for _ in range(4)]).astype(np.float32)
    for metric in (L2, IP, COS):
        with G.GpuCorpus.from_array(rows) as c:
            for k in (10, 100):
                for nq in (1, 4):
                    c.set_scan_path(6)
                    got = c.search(q[:nq], k, metric)
                    assert c.last_timing().repaired_queries == nq
                    c.set_scan_path(1)
                    _same(got, c.search(q[:nq], k, metric), f"metric {metric} k {k} nq {nq}")


def partly_flagged_batch(oracle):
    """Random rows that hold one tight cluster; queries 0 and 2 sit next to the cluster (thousands of rows inside the int8
    bound: flagged), queries 1 and 3 far from it."""
    n, dim = 40_000, 192
    rows = np.ascontiguousarray(oracle.synth_rows(SEED, 0, n, dim, F32))
    rng = np.random.default_rng(12)
    base = rng.standard_normal(dim).astype(np.float32)
    where = rng.choice(n, 6000, replace=False)
    rows[where] = base * 0.5 + rng.standard_normal((6000, dim)).astype(np.float32) * 4e-3
    q = oracle.synth_queries(SEED + 6, 4, dim, F32).copy()
    q[0] = base + rng.standard_normal(dim).astype(np.float32) * 1e-2
    q[2] = base + rng.standard_normal(dim).astype(np.float32) * 1e-2
    return rows, q


PARTLY_FLAGGED_PARENT = 2  # repaired_queries the parent commit reports for partly_flagged_batch, InnerProduct, k = 50


@pytest.mark.gpu
def test_a_batch_in_which_some_queries_are_flagged(oracle):
    rows, q = partly_flagged_batch(oracle)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_scan_path(6)
        got = c.search(q, 50, IP)
        assert c.last_timing().repaired_queries == PARTLY_FLAGGED_PARENT
        calm = c.search(q[1:2], 50, IP)  # flags nothing: the flags of the search before were cleared
        assert c.last_timing().repaired_queries == 0
        again = c.search(q, 50, IP)
        assert c.last_timing().repaired_queries == PARTLY_FLAGGED_PARENT
        c.set_scan_path(1)
        want = c.search(q, 50, IP)
        _same(got, want, "partly flagged batch")
        _same(again, want, "partly flagged batch, again")
        _same(calm, c.search(q[1:2], 50, IP), "the query behind it")


@pytest.mark.gpu
def test_batched_repair_windows_are_unchanged(oracle, monkeypatch):
    """test_gpu_round2.py's adversarial order on the batched route, which keeps its own compaction launch and its launch
    pairs: several repair windows give what one window gives, and what K1 gives."""
    n, dim, nq, k = 50_000, 32, 300, 10
    rng = np.random.default_rng(9)
    base = rng.standard_normal(dim).astype(np.float32)
    rows = (base[None, :] * (np.arange(1, n + 1, dtype=np.float32) / n)[:, None]).astype(np.float32)
    q = (np.tile(base, (nq, 1)) * rng.uniform(0.5, 2.0, (nq, 1))).astype(np.float32)
    q[::9] *= -1
    res = {}
    for window in ("64", None):
        if window:
            monkeypatch.setenv("MVF_REPAIR_WINDOW", window)
        else:
            monkeypatch.delenv("MVF_REPAIR_WINDOW")
        with G.GpuCorpus.from_array(rows, index_base=3) as c:
            c.set_scan_path(2)
            res[window] = c.search(q, k, IP)
            assert c.last_timing().repaired_queries > 64
            _same(res[window], c.search(q, k, IP), "the flags and the list are re-armed")
            c.set_scan_path(1)
            want = c.search(q, k, IP)
        assert (res[window].indices == want.indices).mean() >= 0.999
    _same(res["64"], res[None], "several repair windows / one")


@pytest.mark.gpu
def test_the_feedback_still_switches_a_defeated_corpus_back(oracle):
    """>= 512 MiB of rows that are one tight cluster: every single query on the default route is flagged and repaired; the
    counts reach the host two searches late through the end-of-call event, and after four of them the corpus reads its stored
    rows (feedback_consume)."""
    n, dim = 180_000, 768  # 553 MB
    rng = np.random.default_rng(21)
    base = rng.standard_normal(dim).astype(np.float32)
    rows = np.empty((n, dim), np.float32)
    for r0 in range(0, n, 20_000):
        rows[r0:r0 + 20_000] = base[None, :] + rng.standard_normal((20_000, dim)).astype(np.float32) * 1e-4
    q = np.stack([base + rng.standard_normal(dim).astype(np.float32) * 1e-3 for _ in range(10)]).astype(np.float32)
    kernels, repaired, got = [], [], []
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        for i in range(10):
            got.append(c.search(q[i:i + 1], 20, COS))
            t = c.last_timing()
            kernels.append(t.scan_kernel)
            repaired.append(t.repaired_queries)
        c.set_scan_path(1)
        for i in range(10):
            _same(got[i], c.search(q[i:i + 1], 20, COS), f"search {i} (route {kernels[i]})")
    assert kernels[0] == 7 and kernels[1] == 7, kernels
    assert repaired[0] == 1 and repaired[1] == 1, repaired
    first_k1 = kernels.index(1)
    assert first_k1 <= 7, kernels
    assert all(kn == 1 for kn in kernels[first_k1:]), kernels
    assert all(kn == 7 and r == 1 for kn, r in zip(kernels[:first_k1], repaired[:first_k1])), (kernels, repaired)


@pytest.mark.gpu
def test_two_streams_without_a_host_wait(oracle, mid):
    """Two searches on one handle, issued on two streams with no host wait in between, return what they return on one
    stream: the single end-of-call event still orders the second behind the first (they share the handle's scratch)."""
    import torch
    c, rows = mid
    k = 100
    q = oracle.synth_queries(SEED + 7, 2, MID_DIM, F32).copy()
    dq = torch.from_numpy(q).cuda()

    def run(streams):
        out = []
        for i, st in enumerate(streams):
            s = torch.empty((1, k), dtype=torch.float32, device="cuda")
            ix = torch.empty((1, k), dtype=torch.int64, device="cuda")
            r = torch.empty((1, k), dtype=torch.int32, device="cuda")
            with torch.cuda.stream(st):
                c.search_device(dq[i:i + 1].data_ptr(), 0, MID_DIM, 1, k, COS, s.data_ptr(), ix.data_ptr(), r.data_ptr(), st.cuda_stream)
            out.append((s, ix, r))
        torch.cuda.synchronize()
        return [tuple(t.cpu().numpy() for t in o) for o in out]

    torch.cuda.synchronize()
    c.set_scan_path(0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    one = run([s1, s1])
    for _ in range(3):
        two = run([s1, s2])
        for a, b in zip(one, two):
            assert (a[1] == b[1]).all() and (a[2] == b[2]).all()
            assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all()


@pytest.mark.gpu
def test_profiling_changes_nothing_and_its_times_are_sane(oracle, mid):
    c, rows = mid
    q = oracle.synth_queries(SEED + 8, 6, MID_DIM, F32)
    c.set_scan_path(0)
    c.set_profiling(False)
    off = [c.search(q[i:i + 1], 100, COS) for i in range(6)]
    assert c.last_timing().search_launches == LAUNCHES_SHADOW_STREAM  # counted whether profiled or not
    c.set_profiling(True)
    try:
        on = [c.search(q[i:i + 1], 100, COS) for i in range(6)]
        t = c.last_timing()
        assert t.samples == 6 and t.scan_kernel == 7
        assert 0 < t.scan_ms_avg <= t.search_ms_avg
        assert t.select_ms_avg > 0
        for a, b in zip(off, on):
            _same(a, b, "profiling off / on")
        # K1 over the stored rows: its bytes at 8 TB/s and at 2 TB/s bracket the scan time -- a sanity band for the time base
        # (a wrong clock rate is off by a factor of ten), not a performance claim
        c.set_scan_path(1)
        c.set_profiling(False)
        c.set_profiling(True)
        for i in range(6):
            c.search(q[i:i + 1], 100, COS)
        t = c.last_timing()
        nbytes = MID_ROWS * MID_DIM * 4
        print(f"K1 over {nbytes / 1e9:.2f} GB: scan_ms_avg {t.scan_ms_avg:.4f}, search_ms_avg {t.search_ms_avg:.4f}")
        assert t.samples == 6 and t.scan_kernel == 1 and t.scan_bytes == nbytes
        assert nbytes / 8e12 * 1e3 <= t.scan_ms_avg <= nbytes / 2e12 * 1e3
        assert t.scan_ms_avg <= t.search_ms_avg
    finally:
        c.set_scan_path(0)
        c.set_profiling(False)


@pytest.mark.gpu
def test_the_windows_of_a_join_post_their_feedback_one_by_one(oracle):
    """A join runs all its windows' searches inside ONE call on the handle, so their repair counts cannot ride on the
    end-of-call event: window w + 2 consumes window w's count while the call is still being enqueued.  A quarter of the rows
    are one tight cluster (every query taken from it overflows the int8 selection's budget and is repaired), so the counts of
    the first windows switch the selection off -- the same state, at the same point, as the same windows issued as searches
    of their own, and whatever the state the answers are those of the stored-row route."""
    import torch
    n, dim, k, windows = 40_000, 192, 10, 5
    rows = np.ascontiguousarray(oracle.synth_rows(SEED, 0, n, dim, F32))
    rng = np.random.default_rng(31)
    base = rng.standard_normal(dim).astype(np.float32)
    where = rng.choice(n, n // 4, replace=False)
    rows[where] = base * 0.5 + rng.standard_normal((len(where), dim)).astype(np.float32) * 4e-3
    count = windows * G.JOIN_WINDOW
    with G.GpuCorpus.from_array(rows) as a, G.GpuCorpus.from_array(rows) as b:
        ds = torch.empty((count, k), dtype=torch.float32, device="cuda")
        di = torch.empty((count, k), dtype=torch.int64, device="cuda")
        a.knn_join_device(k, IP, 0, count, ds.data_ptr(), di.data_ptr(), exclude_self=False,
                          stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        state_join = a.info().selection_state
        singly = [b.search(rows[w * G.JOIN_WINDOW:(w + 1) * G.JOIN_WINDOW], k, IP) for w in range(windows)]
        state_singly = b.info().selection_state
        assert state_singly != 0, "the data was meant to defeat the int8 selection"
        assert state_join == state_singly
        b.set_scan_path(1)
        for w in range(windows):
            want = b.search(rows[w * G.JOIN_WINDOW:(w + 1) * G.JOIN_WINDOW], k, IP)
            lo, hi = w * G.JOIN_WINDOW, (w + 1) * G.JOIN_WINDOW
            assert (di[lo:hi].cpu().numpy().view(np.uint64) == want.indices).mean() >= 0.999
            assert (singly[w].indices == want.indices).mean() >= 0.999
