"""Row writes where tests/test_gpu_write_rows.py does not reach (DESIGN.md §3 "Row writes", §5 "W0 / W1", §8 "Row writes"); the
worlds and the comparison rule are tests/_write_rows.py's, the worlds' own properties are held on the CPU by
tests/test_write_rows_cpu.py.  As there, a handle that was written is compared with its TWIN, a fresh handle created from the
changed array with the same path, tuning and objects: by bytes where the library promises bits, else handle and twin by the
tolerance criterion against the oracle over the changed rows.

A  the grid-stride loop of W0 and of the four W1 kernels: ONE write of 16389 = 2 x 8192 + 5 rows (a launch holds 8192 waves), the
   host call's pageable blob;
B  rows of more than 64 16-byte vectors: the second trip of the lane loop, also where it is the row's last, partial vector;
C  the device call with everything resident, three writes in flight on one stream; the pinned upload buffer growing between
   writes in flight;
D  Float32 / Float16 rows behind every entry point that reads the refreshed norms and shadows;
E  "the maxima are never lowered": outlier rows written and replaced, then zero, tiny and huge queries; shadows built behind a
   norm maximum of +inf;
F  a write between two searches in flight whose kernels read the state W1 rewrites."""
import ctypes as C

import numpy as np
import pytest

import _write_rows as W
from _write_rows import COS, COUNTS, F16, F32, I8, IP, K, L2, METRICS, N, NORMS, NP, NQ, ROUTE_IDS, ROUTES, S_F16, U8, _handle, same
from metrovector_amd import _lib
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu


def _es(dt):
    return np.dtype(NP[dt]).itemsize


def _resident(c, w, path):
    """searches of every metric and batch size of the route: whatever the route derives from the rows is resident behind them"""
    for metric in METRICS:
        for nq in W.route_nqs(path):
            c.search(w.q[:nq], K, metric)
    return c.info().shadows


def _expect_report(rep, count, shadows, inf, dt, dim, path):
    assert rep["rows_written"] == count
    want = W.expect_refreshed(shadows)
    assert rep["refreshed"] & want == want, f"shadows {shadows:#x} were resident, refreshed {rep['refreshed']:#x}"
    if path != 1:
        assert rep["refreshed"] & NORMS, "the norms were resident"
    assert rep["launches"] == 1 + bin(rep["refreshed"]).count("1")
    assert rep["bytes_written"] == count * W.row_cost(inf, dt, dim, rep["refreshed"]), rep


def _sweep(oracle, w, dt, path, c, twin, what):
    """every metric at every batch size of the route, by the comparison rule"""
    for metric in METRICS:
        for nq in W.route_nqs(path):
            W.compare(oracle, w, dt, path, metric, nq, c.search(w.q[:nq], K, metric), twin.search(w.q[:nq], K, metric),
                      f"{what}: metric {metric} nq {nq}")


def _host_write_strided(c, pos, rows, stride):
    """the host call from a buffer of 0xFF at an odd address, the rows `stride` bytes apart"""
    row_bytes = rows.shape[1] * rows.itemsize
    buf = np.full(len(pos) * stride + 1, 0xFF, np.uint8)
    src = buf[1:]
    flat = np.ascontiguousarray(rows).view(np.uint8).reshape(len(pos), row_bytes)
    for i in range(len(pos)):
        src[i * stride:i * stride + row_bytes] = flat[i]
    rep = _lib.WriteReport()
    _lib.gpu_check(_lib.gpu().mvfgpu_corpus_write_rows(c._h, pos.ctypes.data_as(C.c_void_p), len(pos), C.c_void_p(src.ctypes.data), stride,
                                                      C.byref(rep)))
    return G._write_report(rep)


# ---- A ------------------------------------------------------------------------------------------------------------------------
def _strided_loops(oracle, monkeypatch, dt, path, env, search_first):
    if env is not None:
        monkeypatch.setenv("MVF_STREAM_5P1", env)
    for dim in W.LARGE_DIMS[dt]:
        w = W.large_world(oracle, dt, dim)
        (pos, new), = w.writes
        what = f"large world dtype {dt} path {path} dim {dim}"
        with _handle(w.rows0, path) as c, _handle(w.rows1, path) as twin:
            inf = c.info()
            if dt == F32:
                assert (len(pos) * 4 + 15) // 16 * 16 + len(pos) * inf.pitch_bytes > 3 << 20, "the blob of the host call is pageable"
            shadows = _resident(c, w, path) if search_first else 0
            rep = c.write_rows(pos, new)
            if search_first:
                _expect_report(rep, W.LARGE_COUNT, shadows, inf, dt, dim, path)
            else:
                assert rep["rows_written"] == W.LARGE_COUNT and rep["refreshed"] == 0 and rep["launches"] == 1
                assert rep["bytes_written"] == W.LARGE_COUNT * inf.pitch_bytes
            _sweep(oracle, w, dt, path, c, twin, what)
            assert c.read_rows(0, W.LARGE_N).tobytes() == w.rows1.tobytes(), what
            assert c.gather_rows(pos[-64:]).tobytes() == new[-64:].tobytes(), what + ": the list's last 64 entries"


@pytest.mark.parametrize("dt, path, env", ROUTES, ids=ROUTE_IDS)
def test_strided_loops(oracle, monkeypatch, dt, path, env):
    """every wave of W0 and of each W1 kernel serves two listed rows, five of them three"""
    _strided_loops(oracle, monkeypatch, dt, path, env, search_first=True)


@pytest.mark.parametrize("dt, path, env", [(F32, 7, "0"), (F32, 7, "1"), (I8, 2, None)], ids=["dt-f32-path7-5p1=0", "dt-f32-path7-5p1=1", "dt-i8-path2"])
def test_strided_loops_with_nothing_resident(oracle, monkeypatch, dt, path, env):
    _strided_loops(oracle, monkeypatch, dt, path, env, search_first=False)


# ---- B ------------------------------------------------------------------------------------------------------------------------
def _same_kernel_same_answer(oracle, w, dt, path, c, twin, what):
    """_sweep, and the kernel each search scanned with: a forced path that a dimension does not allow goes where the twin's goes"""
    for h in (c, twin):
        h.set_profiling(True)
    for metric in METRICS:
        for nq in W.route_nqs(path):
            got = c.search(w.q[:nq], K, metric)
            mine = c.last_timing().scan_kernel
            want = twin.search(w.q[:nq], K, metric)
            assert mine == twin.last_timing().scan_kernel, f"{what}: metric {metric} nq {nq}: scan kernel {mine}, the twin's {twin.last_timing().scan_kernel}"
            W.compare(oracle, w, dt, path, metric, nq, got, want, f"{what}: metric {metric} nq {nq}")
    for h in (c, twin):
        h.set_profiling(False)


def _rows_and_pad_bytes(oracle, w, path, c, twin, what):
    n = len(w.rows1)
    assert c.read_rows(0, n).tobytes() == twin.read_rows(0, n).tobytes() == w.rows1.tobytes(), what
    for metric in (COS, L2):  # K1's 16-byte loads read the pad bytes behind the last element: zero, as after an upload
        for nq in W.route_nqs(path)[:2]:
            (res, vec), (ref, rvec) = c.search_fetch(w.q[:nq], K, metric), twin.search_fetch(w.q[:nq], K, metric)
            W.compare(oracle, w, w.dt, path, metric, nq, res, ref, f"{what}: search_fetch metric {metric} nq {nq}")
            assert vec.tobytes() == w.rows1[res.indices.astype(np.int64)].tobytes(), f"{what}: the payload of search_fetch"
            assert rvec.tobytes() == w.rows1[ref.indices.astype(np.int64)].tobytes()
            assert np.isin(res.indices[0].astype(np.int64), w.written).any()


@pytest.mark.parametrize("dt, path, env", ROUTES, ids=ROUTE_IDS)
def test_wide_rows(oracle, monkeypatch, dt, path, env):
    """W0's and the builders' lane loops take a second trip (pitch > 1024 bytes); the host call from a strided source at an odd
    address and the device call from four sources (aligned at the pitch, aligned with a gap, unaligned by the stride, unaligned by
    the offset) write the same rows"""
    import torch
    if env is not None:
        monkeypatch.setenv("MVF_STREAM_5P1", env)
    for dim in W.WIDE_DIMS[dt]:
        w = W.wide_world(oracle, dt, dim)
        (pos, new), = w.writes
        row_bytes = dim * _es(dt)
        pitch = (row_bytes + 15) // 16 * 16
        assert pitch // 16 > 64
        with _handle(w.rows1, path) as twin:
            for source in ("host", (pitch, 0), (pitch + 16, 0), (row_bytes + 3, 0), (pitch + 16, 1)):
                what = f"wide world dtype {dt} path {path} dim {dim} source {source}"
                with _handle(w.rows0, path) as c:
                    inf = c.info()
                    assert inf.pitch_bytes == pitch
                    shadows = _resident(c, w, path)
                    if source == "host":
                        rep = _host_write_strided(c, pos, new, row_bytes + 24)
                    else:
                        dev, ptr = W.device_source(new, *source)
                        rep = c.write_rows_device(pos, ptr, source[0], torch.cuda.current_stream().cuda_stream)
                        torch.cuda.synchronize()
                    _expect_report(rep, W.WIDE_COUNT, shadows, inf, dt, dim, path)
                    _rows_and_pad_bytes(oracle, w, path, c, twin, what)
                    if source == "host":
                        _same_kernel_same_answer(oracle, w, dt, path, c, twin, what)
                    else:
                        _sweep(oracle, w, dt, path, c, twin, what)


# ---- C ------------------------------------------------------------------------------------------------------------------------
C_ROUTES = [(F32, 7, "0"), (F32, 7, "1"), (F32, 3, None), (F32, 4, None), (F16, 5, None), (I8, 2, None), (U8, 2, None)]
C_IDS = [f"dt{dt}-path{p}" + (f"-5p1={e}" if e else "") for dt, p, e in C_ROUTES]


@pytest.mark.parametrize("dim", [50, 256])
@pytest.mark.parametrize("dt, path, env", C_ROUTES, ids=C_IDS)
def test_device_writes_in_flight_with_everything_resident(oracle, monkeypatch, dt, path, env, dim):
    """the world's three writes through the device call, back to back on one non-default stream, from ONE device buffer at a stride
    of pitch + 16: W1 behind a device call, from a caller's stride, on a caller's stream, the pinned upload buffer reused by a
    write while the copy of the one before may be in flight.  Each report is the host call's on a handle in the same state."""
    import torch
    if env is not None:
        monkeypatch.setenv("MVF_STREAM_5P1", env)
    w = W.world(oracle, dt, dim)
    what = f"dtype {dt} path {path} dim {dim}"
    stride = (dim * _es(dt) + 15) // 16 * 16 + 16
    every = np.concatenate([rows for _, rows in w.writes])
    dev, ptr = W.device_source(every, stride)
    stream = torch.cuda.Stream()
    with _handle(w.rows0, path) as c, _handle(w.rows0, path) as host, _handle(w.rows1, path) as twin:
        shadows = _resident(c, w, path)
        assert _resident(host, w, path) == shadows
        inf = c.info()
        torch.cuda.synchronize()
        reports, at = [], 0
        for pos, rows in w.writes:  # no host synchronisation in between
            reports.append(c.write_rows_device(pos, ptr + at * stride, stride, stream.cuda_stream))
            at += len(pos)
        for rep, (pos, rows) in zip(reports, w.writes):
            assert rep == host.write_rows(pos, rows), f"{what}: the report of the device call and of the host call"
            _expect_report(rep, len(pos), shadows, inf, dt, dim, path)
        torch.cuda.synchronize()
        _sweep(oracle, w, dt, path, c, twin, what)
        assert c.read_rows(0, N).tobytes() == w.rows1.tobytes(), what
        del dev


@pytest.mark.parametrize("dt, path, env, dim", [(F32, 7, "0", 50), (F32, 7, "1", 256), (I8, 2, None, 50)],
                         ids=["f32-path7-5p1=0-dim50", "f32-path7-5p1=1-dim256", "i8-path2-dim50"])
def test_the_upload_buffer_grows_between_writes_in_flight(oracle, monkeypatch, dt, path, env, dim):
    """a write of 1 row (its list fits the upload buffer's first 16 KiB), the large world's write of 16389 rows (a list of 64 KiB: the
    buffer is replaced by a larger one) and a write of 37 other rows (the larger buffer reused), on one stream with no wait in
    between.  The first write puts a WRONG row where the second puts the right one; the third turns 37 rows that are the worst of
    their queries under InnerProduct (the negated old rank 1) into their best (the query times 2e3)."""
    import torch
    if env is not None:
        monkeypatch.setenv("MVF_STREAM_5P1", env)
    w = W.large_world(oracle, dt, dim)
    (pos, new), = w.writes
    what = f"large world dtype {dt} path {path} dim {dim}"
    wrong = (pos[:1], np.ascontiguousarray(w.rows0[pos[-1:].astype(np.int64)]))
    own = {i: mine for s in w.planted for i, mine in w.planted[s]}
    late = [(i, own[i][-1]) for i in range(5, NQ) if len(own[i]) == 3][:37]  # (query, the position of its negated old rank 1)
    assert len(late) == 37
    third = (np.array([p for _, p in late], np.uint64), np.stack([W._scaled(w.q[i], dt) * 2 if dt in (F32, F16) else W._scaled(w.q[i], dt)
                                                                  for i, _ in late]).astype(NP[dt]))
    rows2 = w.rows1.copy()
    rows2[third[0].astype(np.int64)] = third[1]
    if dt in (F32, F16):  # (a property of the reference alone)
        best = oracle.search(rows2, dt, IP, w.q, 1)[1][:, 0].astype(np.int64)
        assert all(best[i] == p for i, p in late), "the rows of the third write are their queries' best"
    stride = (dim * _es(dt) + 15) // 16 * 16 + 16
    writes = [wrong, (pos, new), third]
    dev, ptr = W.device_source(np.concatenate([r for _, r in writes]), stride)
    stream = torch.cuda.Stream()
    with _handle(w.rows0, path) as c, _handle(w.rows0, path) as host, _handle(rows2, path) as twin:
        shadows = _resident(c, w, path)
        assert _resident(host, w, path) == shadows
        inf = c.info()
        torch.cuda.synchronize()
        reports, at = [], 0
        for p, rows in writes:
            reports.append(c.write_rows_device(p, ptr + at * stride, stride, stream.cuda_stream))
            at += len(p)
        for rep, (p, rows) in zip(reports, writes):
            assert rep == host.write_rows(p, rows), f"{what}: the report of the device call and of the host call"
            _expect_report(rep, len(p), shadows, inf, dt, dim, path)
        torch.cuda.synchronize()
        assert c.read_rows(0, W.LARGE_N).tobytes() == rows2.tobytes(), what
        rows32 = rows2.astype(np.float32)
        for metric in METRICS:
            for nq in W.route_nqs(path):
                got, want = c.search(w.q[:nq], K, metric), twin.search(w.q[:nq], K, metric)
                tell = f"{what}: metric {metric} nq {nq}"
                if W.bits_promised(dt, path, nq):
                    same(got, want, tell)
                else:
                    W.check_rows_against_oracle(oracle, dt, rows2, w.q[:nq], metric, want, tell + " (twin)", rows32)
                W.check_rows_against_oracle(oracle, dt, rows2, w.q[:nq], metric, got, tell, rows32)
        del dev


# ---- D ------------------------------------------------------------------------------------------------------------------------
def _masked_scores(oracle, dt, rows, q, metric, allowed):
    """the oracle's score of every row for one query, NaN (behind every other score) where the row may not be reported"""
    ref = oracle.scores(rows, dt, metric, q)[0].copy()
    ref[~allowed] = np.nan
    return ref


def _check_listed(oracle, w, metric, queries, allowed, res, rows32, what):
    """the tolerance criterion of one result row per query over the rows `allowed` [nq, N] admits"""
    from _util import assert_float_topk
    for qi in range(len(queries)):
        ref = _masked_scores(oracle, w.dt, w.rows1, queries[qi], metric, allowed[qi])
        try:
            assert_float_topk(metric, res.scores[qi], res.indices[qi], ref, rows32, queries[qi].astype(np.float32), min(K, int(allowed[qi].sum())))
        except AssertionError as e:
            raise AssertionError(f"{what}, query {qi}: {e}") from e


@pytest.mark.parametrize("route", ["1", "2"])
@pytest.mark.parametrize("dt", [F32, F16])
def test_float_rows_behind_every_entry_point(oracle, monkeypatch, dt, route):
    """the consumers of the norms and shadows W1 refreshed, on float rows: the mask route of a filtered search, the batched radius
    route (corpus_row_norms, batched_tau), the MaxSim MFMA selection (norms, maxsim_margin), the join's batched windows, and the
    list searches.  Norms and shadows are resident and every object exists BEFORE the write; the twin's objects are made behind it."""
    monkeypatch.setenv("MVF_FILTER_ROUTE", route)
    dim = 50
    w = W.world(oracle, dt, dim)
    rows32 = W.rows_f32(w)
    rng = np.random.default_rng(5)
    mask = rng.random(N) < 0.5
    mask[w.written[::2]] = True
    values = (np.arange(N) % 37).astype(np.uint32)
    where = values < 20
    q3 = w.q[:3]
    cand = np.stack([np.concatenate([w.written[i::7][:40], rng.integers(0, N, 24)]) for i in range(3)]).astype(np.uint64)
    sets = np.ascontiguousarray(w.q[:12].reshape(3, 4, dim))
    ckeys = np.arange(0, 30, 2)
    for metric in (IP, COS):
        assert G.maxsim_route(N, 37, dim, dt, metric, 3, 4, K, 2) == 2, "Float rows under InnerProduct / Cosine: the MFMA selection route"
    assert G.maxsim_route(N, 37, dim, dt, L2, 3, 4, K, 2) == 1
    if dt == F32:
        assert G.radius_route(F32, 32, 0) == 1 and G.radius_route(F32, 3, 0) == 0

    def objects(c):
        col = c.attach_column(values)
        return dict(bitmap=c.make_filter(mask), col=col, where=c.make_filter_where([(col, "<", 20)]), part=c.make_partition(col))

    def bits(c, o, radius):
        out = {}
        for metric in METRICS:
            out["partitioned", metric] = c.search_partitioned(q3, [3, 4, 36], K, metric, o["part"])
            out["grouped", metric] = c.search_grouped(q3, K, 2, metric, o["part"])
            for r in (1, 2):
                c.set_maxsim_route(r)
                out["maxsim", r, metric] = c.search_maxsim(sets, K, metric, o["part"])
                out["maxsim_candidates", r, metric] = c.search_maxsim_candidates(sets, ckeys, K, metric, o["part"])
            c.set_maxsim_route(0)
            out["candidates", metric] = c.search_candidates(q3, cand, K, metric)
            out["mmr", metric] = c.search_mmr(q3, cand, K, 0.5, metric)
            out["radius 3", metric] = c.search_radius(q3, radius[metric][:3], 20, metric)
            out["radius 32", metric] = c.search_radius(w.q[:32], radius[metric], 20, metric)
        return out

    def tolerance(c, o):
        out = {}
        for metric in METRICS:
            for nq in (3, NQ):
                out["bitmap", metric, nq] = c.search_filtered(w.q[:nq], K, metric, o["bitmap"])
                out["where", metric, nq] = c.search_filtered(w.q[:nq], K, metric, o["where"])
            out["join 0", metric] = c.knn_join(K, metric, 0, 128)
            out["join 4000", metric] = c.knn_join(K, metric, 4000, N - 4000)
        return out

    with _handle(w.rows0, 0) as c, _handle(w.rows1, 0) as twin:
        o = objects(c)  # before the write
        for metric in METRICS:  # norms and shadows resident
            c.search(w.q[:1], K, metric)
            c.search(w.q, K, metric)
        c.search_radius(w.q[:32], 0.0, 20, IP)
        c.set_maxsim_route(2)
        c.search_maxsim(sets, K, IP, o["part"])
        c.set_maxsim_route(0)
        shadows = c.info().shadows
        reports = [c.write_rows(pos, rows) for pos, rows in w.writes]
        for rep, count in zip(reports, COUNTS):
            assert rep["rows_written"] == count and rep["refreshed"] & NORMS, "the norms were resident"
            assert rep["refreshed"] & W.expect_refreshed(shadows) == W.expect_refreshed(shadows)
        ot = objects(twin)
        radius = {m: twin.search(w.q[:32], 15, m).scores[:, -1].copy() for m in METRICS}  # about fifteen matches per query
        got, want = bits(c, o, radius), bits(twin, ot, radius)
        for key in got:
            same(got[key], want[key], f"dtype {dt} MVF_FILTER_ROUTE={route}: {key}")
            if key[0] not in ("maxsim", "maxsim_candidates"):  # (their answers are keys, not positions)
                real = got[key].indices[got[key].indices != np.uint64(0xFFFFFFFFFFFFFFFF)].astype(np.int64)
                assert np.isin(real, w.written).any(), f"{key}: no written position in any answer"
        assert (got["radius 32", L2].counts >= 15).all()
        got, want = tolerance(c, o), tolerance(twin, ot)
        for key in got:
            metric = key[1]
            if key[0] in ("bitmap", "where"):
                queries, allowed = w.q[:key[2]], np.broadcast_to(mask if key[0] == "bitmap" else where, (key[2], N))
            else:
                first = 0 if key[0] == "join 0" else 4000
                queries = w.rows1[first:first + (128 if first == 0 else N - 4000)].astype(np.float32)
                allowed = np.ones((len(queries), N), bool)
                allowed[np.arange(len(queries)), first + np.arange(len(queries))] = False  # the join leaves the query row itself out
            for res, side in ((got[key], ""), (want[key], " (twin)")):
                _check_listed(oracle, w, metric, queries, allowed, res, rows32, f"dtype {dt} MVF_FILTER_ROUTE={route}: {key}{side}")
            assert np.isin(got[key].indices.astype(np.int64), w.written).any(), f"{key}: no written position in any answer"
        for x in list(o.values()) + list(ot.values()):
            x.close()


# ---- E ------------------------------------------------------------------------------------------------------------------------
E_ROUTES = ([(F32, 7, "0", 50), (F32, 7, "1", 256)] + [(F32, p, None, 50) for p in (3, 4, 2, 5, 6, 0)] + [(F16, p, None, 50) for p in (5, 2, 6, 0)])
E_CASES = [(dt, p, e, dim, kind) for dt, p, e, dim in E_ROUTES for kind in W.OUTLIER_KINDS[dt]]
E_IDS = [f"dt{dt}-path{p}" + (f"-5p1={e}" if e else "") + f"-{kind}" for dt, p, e, dim, kind in E_CASES]


def _check_queries(oracle, w, metric, q, res, cached, what):
    """the tolerance criterion for the queries q over the world's changed rows; cached[i]: q[i] is w.q[i]"""
    from _util import assert_float_topk
    for qi in range(len(q)):
        ref = W.all_scores(oracle, w, metric, qi) if cached[qi] else oracle.scores(w.rows1, w.dt, metric, q[qi])[0]
        try:
            assert_float_topk(metric, res.scores[qi], res.indices[qi], ref, W.rows_f32(w), q[qi].astype(np.float32), K)
        except AssertionError as e:
            raise AssertionError(f"{what}, query {qi}: {e}") from e


@pytest.mark.parametrize("dt, path, env, dim, kind", E_CASES, ids=E_IDS)
def test_lowered_outliers(oracle, monkeypatch, dt, path, env, dim, kind):
    """DESIGN.md §3 "The maxima are never lowered": a handle whose maxima -- the norm maximum, qs_stats, qs6_stats -- were raised by
    rows that are gone again answers as its twin does, also for the all-zero query (0 x inf in the bounds), a query of norm 1e-20
    and one of norm 1e15 (Float16 rows: 1e3).  The outliers go to the positions 64 and 4100 while everything is resident, the
    world's own content and its three writes follow.  Only answers are compared: the handle may scan with another kernel than its
    twin (a maximum of +inf sends a shadow route to the stored rows), and nothing is said about time.  (Integer spaces have no
    maxima and no rows of this kind.)

    The kernels (mvfgpu_timing::scan_kernel) as an MI355X reported them behind the last write, handle / twin, the same under every
    metric: on path 7 one query scans with kernel 7 on both sides behind the huge rows and with 1 / 7 behind the overflowing and the
    Inf / NaN rows (qs6_stats is +inf: the handle reads the stored rows); on path 0 one query scans with 1 / 1 and 64 queries with
    4 / 6 on Float32 and 3 / 6 on Float16 rows behind every kind of outlier (presumably the handle's int8 selection went off while
    the outliers were resident: the repair feedback is left as it is); on the paths 2, 3, 4, 5 and 6 both sides use one kernel
    (Float32: 2, 4, 5, 6 and 7 for one query / 6 for 64; Float16: 3, 6 and 7 / 6)."""
    if env is not None:
        monkeypatch.setenv("MVF_STREAM_5P1", env)
    w = W.world(oracle, dt, dim)
    at = np.array(W.OUTLIER_AT, np.uint64)
    what = f"dtype {dt} path {path} dim {dim}, {kind} rows written and replaced"
    with _handle(w.rows0, path) as c, _handle(w.rows1, path) as twin:
        shadows = _resident(c, w, path)
        rep = c.write_rows(at, W.outlier_rows(dt, dim, kind, w.rows0[at.astype(np.int64)]))
        assert rep["refreshed"] & W.expect_refreshed(shadows) == W.expect_refreshed(shadows) and (path == 1 or rep["refreshed"] & NORMS)
        for metric in METRICS:  # the outliers are seen: what is cached from a read-back of the maxima is cached now
            c.search(w.q[:1], K, metric)
            c.search(w.q[:W.route_nqs(path)[-1]], K, metric)
        c.write_rows(at, w.rows1[at.astype(np.int64)])
        for pos, rows in w.writes:
            c.write_rows(pos, rows)
        assert c.read_rows(0, N).tobytes() == w.rows1.tobytes()
        _sweep(oracle, w, dt, path, c, twin, what)
        for name, x in W.extreme_queries(dt, dim, w.q[0]).items():
            batch = np.concatenate([w.q[:NQ - 1], x[None, :]]).astype(np.float32)
            for metric in METRICS:
                for q, cached in ((x[None, :], [False]), (batch, [True] * (NQ - 1) + [False])):
                    got, want = c.search(q, K, metric), twin.search(q, K, metric)
                    tell = f"{what}: the {name} query{' in a batch of 64' if len(q) > 1 else ''}, metric {metric}"
                    if W.bits_promised(dt, path, len(q)):
                        same(got, want, tell)
                    else:
                        _check_queries(oracle, w, metric, q, want, cached, tell + " (twin)")
                    _check_queries(oracle, w, metric, q, got, cached, tell)


@pytest.mark.parametrize("dim", [50, 256])
def test_shadows_built_behind_a_lowered_overflow(oracle, monkeypatch, dim):
    """A state only writes reach: the norms and the f16 shadow are resident (64 queries on path 3), a row whose sum of squares
    overflows f32 is written and replaced, and only THEN the int8 and the 6-bit shadow are built -- from clean rows, their own maxima
    finite, beside a norm maximum of +inf.  One query on the paths 0, 6 and 7, the batched radius search and the MaxSim MFMA
    selection answer with the twin's bytes.  Both sides scan with the same kernel here (an MI355X reported 1 on path 0 and 7, K1
    over the selection shadow, on the paths 6 and 7, at both dimensions): the shadows' own maxima are finite, so the handle stays
    on its shadow routes, and the test holds that too."""
    monkeypatch.setenv("MVF_STREAM_5P1", "1")
    w = W.world(oracle, F32, dim)
    at = np.array(W.OUTLIER_AT, np.uint64)
    values = (np.arange(N) % 37).astype(np.uint32)
    sets = np.ascontiguousarray(w.q[:12].reshape(3, 4, dim))
    with _handle(w.rows0, 3) as c, _handle(w.rows0, 3) as twin:
        for h in (c, twin):
            h.set_profiling(True)
        for metric in METRICS:
            c.search(w.q, K, metric)
        assert c.info().shadows & 2 and not c.info().shadows & (1 | 4 | 8), "norms and the f16 shadow, no int8 / 6-bit shadow"
        rep = c.write_rows(at, W.outlier_rows(F32, dim, "overflowing", None))
        assert rep["refreshed"] == NORMS | S_F16
        c.write_rows(at, w.rows0[at.astype(np.int64)])
        assert c.read_rows(0, N).tobytes() == w.rows0.tobytes()
        for path in (0, 6, 7):
            for h in (c, twin):
                h.set_scan_path(path)
            for metric in METRICS:
                got, want = c.search(w.q[:1], K, metric), twin.search(w.q[:1], K, metric)
                assert c.last_timing().scan_kernel == twin.last_timing().scan_kernel == (1 if path == 0 else 7), "K1 over the selection shadow"
                same(got, want, f"dim {dim} path {path} metric {metric}: shadows built behind a lowered overflow")
        assert c.info().shadows & (1 | 8) == 9, "the int8 and the 6-bit shadow were built behind the replacement"
        for h in (c, twin):
            h.set_scan_path(0)
        radius = {m: twin.search(w.q[:32], 15, m).scores[:, -1].copy() for m in METRICS}
        for metric in METRICS:
            same(c.search_radius(w.q[:32], radius[metric], 20, metric), twin.search_radius(w.q[:32], radius[metric], 20, metric),
                 f"dim {dim} metric {metric}: the batched radius search behind a lowered overflow")
        objs = []
        for h in (c, twin):
            col = h.attach_column(values)
            objs += [col, h.make_partition(col)]
            h.set_maxsim_route(2)
        for metric in METRICS:
            same(c.search_maxsim(sets, K, metric, objs[1]), twin.search_maxsim(sets, K, metric, objs[3]),
                 f"dim {dim} metric {metric}: the MaxSim MFMA selection behind a lowered overflow")
        for x in objs[::-1]:
            x.close()


# ---- F ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt, path, env, dim, nq", [(F32, 3, None, 50, NQ), (F32, 7, "0", 50, 1), (F32, 7, "1", 256, 1), (F16, 5, None, 50, NQ)],
                         ids=["f32-path3-nq64", "f32-path7-5p1=0-nq1", "f32-path7-5p1=1-nq1", "f16-path5-nq64"])
def test_a_write_between_searches_that_read_the_refreshed_state(oracle, monkeypatch, dt, path, env, dim, nq):
    """search on stream A, a device write of 700 rows on stream B, search on stream A, ONE synchronisation, with the shadow the
    searches select on resident: W1 is ordered behind the kernel that reads the shadow it rewrites and before the next.  The first
    search answers as a handle of the old rows, the second as the twin; the planting keeps them apart (a new row in the first
    answer, or an old rank 1 in the second, is outside the tolerance)."""
    import torch
    if env is not None:
        monkeypatch.setenv("MVF_STREAM_5P1", env)
    w = W.world(oracle, dt, dim)
    pos, new = w.writes[2]
    rows1 = w.rows0.copy()
    rows1[pos.astype(np.int64)] = new
    r32 = {0: w.rows0.astype(np.float32), 1: rows1.astype(np.float32)}
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    q = np.ascontiguousarray(w.q[:nq])
    dq = torch.from_numpy(q).cuda()
    dnew = torch.from_numpy(new.view(np.uint8).reshape(len(pos), -1)).cuda()
    qcode = G.query_dtype_code(dt)
    with _handle(w.rows0, path) as old, _handle(rows1, path) as twin:
        for metric in METRICS:
            outs = [(torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda"),
                     torch.empty((nq, K), dtype=torch.int32, device="cuda")) for _ in range(2)]
            with _handle(w.rows0, path) as c:
                shadows = _resident(c, w, path)
                assert shadows & (2 if path == 3 else 1) and (path != 7 or shadows & 8)
                torch.cuda.synchronize()
                c.search_device(dq.data_ptr(), qcode, dim, nq, K, metric, outs[0][0].data_ptr(), outs[0][1].data_ptr(), outs[0][2].data_ptr(), a.cuda_stream)
                rep = c.write_rows_device(pos, dnew.data_ptr(), dim * _es(dt), b.cuda_stream)
                c.search_device(dq.data_ptr(), qcode, dim, nq, K, metric, outs[1][0].data_ptr(), outs[1][1].data_ptr(), outs[1][2].data_ptr(), a.cuda_stream)
                torch.cuda.synchronize()
                assert rep["refreshed"] & W.expect_refreshed(shadows) == W.expect_refreshed(shadows) and rep["refreshed"] & NORMS
                for i, (ref, rows, side) in enumerate(((old, w.rows0, "the search before the write"), (twin, rows1, "the search behind the write"))):
                    s, ix, r = outs[i]
                    got = G.SearchResult(s.cpu().numpy(), ix.cpu().numpy().view(np.uint64), r.cpu().numpy())
                    tell = f"dtype {dt} path {path} dim {dim} metric {metric}: {side}"
                    want = ref.search(q, K, metric)
                    if W.bits_promised(dt, path, nq):
                        same(got, want, tell)
                    else:
                        W.check_rows_against_oracle(oracle, dt, rows, q, metric, want, tell + " (its reference handle)", r32[i])
                    W.check_rows_against_oracle(oracle, dt, rows, q, metric, got, tell, r32[i])
                assert c.read_rows(0, N).tobytes() == rows1.tobytes()
