"""Wide rows on the GPU: every route at its dimension switches and at the limits of i32 (references: tests/_wide.py).

Between dimension 3000 and the widest row the library accepts the code changes route at least nine times (DESIGN.md
section 5, "Dimension switches"); each group below sits on both sides of some of them and asserts WHICH KERNEL RAN
(`last_timing().scan_kernel`) next to the answer, and that no query of a batched search was handed to the repair pass
(`repaired_queries == 0`): a repaired query is answered by K1, and a test that lets K1 answer for K2 checks nothing about K2.

  A  saturated Int8 / UInt8 rows on the batched route: 8192 (the folded pre-filter at the edge of its range), 8193 and
     33025 (the old epilogue without its first stage); sums next to 2^31
  B  the same rows through K1 on both sides of the four-query pass' LDS rule; k up to 2048 by passes and by the sort
  C  ... through radius and candidate search at dimension 33025
  D  wide Float32 / Float16 top-k against float64 on both sides of the int8-shadow and f16-shadow switches, up to the
     largest dimension K1 takes
  E  one Float32 query streaming the int8 shadow at its widest (8192), and not at 8200
  F  the bit-identity contracts (candidates = K1, radius = K1, batched radius = streaming radius, a call of several
     queries = the same queries one by one) at 12296 and 33000
  G  the refusal past K1's and R1's limits: a clean MVF_ERR_BUILD, nothing left behind

Integer answers are bit-exact against exact int64 sums; float answers are held to DESIGN.md section 3's tolerance against
float64 (not against the strict-order f32 oracle, whose own rounding reaches most of that tolerance at these widths:
tests/test_wide_cpu.py).  Every query of every case is compared."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from metrovector_amd import errors as E
from metrovector_amd import gpu as G

import _wide as W
from _candidates import oracle_candidates
from _radius import assert_float_radius, oracle_radius
from _util import assert_exact, assert_float_topk
from _wide import COS, F16, F32, I8, IP, L2, U8

pytestmark = pytest.mark.gpu
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
METRICS = (L2, IP, COS)
K1_STORED, K2_F32, K2_STORED, K2_F16_SHADOW, K2_I8_SHADOW, K1_I8_SHADOW, K1_DUMP_SORT = 1, 2, 3, 4, 6, 7, 8  # mvfgpu_timing.scan_kernel


def _route(rows, dim, dtype, metric, nq, k):
    out = C.c_uint32(99)
    G._lib.gpu_check(G._lib.gpu().mvfgpu_selftest_route(rows, dim, dtype, metric, nq, k, C.byref(out)))
    return out.value


def _same(a, b, what=""):
    assert (a.indices == b.indices).all(), f"{what}: other rows"
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), f"{what}: other score bits"
    assert (a.raw == b.raw).all(), f"{what}: other raw values"


# =====================================================================================================================
# A / B / C -- saturated Int8 / UInt8 rows
# =====================================================================================================================
N_INT = 9000          # thresholded phases of the batched kernels run (the direct phase alone never reaches the pre-filter)
NQ_INT = 257


def _int_corpus(oracle, dtype, dim, nq):
    seed = 0x5A70000 + 100_000 * dtype + dim
    rows, pos = W.saturated_rows(oracle, seed, N_INT, dim, dtype)
    q = W.saturated_queries(oracle, seed + 1, nq, dim, dtype)
    dot, qq, xx = W.int_raw(rows, q)
    c = G.GpuCorpus.from_array(rows)
    c.set_profiling(True)
    return SimpleNamespace(dtype=dtype, dim=dim, rows=rows, pos=pos, q=q, dot=dot, qq=qq, xx=xx, c=c)


@pytest.fixture(scope="module", params=[(dt, dim) for dt in (I8, U8) for dim in (8192, 8193, 33025)],
                ids=lambda p: f"{'i8' if p[0] == I8 else 'u8'}-{p[1]}")
def int_batched(request, oracle):
    s = _int_corpus(oracle, *request.param, NQ_INT + 4)   # four spare: a sane batch of 257 without the all-zero queries
    yield s
    s.c.close()


def _batches(s, metric, nq):
    """[(first nq queries of a batch, their positions in s.q, may the repair pass run)].  Always the SANE batch: queries some
    row answers better than another -- no query of it may be repaired.  Under InnerProduct / Cosine an all-zero query (the
    all-zero and, on UInt8, the all-min query) scores every row alike: all 9000 rows tie at its threshold, no candidate budget
    holds them and the batched route hands it to K1 by design.  The batch WITH such queries is searched too and must be
    answered exactly, but is a repair case: on UInt8 cosine at dimension <= 8192 the zero query also takes the 64 queries
    of its half of the tile along (64-66 of 128 repaired, none in the sane batch; the folded pre-filter's per-row bound is
    shared by a query half, and a threshold of 0 in it presumably loosens every other query's)."""
    sane = np.nonzero(s.qq != 0)[0] if metric in (IP, COS) else np.arange(len(s.qq))
    out = [(sane[:nq], False)]
    if len(sane) < len(s.qq):
        out.append((np.arange(nq), True))
    return out


@pytest.mark.parametrize("metric", METRICS)
def test_a_saturated_integers_on_the_batched_route(oracle, int_batched, metric):
    s = int_batched
    assert int((s.qq[:, None] + s.xx[None, :] - 2 * s.dot).max()) == 65025 * s.dim  # all-min against all-max is in play
    want100 = W.int_topk(metric, s.dot, s.qq, s.xx, 100)
    # the C oracle as a second witness of the reference, first 16 queries (k = 10 is a prefix of k = 100)
    osc, oidx, oraw = oracle.search(s.rows, s.dtype, metric, s.q[:16], 100)
    assert (want100[1][:16] == oidx).all() and (want100[2][:16] == oraw).all()
    assert (want100[0][:16].view(np.uint32) == osc.view(np.uint32)).all()
    for path in (2, 0):
        s.c.set_scan_path(path)
        for nq in (40, 128, 257):          # the <= 64-query streaming kernel; both tile shapes, the last tile ragged
            assert path == 2 or _route(N_INT, s.dim, s.dtype, metric, nq, 100) == 1
            for k in (10, 100):
                for sel, repair_case in _batches(s, metric, nq):
                    assert len(sel) == nq
                    res = s.c.search(s.q[sel], k, metric)
                    t = s.c.last_timing()
                    tag = f"dtype {s.dtype} dim {s.dim} metric {metric} path {path} nq {nq} k {k} repair case {repair_case}"
                    assert t.scan_kernel == K2_STORED, tag
                    assert repair_case or t.repaired_queries == 0, f"{tag}: {t.repaired_queries} queries repaired"
                    assert (res.indices == want100[1][sel, :k]).all(), tag
                    assert (res.raw == want100[2][sel, :k]).all(), tag
                    assert (res.scores.view(np.uint32) == want100[0][sel, :k].view(np.uint32)).all(), tag
    s.c.set_scan_path(0)


@pytest.mark.parametrize("dtype,dim", [(U8, 8192), (I8, 8193)])
def test_a_saturated_integers_with_tombstones_and_ids(oracle, dtype, dim):
    """Half of the planted rows deleted (the all-min row among them: the largest values left are near-ties), vector ids."""
    s = _int_corpus(oracle, dtype, dim, 128 + 4)
    try:
        dead = np.zeros(N_INT, bool)
        dead[s.pos[::2]] = True
        dead[::7] = True
        ids = np.random.default_rng(dim).permutation(np.arange(1 << 40, (1 << 40) + N_INT)).astype(np.uint64)
        s.c.set_tombstones(np.packbits(dead, bitorder="little"))
        s.c.set_vector_ids(ids)
        for metric in METRICS:
            want = W.int_topk(metric, s.dot, s.qq, s.xx, 100, dead=dead, labels=ids)
            for nq in (40, 128):
                for sel, repair_case in _batches(s, metric, nq):
                    res = s.c.search(s.q[sel], 100, metric)
                    t = s.c.last_timing()
                    assert t.scan_kernel == K2_STORED and (repair_case or t.repaired_queries == 0), (metric, nq, t.repaired_queries)
                    assert_exact(res, want[0][sel], want[1][sel], want[2][sel])
    finally:
        s.c.close()


@pytest.fixture(scope="module", params=[(dt, dim) for dt in (I8, U8) for dim in (28000, 33025)],
                ids=lambda p: f"{'i8' if p[0] == I8 else 'u8'}-{p[1]}")
def int_k1(request, oracle):
    s = _int_corpus(oracle, *request.param, 8)
    s.c.set_scan_path(1)
    yield s
    s.c.close()


def test_b_the_two_dimensions_straddle_the_four_query_rule():
    """scan_lds_bytes restated (tests/_wide.py): at k <= 512 two to four Int8 / UInt8 queries share one pass up to
    dimension 29696 and run as one-query passes beyond; group B runs 28000 and 33025."""
    for k in (1, 100, 512):
        assert W.k1_four_query_pass(I8, 28000, k) and not W.k1_four_query_pass(I8, 33025, k)
    assert W.k1_lds_bytes(U8, 33025, 1, 2048) <= W.K1_MAX_LDS  # integer rows never meet the refusal


@pytest.mark.parametrize("metric", METRICS)
def test_b_saturated_integers_on_k1(int_k1, monkeypatch, metric):
    s = int_k1
    for k in (1, 100, 1024):
        want = W.int_topk(metric, s.dot, s.qq, s.xx, k)
        for sel in ([0], [1], [2], [3], [5], [0, 1, 2], [3, 4, 5]):     # one query; three queries in one call
            res = s.c.search(s.q[sel], k, metric)
            assert s.c.last_timing().scan_kernel == K1_STORED
            assert_exact(res, want[0][sel], want[1][sel], want[2][sel])
    # k = 2048: by passes behind a floor and by the whole-shard sort -- the largest and the smallest integer keys go
    # through the rank entries (whose two top key values are reserved)
    want = W.int_topk(metric, s.dot, s.qq, s.xx, 2048)
    try:
        for mode, kernel in ((1, K1_STORED), (2, K1_DUMP_SORT)):
            monkeypatch.setenv("MVF_LARGE_K", str(mode))
            s.c.reload_tuning()
            for sel in ([0], [1], [3, 4, 5]):
                res = s.c.search(s.q[sel], 2048, metric)
                assert s.c.last_timing().scan_kernel == kernel, (mode, sel)
                assert_exact(res, want[0][sel], want[1][sel], want[2][sel])
    finally:
        monkeypatch.delenv("MVF_LARGE_K", raising=False)
        s.c.reload_tuning()


@pytest.mark.parametrize("dtype", [I8, U8])
def test_c_saturated_integers_through_radius_and_candidates(oracle, dtype):
    dim = W.MAX_INT_DIM
    s = _int_corpus(oracle, dtype, dim, 6)
    ref = W.IntScores(s.rows, s.q)
    try:
        near = np.float32
        for metric in METRICS:
            for qi, row in ((1, s.pos[0]), (1, s.pos[4]), (0, s.pos[1]), (2, s.pos[2]), (4, s.pos[3])):
                sc = ref.scores(s.rows, dtype, metric, s.q[qi])[0]
                at = near(sc[row])  # the planted row's own score: exactly on it, one f32 below, one above
                for radius in (at, np.nextafter(at, near(-np.inf)), np.nextafter(at, near(np.inf))):
                    want_n = oracle_radius(ref, s.rows, dtype, metric, s.q[qi], radius, 0)[0]
                    res0 = s.c.search_radius(s.q[qi], float(radius), 0, metric)       # counts only
                    tag = f"dtype {dtype} metric {metric} query {qi} row {row} radius {float(radius)!r}"
                    assert int(res0.counts[0]) == want_n, tag
                    for m in (40, want_n + 3) if want_n <= 5000 else (40,):        # fewer than the count; more than it
                        cnt, wsc, widx, wraw = oracle_radius(ref, s.rows, dtype, metric, s.q[qi], radius, m)
                        res = s.c.search_radius(s.q[qi], float(radius), m, metric)
                        assert int(res.counts[0]) == cnt, tag
                        assert (res.indices[0] == widx).all(), tag
                        assert (res.scores[0].view(np.uint32) == wsc.view(np.uint32)).all(), tag
                        live = widx != PAD
                        assert (res.raw[0][live] == wraw[live]).all(), tag
        # several queries in one call, a radius each
        for metric in METRICS:
            radii = []
            for qi in range(6):
                sc, keys, _ = ref.scores(s.rows, dtype, metric, s.q[qi])
                radii.append(sc[np.lexsort((np.arange(N_INT), keys))[30]])        # the 31st best: >= 31 matches
            res = s.c.search_radius(s.q, np.array(radii, np.float32), 64, metric)
            for qi in range(6):
                cnt, wsc, widx, wraw = oracle_radius(ref, s.rows, dtype, metric, s.q[qi], radii[qi], 64)
                assert int(res.counts[qi]) == cnt and (res.indices[qi] == widx).all(), (metric, qi)
                assert (res.scores[qi].view(np.uint32) == wsc.view(np.uint32)).all(), (metric, qi)
        # candidate lists naming the planted rows: duplicates, padding, positions outside the shard
        rng = np.random.default_rng(dtype)
        lists = np.full((6, 96), PAD, np.uint64)
        for qi in range(6):
            names = list(s.pos) + list(s.pos[:8]) + [N_INT, N_INT + 5, 1 << 40] + rng.integers(0, N_INT, 40).tolist()
            rng.shuffle(names)
            lists[qi, :len(names)] = names
        for metric in METRICS:
            for k in (5, 200):      # fewer than the list holds; more than it
                res = s.c.search_candidates(s.q, lists, k, metric)
                for qi in range(6):
                    cnt, wsc, widx, wraw = oracle_candidates(ref, s.rows, dtype, metric, s.q[qi], lists[qi], k)
                    tag = f"dtype {dtype} metric {metric} query {qi} k {k}"
                    assert int(res.counts[qi]) == cnt, tag
                    assert (res.indices[qi] == widx).all(), tag
                    assert (res.scores[qi].view(np.uint32) == wsc.view(np.uint32)).all(), tag
                    assert (res.raw[qi][widx != PAD] == wraw[widx != PAD]).all(), tag
    finally:
        s.c.close()


# =====================================================================================================================
# D / F -- wide Float32 / Float16 rows
# =====================================================================================================================
def _float_id(p):
    return f"{'f32' if p[0] == F32 else 'f16'}-{p[1]}-{p[2]}-k{max(p[3])}"


@pytest.fixture(scope="module", params=W.float_cases(), ids=_float_id)
def float_case(request, oracle):
    dtype, dim, kind, ks = request.param
    rows, pool = W.float_inputs(oracle, W.float_case_seed(dtype, dim, kind), W.FLOAT_N, dim, dtype, W.FLOAT_POOL, kind)
    ref = W.f64_scores_all(rows, pool)
    rows32 = rows if dtype == F32 else rows.astype(np.float32)
    use = W.thin_band_queries(ref, rows32, pool, ks)   # tests/test_wide_cpu.py: there are always FLOAT_NQ of them
    assert len(use) == W.FLOAT_NQ
    c = G.GpuCorpus.from_array(rows)
    c.set_profiling(True)
    yield SimpleNamespace(dtype=dtype, dim=dim, kind=kind, ks=ks, rows=rows, rows32=rows32, q=np.ascontiguousarray(pool[use]),
                          ref={m: ref[m][use] for m in METRICS}, c=c)
    c.close()


def expected_float_kernel(dtype, dim, metric, nq, k):
    """The kernel a search on scan path 0 runs, DESIGN.md section 5 "Dimension switches" restated: the route (K1 or batched)
    from the route self-test; on the batched route the int8 shadow selects up to dimension 8192 (its re-scoring keeps the
    query and 8192 candidates in 64 KiB of LDS), the f16 shadow of Float32 rows up to 12288 (query + 4096 candidates), and
    beyond only the exact f32 MFMA kernel is left, which serves Float32 InnerProduct / Cosine up to dimension 16384: its keys
    are final, and on wider rows its one long chain per sum does not hold the tolerance on one-signed data (this group
    measured 0.90-1.006 of it at 38656 on the non-negative rows, against K1's 0.02), so K1 serves every batch there."""
    if _route(W.FLOAT_N, dim, dtype, metric, nq, k) == 0:
        return K1_STORED
    if dim <= 8192:
        return K2_I8_SHADOW
    if dtype == F32:
        return K2_F16_SHADOW if dim <= 12288 else K2_F32   # (beyond 16384 the route self-test has already answered K1)
    return K2_STORED


def test_d_expected_kernels_at_the_switches():
    """The table the cases below are held to, for 40 queries: on / off at each switch (no GPU work; the searches assert it)."""
    dims = (8192, 8200, 12288, 12296, 16384, 16392, 33000)
    table = {dim: [expected_float_kernel(dt, dim, m, 40, 10) for dt in (F32, F16) for m in METRICS] for dim in dims}
    assert table[8192] == [6, 6, 6, 6, 6, 6]
    assert table[8200] == table[12288] == [4, 4, 4, 3, 3, 3]
    assert table[12296] == table[16384] == [1, 2, 2, 1, 1, 1]  # L2 and every Float16 batch arrive at K1, Float32 dot / cosine at kernel 2
    assert table[16392] == table[33000] == [1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("metric", METRICS)
def test_d_wide_float_topk_against_float64(float_case, metric):
    s = float_case
    s.c.set_scan_path(0)
    for k in s.ks:
        for nq in W.FLOAT_BATCHES:
            res = s.c.search(s.q[:nq], k, metric)
            t = s.c.last_timing()
            tag = f"dtype {s.dtype} dim {s.dim} {s.kind} metric {metric} nq {nq} k {k}"
            want_kernel = expected_float_kernel(s.dtype, s.dim, metric, nq, k)
            assert t.scan_kernel == want_kernel, f"{tag}: kernel {t.scan_kernel}, expected {want_kernel}"
            if want_kernel != K1_STORED:
                assert t.repaired_queries == 0, f"{tag}: {t.repaired_queries} queries were answered by the repair pass"
            for qi in range(nq):
                try:
                    assert_float_topk(metric, res.scores[qi], res.indices[qi], s.ref[metric][qi], s.rows32, s.q[qi], k)
                except AssertionError as e:
                    raise AssertionError(f"{tag} query {qi}: {e}") from None


F_CASES = [p for p in W.float_cases() if p[1] in (12296, 33000)]


@pytest.fixture(scope="module", params=F_CASES, ids=_float_id)
def identity_case(request, oracle):
    dtype, dim, kind, _ = request.param
    rows, q = W.float_inputs(oracle, W.float_case_seed(dtype, dim, kind), W.FLOAT_N, dim, dtype, 16, kind)
    c = G.GpuCorpus.from_array(rows)
    c.set_profiling(True)
    yield SimpleNamespace(dtype=dtype, dim=dim, rows=rows, q=q, c=c)
    c.close()


@pytest.mark.parametrize("metric", METRICS)
def test_f_bit_identity_contracts_at_wide_dimensions(identity_case, metric):
    """candidate search and the streaming radius search report K1's one-query bits; no reference
    needed.  Both dimensions lie above the 150-KiB rule (two to four queries run as one-query passes), so a call of
    several queries equals the same queries one at a time bit for bit."""
    s, k = identity_case, 100
    assert not W.k1_four_query_pass(s.dtype, s.dim, k)
    s.c.set_scan_path(1)
    one = [s.c.search(s.q[qi], k, metric) for qi in range(4)]
    assert s.c.last_timing().scan_kernel == K1_STORED
    for nq in (2, 3, 4):
        many = s.c.search(s.q[:nq], k, metric)
        for qi in range(nq):
            _same(G.SearchResult(many.scores[qi:qi + 1], many.indices[qi:qi + 1], many.raw[qi:qi + 1]), one[qi], f"{nq} queries in one call, query {qi}")
    every = np.arange(W.FLOAT_N, dtype=np.uint64)[None, :]
    for qi in range(2):
        got = s.c.search_candidates(s.q[qi], one[qi].indices, k, metric)          # (i) the rows the search returned
        _same(got, one[qi], "candidates = the search's rows")
        assert int(got.counts[0]) == k
        got = s.c.search_candidates(s.q[qi], every, k, metric)                    # (ii) every row
        _same(got, one[qi], "candidates = every row")
        # the streaming radius search at the search's k-th score: the same rows, the same bits (rows that tie with the
        # k-th beyond rank k only raise the count)
        rad = s.c.search_radius(s.q[qi], float(one[qi].scores[0, k - 1]), k, metric)
        assert int(rad.counts[0]) >= k
        assert (rad.indices == one[qi].indices).all() and (rad.scores.view(np.uint32) == one[qi].scores.view(np.uint32)).all()
    s.c.set_scan_path(0)


@pytest.mark.parametrize("dim", [12288, 12296, 20000])
@pytest.mark.parametrize("metric", METRICS)
def test_f_batched_radius_route_equals_the_streaming_route(oracle, dim, metric):
    """Float32, 16 queries: scan path 0 takes the batched radius route (one thresholded pass of the exact f32 MFMA kernel,
    candidates re-scored with K1's one-query arithmetic), scan path 1 the streaming radius kernel, which above the 150-KiB
    rule also runs one query per pass: the same counts, rows and score bits."""
    assert G.radius_route(F32, 16, 0) == 1 and G.radius_route(F32, 16, 1) == 0 and not W.k1_four_query_pass(F32, dim, 100)
    n = 2000
    rows, q = W.float_inputs(oracle, 0xF00 + dim, n, dim, F32, 16, "planted")
    with G.GpuCorpus.from_array(rows) as c:
        c.set_scan_path(1)
        top = c.search(q, 60, metric)
        radii = top.scores[:, 49].copy()                      # the 50th best of each query: 50 matches, more on a tie
        a = c.search_radius(q, radii, 64, metric)
        c.set_scan_path(0)
        b = c.search_radius(q, radii, 64, metric)
    assert (a.counts >= 50).all()
    assert (a.counts == b.counts).all(), (a.counts, b.counts)
    assert (a.indices == b.indices).all()
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all()
    for qi in range(16):
        m = int(min(a.counts[qi], 60))
        assert (a.indices[qi, :m] == top.indices[qi, :m]).all() and (a.scores[qi, :m].view(np.uint32) == top.scores[qi, :m].view(np.uint32)).all()


# =====================================================================================================================
# E -- one Float32 query over the int8 shadow at its widest
# =====================================================================================================================
@pytest.mark.parametrize("dim,kernel", [(8192, K1_I8_SHADOW), (8200, K1_STORED)])
def test_e_single_query_stream_over_the_int8_shadow_at_its_widest(oracle, dim, kernel):
    """>= 512 MiB of Float32 rows, one query, scan path 0: at dimension 8192 (the longest row whose re-scoring fits) K1
    streams the int8 shadow and re-scores with K1's arithmetic -- indices and score bits of scan path 1; eight dimensions
    on, the stored rows are read.

    The route is pinned at k = 10.  At k = 100 the answer is held to the same bits, the kernel is not: from ~6000
    dimensions on the int8 bound's margin (it grows with the dimension, the scores' spread with its square root) outgrows
    the stream's 2048 candidate slots, InnerProduct / Cosine queries are flagged and redone by K1 -- the
    same bits -- and after five such queries the handle's feedback switches the int8 selection off (measured: every
    query repaired at 8192 and 4 of 5 at 6144, none at 4096 or at k = 10)."""
    n = 16_400
    assert G.stream_rows(n, dim, F32, COS, 1, 10) == G.stream_rows(n, dim, F32, L2, 1, 100) == (1 if kernel == K1_I8_SHADOW else 0)
    rows = oracle.synth_rows(0xE0 + dim, 0, n, dim, F32)
    q = oracle.synth_queries(0xE1 + dim, 3, dim, F32)
    ref = W.f64_scores_all(rows, q[2:3])
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        for k in (10, 100):
            for metric in METRICS:
                for qi in range(3):
                    c.set_scan_path(0)
                    got = c.search(q[qi], k, metric)
                    ran = c.last_timing().scan_kernel
                    assert ran == kernel if k == 10 else ran in (kernel, K1_STORED), (k, metric, qi, ran)
                    c.set_scan_path(1)
                    want = c.search(q[qi], k, metric)
                    assert c.last_timing().scan_kernel == K1_STORED
                    _same(got, want, f"dim {dim} metric {metric} k {k} query {qi}: scan path 0 against scan path 1")
                assert_float_topk(metric, got.scores[0], got.indices[0], ref[metric][0], rows, q[2], k)  # and it is the right answer


# =====================================================================================================================
# G -- the refusal
# =====================================================================================================================
TOO_LARGE = "dimension too large"


def _ordinary_handle_still_searches(oracle):
    rows = oracle.synth_rows(91, 0, 2000, 128, F32)
    q = oracle.synth_queries(92, 3, 128, F32)
    with G.GpuCorpus.from_array(rows) as c:
        res = c.search(q, 10, G.L2)
    osc, oidx, _ = oracle.search(rows, F32, L2, q, 10)
    assert (res.indices == oidx).all() and np.allclose(res.scores, osc, rtol=1e-5, atol=0)


def test_g_restated_limits():
    """One dimension past a limit = the next row length that needs another 16-byte step per lane (J of choose_group)."""
    assert W.k1_lds_bytes(F32, W.k1_max_dim(F32, 10) + 1, 1, 10) > W.K1_MAX_LDS >= W.k1_lds_bytes(F32, W.k1_max_dim(F32, 10), 1, 10)
    assert W.k1_max_dim(F32, 1000) < W.k1_max_dim(F32, 10) and W.k1_max_dim(F16, 10) < W.radius_max_dim(F16)
    assert W.radius_max_dim(F32) == 40704 and W.radius_max_dim(F16) == 40448


def test_g_float32_past_the_k1_limit_is_refused_cleanly(oracle):
    dim, n = W.k1_max_dim(F32, 10) + 1, 600
    rows, q = W.float_inputs(oracle, 0x61, n, dim, F32, 40, "synthetic")
    ref = W.f64_scores_all(rows, q[:2])
    with G.GpuCorpus.from_array(rows) as c:
        for _ in range(2):
            with pytest.raises(E.BuildError, match=TOO_LARGE):
                c.search(q[0], 10, G.L2)                        # one query: K1
            with pytest.raises(E.BuildError, match=TOO_LARGE):
                c.search(q[:3], 10, G.COSINE)
            with pytest.raises(E.BuildError, match=TOO_LARGE):
                c.search(q, 10, G.INNER_PRODUCT)                # 40 queries: the batched route, whose repair pass is K1
            # nothing is left behind: the handle still reads its rows and re-ranks candidates -- correctly
            assert (c.read_rows(n - 3, 3).view(np.uint32) == rows[n - 3:].view(np.uint32)).all()
            every = np.arange(n, dtype=np.uint64)[None, :]
            for metric in METRICS:
                got = c.search_candidates(q[1], every, 10, metric)
                assert_float_topk(metric, got.scores[0], got.indices[0], ref[metric][1], rows, q[1], 10)
            # and a radius search in the gap between K1's limit and R1's succeeds while no list overflows
            srt = np.sort(ref[L2][0])
            radius = float(np.float32((srt[19] + srt[20]) / 2))
            rad = c.search_radius(q[0], radius, 64, G.L2)
            assert_float_radius(L2, int(rad.counts[0]), rad.scores[0], rad.indices[0], ref[L2][0], rows, q[0], radius, 64)
    _ordinary_handle_still_searches(oracle)


def test_g_a_larger_k_moves_the_limit(oracle):
    """k = 1000 doubles K1's candidate lists (2048 entries): the limit drops from 38656 to 36608 Float32 dimensions.  One
    dimension past that: k = 10 is served, k = 1000 refused, and the next k = 10 search on the handle is served again."""
    dim, n = W.k1_max_dim(F32, 1000) + 1, 600
    assert dim <= W.k1_max_dim(F32, 10)
    rows, q = W.float_inputs(oracle, 0x62, n, dim, F32, 3, "planted")
    ref = W.f64_scores_all(rows, q)
    with G.GpuCorpus.from_array(rows) as c:
        first = c.search(q, 10, G.L2)
        with pytest.raises(E.BuildError, match=TOO_LARGE):
            c.search(q, 1000, G.L2)
        with pytest.raises(E.BuildError, match=TOO_LARGE):
            c.search(q[0], 513, G.COSINE)
        again = c.search(q, 10, G.L2)
        _same(first, again, "before / after the refusal")
        for qi in range(3):
            assert_float_topk(L2, again.scores[qi], again.indices[qi], ref[L2][qi], rows, q[qi], 10)
        big = c.search(q[0], 512, G.COSINE)                     # the largest k at the higher limit
        assert_float_topk(COS, big.scores[0], big.indices[0], ref[COS][0], rows, q[0], 512)
    _ordinary_handle_still_searches(oracle)


def test_g_radius_search_between_and_past_the_limits(oracle):
    """Float16 rows: K1 refuses from dimension 38401, R1 (no candidate lists in its LDS) from 40449.  In the gap a radius
    search works while no query's matches overflow the device list (8192); one that overflows is finished by a top-k
    search, i.e. by K1, which refuses: the call fails with the same code -- it never returns a partial answer as MVF_OK."""
    dim, n = W.k1_max_dim(F16, 10) + 1, 8300
    assert dim <= W.radius_max_dim(F16)
    rows, q = W.float_inputs(oracle, 0x63, n, dim, F16, 2, "synthetic")
    ref = W.f64_scores_all(rows, q)
    rows32 = rows.astype(np.float32)
    with G.GpuCorpus.from_array(rows) as c:
        with pytest.raises(E.BuildError, match=TOO_LARGE):
            c.search(q[0], 10, G.L2)
        for metric in METRICS:
            srt = np.sort(ref[metric][0]) if metric == L2 else -np.sort(-ref[metric][0])
            radius = float(np.float32((srt[29] + srt[30]) / 2))
            rad = c.search_radius(q, radius, 64, metric)
            assert_float_radius(metric, int(rad.counts[0]), rad.scores[0], rad.indices[0], ref[metric][0], rows32, q[0], radius, 64)
        everything = float("inf")
        counts = c.search_radius(q, everything, 0, G.L2)            # counts only: no list, nothing to overflow
        assert (counts.counts == n).all()
        try:
            res = c.search_radius(q, everything, 10, G.L2)          # 8300 matches > 8192: finished by K1
        except E.BuildError as e:
            assert TOO_LARGE in str(e)
        else:                                                       # served another way: then served correctly
            assert (res.counts == n).all()
            for qi in range(2):
                assert_float_topk(L2, res.scores[qi], res.indices[qi], ref[L2][qi], rows32, q[qi], 10)
        again = c.search_radius(q, everything, 0, G.L2)             # no device error is left behind
        assert (again.counts == n).all()
    del rows32
    dim = W.radius_max_dim(F16) + 1
    rows = oracle.synth_rows(0x64, 0, 300, dim, F16)
    q = oracle.synth_queries(0x65, 2, dim, F16)
    with G.GpuCorpus.from_array(rows) as c:
        for m in (0, 10):
            with pytest.raises(E.BuildError, match=TOO_LARGE):
                c.search_radius(q, 1.0, m, G.COSINE)
        assert (c.read_rows(0, 2).view(np.uint16) == rows[:2].view(np.uint16)).all()
    _ordinary_handle_still_searches(oracle)
