"""One Float32 query streams the int8 shadow by default from 512 MiB of rows (scan path 0), and the streamed shadow -- by
default or on scan path 6 -- returns K1's bits: the candidates are re-scored with K1's arithmetic at K1's one-query lane
width, and a flagged query is redone by K1 at that width.  "Identical" below means identical indices, raw values and
score bits."""
import numpy as np
import pytest

from metrovector_amd import gpu as G

SEED = 0x4D564631
L2, IP, COS = 0, 1, 2
F32, F16, I8 = 0, 1, 2
STREAM_I8_MIN_BYTES = 512 << 20  # api.hip kStreamI8MinBytes
STREAM_MAX_K = 204             # api.hip kQsStreamMaxK

STORED, SHADOW = 0, 1


def _same(a, b, what):
    assert (a.indices == b.indices).all(), f"{what}: indices differ"
    assert (a.raw == b.raw).all(), f"{what}: raw values differ"
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), f"{what}: score bits differ"


# ---- CPU tier: the shape part of the rule ------------------------------------------------------------------------------

def test_the_rows_a_single_query_reads_are_a_function_of_its_shape():
    rows_at = STREAM_I8_MIN_BYTES // (256 * 4)  # 256-dim f32 rows: 1 KiB each
    assert G.stream_rows(rows_at, 256, F32, COS, 1, 100) == SHADOW
    assert G.stream_rows(rows_at - 1, 256, F32, COS, 1, 100) == STORED
    assert G.stream_rows(10_000_000, 768, F32, COS, 1, 100) == SHADOW          # the headline
    for metric in (L2, IP, COS):
        assert G.stream_rows(10_000_000, 768, F32, metric, 1, 100) == SHADOW
    assert G.stream_rows(10_000_000, 768, F32, COS, 1, STREAM_MAX_K) == SHADOW
    assert G.stream_rows(10_000_000, 768, F32, COS, 1, STREAM_MAX_K + 1) == STORED
    assert G.stream_rows(10_000_000, 768, F32, COS, 1, 1) == SHADOW
    assert G.stream_rows(10_000_000, 768, F32, COS, 2, 100) == STORED          # two queries and more: other routes
    assert G.stream_rows(10_000_000, 768, F16, COS, 1, 100) == STORED          # Float16 rows: stored rows by default
    assert G.stream_rows(10_000_000, 768, I8, IP, 1, 100) == STORED
    assert G.stream_rows(1_000_000, 8192, F32, COS, 1, 10) == SHADOW           # the longest row the re-scoring takes
    assert G.stream_rows(1_000_000, 8200, F32, COS, 1, 10) == STORED
    # the route itself is unchanged: K1 either way (over the shadow or the stored rows)
    route = G._lib.gpu().mvfgpu_selftest_route
    import ctypes as C
    out = C.c_uint32(9)
    G._lib.gpu_check(route(10_000_000, 768, F32, COS, 1, 100, C.byref(out)))
    assert out.value == 0


# ---- GPU tier ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def headline():
    c = G.GpuCorpus.synthetic(10_000_000, 768, F32, SEED)
    yield c
    c.close()


def _headline_queries(oracle, nq=64):
    q = oracle.synth_queries(SEED + 1, nq, 768, F32).copy()
    q[0] = oracle.synth_rows(SEED, 4_321_987, 1, 768, F32)[0]  # a stored row
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_headline_default_route_is_bit_identical_to_k1(oracle, headline, metric):
    c = headline
    q = _headline_queries(oracle)
    if metric == COS:
        q[1] = 0.0  # a zero query: every score 0
    c.set_profiling(True)
    try:
        for k in (1, 100, STREAM_MAX_K):
            for i in range(q.shape[0]):
                c.set_scan_path(0)
                got = c.search(q[i:i + 1], k, metric)
                assert c.last_timing().scan_kernel == 7
                c.set_scan_path(1)
                want = c.search(q[i:i + 1], k, metric)
                assert c.last_timing().scan_kernel == 1
                _same(got, want, f"metric {metric} k {k} query {i}")
        c.set_scan_path(0)
        c.search(q[:1], STREAM_MAX_K + 1, metric)
        assert c.last_timing().scan_kernel == 1  # beyond the stream's margin budget: the stored rows
    finally:
        c.set_scan_path(0)
        c.set_profiling(False)


@pytest.mark.gpu
def test_headline_answer_does_not_depend_on_the_handles_history(oracle, headline, monkeypatch):
    c = headline
    q = _headline_queries(oracle, 1024)
    before = [c.search(q[i:i + 1], 100, COS) for i in (0, 5, 17)]
    c.search(q, 100, COS)  # a batched search on the same handle
    after = [c.search(q[i:i + 1], 100, COS) for i in (0, 5, 17)]
    monkeypatch.setenv("MVF_STREAM_I8", "0")
    c.reload_tuning()
    try:
        c.set_profiling(True)
        off = [c.search(q[i:i + 1], 100, COS) for i in (0, 5, 17)]
        assert c.last_timing().scan_kernel == 1
        c.set_profiling(False)
    finally:
        monkeypatch.delenv("MVF_STREAM_I8")
        c.reload_tuning()
    for a, b, o in zip(before, after, off):
        _same(a, b, "before / after a batched search")
        _same(a, o, "default / MVF_STREAM_I8=0")


def _rows(oracle, n, dim, seed=SEED):
    return np.ascontiguousarray(oracle.synth_rows(seed, 0, n, dim, F32))


def _path6_vs_path1(rows, q, ks, metrics, setup=None):
    for metric in metrics:
        with G.GpuCorpus.from_array(rows) as c:
            if setup:
                setup(c)
            c.set_profiling(True)
            for k in ks:
                for i in range(q.shape[0]):
                    c.set_scan_path(6)
                    got = c.search(q[i:i + 1], k, metric)
                    assert c.last_timing().scan_kernel in (7, 1)
                    c.set_scan_path(1)
                    want = c.search(q[i:i + 1], k, metric)
                    _same(got, want, f"dim {rows.shape[1]} metric {metric} k {k} query {i}")


# dims whose one-query lane width (api.hip choose_group) is 1, 4, 8, 16, 32 and 64
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 13, 30, 128, 100, 200])
def test_streamed_shadow_is_bit_identical_to_k1_at_every_lane_width(oracle, dim):
    n = 40_000
    rows = _rows(oracle, n, dim)
    q = oracle.synth_queries(SEED + 2, 6, dim, F32).copy()
    q[0] = rows[1234]
    _path6_vs_path1(rows, q, (10, 100), (L2, IP, COS))


@pytest.mark.gpu
def test_streamed_shadow_is_bit_identical_with_ids_and_tombstones(oracle):
    n, dim = 50_000, 128
    rows = _rows(oracle, n, dim)
    q = oracle.synth_queries(SEED + 3, 6, dim, F32)
    dead = np.zeros(n, bool)
    dead[::7] = True
    ids = (np.arange(n, dtype=np.uint64) * 3 + 1000)

    def setup(c):
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        c.set_vector_ids(ids)
    _path6_vs_path1(rows, q, (20,), (L2, IP, COS), setup)


@pytest.mark.gpu
def test_streamed_shadow_is_bit_identical_with_non_finite_rows(oracle):
    n, dim = 30_000, 100
    rows = _rows(oracle, n, dim)
    rows[17, 3] = np.inf
    rows[23, 0] = np.nan
    q = oracle.synth_queries(SEED + 4, 4, dim, F32)
    _path6_vs_path1(rows, q, (10,), (L2, IP, COS))


@pytest.mark.gpu
def test_streamed_shadow_is_bit_identical_when_queries_are_repaired(oracle):
    """A dense cluster of near-duplicates: every row is inside the int8 bound, the margin overflows, K1 redoes the query."""
    n, dim = 40_000, 64
    rng = np.random.default_rng(11)
    base = rng.standard_normal(dim).astype(np.float32)
    rows = (base[None, :] + rng.standard_normal((n, dim)).astype(np.float32) * 1e-4).astype(np.float32)
    rows[::97] = base  # exact duplicates: ties
    q = np.stack([base + rng.standard_normal(dim).astype(np.float32) * 1e-3 for _ in range(4)]).astype(np.float32)
    _path6_vs_path1(rows, q, (10, 100), (L2, IP, COS))


@pytest.mark.gpu
def test_default_route_needs_a_whole_finite_shadow(oracle):
    """Below 512 MiB path 0 reads the stored rows; a corpus with an Inf row goes to the stored rows even when large."""
    n, dim = 400_000, 768  # 1.2 GB of rows
    rows = _rows(oracle, n, dim)
    q = oracle.synth_queries(SEED + 5, 2, dim, F32)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        got = c.search(q[:1], 50, COS)
        assert c.last_timing().scan_kernel == 7
        c.set_scan_path(1)
        _same(got, c.search(q[:1], 50, COS), "1.2 GB corpus")
    rows[99, 5] = np.inf
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        c.search(q[:1], 50, COS)  # builds the shadow; its maxima are +inf
        got = c.search(q[1:2], 50, COS)
        assert c.last_timing().scan_kernel == 1
    with G.GpuCorpus.from_array(rows[:170_000].copy()) as c:  # 522 MB < 512 MiB
        c.set_profiling(True)
        c.search(q[:1], 50, COS)
        assert c.last_timing().scan_kernel == 1
