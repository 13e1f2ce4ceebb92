"""ONE Float32 query over the 6-bit shadow held in the 5+1 LAYOUT (csrc/shadow_5p1.h; scan path 7 forces the route): five bits
of every row are read, the sixth only of the rows that can still reach the margin of the k-th best.  Whatever the rows hold, the
answer is K1's on the stored rows and the 6-bit layout's -- identical indices, raw values and score bits -- and the counter of
low-plane lines shows that the skip path ran."""
import os
import sys

import numpy as np
import pytest

import _stream_5p1 as S
from _children import RUNNER
from metrovector_amd import gpu as G

L2, IP, COS = S.L2, S.IP, S.COS


@pytest.fixture(autouse=True)
def _five_plus_one(monkeypatch):
    monkeypatch.setenv("MVF_STREAM_5P1", "1")  # read when a handle is created


def _same(a, b, what):
    assert (a.indices == b.indices).all(), f"{what}: indices differ"
    assert (a.raw == b.raw).all(), f"{what}: raw values differ"
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), f"{what}: score bits differ"


def _both(c, q, k, metric):
    """the query on the forced 6-bit route (its timing, its low-plane lines) and on K1 over the stored rows"""
    c.set_scan_path(7)
    got = c.search(q, k, metric)
    t, lines = c.last_timing(), c.stream_lo_lines()
    c.set_scan_path(1)
    want = c.search(q, k, metric)
    return got, t, lines, want


def _lines(n, dim):
    """128-byte lines of the low-bit planes that hold rows: eight rows' 16 bytes per 128-element unit"""
    return (n + 7) // 8 * ((dim + 127) // 128)


@pytest.fixture(scope="module")
def six_bit_layout(tmp_path_factory):
    """the grid answered from the 6-bit layout, by a fresh process under MVF_STREAM_5P1=0"""
    path = str(tmp_path_factory.mktemp("s51") / "six.npz")
    env = dict(os.environ, MVF_STREAM_5P1="0")
    out = RUNNER.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_stream_5p1.py"), path], env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    return np.load(path)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", S.DIMS)
def test_identical_to_k1_and_to_the_6_bit_layout(oracle, six_bit_layout, dim):
    rows, q = S.rows_of(oracle, dim), S.query_of(oracle, dim)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        got = S.grid(c, q)
        c.set_scan_path(1)
        for (metric, k), (res, t, (fetched, total)) in got.items():
            what = f"dim {dim} metric {metric} k {k}"
            _same(res, c.search(q, k, metric), what)
            assert t.scan_kernel == 7 and t.repaired_queries == 0 and t.search_launches == 6, what
            assert t.scan_bytes == G.shadow6_bytes(S.N, dim), what
            print(f"{what}: {fetched} of {total} low-plane lines")
            if not S.eligible(dim):
                assert (fetched, total) == (0, 0), what  # the 6-bit layout
                continue
            assert (res.indices == six_bit_layout[f"{dim}/{metric}/{k}/i"]).all(), what
            assert (res.raw == six_bit_layout[f"{dim}/{metric}/{k}/r"]).all(), what
            assert (res.scores.view(np.uint32) == six_bit_layout[f"{dim}/{metric}/{k}/s"]).all(), what
            assert total == _lines(S.N, dim), what
            if k <= 10:   # about 40 blocks publish a best each: there is a k-th best of them
                assert fetched < total, what
            else:         # fewer blocks than k: no threshold, every row's low bit is read
                assert fetched == total, what
        assert c.info().shadows & 8


@pytest.mark.gpu
def test_more_blocks_than_k(oracle):
    n, dim, k = 300_001, 128, 100
    rows, q = S.rows_of(oracle, dim, n), S.query_of(oracle, dim)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        for metric in (L2, IP, COS):
            got, t, (fetched, total), want = _both(c, q, k, metric)
            print(f"metric {metric}: {fetched} of {total} low-plane lines")
            assert t.scan_kernel == 7 and t.repaired_queries == 0
            _same(got, want, f"metric {metric}")
            assert total == _lines(n, dim) and fetched < total


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["one_block", "block_ends"])
def test_the_best_rows_in_awkward_places(oracle, where):
    """the k best rows all inside one block's range (every other block publishes a poor best: a weak but valid bound), and the
    best rows as the last rows of every block's range (each block's best arrives behind everything it could have skipped)"""
    dim, k = 200, 100
    rows, q = S.rows_of(oracle, dim).copy(), S.query_of(oracle, dim)
    rng = np.random.default_rng(3)
    if where == "one_block":
        at = 5 * 1024 + 200 + np.arange(k)
    else:
        at = np.concatenate([np.arange(1023, S.N, 1024), np.arange(1022, S.N, 1024), np.arange(511, S.N, 1024)])
    rows[at] = q[0][None, :] * rng.uniform(0.9, 1.1, (len(at), 1)).astype(np.float32) + rng.standard_normal((len(at), dim)).astype(np.float32) * 0.05
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        for metric in (L2, IP, COS):
            for kk in (10, k):
                got, t, (fetched, total), want = _both(c, q, kk, metric)
                assert t.scan_kernel == 7 and total > 0
                _same(got, want, f"{where} metric {metric} k {kk}")
                if where == "one_block" or metric != L2:
                    assert np.isin(got.indices[0].astype(np.int64), at).all()


@pytest.mark.gpu
def test_every_row_identical(oracle):
    """every row ties: the margin overflows and K1 redoes the query, as on the 6-bit layout"""
    dim = 128
    rows = np.repeat(S.rows_of(oracle, dim, 1), S.N, 0)
    q = S.query_of(oracle, dim)
    for metric in (L2, IP, COS):  # (a handle each: a handle whose queries keep being repaired goes back to its int8 shadow)
        with G.GpuCorpus.from_array(rows) as c:
            c.set_profiling(True)
            got, t, (fetched, total), want = _both(c, q, 10, metric)
            assert t.scan_kernel == 7 and t.repaired_queries == 1 and total > 0
            _same(got, want, f"metric {metric}")


@pytest.mark.gpu
def test_deleted_rows_hold_the_best_scores(oracle):
    dim = 200
    rows, q = S.rows_of(oracle, dim), S.query_of(oracle, dim)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        c.set_scan_path(1)
        dead = np.zeros(S.N, bool)
        for metric in (L2, IP, COS):
            dead[c.search(q, 204, metric).indices[0].astype(np.int64)] = True  # the best 204 under every metric
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        for metric in (L2, IP, COS):
            for k in (10, 100):
                got, t, (fetched, total), want = _both(c, q, k, metric)
                assert t.scan_kernel == 7 and total > 0
                assert not dead[got.indices[0].astype(np.int64)].any()
                _same(got, want, f"metric {metric} k {k} under a deletion mask")


@pytest.mark.gpu
def test_two_queries_in_a_row_on_one_handle(oracle):
    """the published bests of one search mean nothing to the next: the second query's best rows score poorly for the first"""
    dim, k = 768, 10
    rows = S.rows_of(oracle, dim)
    q = oracle.synth_queries(S.SEED + 7, 2, dim, S.F32).copy()
    q[1] = -q[0]
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        c.set_scan_path(1)
        want = [c.search(q[i:i + 1], k, metric) for i in range(2) for metric in (L2, IP, COS)]
        c.set_scan_path(7)
        got = []
        for i in range(2):
            for metric in (L2, IP, COS):
                got.append(c.search(q[i:i + 1], k, metric))
                fetched, total = c.stream_lo_lines()
                assert c.last_timing().scan_kernel == 7 and 0 < fetched < total
        for g, w in zip(got, want):
            _same(g, w, "alternating queries")


@pytest.mark.gpu
def test_dim_129_stays_on_the_6_bit_layout(oracle, six_bit_layout):
    dim = S.OLD_LAYOUT_DIM
    rows, q = S.rows_of(oracle, dim), S.query_of(oracle, dim)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        for (metric, k), (res, t, lines) in S.grid(c, q).items():
            assert t.scan_kernel == 7 and lines == (0, 0)
            assert t.scan_bytes == G.shadow6_bytes(S.N, dim) < G.shadow51_bytes(S.N, dim)
            assert (res.indices == six_bit_layout[f"{dim}/{metric}/{k}/i"]).all()
            assert (res.scores.view(np.uint32) == six_bit_layout[f"{dim}/{metric}/{k}/s"]).all()
        assert c.info().device_bytes == int(six_bit_layout[f"{dim}/bytes"][0])


@pytest.mark.gpu
def test_a_non_finite_row_is_refused(oracle):
    dim = 200
    rows = S.rows_of(oracle, dim).copy()
    rows[31_007, 5] = np.inf
    q = S.query_of(oracle, dim)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        for _ in range(2):
            got, t, lines, want = _both(c, q, 10, IP)
            assert t.scan_kernel == 1 and t.scan_bytes == S.N * dim * 4 and lines == (0, 0)
            _same(got, want, "a row holding Inf")
