"""ONE Float32 query over the 6-bit shadow (scan path 7 forces the route at any size; scan path 0 takes it from 4 GiB of rows
where the shape rule holds): whatever the dimension, k, metric or the handle's history, the answer is K1's on the stored rows
-- identical indices, raw values and score bits -- and the timing shows which rows the scan read."""
import itertools

import numpy as np
import pytest

from metrovector_amd import gpu as G

SEED = 0x4D564631
L2, IP, COS = 0, 1, 2
F32 = 0
N = 40_001  # not a multiple of the 64-row tile
KS = (1, 10, 100, 204)


def _same(a, b, what):
    assert (a.indices == b.indices).all(), f"{what}: indices differ"
    assert (a.raw == b.raw).all(), f"{what}: raw values differ"
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), f"{what}: score bits differ"


def _both(c, q, k, metric):
    """the query on the forced 6-bit route (with its timing) and on K1 over the stored rows"""
    c.set_scan_path(7)
    got = c.search(q, k, metric)
    t = c.last_timing()
    c.set_scan_path(1)
    want = c.search(q, k, metric)
    return got, t, want


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 13, 64, 65, 100, 192, 200, 768, 1000])
def test_identical_to_k1_at_every_dimension_k_and_metric(oracle, dim):
    rows = np.ascontiguousarray(oracle.synth_rows(SEED, 0, N, dim, F32))
    q = oracle.synth_queries(SEED + 1, 2, dim, F32).copy()
    stored = rows[N - 2:N - 1].copy()  # a stored row of the last, partial tile
    zero = np.zeros((1, dim), np.float32)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        for metric in (L2, IP, COS):
            for k in KS:
                for i in range(2):
                    got, t, want = _both(c, q[i:i + 1], k, metric)
                    what = f"dim {dim} metric {metric} k {k} query {i}"
                    assert t.scan_kernel == 7, what
                    assert t.scan_bytes == G.shadow6_bytes(N, dim), what
                    assert t.repaired_queries == 0, what
                    assert t.search_launches == 6, what
                    _same(got, want, what)
                got, t, want = _both(c, stored, k, metric)
                assert t.scan_kernel == 7 and t.scan_bytes == G.shadow6_bytes(N, dim)
                _same(got, want, f"dim {dim} metric {metric} k {k}: a stored row as the query")
            # (once per metric: under InnerProduct and Cosine every row ties, the query is flagged and K1 redoes it -- more than
            # one repaired search in eight would send the handle back to its int8 shadow)
            got, t, want = _both(c, zero, 10, metric)
            assert t.scan_kernel == 7 and t.scan_bytes == G.shadow6_bytes(N, dim)
            _same(got, want, f"dim {dim} metric {metric}: the zero query")
        info = c.info()
        assert info.shadows & 8 and not info.shadows & 1, "the 6-bit shadow is built from the stored rows alone"
        assert info.selection_state == 0


@pytest.mark.gpu
def test_five_rows(oracle):
    rows = np.ascontiguousarray(oracle.synth_rows(SEED, 0, 5, 64, F32))
    q = oracle.synth_queries(SEED + 2, 1, 64, F32)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        for metric in (L2, IP, COS):
            for k in (1, 10):
                got, t, want = _both(c, q, k, metric)
                assert t.scan_kernel == 7 and t.scan_bytes == G.shadow6_bytes(5, 64) == 3072
                _same(got, want, f"metric {metric} k {k}")


@pytest.mark.gpu
def test_an_overflowing_corpus_is_answered_by_k1_and_goes_back_to_the_int8_shadow(oracle):
    """test_gpu_stream_fixed_cost.py's dense cluster of near-duplicates: every query is flagged and redone by K1; the counts
    reach the host two searches late, and after four of them the handle streams its int8 shadow instead -- never the stored
    rows, and the int8 selection's own switch stays untouched."""
    n, dim = 40_000, 64
    rng = np.random.default_rng(11)
    base = rng.standard_normal(dim).astype(np.float32)
    rows = (base[None, :] + rng.standard_normal((n, dim)).astype(np.float32) * 1e-4).astype(np.float32)
    rows[::97] = base  # exact duplicates: ties
    q = np.stack([base + rng.standard_normal(dim).astype(np.float32) * 1e-3 for _ in range(10)]).astype(np.float32)
    got, kernels, nbytes, repaired = [], [], [], []
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        c.set_scan_path(7)
        for i in range(10):
            got.append(c.search(q[i:i + 1], 20, COS))
            t = c.last_timing()
            kernels.append(t.scan_kernel)
            nbytes.append(t.scan_bytes)
            repaired.append(t.repaired_queries)
        state = c.info().selection_state
        c.set_scan_path(1)
        for i in range(10):
            _same(got[i], c.search(q[i:i + 1], 20, COS), f"search {i} ({nbytes[i]} bytes scanned)")
    six, eight = G.shadow6_bytes(n, dim), n * dim
    assert all(kn == 7 for kn in kernels), kernels
    assert nbytes[0] == six and nbytes[1] == six and repaired[0] == 1 and repaired[1] == 1, (nbytes, repaired)
    first8 = nbytes.index(eight)
    assert first8 <= 7, nbytes
    assert all(b == six and r == 1 for b, r in zip(nbytes[:first8], repaired[:first8])), (nbytes, repaired)
    assert all(b == eight for b in nbytes[first8:]), nbytes
    assert state & 4 and not state & 1, state


@pytest.mark.gpu
def test_a_non_finite_row_sends_the_query_to_the_stored_rows(oracle):
    rows = np.ascontiguousarray(oracle.synth_rows(SEED, 0, N, 192, F32)).copy()
    rows[31_007, 5] = np.inf
    q = oracle.synth_queries(SEED + 3, 1, 192, F32)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        for _ in range(2):
            got, t, want = _both(c, q, 10, IP)
            assert t.scan_kernel == 1 and t.scan_bytes == N * 192 * 4
            _same(got, want, "a row holding Inf")


@pytest.mark.gpu
def test_deleted_rows_are_honoured(oracle):
    rows = np.ascontiguousarray(oracle.synth_rows(SEED, 0, N, 192, F32))
    q = oracle.synth_queries(SEED + 4, 1, 192, F32)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        c.set_scan_path(1)
        best = c.search(q, 100, COS).indices[0].astype(np.int64)
        dead = np.zeros(N, bool)
        dead[best[::2]] = True  # half of the answer, and a third of everything else
        dead[::3] = True
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        for metric in (L2, IP, COS):
            got, t, want = _both(c, q, 100, metric)
            assert t.scan_kernel == 7 and t.scan_bytes == G.shadow6_bytes(N, 192)
            assert not dead[got.indices[0].astype(np.int64)].any()
            _same(got, want, f"metric {metric} under a deletion mask")


@pytest.mark.gpu
def test_the_answer_does_not_depend_on_the_handles_history(oracle):
    """An int8-route search, a batched search and a 6-bit search on one handle, in every order: each gives the bits it gives
    on a fresh handle (they share the candidate lists, the per-query state and the repair buffers)."""
    rows = np.ascontiguousarray(oracle.synth_rows(SEED, 0, N, 192, F32))
    q = oracle.synth_queries(SEED + 5, 16, 192, F32)
    k = 50
    steps = {"int8": (6, q[:1]), "batched": (5, q), "6bit": (7, q[:1])}
    seen = {}
    for order in itertools.permutations(steps):
        with G.GpuCorpus.from_array(rows) as c:
            c.set_profiling(True)
            for name in order:
                path, qs = steps[name]
                c.set_scan_path(path)
                res = c.search(qs, k, COS)
                if name == "6bit":
                    t = c.last_timing()
                    assert t.scan_kernel == 7 and t.scan_bytes == G.shadow6_bytes(N, 192) and t.repaired_queries == 0, order
                if name in seen:
                    _same(res, seen[name], f"{name} in order {order}")
                seen[name] = res
            c.set_scan_path(1)
            _same(seen["6bit"], c.search(q[:1], k, COS), f"6-bit route in order {order}")
            _same(seen["int8"], c.search(q[:1], k, COS), f"int8 route in order {order}")
