"""Filtered search on the GPU (mvfgpu_filter_*, mvfgpu_search_filtered[_device]; DESIGN.md §3 "Filtered search", §5
"F0 / F1 / F2"): the bit geometry of the mask and the list, every route against the oracle over the admitted rows
(tests/_filtered.py) and, bit for bit, against a twin handle whose tombstones are `deleted | ~allow`; large k, short results,
ties, wide rows, the filter's lifecycle, the handle's untouched state, row-range shards and the C++ mirror."""
import os
import subprocess
import threading

import numpy as np
import pytest

from metrovector_amd import errors as E
from metrovector_amd import gpu as G

from _children import RUNNER
from _filtered import PAD, admitted_mask, assert_float_filtered, device_words, mask_patterns, oracle_filtered, shard_bitmap
from _util import assert_exact

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "metrovector_amd")
B = 32768  # rows one block of F0 / F1 covers (scan_filter.h: kFilterBlockRows)
MASK, LIST = 1, 2


def _force(monkeypatch, c, route):
    """MVF_FILTER_ROUTE is read into the handle's tuning; a filter takes it from the handle when it is created."""
    if route is None:
        monkeypatch.delenv("MVF_FILTER_ROUTE", raising=False)
    else:
        monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    c.reload_tuning()


def _same(a, b):
    return (a.indices == b.indices).all() and (a.raw == b.raw).all() and (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all()


# ---- F0 / F1 bit geometry ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 2 * B + 33])
def test_bit_geometry_of_mask_and_list(oracle, monkeypatch, n):
    import torch
    rows = oracle.synth_rows(31, 0, n, 8, 0)
    q = oracle.synth_queries(32, 1, 8, 0)
    dead = np.zeros(n, bool)
    if n > 33:
        dead[np.random.default_rng(n).random(n) < 0.1] = True
        dead[[0, n - 1]] = False
    with G.GpuCorpus.from_array(rows, index_base=3) as c:
        if dead.any():
            c.set_tombstones(np.packbits(dead, bitorder="little"))
        for route in (MASK, LIST):
            _force(monkeypatch, c, route)
            for name, allow in mask_patterns(n, B).items():
                want = np.nonzero(allow & ~dead)[0].astype(np.uint64) + np.uint64(3)
                k = want.size + 5

                def check(f, what):
                    inf = f.info()
                    assert inf.admitted == want.size == f.admitted and inf.rows == n, what
                    assert inf.has_row_list == (1 if route == LIST and want.size else 0), what
                    assert inf.device_bytes >= ((n + 31) // 32 + 1) * 4 + (want.size * 4 if inf.has_row_list else 0), what
                    res = c.search_filtered(q, k, G.L2, f)
                    got = res.indices[0]
                    assert (np.sort(got[:want.size]) == want).all(), f"{what}: the returned rows are not the admitted live rows"
                    assert (got[want.size:] == PAD).all() and np.isinf(res.scores[0][want.size:]).all(), f"{what}: padding"
                    return res

                host = None
                for fb in (0, 1, 7, 31, 32, 37):
                    with c.make_filter(shard_bitmap(allow, fb), first_bit=fb) as f:  # every bit outside the shard's range is 1
                        res = check(f, f"route {route} {name} first_bit {fb}")
                    assert host is None or _same(res, host), "the answer depends on first_bit"
                    host = res
                words = torch.from_numpy(device_words(allow).view(np.int32)).cuda()
                with c.make_filter_device(words.data_ptr()) as f:
                    assert _same(check(f, f"route {route} {name} device form"), host), "device and host form differ"
                with c.make_filter(allow) as f:  # a bool array over the rows
                    assert _same(check(f, f"route {route} {name} bool form"), host)


# ---- every route against the oracle and the twin -----------------------------------------------------------------------

N, DIM, K, BASE, NQ = 20_011, 96, 33, 7, 300
ROUTES = [(MASK, 1, 1), (MASK, 1, 6), (MASK, 2, 40), (MASK, 3, 40), (MASK, 0, 300), (LIST, 0, 1), (LIST, 0, 5), (LIST, 0, 40)]
_CASES = {}


def _case(oracle, dtype, metric):
    """Rows, queries, masks and the oracle's answers of one (dtype, metric): computed once, shared, never changed."""
    hit = _CASES.get((dtype, metric))
    if hit is None:
        rows = oracle.synth_rows(41, 0, N, DIM, dtype)
        q = oracle.synth_queries(42, NQ, DIM, dtype)
        rng = np.random.default_rng(5)
        dead = rng.random(N) < 0.3
        allow = rng.random(N) < 0.4
        allow[4000:4200] = True  # a run across a 4096-row phase boundary
        # none of query 0's unfiltered top-k (among the live rows) is admitted
        live = np.nonzero(~dead)[0]
        allow[live[oracle.search(rows[live], dtype, metric, q[:1], K)[1][0].astype(np.int64)]] = False
        admit = allow & ~dead
        want = oracle_filtered(oracle, rows, dtype, metric, q, K, admit, index_base=BASE)
        hit = _CASES[(dtype, metric)] = (rows, q, dead, allow, admit, want)
    return hit


@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("route,scan_path,nq", ROUTES)
def test_every_route_against_the_oracle_and_the_twin(oracle, monkeypatch, dtype, metric, route, scan_path, nq):
    rows, q, dead, allow, admit, want = _case(oracle, dtype, metric)
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    with G.GpuCorpus.from_array(rows, index_base=BASE) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        c.set_scan_path(scan_path)
        with c.make_filter(np.packbits(allow, bitorder="little")) as f:
            assert f.admitted == int(admit.sum())
            res = c.search_filtered(q[:nq], K, metric, f)
    assert res.indices.shape == (nq, K)
    if dtype in (2, 3):
        assert_exact(res, want[0][:nq], want[1][:nq], want[2][:nq])
        # the definition: mvfgpu_search on a twin handle whose tombstones are dead | ~allow, bit for bit
        with G.GpuCorpus.from_array(rows, index_base=BASE) as twin:
            twin.set_tombstones(np.packbits(dead | ~allow, bitorder="little"))
            twin.set_scan_path(scan_path)
            assert _same(res, twin.search(q[:nq], K, metric))
    else:
        for j in range(nq):
            assert_float_filtered(oracle, rows, dtype, metric, q[j], K, admit, res.scores[j], res.indices[j], index_base=BASE)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_one_float32_query_has_the_twins_scan_path_1_bits_on_both_routes(oracle, monkeypatch, metric):
    rows, q, dead, allow, admit, _ = _case(oracle, 0, metric)
    with G.GpuCorpus.from_array(rows, index_base=BASE) as twin:
        twin.set_tombstones(np.packbits(dead | ~allow, bitorder="little"))
        twin.set_scan_path(1)
        yard = [twin.search(q[j:j + 1], K, metric) for j in range(3)]
    with G.GpuCorpus.from_array(rows, index_base=BASE) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        for route in (MASK, LIST):
            _force(monkeypatch, c, route)
            with c.make_filter(allow) as f:
                for j in range(3):
                    assert _same(c.search_filtered(q[j:j + 1], K, metric, f), yard[j]), f"route {route}, query {j}"
                if route == LIST:  # F2 keeps K1's one-query arithmetic for any number of queries
                    many = c.search_filtered(q[:7], K, metric, f)
                    for j in range(3):
                        assert (many.indices[j] == yard[j].indices[0]).all()
                        assert (many.scores[j].view(np.uint32) == yard[j].scores[0].view(np.uint32)).all()


def test_the_int8_shadow_stream_answers_the_mask_route_with_the_twins_bits(oracle, monkeypatch):
    n, dim, k = 60_000, 128, 20
    rows = oracle.synth_rows(51, 0, n, dim, 0)
    q = oracle.synth_queries(52, 300, dim, 0)
    rng = np.random.default_rng(6)
    dead, allow = rng.random(n) < 0.3, rng.random(n) < 0.4
    with G.GpuCorpus.from_array(rows) as twin:
        twin.set_tombstones(np.packbits(dead | ~allow, bitorder="little"))
        twin.set_scan_path(1)
        yard = twin.search(q[:1], k, G.COSINE)
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(MASK))
    monkeypatch.setenv("MVF_STREAM_I8", "1")  # one query streams the int8 shadow at any size once it exists
    with G.GpuCorpus.from_array(rows) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        c.set_scan_path(5)
        c.search(q, k, G.COSINE)  # builds the shadow
        c.set_scan_path(0)
        c.set_profiling(True)
        with c.make_filter(allow) as f:
            res = c.search_filtered(q[:1], k, G.COSINE, f)
            assert c.last_timing().scan_kernel == 7, "the filtered search did not stream the int8 shadow"
    assert _same(res, yard)


@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
@pytest.mark.parametrize("dim", [7, 100])
def test_the_list_route_and_the_candidate_search_share_their_bits(oracle, monkeypatch, dtype, dim):
    """The gathered-row kernel's two addressings on one handle: one list for groups of queries (the list route under a filter
    that admits every row; five queries: a group of four and a short one) and a list and a count per query (the candidate
    search given every row) write the same bytes."""
    n, nq, k = 2 * 1024 + 33, 5, 10
    rows = oracle.synth_rows(91, 0, n, dim, dtype)
    q = oracle.synth_queries(92, nq, dim, dtype)
    every = np.tile(np.arange(n, dtype=np.uint64), (nq, 1))
    with G.GpuCorpus.from_array(rows) as c:
        _force(monkeypatch, c, LIST)
        with c.make_filter(np.ones(n, bool)) as f:
            assert f.admitted == n and f.info().has_row_list == 1
            for metric in (G.L2, G.COSINE):
                a = c.search_filtered(q, k, metric, f)
                b = c.search_candidates(q, every, k, metric)
                assert (b.counts == n).all()
                assert a.scores.tobytes() == b.scores.tobytes(), f"metric {metric}: scores"
                assert a.indices.tobytes() == b.indices.tobytes(), f"metric {metric}: indices"
                assert a.raw.tobytes() == b.raw.tobytes(), f"metric {metric}: raw"


# ---- large k, short results --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,metric", [(2, G.L2), (0, G.COSINE)])
@pytest.mark.parametrize("route,large_k", [(MASK, 1), (MASK, 2), (LIST, 0)])
def test_k_2048_on_both_routes(oracle, monkeypatch, dtype, metric, route, large_k):
    rows, q, dead, allow, admit, _ = _case(oracle, dtype, metric)
    k, nq = 2048, 3
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    if large_k:
        monkeypatch.setenv("MVF_LARGE_K", str(large_k))
    with G.GpuCorpus.from_array(rows, index_base=BASE) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        with c.make_filter(allow) as f:
            res = c.search_filtered(q[:nq], k, metric, f)
    if dtype == 2:
        assert_exact(res, *oracle_filtered(oracle, rows, dtype, metric, q[:nq], k, admit, index_base=BASE))
    else:
        for j in range(nq):
            assert_float_filtered(oracle, rows, dtype, metric, q[j], k, admit, res.scores[j], res.indices[j], index_base=BASE)


@pytest.mark.parametrize("route", [MASK, LIST])
@pytest.mark.parametrize("nq", [1, 5, 70])
def test_fewer_admitted_rows_than_k_pad(oracle, monkeypatch, route, nq):
    rows, q, dead, _, _, _ = _case(oracle, 2, G.L2)
    allow = np.zeros(N, bool)
    allow[[3, 4095, 4096, N - 1] + list(range(5000, 5040))] = True
    admit = allow & ~dead
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    with G.GpuCorpus.from_array(rows, index_base=BASE) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        with c.make_filter(allow) as f:
            for k in (50, 2048):
                res = c.search_filtered(q[:nq], k, G.L2, f)
                assert_exact(res, *oracle_filtered(oracle, rows, 2, G.L2, q[:nq], k, admit, index_base=BASE))
                assert (res.indices[:, int(admit.sum()):] == PAD).all() and np.isinf(res.scores[:, int(admit.sum()):]).all()
        with c.make_filter(np.zeros(N, bool)) as f:  # nothing admitted: all padding, whatever the route
            assert f.admitted == 0 and f.info().has_row_list == 0
            res = c.search_filtered(q[:nq], 9, G.INNER_PRODUCT, f)
            assert (res.indices == PAD).all() and (res.scores == -np.inf).all() and (res.raw == 0).all()
        with c.make_filter(dead) as f:  # only deleted rows allowed: the same
            assert f.admitted == 0
            assert (c.search_filtered(q[:nq], 9, G.L2, f).indices == PAD).all()


# ---- ties ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", [MASK, LIST])
@pytest.mark.parametrize("with_ids", [False, True])
def test_ties_come_out_in_ascending_position(oracle, monkeypatch, route, with_ids):
    n, dim, k = 12_345, 48, 25
    rows = oracle.synth_rows(61, 0, n, dim, 0).copy()
    rows[100:140] = rows[100]
    allow = np.random.default_rng(7).random(n) < 0.5
    allow[100:140] = False
    tied = [101, 104, 105, 117, 128, 139]
    allow[tied] = True
    ids = (np.arange(n, dtype=np.uint64)[::-1] * 5 + 11).copy()  # descending ids: positions decide, never ids
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    with G.GpuCorpus.from_array(rows, index_base=BASE) as c:
        if with_ids:
            c.set_vector_ids(ids)
        with c.make_filter(allow) as f:
            for q in (rows[100][None, :], np.repeat(rows[100][None, :], 6, axis=0)):
                res = c.search_filtered(q, k, G.L2, f)
                want = ids[tied] if with_ids else np.array(tied, np.uint64) + np.uint64(BASE)
                assert (res.indices[:, :len(tied)] == want[None, :]).all()
                assert (res.scores[:, :len(tied)] == 0).all() and (res.scores[:, len(tied)] > 0).all()


# ---- wide rows ----------------------------------------------------------------------------------------------------------

def test_wide_float32_rows_read_the_query_through_the_cache(oracle, monkeypatch):
    """dim 12 296: one padded query exceeds the LDS budget of F2 (the QLDS = false kernels); both routes, float64 reference"""
    import _wide
    n, dim, k = 600, 12_296, 10
    rows = oracle.synth_rows(71, 0, n, dim, 0)
    q = oracle.synth_queries(72, 5, dim, 0)
    allow = np.random.default_rng(8).random(n) < 0.4
    with G.GpuCorpus.from_array(rows) as c:
        for metric in (G.L2, G.COSINE):
            ref = _wide.f64_scores(rows, q, metric)
            for route in (MASK, LIST):
                _force(monkeypatch, c, route)
                with c.make_filter(allow) as f:
                    res = c.search_filtered(q, k, metric, f)
                for j in range(q.shape[0]):
                    assert_float_filtered(oracle, rows, 0, metric, q[j], k, allow, res.scores[j], res.indices[j], all_scores=ref[j])


def test_widest_int8_rows_on_the_list_route_are_exact(oracle, monkeypatch):
    import _wide
    n, dim, k = 300, 33_025, 12
    rows = oracle.synth_rows(73, 0, n, dim, 2).copy()
    rows[0], rows[1], rows[n - 1] = -128, 127, -128  # saturated rows: the sums reach the i32 bound the dimension limit allows
    planted = [0, 1, n - 1]
    q = _wide.saturated_queries(oracle, 74, 5, dim, 2)
    allow = np.random.default_rng(9).random(n) < 0.5
    allow[planted] = True  # the saturated rows
    dot, qq, xx = _wide.int_raw(rows, q)
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(LIST))
    with G.GpuCorpus.from_array(rows) as c:
        with c.make_filter(allow) as f:
            for metric in (G.L2, G.INNER_PRODUCT, G.COSINE):
                assert_exact(c.search_filtered(q, k, metric, f), *_wide.int_topk(metric, dot, qq, xx, k, dead=~allow))


# ---- lifecycle ----------------------------------------------------------------------------------------------------------

def test_a_stale_or_foreign_filter_is_refused(oracle):
    rows, q, dead, allow, admit, _ = _case(oracle, 2, G.L2)
    with G.GpuCorpus.from_array(rows, index_base=BASE) as c, G.GpuCorpus.from_array(rows[:5000]) as other:
        old = c.make_filter(allow)
        assert old.admitted == int(allow.sum())
        c.search_filtered(q[:2], K, G.L2, old)
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        with pytest.raises(E.InvalidArgument, match="stale filter.*set_tombstones"):
            c.search_filtered(q[:2], K, G.L2, old)
        with c.make_filter(allow) as f:
            assert f.admitted == int(admit.sum())
            assert_exact(c.search_filtered(q[:2], K, G.L2, f), *oracle_filtered(oracle, rows, 2, G.L2, q[:2], K, admit, index_base=BASE))
            with pytest.raises(E.InvalidArgument, match="another corpus handle"):
                other.search_filtered(q[:2], K, G.L2, f)
        old.close()
        with pytest.raises(E.InvalidArgument):
            c.search_filtered(q[:2], K, G.L2, old)  # closed
        short = np.zeros((N + 7) // 8 - 1, np.uint8)
        import ctypes as C
        from metrovector_amd import _lib
        h = C.c_void_p()
        rc = _lib.gpu().mvfgpu_filter_create(c._h, short.ctypes.data_as(C.c_void_p), 0, short.size * 8, C.byref(h))
        assert rc == 12 and "fewer rows" in _lib.gpu().mvfgpu_last_error_message().decode() and not h.value
        bits = np.packbits(allow, bitorder="little")
        rc = _lib.gpu().mvfgpu_filter_create(c._h, bits.ctypes.data_as(C.c_void_p), 8, bits.size * 8, C.byref(h))
        assert rc == 12 and not h.value  # nbits < first_bit + rows


@pytest.mark.parametrize("route", [MASK, LIST])
def test_two_threads_share_one_filter(oracle, monkeypatch, route):
    rows, q, dead, allow, admit, want = _case(oracle, 3, G.INNER_PRODUCT)
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    out = {}
    with G.GpuCorpus.from_array(rows, index_base=BASE) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        with c.make_filter(allow) as f:
            def work(t):
                out[t] = [c.search_filtered(q[:nq], K, G.INNER_PRODUCT, f) for nq in (1, 40, 5, 40, 1)]
            th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
            [t.start() for t in th]
            [t.join() for t in th]
    for a, b, nq in zip(out[0], out[1], (1, 40, 5, 40, 1)):
        assert _same(a, b)
        assert_exact(a, want[0][:nq], want[1][:nq], want[2][:nq])


# ---- the handle's state -------------------------------------------------------------------------------------------------

def test_filtered_searches_leave_the_handles_plain_searches_alone(oracle, monkeypatch):
    """MVF_K2_REGION_RECORDS makes batched searches repair most queries: a series of PLAIN searches would feed that to the
    repair feedback and switch selections off.  Filtered searches neither read nor feed it."""
    n, dim, nq, k = 200_000, 64, 300, 20
    rows = oracle.synth_rows(81, 0, n, dim, 0)
    q = oracle.synth_queries(82, nq, dim, 0)
    allow = np.random.default_rng(10).random(n) < 0.5
    monkeypatch.setenv("MVF_K2_REGION_RECORDS", "4096")
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(MASK))
    with G.GpuCorpus.from_array(rows) as fresh:
        want = fresh.search(q, k, G.COSINE)
        assert fresh.last_timing().repaired_queries > nq // 2, "the regions were not small"
    with G.GpuCorpus.from_array(rows) as c:
        before = c.info().selection_state
        with c.make_filter(allow) as f:
            for _ in range(8):
                res = c.search_filtered(q, k, G.COSINE, f)
            assert c.last_timing().repaired_queries > 0, "the filtered searches repaired nothing"
            assert not np.isin(res.indices, np.nonzero(~allow)[0]).any()
        assert c.info().selection_state == before
        got = c.search(q, k, G.COSINE)
        assert c.info().selection_state == before
    assert _same(got, want), "a plain search behind filtered searches differs from a fresh handle's"


# ---- row-range shards ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", [MASK, LIST])
@pytest.mark.parametrize("dtype,metric", [(2, G.L2), (0, G.INNER_PRODUCT)])
def test_two_shards_given_the_whole_bitmap_merge_into_the_single_handle_answer(oracle, monkeypatch, route, dtype, metric):
    rows, q, dead, allow, admit, _ = _case(oracle, dtype, metric)
    nq, cut = 6, 9_999
    bits = np.packbits(allow, bitorder="little")      # ONE bitmap over the whole space
    tomb = np.packbits(dead, bitorder="little")
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    per = []
    for a, b in ((0, cut), (cut, N)):
        with G.GpuCorpus.from_array(rows[a:b], index_base=a) as c:
            c.set_tombstones(tomb, first_bit=a)
            c.set_scan_path(1)
            with c.make_filter(bits, first_bit=a) as f:
                assert f.admitted == int(admit[a:b].sum())
                per.append(c.search_filtered(q[:nq], K, metric, f))
    merged = G.merge_topk_host(np.stack([p.scores for p in per]), np.stack([p.indices for p in per]), np.stack([p.raw for p in per]),
                               metric, dtype)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_tombstones(tomb)
        c.set_scan_path(1)
        with c.make_filter(bits) as f:
            assert _same(merged, c.search_filtered(q[:nq], K, metric, f))


# ---- C++ ----------------------------------------------------------------------------------------------------------------

_CPP = r"""
#include "mvf.hpp"
#include <cstdio>
int main(int argc, char** argv) {
    using namespace mvf;
    if (argc < 2) return 2;
    try {
        std::vector<std::vector<float>> rows;
        for (int i = 0; i < 60; i++) rows.push_back({(float)i, 1.0f, 0.0f, 0.0f});
        MvfBuilder b;
        b.add_vector_space("s", 4, VectorType::Dense, DistanceMetric::L2, DataType::Float32);
        b.add_vectors("s", rows);
        b.build().save(argv[1]);
        MvfReader r = MvfReader::open(argv[1]);
        const VectorSpace space = r.vector_space("s");
        const GpuVectorSpace resident(space);
        std::vector<uint8_t> allow(8, 0);
        for (int i = 0; i < 60; i += 5) allow[i >> 3] |= (uint8_t)(1u << (i & 7));  // rows 0, 5, .., 55
        for (const ScoredVector& v : resident.find_top_k_filtered({21.0f, 1.0f, 0.0f, 0.0f}, 4, allow)) std::printf("%llu:%.1f ", (unsigned long long)v.index, v.score);
        std::printf("\n");
        std::printf("%zu\n", resident.find_top_k_filtered({21.0f, 1.0f, 0.0f, 0.0f}, 40, allow).size());
        try { resident.find_top_k_filtered({1, 1, 1}, 1, allow); } catch (const MvfError&) { std::printf("short query refused\n"); }
        try { resident.find_top_k_filtered({1, 1, 1, 1}, 1, std::vector<uint8_t>(7, 0xFF)); } catch (const MvfError&) { std::printf("short bitmap refused\n"); }
    } catch (const MvfError& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
"""


def test_cpp_find_top_k_filtered(tmp_path):
    src, exe = tmp_path / "filtered.cpp", str(tmp_path / "filtered_cpp")
    src.write_text(_CPP)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", LIBDIR, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe, str(tmp_path / "filtered.mvf")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ["20:1.0", "25:4.0", "15:6.0", "30:9.0"]
    assert lines[1] == "12" and lines[2] == "short query refused" and lines[3] == "short bitmap refused"


@pytest.mark.parametrize("poison", [None, 0x00, 0xFF])
def test_cpp_find_top_k_filtered_with_poisoned_allocations(tmp_path, poison):
    """The same executable, its process started with every allocation of the library filled with a byte before its first use
    (MVF_DEBUG_POISON): the answer does not depend on what the memory held."""
    src, exe = tmp_path / "filtered.cpp", str(tmp_path / "filtered_cpp")
    src.write_text(_CPP)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", LIBDIR, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    env = {k: v for k, v in os.environ.items() if k != "MVF_DEBUG_POISON"}
    if poison is not None:
        env["MVF_DEBUG_POISON"] = str(poison)
    out = RUNNER.run([exe, str(tmp_path / "filtered.mvf")], env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ["20:1.0", "25:4.0", "15:6.0", "30:9.0"]
    assert lines[1] == "12" and lines[2] == "short query refused" and lines[3] == "short bitmap refused"
