"""k-NN join on the GPU (mvfgpu_knn_join[_device], DESIGN.md §3 "Join"): against the oracle's score of ALL rows for EVERY
query row of the range (exact on Int8 / UInt8 L2 / InnerProduct, the tolerance-aware criterion elsewhere, self's score
set to NaN so that it ranks last); bit for bit against the contract (mvfgpu_search per hand-staged window + the removal
rule of tests/_knn.py); the edge cases; two handles; device call == host call; the Python and C++ mirrors."""
import os
import subprocess

import numpy as np
import pytest

from metrovector_amd import gpu as G

import _knn as K
from _util import assert_float_topk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = K.PAD
DTYPES = [G.FLOAT32, G.FLOAT16, G.INT8, G.UINT8]
METRICS = [G.L2, G.INNER_PRODUCT, G.COSINE]
STREAMING, BATCHED = {1}, {2, 3, 4, 6}   # mvfgpu_timing.scan_kernel


def _exact(dtype, metric):
    return dtype in (G.INT8, G.UINT8) and metric != G.COSINE


def _same(a, b):
    assert (a.indices == b.indices).all(), "indices differ"
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), "score bits differ"
    assert (a.raw == b.raw).all(), "raw differs"


def _check_row_against_oracle(oracle, rows, rows_f32, dtype, metric, i, k, got_s, got_i, got_r, index_base=0):
    """Query row i (local) of a self-join with the flag, against the oracle's score of every row."""
    n = rows.shape[0]
    q = K.widen(rows[i])
    sc, keys, raw = oracle.scores(rows, dtype, metric, q)
    if _exact(dtype, metric):
        comp = (keys.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        comp[i] = PAD
        kk = min(k, n - 1)
        best = np.sort(np.partition(comp, kk - 1)[:kk]) if kk else comp[:0]
        pos = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert (got_i[:kk] == pos.astype(np.uint64) + np.uint64(index_base)).all(), f"row {i}: indices"
        assert (got_r[:kk] == raw[pos]).all(), f"row {i}: raw"
        assert (got_s[:kk].view(np.uint32) == sc[pos].view(np.uint32)).all(), f"row {i}: score bits"
        assert (got_i[kk:] == PAD).all()
        return
    assert k < n
    all_s = sc.astype(np.float32).copy()
    all_s[i] = np.nan  # self ranks last: it may never be returned (k < n)
    assert np.uint64(index_base + i) not in got_i, f"row {i} is its own neighbour"
    assert_float_topk(metric, got_s, got_i, all_s, rows_f32, np.asarray(q, np.float32), k, index_base=index_base)


def _check_range_against_oracle(oracle, rows, dtype, metric, res, first, count, k):
    assert res.indices.shape == (count, k)
    rows_f32 = rows.astype(np.float32)
    for j in range(count):  # every query row of the range
        _check_row_against_oracle(oracle, rows, rows_f32, dtype, metric, first + j, k, res.scores[j], res.indices[j], res.raw[j])


# (dim, rows, first, count, k, the route the windows must take): ranges start mid-corpus and end in a short window;
# 1 / 7 / 100 / 128 / 768 / 3000 dimensions; k' = k + 1 crosses 410 / 1024 / 1025
SHAPES = [
    (1, 3001, 1500, 1501, 1, None),
    (7, 2003, 0, 2003, 1023, None),
    (7, 2003, 900, 1100, 1024, None),          # k' = 1025: the large-k route
    (100, 100_003, 49_000, 1324, 10, BATCHED),   # the newest search (what last_timing shows) is the short window: 300 rows
    (128, 5003, 2501, 3, 10, STREAMING),       # three queries on a small corpus: the streaming kernel
    (768, 20_011, 5000, 1100, 100, BATCHED),
    (3000, 4001, 2990, 1011, 409, None),
    (96, 3001, 1000, 1500, 410, None),
]


@pytest.mark.parametrize("dim,n,first,count,k,route", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_oracle(oracle, dtype, metric, dim, n, first, count, k, route):
    rows = oracle.synth_rows(900 + dim, 0, n, dim, dtype)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_profiling(True)
        res = c.knn_join(k, metric, first=first, count=count)
        if route is not None:
            kern = c.last_timing().scan_kernel
            assert kern in route, f"scan_kernel {kern}: the route this case is here for was not taken"
    _check_range_against_oracle(oracle, rows, dtype, metric, res, first, count, k)


@pytest.mark.parametrize("scan_path", [0, 1])
@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("metric", [G.L2, G.COSINE])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_contract_bit_for_bit(oracle, dtype, metric, exclude, scan_path):
    """The join == mvfgpu_search with k' on the hand-staged windows (read_rows, numpy widening) of a second handle with
    identical content, scan path and search history, + the removal rule: indices, score bits, raw."""
    n, dim, first, count, k = 30_011, 96, 1000, 2100, 10
    rows = oracle.synth_rows(77, 0, n, dim, dtype)
    rows[1500] = rows[1499]  # a duplicate pair inside the range
    with G.GpuCorpus.from_array(rows) as a, G.GpuCorpus.from_array(rows) as b:
        a.set_scan_path(scan_path)
        b.set_scan_path(scan_path)
        got = a.knn_join(k, metric, first=first, count=count, exclude_self=exclude)
        kk = K.k_prime(k, exclude, 0, n, 0, n)
        assert kk == (k + 1 if exclude else k)
        S, I, R = [], [], []
        for w0, wn in K.windows(first, count):
            q = K.widen(b.read_rows(w0, wn))
            r = b.search(q, kk, metric)
            s_, i_, r_ = K.join_from_lists(r.scores, r.indices, r.raw, np.arange(w0, w0 + wn), k, metric)
            S.append(s_), I.append(i_), R.append(r_)
        _same(got, G.SearchResult(np.concatenate(S), np.concatenate(I), np.concatenate(R)))
        if exclude:
            assert (got.indices != np.arange(first, first + count, dtype=np.uint64)[:, None]).all()
        else:
            assert got.indices[500 - 0, 0] in (1499, 1500)  # row 1500 and its duplicate: whichever comes first


@pytest.mark.parametrize("metric", [G.L2, G.COSINE])
def test_fifty_identical_rows(metric):
    """50 copies of one point in front of other rows, k = 10: every copy's neighbours are copies, in position order, without
    itself -- rows 0..10 lose themselves from the top 11, rows 11..49 are not in it and lose its last entry."""
    rng = np.random.default_rng(1)
    other = rng.standard_normal((200, 24)).astype(np.float32) * 3 + 9
    rows = np.concatenate([np.tile(np.linspace(1, 2, 24, dtype=np.float32), (50, 1)), other])
    with G.GpuCorpus.from_array(rows) as c:
        res = c.knn_join(10, metric)
    for i in range(50):
        want = [p for p in range(11) if p != i][:10]
        assert res.indices[i].tolist() == want, f"row {i}"
        assert (res.scores[i].view(np.uint32) == res.scores[i].view(np.uint32)[0]).all()
    if metric == G.L2:
        assert (res.scores[:50] == 0).all()


def _int_rows(oracle, n=700, dim=20, seed=5):
    rows = oracle.synth_rows(seed, 0, n, dim, G.INT8)
    rows[100] = rows[7]
    rows[101] = rows[7]
    rows[650] = rows[7]
    return rows


def _want_int(oracle, rows, metric, k, first, count, index_base=0, dead=None, ids=None, q_rows=None, q_base=None, exclude=True):
    """The expected join of Int8 rows from the oracle's exact integer scores and tests/_knn.py."""
    q_rows = rows if q_rows is None else q_rows
    q_base = index_base if q_base is None else q_base
    n = rows.shape[0]
    per = [oracle.scores(rows, G.INT8, metric, q_rows[first + j]) for j in range(count)]
    sc, raw = np.stack([p[0] for p in per]), np.stack([p[2] for p in per])
    keys = np.stack([p[1] for p in per]).astype(np.float64)   # ascending = best first
    kk = K.k_prime(k, exclude, q_base, q_rows.shape[0], index_base, n)
    # order by the oracle's keys (ascending = best first); scores and raw ride along
    S = np.full((count, kk), K.pad_score(metric), np.float32)
    I = np.full((count, kk), PAD, np.uint64)
    R = np.zeros((count, kk), np.int32)
    for j in range(count):
        order = K.best_first(keys[j], G.L2)
        if dead is not None:
            order = order[~dead[order]]
        order = order[:kk]
        S[j, :order.size], I[j, :order.size], R[j, :order.size] = sc[j][order], order.astype(np.uint64) + np.uint64(index_base), raw[j][order]
    qd = None if dead is None or q_rows is not rows else dead[first:first + count]
    return K.join_from_lists(S, I, R, np.arange(q_base + first, q_base + first + count), k, metric, index_base, ids, qd)


@pytest.mark.parametrize("metric", [G.L2, G.INNER_PRODUCT])
def test_tombstones_ids_index_base_and_padding(oracle, metric):
    """Int8 rows (bit-exact expectations): duplicate ids on duplicate rows, deleted query rows and neighbours,
    index_base != 0, ids attached (results are ids, exclusion still by position), k >= rows, count = 0."""
    rows = _int_rows(oracle)
    n, base = rows.shape[0], 1_000_000
    dead = np.zeros(n, bool)
    dead[[3, 101, 300, 699]] = True
    ids = (np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(11))
    ids[100] = ids[7]     # duplicate rows sharing one id
    ids[650] = ids[7]
    with G.GpuCorpus.from_array(rows, index_base=base) as c:
        res = c.knn_join(5, metric)
        w = _want_int(oracle, rows, metric, 5, 0, n, index_base=base)
        _same(res, G.SearchResult(*w))
        assert res.indices[7][:3].tolist() == [base + 100, base + 101, base + 650] or metric != G.L2
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        res = c.knn_join(5, metric)
        _same(res, G.SearchResult(*_want_int(oracle, rows, metric, 5, 0, n, index_base=base, dead=dead)))
        assert (res.indices[dead] == PAD).all() and (res.raw[dead] == 0).all()
        assert not np.isin(res.indices, np.nonzero(dead)[0].astype(np.uint64) + np.uint64(base)).any()
        c.set_vector_ids(ids)
        res = c.knn_join(5, metric, first=2, count=690)
        _same(res, G.SearchResult(*_want_int(oracle, rows, metric, 5, 2, 690, index_base=base, dead=dead, ids=ids)))
        if metric == G.L2:  # row 7's neighbours are its live duplicates 100 and 650: both carry row 7's own id
            assert res.indices[5][:2].tolist() == [int(ids[7]), int(ids[7])]
        big = c.knn_join(n + 5, metric, first=0, count=12)   # k >= rows: padded
        _same(big, G.SearchResult(*_want_int(oracle, rows, metric, n + 5, 0, 12, index_base=base, dead=dead, ids=ids)))
        live_others = n - int(dead.sum()) - 1
        assert (big.indices[0][live_others:] == PAD).all() and (big.indices[0][:live_others] != PAD).all()
        empty = c.knn_join(5, metric, first=n, count=0)
        assert empty.indices.shape == (0, 5)


def test_nan_and_inf_rows(oracle):
    n, dim = 900, 32
    rows = oracle.synth_rows(8, 0, n, dim, G.FLOAT32)
    rows[10, 3] = np.nan
    rows[11, 0] = np.inf
    rows[12, 5] = -np.inf
    rows_f32 = rows.astype(np.float32)
    for metric in METRICS:
        with G.GpuCorpus.from_array(rows) as c:
            res = c.knn_join(20, metric)
            full = c.knn_join(n - 1, metric, first=0, count=14)
        for i in list(range(0, 10)) + list(range(13, n)):
            _check_row_against_oracle(oracle, rows, rows_f32, G.FLOAT32, metric, i, 20, res.scores[i], res.indices[i], res.raw[i])
        # the NaN row as a query: every score is NaN (Cosine: 0, its denominator is not > 0 -- the oracle's rule), so the order
        # is by position, and self leaves by POSITION
        assert res.indices[10].tolist() == [p for p in range(21) if p != 10]
        want = oracle.scores(rows, G.FLOAT32, metric, rows[10])[0][res.indices[10].astype(np.int64)]
        assert (np.isnan(res.scores[10]) if metric != G.COSINE else res.scores[10] == 0).all()
        assert (np.isnan(want) | (want == res.scores[10])).all()
        # ... and as a neighbour: last of every finite row's complete list
        for i in (0, 5, 13):
            assert full.indices[i][-1] == 10 or not np.isfinite(full.scores[i][-2])
            assert i not in full.indices[i].tolist() and len(set(full.indices[i].tolist())) == n - 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_three_shards_merge_into_the_self_join(oracle, dtype, metric):
    """Three row-range shards of one corpus on one device: every (Q, C) pair joined with the flag and each Q's lists merged
    in ascending row-range order == the one-handle self-join, byte for byte (float types on scan path 1)."""
    n, dim, k = 7000, 64, 20
    rows = oracle.synth_rows(31, 0, n, dim, dtype)
    rows[5000] = rows[10]
    rows[2600] = rows[10]
    bounds = [0, 2500, 4600, n]
    dead = np.zeros(n, bool)
    dead[[11, 2600, 6999]] = True
    with G.GpuCorpus.from_array(rows) as whole:
        whole.set_scan_path(1)
        whole.set_tombstones(np.packbits(dead, bitorder="little"))
        want = whole.knn_join(k, metric)
    shards = []
    try:
        for s in range(3):
            c = G.GpuCorpus.from_array(rows[bounds[s]:bounds[s + 1]], index_base=bounds[s])
            c.set_scan_path(1)
            c.set_tombstones(np.packbits(dead, bitorder="little"), first_bit=bounds[s])
            shards.append(c)
        for qs in range(3):
            lists = [shards[cs].knn_join(k, metric, queries_from=shards[qs]) for cs in range(3)]
            m = G.merge_topk_host(np.stack([r.scores for r in lists]), np.stack([r.indices for r in lists]),
                                  np.stack([r.raw for r in lists]), metric, dtype)
            sl = slice(bounds[qs], bounds[qs + 1])
            live = ~dead[sl]
            assert (m.indices[live] == want.indices[sl][live]).all()
            assert (m.scores[live].view(np.uint32) == want.scores[sl][live].view(np.uint32)).all()
            if _exact(dtype, metric):
                assert (m.raw[live] == want.raw[sl][live]).all()
            assert (m.indices[~live] == PAD).all() and (want.indices[sl][~live] == PAD).all()
    finally:
        for c in shards:
            c.close()


def test_two_handles_disjoint_ranges_the_flag_changes_nothing(oracle):
    rows = _int_rows(oracle)
    with G.GpuCorpus.from_array(rows[:400]) as c, G.GpuCorpus.from_array(rows[400:], index_base=400) as q:
        a = c.knn_join(6, G.L2, queries_from=q, exclude_self=True)
        b = c.knn_join(6, G.L2, queries_from=q, exclude_self=False)
        _same(a, b)
        w = _want_int(oracle, rows[:400], G.L2, 6, 0, 300, q_rows=rows[400:], q_base=400)
        _same(a, G.SearchResult(*w))
        assert a.indices[250][:3].tolist() == [7, 100, 101]  # row 650 = row 7 and its duplicates in C


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_call_equals_host_call_and_orders_through_ev_done(oracle, dtype):
    import torch
    n, dim, k, first, count = 20_000, 128, 33, 700, 2500
    rows = oracle.synth_rows(41, 0, n, dim, dtype)
    with G.GpuCorpus.from_array(rows) as c:
        host = c.knn_join(k, G.INNER_PRODUCT, first=first, count=count)
        ds = torch.empty((count, k), dtype=torch.float32, device="cuda")
        di = torch.empty((count, k), dtype=torch.int64, device="cuda")
        dr = torch.empty((count, k), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        c.knn_join_device(k, G.INNER_PRODUCT, first, count, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), stream=side.cuda_stream)
        # another search on the handle's own stream at once: it orders itself behind the join (ev_done) and both are right
        q = K.widen(rows[:5])
        again = c.search(q, 10, G.INNER_PRODUCT)
        side.synchronize()
        dev = G.SearchResult(ds.cpu().numpy(), di.cpu().numpy().view(np.uint64), dr.cpu().numpy())
        _same(dev, host)
        ref = c.search(q, 10, G.INNER_PRODUCT)
        _same(again, ref)
        # without a raw buffer, on the null stream
        c.knn_join_device(k, G.INNER_PRODUCT, first, count, ds.data_ptr(), di.data_ptr())
        torch.cuda.synchronize()
        assert (di.cpu().numpy().view(np.uint64) == host.indices).all()


def test_build_knn_graph_from_a_file(oracle, tmp_path):
    from metrovector_amd import MvfBuilder, MvfReader, build_knn_graph, upload_space
    from metrovector_amd.reader import VectorType
    n, dim = 1500, 16
    rows = oracle.synth_rows(131, 0, n, dim, G.FLOAT16)
    b = MvfBuilder()
    b.add_vector_space("emb", dim, VectorType.Dense, G.COSINE, G.FLOAT16)
    b.add_vectors_raw("emb", rows)
    path = str(tmp_path / "graph.mvf")
    b.build().save(path)
    space = MvfReader.open(path).vector_space("emb")
    g = build_knn_graph(space, 8)
    assert g.indices.shape == (n, 8)
    rows_f32 = rows.astype(np.float32)
    for i in range(n):
        _check_row_against_oracle(oracle, rows, rows_f32, G.FLOAT16, G.COSINE, i, 8, g.scores[i], g.indices[i], g.raw[i])
    with upload_space(space) as c:  # a resident corpus, a range, another metric
        part = build_knn_graph(space, 8, metric=G.L2, corpus=c, first=1000, count=100)
        _same(part, c.knn_join(8, G.L2, first=1000, count=100))


CPP = r'''
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "mvf.hpp"
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    auto reader = mvf::MvfReader::open(argv[1]);
    auto space = reader.vector_space(reader.vector_space_names()[0]);
    mvf::GpuVectorSpace gs(space);
    auto part = gs.knn_graph(3, 10, 5);
    auto all = gs.knn_graph(3);
    std::printf("%zu %zu\n", part.size(), all.size());
    for (size_t i = 0; i < all.size(); i++) {
        std::printf("%zu", i);
        for (const auto& h : all[i]) {
            uint32_t b;
            std::memcpy(&b, &h.score, 4);
            std::printf(" %llu:%08x", (unsigned long long)h.index, b);
        }
        std::printf("\n");
    }
    for (size_t i = 0; i < part.size(); i++)
        for (size_t j = 0; j < part[i].size(); j++)
            if (part[i][j].index != all[10 + i][j].index) return 3;
    return 0;
}
'''


def test_cpp_knn_graph(tmp_path, golden_dir):
    from metrovector_amd import MvfReader, build_knn_graph
    src = tmp_path / "knn_graph.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "knn_graph_cpp")
    libdir = os.path.join(ROOT, "metrovector_amd")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                          "-L", libdir, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    path = os.path.join(golden_dir, "clusters_60x4_f32.mvf")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[0] == "5 60"
    r = MvfReader.open(path)
    want = build_knn_graph(r.vector_space(r.vector_space_names()[0]), 3)
    for i, line in enumerate(lines[1:]):
        toks = line.split()
        assert int(toks[0]) == i
        got = [(int(a), int(b, 16)) for a, b in (t.split(":") for t in toks[1:])]
        real = want.indices[i] != PAD
        assert got == list(zip(want.indices[i][real].tolist(), want.scores[i][real].view(np.uint32).tolist()))
        assert i not in [g[0] for g in got]
