"""Candidate search on the GPU (mvfgpu_search_candidates[_device], DESIGN.md §3 "Candidate search"): against the oracle
restricted to each list (exact on Int8 / UInt8 L2 / InnerProduct, within the score tolerance elsewhere) and, bit for bit,
against K1's one-query scores -- the yardstick is a one-query mvfgpu_search on scan path 1 with k = rows."""
import os
import subprocess

import numpy as np
import pytest

from metrovector_amd import gpu as G

from _candidates import PAD, candidate_rows, oracle_candidates
from _util import assert_float_topk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [G.FLOAT32, G.FLOAT16, G.INT8, G.UINT8]
METRICS = [G.L2, G.INNER_PRODUCT, G.COSINE]
# (dim, rows, m, nq): dims 1 / 7 / 100 / 128 / 768 / 3000 give every K1 lane width 1..64 across the four types; lists of
# 1 / 37 / 1000 / 20000 entries (one chunk, many chunks, the LDS sort and the long-list sort of C0); 1 .. 1500 queries
# (windows of 1024)
SHAPES = [(1, 3001, 37, 3), (7, 2003, 1000, 64), (100, 5003, 1, 1500), (128, 4001, 20000, 3), (768, 3001, 1000, 64),
          (3000, 1003, 37, 1)]


def _exact(dtype, metric):
    return dtype in (G.INT8, G.UINT8) and metric != G.COSINE


def _lists(rng, n, nq, m, index_base=0, foreign=True):
    hi = n + (n // 10 if foreign else 0)
    lists = (rng.integers(0, max(hi, 1), size=(nq, m)) + index_base).astype(np.uint64)
    if m > 4:
        lists[:, ::7] = PAD
    return lists


def _k1_yardstick(c, q, metric, n):
    """K1's one-query scores and order of every live row (the handle on scan path 1)"""
    return c.search(q[None, :], n, metric)


def _check_k1_bits(res_j, yard, sel, k, index_base=0):
    """Scores and order equal the yardstick's (one-query scan path 1, k = rows) filtered to the list, bit for bit."""
    yi = yard.indices[0]
    keep = np.isin(yi, sel.astype(np.uint64) + np.uint64(index_base))
    want_i, want_s, want_r = yi[keep][:k], yard.scores[0][keep][:k], yard.raw[0][keep][:k]
    kk = want_i.size
    assert (res_j[1][:kk] == want_i).all(), "order differs from K1's"
    assert (res_j[0][:kk].view(np.uint32) == want_s.view(np.uint32)).all(), "score bits differ from K1's"
    assert (res_j[2][:kk] == want_r).all()
    assert (res_j[1][kk:] == PAD).all()


def _check_oracle(oracle, rows, dtype, metric, q, lst, k, got_s, got_i, got_r, got_c, all_scores, dead=None, index_base=0):
    cnt, S, I, R = oracle_candidates(oracle, rows, dtype, metric, q, lst, k, dead=dead, index_base=index_base, all_scores=all_scores)
    assert got_c == cnt, f"count {got_c} != {cnt}"
    if _exact(dtype, metric):
        assert (got_i == I).all() and (got_r == R).all()
        assert (got_s.view(np.uint32) == S.view(np.uint32)).all()
        return
    sel = candidate_rows(lst, rows.shape[0], index_base=index_base, dead=dead)
    kk = min(k, sel.size)
    li = (got_i[:kk] - np.uint64(index_base)).astype(np.int64)
    pos = np.searchsorted(sel, li)
    assert (pos < sel.size).all() and (sel[np.minimum(pos, sel.size - 1)] == li).all(), "a returned row is not a candidate"
    sub_i = np.concatenate([pos.astype(np.uint64), np.full(k - kk, PAD, np.uint64)])
    rows_f32 = rows[sel].astype(np.float32)
    assert_float_topk(metric, got_s, sub_i, all_scores[0][sel], rows_f32, np.asarray(q, np.float32), k)


@pytest.mark.parametrize("dim,n,m,nq", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_matrix(oracle, dtype, metric, dim, n, m, nq):
    rows = oracle.synth_rows(500 + dim, 0, n, dim, dtype)
    qs = oracle.synth_queries(600 + nq, nq, dim, dtype)
    rng = np.random.default_rng(dim * 7 + m)
    lists = _lists(rng, n, nq, m)
    k = 100
    with G.GpuCorpus.from_array(rows) as c:
        res = c.search_candidates(qs, lists, k, metric)
        assert res.indices.shape == (nq, k) and res.counts.shape == (nq,)
        c.set_scan_path(1)
        check = sorted(set(list(range(min(nq, 6))) + [nq - 1]))
        for j in check:
            all_s = oracle.scores(rows, dtype, metric, qs[j])
            _check_oracle(oracle, rows, dtype, metric, qs[j], lists[j], k, res.scores[j], res.indices[j], res.raw[j],
                          int(res.counts[j]), all_s)
            sel = candidate_rows(lists[j], n)
            _check_k1_bits((res.scores[j], res.indices[j], res.raw[j]), _k1_yardstick(c, qs[j], metric, n), sel, k)
        if nq > 6:  # every query's count
            for j in range(nq):
                assert int(res.counts[j]) == candidate_rows(lists[j], n).size


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_a_list_of_every_row_reproduces_the_search(oracle, dtype, metric):
    n, dim, k = 4099, 96, 64
    rows = oracle.synth_rows(71, 0, n, dim, dtype)
    qs = oracle.synth_queries(72, 3, dim, dtype)
    rng = np.random.default_rng(5)
    lists = np.stack([rng.permutation(n) for _ in range(3)]).astype(np.uint64)
    with G.GpuCorpus.from_array(rows) as c:
        res = c.search_candidates(qs, lists, k, metric)
        c.set_scan_path(1)
        for j in range(3):
            ref = c.search(qs[j][None, :], k, metric)
            assert (res.indices[j] == ref.indices[0]).all()
            assert (res.scores[j].view(np.uint32) == ref.scores[0].view(np.uint32)).all()
            assert (res.raw[j] == ref.raw[0]).all()
            assert int(res.counts[j]) == n


def test_edge_entries(oracle):
    """Duplicates inside a chunk and 15000 entries apart, padding, foreign positions, tombstones, index_base, NaN / Inf
    rows, k > 1024 and k > m; positions in the host and the device call."""
    import torch
    n, dim, base = 6007, 64, 1_000_000
    rows = oracle.synth_rows(81, 0, n, dim, G.FLOAT32)
    rows[10, 3] = np.nan
    rows[11, 0] = np.inf
    rows[12, 5] = -np.inf
    dead = np.zeros(n, bool)
    dead[[13, 500, 4000]] = True
    bitmap = np.packbits(dead, bitorder="little")
    qs = oracle.synth_queries(82, 2, dim, G.FLOAT32)
    rng = np.random.default_rng(9)
    m = 20000
    lists = (rng.integers(0, n, size=(2, m)) + base).astype(np.uint64)
    lists[:, 100:110] = lists[:, 90:100]              # duplicates inside a chunk
    lists[:, 18000:18050] = lists[:, 3000:3050]       # ... and far apart
    lists[:, 5:15] = np.array([10, 11, 12, 13, 500, 4000, 10, 11, 12, 13], np.uint64) + np.uint64(base)
    lists[:, 200:260] = PAD
    lists[:, 300:320] = np.uint64(base + n) + np.arange(20, dtype=np.uint64)   # past the shard
    lists[:, 320:330] = np.uint64(base - 5) + np.arange(10, dtype=np.uint64) % 5  # in front of it
    with G.GpuCorpus.from_array(rows, index_base=base) as c:
        c.set_tombstones(bitmap)
        for metric in METRICS:
            for k in (5, 100, 3000, 30000):
                res = c.search_candidates(qs, lists, k, metric)
                for j in range(2):
                    all_s = oracle.scores(rows, G.FLOAT32, metric, qs[j])
                    _check_oracle(oracle, rows, G.FLOAT32, metric, qs[j], lists[j], k, res.scores[j], res.indices[j],
                                  res.raw[j], int(res.counts[j]), all_s, dead=dead, index_base=base)
                dq = torch.from_numpy(qs).cuda()
                dl = torch.from_numpy(lists.view(np.int64)).cuda()
                ds = torch.empty((2, k), dtype=torch.float32, device="cuda")
                di = torch.empty((2, k), dtype=torch.int64, device="cuda")
                dr = torch.empty((2, k), dtype=torch.int32, device="cuda")
                dc = torch.empty(2, dtype=torch.int64, device="cuda")
                st = torch.cuda.Stream()
                c.search_candidates_device(dq.data_ptr(), G.FLOAT32, dim, 2, dl.data_ptr(), m, k, metric, ds.data_ptr(),
                                           di.data_ptr(), dr.data_ptr(), dc.data_ptr(), st.cuda_stream)
                st.synchronize()
                assert (di.cpu().numpy().view(np.uint64) == res.indices).all()
                assert (ds.cpu().numpy().view(np.uint32) == res.scores.view(np.uint32)).all()
                assert (dr.cpu().numpy() == res.raw).all()
                assert (dc.cpu().numpy().view(np.uint64) == res.counts).all()
        # NaN ranks last (L2), deleted rows never appear
        res = c.search_candidates(qs[:1], lists[:1, 5:15], 10, G.L2)
        assert int(res.counts[0]) == 3 and res.indices[0][2] == base + 10 and np.isnan(res.scores[0][2])


@pytest.mark.parametrize("dtype,metric", [(G.FLOAT32, G.L2), (G.INT8, G.COSINE)])
@pytest.mark.parametrize("k", [10, 1500])
def test_per_query_counts_next_to_full_chunks(oracle, dtype, metric, k):
    """One launch of the gathered-row kernel with per-query counts: a list of three chunks (the last partial) of distinct
    live rows, next to a list that holds one row (its chunks 1 and 2 are empty) and a list of dead entries only (count 0);
    k = 10 merges the chunks' lists, k = 1500 sorts the dump.  The full list's results do not depend on its neighbours."""
    n, dim, nq, m = 4001, 7, 3, 2 * 1024 + 5
    rows = oracle.synth_rows(141, 0, n, dim, dtype)
    qs = oracle.synth_queries(142, nq, dim, dtype)
    dead = np.zeros(n, bool)
    dead[77] = True
    live = np.nonzero(~dead)[0]
    lists = np.empty((nq, m), np.uint64)
    lists[0] = np.random.default_rng(14).permutation(live)[:m]
    lists[1] = 1234
    lists[2] = np.resize(np.array([PAD, n, n + 9, 77, 2 ** 40], np.uint64), m)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        res = c.search_candidates(qs, lists, k, metric)
        assert res.counts.tolist() == [m, 1, 0]
        for j in range(nq):
            all_s = oracle.scores(rows, dtype, metric, qs[j])
            _check_oracle(oracle, rows, dtype, metric, qs[j], lists[j], k, res.scores[j], res.indices[j], res.raw[j],
                          int(res.counts[j]), all_s, dead=dead)
            cnt = int(res.counts[j])
            assert (res.indices[j][cnt:] == PAD).all() and (res.raw[j][cnt:] == 0).all()
            assert (res.scores[j][cnt:] == (np.inf if metric == G.L2 else -np.inf)).all()
        assert res.indices[1][0] == 1234
        alone = c.search_candidates(qs[:1], lists[:1], k, metric)
        assert alone.indices.tobytes() == res.indices[:1].tobytes()
        assert alone.scores.tobytes() == res.scores[:1].tobytes()
        assert alone.raw.tobytes() == res.raw[:1].tobytes() and alone.counts[0] == res.counts[0]


def test_a_second_host_window(oracle):
    """The host-buffer calls of the list searches stage their queries, lists and results in windows of at most 256 MiB of
    device copies (csrc/host_staging.h: kHostWindowBytes = 256 MiB; windows of up to kPinnedBytes = 1 MiB travel through
    the handle's pinned mirrors).  Lists of 20000 entries make a query 160680 bytes, a window 1670 queries: 1700 queries
    are windows of 1670 and 30.  The queries on both sides of the seam answer as they do alone, every count is right."""
    n, dim, m, k, nq, metric = 4001, 128, 20000, 10, 1700, G.L2
    W = (256 << 20) // (dim * 4 + m * 8 + k * 16 + 8)
    assert W == 1670 and W < nq < 2 * W
    rows = oracle.synth_rows(151, 0, n, dim, G.FLOAT32)
    qs = oracle.synth_queries(152, nq, dim, G.FLOAT32)
    lists = _lists(np.random.default_rng(15), n, nq, m)
    with G.GpuCorpus.from_array(rows) as c:
        res = c.search_candidates(qs, lists, k, metric)
        for j in (0, W - 1, W, nq - 1):
            alone = c.search_candidates(qs[j:j + 1], lists[j:j + 1], k, metric)
            for name in ("scores", "indices", "raw", "counts"):
                assert getattr(alone, name).tobytes() == getattr(res, name)[j:j + 1].tobytes(), f"{name} of query {j}"
    for j in range(nq):
        assert int(res.counts[j]) == candidate_rows(lists[j], n).size, f"count of query {j}"


def test_ids_in_the_host_call_and_nothing_listed(oracle):
    n, dim = 3001, 24
    rows = oracle.synth_rows(91, 0, n, dim, G.INT8)
    ids = (np.arange(n, dtype=np.uint64) * 11 + 7)
    ids[5] = ids[6]  # a duplicate id: the first row holding it
    qs = oracle.synth_queries(92, 4, dim, G.INT8)
    rng = np.random.default_rng(4)
    lists = ids[rng.integers(0, n, size=(4, 500))].copy()
    lists[:, :3] = np.array([ids[6], 3, ids[6] + 1], np.uint64)  # a shared id, ids nobody holds
    with G.GpuCorpus.from_array(rows) as c:
        c.set_vector_ids(ids)
        for metric in METRICS:
            res = c.search_candidates(qs, lists, 50, metric)
            for j in range(4):
                cnt, S, I, R = oracle_candidates(oracle, rows, G.INT8, metric, qs[j], lists[j], 50, ids=ids)
                assert int(res.counts[j]) == cnt and (res.indices[j] == I).all()
                if metric != G.COSINE:
                    assert (res.scores[j].view(np.uint32) == S.view(np.uint32)).all() and (res.raw[j] == R).all()
        empty = c.search_candidates(qs, np.zeros((4, 0), np.uint64), 3, G.L2)
        assert (empty.counts == 0).all() and (empty.indices == PAD).all() and (empty.scores == np.inf).all()
        every = np.full((1, 8), PAD, np.uint64)
        assert int(c.search_candidates(qs[:1], every, 3, G.L2).counts[0]) == 0


def test_a_query_larger_than_lds(oracle):
    n, dim = 700, 20000
    rows = oracle.synth_rows(101, 0, n, dim, G.FLOAT32)
    qs = oracle.synth_queries(102, 2, dim, G.FLOAT32)
    lists = np.random.default_rng(2).integers(0, n, size=(2, 300)).astype(np.uint64)
    with G.GpuCorpus.from_array(rows) as c:
        res = c.search_candidates(qs, lists, 40, G.COSINE)
        c.set_scan_path(1)
        for j in range(2):
            sel = candidate_rows(lists[j], n)
            _check_k1_bits((res.scores[j], res.indices[j], res.raw[j]), _k1_yardstick(c, qs[j], G.COSINE, n), sel, 40)
            all_s = oracle.scores(rows, G.FLOAT32, G.COSINE, qs[j])
            _check_oracle(oracle, rows, G.FLOAT32, G.COSINE, qs[j], lists[j], 40, res.scores[j], res.indices[j], res.raw[j],
                          int(res.counts[j]), all_s)


@pytest.mark.parametrize("dtype", [G.FLOAT32, G.INT8])
def test_row_range_shards_merge_into_one_handle(oracle, dtype):
    n, dim, nq, m, k = 9001, 40, 5, 3000, 60
    rows = oracle.synth_rows(111, 0, n, dim, dtype)
    qs = oracle.synth_queries(112, nq, dim, dtype)
    lists = _lists(np.random.default_rng(8), n, nq, m)
    cuts = [0, 2500, 6100, n]
    for metric in METRICS:
        with G.GpuCorpus.from_array(rows) as whole:
            ref = whole.search_candidates(qs, lists, k, metric)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            with G.GpuCorpus.from_array(rows[a:b], index_base=a) as c:
                parts.append(c.search_candidates(qs, lists, k, metric))
        merged = G.merge_topk_host(np.stack([p.scores for p in parts]), np.stack([p.indices for p in parts]),
                                   np.stack([p.raw for p in parts]), metric, dtype)
        assert (merged.indices == ref.indices).all()
        assert (merged.scores.view(np.uint32) == ref.scores.view(np.uint32)).all()
        assert (merged.raw == ref.raw).all()
        assert (sum(p.counts for p in parts) == ref.counts).all()


def test_permutations_and_repeats_change_no_byte(oracle):
    n, dim, nq, m, k = 5000, 200, 8, 2500, 100
    rows = oracle.synth_rows(121, 0, n, dim, G.FLOAT16)
    qs = oracle.synth_queries(122, nq, dim, G.FLOAT16)
    rng = np.random.default_rng(12)
    lists = _lists(rng, n, nq, m)
    perm = np.stack([l[rng.permutation(m)] for l in lists])
    with G.GpuCorpus.from_array(rows) as c:
        for metric in METRICS:
            a = c.search_candidates(qs, lists, k, metric)
            b = c.search_candidates(qs, lists, k, metric)
            p = c.search_candidates(qs, perm, k, metric)
            for r in (b, p):
                assert (r.indices == a.indices).all() and (r.scores.view(np.uint32) == a.scores.view(np.uint32)).all()
                assert (r.raw == a.raw).all() and (r.counts == a.counts).all()


def test_rerank_top_k_python(oracle):
    from metrovector_amd import MvfBuilder, MvfReader, find_top_k_similar_batch, rerank_top_k
    from metrovector_amd.reader import VectorType
    n, dim = 500, 16
    rows = oracle.synth_rows(131, 0, n, dim, G.FLOAT32)
    b = MvfBuilder()
    b.add_vector_space("emb", dim, VectorType.Dense, G.COSINE, G.FLOAT32)
    b.add_vectors_raw("emb", rows)
    img = b.build().to_bytes()
    space = MvfReader.from_bytes(img).vector_space("emb")
    qs = oracle.synth_queries(132, 2, dim, G.FLOAT32)
    top = find_top_k_similar_batch(space, qs, 10)
    cand = np.array([[h.index for h in hits] + [int(PAD)] * 5 for hits in top], np.uint64)
    rr = rerank_top_k(space, qs, cand, 7, with_vectors=True)
    for hits, ref in zip(rr, top):
        assert [h.index for h in hits] == [h.index for h in ref[:7]]
        assert [np.float32(h.score).view(np.uint32) for h in hits] == [np.float32(h.score).view(np.uint32) for h in ref[:7]]
        assert all((h.vector == rows[h.index]).all() for h in hits)


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
    std::vector<float> q = {1.0f, 1.0f, 1.0f, 1.0f};
    std::vector<uint64_t> cand = {5, 3, 3, 59, 58, 1000, ~0ull, 0, 17};
    for (const auto& h : gs.rerank_top_k(q, cand, 4)) {
        uint32_t b;
        std::memcpy(&b, &h.score, 4);
        std::printf("%llu:%08x\n", (unsigned long long)h.index, b);
    }
    return 0;
}
'''


def test_cpp_rerank_top_k(tmp_path, golden_dir):
    from metrovector_amd import MvfReader, rerank_top_k
    src = tmp_path / "rerank.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "rerank_cpp")
    libdir = os.path.join(ROOT, "metrovector_amd")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                          "-L", libdir, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    path = os.path.join(golden_dir, "clusters_60x4_f32.mvf")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [(int(a), int(b, 16)) for a, b in (l.split(":") for l in run.stdout.split())]
    r = MvfReader.open(path)
    cand = np.array([[5, 3, 3, 59, 58, 1000, int(PAD), 0, 17]], np.uint64)
    want = rerank_top_k(r.vector_space(r.vector_space_names()[0]), np.ones((1, 4), np.float32), cand, 4)[0]
    assert got == [(h.index, int(np.float32(h.score).view(np.uint32))) for h in want]
    assert len(got) == 4
