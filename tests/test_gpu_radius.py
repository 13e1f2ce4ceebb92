"""Radius search on the GPU (mvfgpu_search_radius, DESIGN.md §3 "Radius search"): every check against the oracle's score
of every row and the match rule -- exact on Int8 / UInt8 L2 / InnerProduct, within the score tolerance elsewhere."""
import os
import subprocess

import numpy as np
import pytest

from metrovector_amd import errors as E
from metrovector_amd import gpu as G

from _radius import PAD, assert_float_radius, oracle_radius, radius_for_count
from _util import assert_float_topk, oracle_scores_all_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [G.FLOAT32, G.FLOAT16, G.INT8, G.UINT8]
METRICS = [G.L2, G.INNER_PRODUCT, G.COSINE]
# (dim, rows, queries): row counts that are not multiples of any tile; 1 / 4 queries per pass, remainders, windows
SHAPES = [(1, 1000, 3), (7, 3001, 1024), (100, 5003, 5), (128, 20011, 64), (768, 10007, 4), (768, 4001, 1), (100, 2003, 300)]


def _exact(dtype, metric):
    return dtype in (G.INT8, G.UINT8) and metric != G.COSINE


def _check(oracle, res, rows, dtype, metric, qs, radii, m, all_s=None, dead=None, index_base=0):
    rows_f32 = rows.astype(np.float32)
    for j, q in enumerate(qs):
        if _exact(dtype, metric):
            c, S, I, R = oracle_radius(oracle, rows, dtype, metric, q, radii[j], m, dead=dead, index_base=index_base)
            assert int(res.counts[j]) == c, f"query {j}: count {res.counts[j]} != {c}"
            assert (res.indices[j] == I).all(), f"query {j}: indices"
            assert (res.raw[j] == R).all(), f"query {j}: raw"
            assert (res.scores[j].view(np.uint32) == S.view(np.uint32)).all(), f"query {j}: score bits"
        else:
            s = all_s[j] if all_s is not None else oracle.scores(rows, dtype, metric, q)[0]
            assert_float_radius(metric, int(res.counts[j]), res.scores[j], res.indices[j], s, rows_f32,
                                np.asarray(q, np.float32), radii[j], m, dead=dead, index_base=index_base)


@pytest.mark.parametrize("dim,n,nq", SHAPES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_matrix(oracle, dtype, metric, dim, n, nq):
    rows = oracle.synth_rows(1000 + dim, 0, n, dim, dtype)
    qs = oracle.synth_queries(2000 + nq, nq, dim, dtype)
    all_s = [oracle.scores(rows, dtype, metric, q)[0] for q in qs]
    radii = [radius_for_count(all_s[j], metric, (0, 10, 1000)[j % 3]) for j in range(nq)]
    m = 1500
    with G.GpuCorpus.from_array(rows) as c:
        res = c.search_radius(qs, np.array(radii, np.float32), m, metric)
        assert res.counts.shape == (nq,) and res.indices.shape == (nq, m)
        _check(oracle, res, rows, dtype, metric, qs, radii, m, all_s=all_s)
        cnt = c.search_radius(qs, np.array(radii, np.float32), 0, metric)
        assert (cnt.counts == res.counts).all(), "counts only differ from the full call"


@pytest.mark.parametrize("dtype,metric", [(G.INT8, G.L2), (G.UINT8, G.L2), (G.INT8, G.INNER_PRODUCT), (G.UINT8, G.INNER_PRODUCT)])
def test_boundary_is_inclusive_and_the_next_float_excludes(oracle, dtype, metric):
    rows = oracle.synth_rows(41, 0, 5000, 33, dtype)
    q = oracle.synth_queries(42, 1, 33, dtype)[0]
    s = oracle.scores(rows, dtype, metric, q)[0]
    order = np.sort(s) if metric == G.L2 else np.sort(s)[::-1]
    with G.GpuCorpus.from_array(rows) as c:
        for target in (order[0], order[50], order[2000]):
            ties = int((s == target).sum())
            better = int(((s < target) if metric == G.L2 else (s > target)).sum())
            inside = c.search_radius(q, float(target), 0, metric).counts[0]
            nxt = np.nextafter(np.float32(target), np.float32(-np.inf if metric == G.L2 else np.inf))
            outside = c.search_radius(q, float(nxt), 0, metric).counts[0]
            assert inside == better + ties and outside == better, (target, inside, outside, better, ties)


def test_invalid_arguments_with_a_handle(oracle):
    rows = oracle.synth_rows(5, 0, 100, 8, G.FLOAT32)
    with G.GpuCorpus.from_array(rows) as c:
        with pytest.raises(E.DimensionMismatch):
            c.search_radius(np.zeros(7, np.float32), 1.0, 3)
        with pytest.raises(E.InvalidArgument, match="NaN"):
            c.search_radius(np.zeros((2, 8), np.float32), [1.0, float("nan")], 3)
        with pytest.raises(E.InvalidArgument, match="max_per_query"):
            c.search_radius(np.zeros(8, np.float32), 1.0, 2**31 + 1)
        with pytest.raises(E.BuildError):
            c.search_radius(np.zeros(8, np.int8), 1.0, 3)


@pytest.mark.parametrize("dtype,metric,nq", [(G.INT8, G.L2, 5), (G.UINT8, G.INNER_PRODUCT, 1), (G.FLOAT32, G.INNER_PRODUCT, 6),
                                             (G.FLOAT16, G.L2, 2)])
def test_overflow_of_max_per_query_is_the_top_k(oracle, dtype, metric, nq):
    n, dim, m = 20011, 64, 7
    rows = oracle.synth_rows(61, 0, n, dim, dtype)
    qs = oracle.synth_queries(62, nq, dim, dtype)
    all_s = [oracle.scores(rows, dtype, metric, q)[0] for q in qs]
    radii = np.array([radius_for_count(s, metric, 1000) for s in all_s], np.float32)
    with G.GpuCorpus.from_array(rows) as c:
        res = c.search_radius(qs, radii, m, metric)
        top = c.search(qs, m, metric)
    assert (res.counts >= m).all()
    _check(oracle, res, rows, dtype, metric, qs, radii, m, all_s=all_s)
    if _exact(dtype, metric):
        assert (res.indices == top.indices).all() and (res.raw == top.raw).all()
        assert (res.scores.view(np.uint32) == top.scores.view(np.uint32)).all()
    else:
        for j, q in enumerate(qs):
            assert_float_topk(metric, res.scores[j], res.indices[j], all_s[j], rows.astype(np.float32), np.asarray(q, np.float32), m)


@pytest.mark.parametrize("dtype,nq", [(G.FLOAT32, 3), (G.INT8, 6)])
def test_overflow_of_the_device_list(oracle, dtype, nq):
    """+inf (L2) matches every live row: far more than a device list holds; the counts stay exact and the entries are
    completed by the top-k search."""
    n, dim, m = 20011, 16, 50
    assert n > G.RADIUS_LIST_CAP
    rows = oracle.synth_rows(81, 0, n, dim, dtype)
    qs = oracle.synth_queries(82, nq, dim, dtype)
    dead = np.zeros(n, bool)
    dead[3::13] = True
    with G.GpuCorpus.from_array(rows) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        res = c.search_radius(qs, np.inf, m, G.L2)
        only = c.search_radius(qs, np.inf, 0, G.L2)
        top = c.search(qs, m, G.L2)
    assert (res.counts == n - dead.sum()).all() and (only.counts == res.counts).all()
    assert res.overflowed.all()
    assert (res.indices == top.indices).all()
    assert not dead[res.indices.astype(np.int64)].any()
    _check(oracle, res, rows, dtype, G.L2, qs, [np.inf] * nq, m, dead=dead)


def test_tombstones_ids_index_base_nan_rows_and_determinism(oracle):
    n, dim, base = 3001, 24, 1000
    rows = oracle.synth_rows(91, 0, n, dim, G.FLOAT32)
    rows[5::97, 3] = np.nan
    nan_row = np.isnan(rows).any(axis=1)
    dead = np.zeros(n, bool)
    dead[::7] = True
    qs = oracle.synth_queries(92, 9, dim, G.FLOAT32)
    all_s = [oracle.scores(rows, G.FLOAT32, G.L2, q)[0] for q in qs]
    radii = [radius_for_count(s, G.L2, 100, dead=dead) for s in all_s]
    radii[0] = np.inf
    ids = (np.random.default_rng(3).permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(5))
    m = 300
    with G.GpuCorpus.from_array(rows, index_base=base) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        a = c.search_radius(qs, np.array(radii, np.float32), m, G.L2)
        b = c.search_radius(qs, np.array(radii, np.float32), m, G.L2)
        c.set_vector_ids(ids)
        d = c.search_radius(qs, np.array(radii, np.float32), m, G.L2)
    for f in ("counts", "indices", "raw"):
        assert (getattr(a, f) == getattr(b, f)).all(), f"two identical calls differ in {f}"
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all()
    assert int(a.counts[0]) == int((~dead & ~nan_row).sum()), "+inf must match every live non-NaN row"
    _check(oracle, a, rows, G.FLOAT32, G.L2, qs, radii, m, all_s=all_s, dead=dead, index_base=base)
    valid = a.indices != PAD
    loc = (a.indices[valid] - np.uint64(base)).astype(np.int64)
    assert not dead[loc].any() and not nan_row[loc].any()
    assert (d.indices[valid] == ids[loc]).all() and (d.indices[~valid] == PAD).all()
    assert (d.counts == a.counts).all()


def test_int8_with_tombstones_is_exact(oracle):
    n, dim = 7777, 48
    rows = oracle.synth_rows(95, 0, n, dim, G.INT8)
    qs = oracle.synth_queries(96, 4, dim, G.INT8)
    dead = np.zeros(n, bool)
    dead[1::5] = True
    all_s = [oracle.scores(rows, G.INT8, G.INNER_PRODUCT, q)[0] for q in qs]
    radii = [radius_for_count(s, G.INNER_PRODUCT, 300, dead=dead) for s in all_s]
    with G.GpuCorpus.from_array(rows, index_base=77) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        res = c.search_radius(qs, np.array(radii, np.float32), 500, G.INNER_PRODUCT)
    _check(oracle, res, rows, G.INT8, G.INNER_PRODUCT, qs, radii, 500, dead=dead, index_base=77)


def test_every_scan_path_gives_the_same_rows(oracle):
    """Scan path 1 streams (R1); 2, 3 and 5 take the batched route (one thresholded f32 MFMA pass + exact re-scoring):
    the same counts and rows, bit-identical since the re-scoring sums like R1."""
    n, dim, nq, seed = 1_000_000, 768, 1024, 0x5EED
    assert G.radius_route(G.FLOAT32, nq, 1) == 0 and all(G.radius_route(G.FLOAT32, nq, p) == 1 for p in (2, 3, 5))
    qs = oracle.synth_queries(seed + 1, nq, dim, G.FLOAT32)
    with G.GpuCorpus.synthetic(n, dim, G.FLOAT32, seed) as c:
        top = c.search(qs, 100, G.L2)
        radii = top.scores[:, 99].copy()  # about 100 matches per query
        ref = None
        for path in (1, 2, 3, 5):
            c.set_scan_path(path)
            res = c.search_radius(qs, radii, 128, G.L2)
            if ref is None:
                ref = res
                continue
            assert (res.counts == ref.counts).all() and (res.indices == ref.indices).all(), f"scan path {path}"
            assert (res.scores.view(np.uint32) == ref.scores.view(np.uint32)).all(), f"scan path {path}"
    assert (ref.counts >= 90).all()
    all_s = oracle_scores_all_rows(oracle, seed, 0, n, dim, G.FLOAT32, G.L2, qs[:4])
    for j in range(4):
        assert_float_radius(G.L2, int(ref.counts[j]), ref.scores[j], ref.indices[j], all_s[j], None, qs[j], float(radii[j]), 128)


def _large_dataset_rows(n, dim):
    """The reference's large_dataset generator (examples/large_dataset.rs: base / noise / trend, tanh), restated in f32
    numpy: near-duplicates recur about every 63 rows."""
    i = np.arange(n, dtype=np.float32)[:, None]
    d = np.arange(dim, dtype=np.float32)[None, :]
    base = i * np.float32(0.1) + d * np.float32(0.01)
    noise = np.sin((np.arange(n)[:, None] + np.arange(dim)[None, :]).astype(np.float32) * np.float32(12345.0)) * np.float32(0.1)
    trend = (d / np.float32(dim) - np.float32(0.5)) * np.float32(2.0)
    return np.tanh(np.sin(base) + noise + trend * np.float32(0.1)).astype(np.float32)


def _mixture_rows(n, dim, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((8, dim)).astype(np.float32)
    return (centers[rng.integers(0, 8, n)] + np.float32(0.01) * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("kind", ["large_dataset", "mixture"])
def test_adversarial_corpora(oracle, kind):
    n, dim, m = 30011, 64, 200
    rows = _large_dataset_rows(n, dim) if kind == "large_dataset" else _mixture_rows(n, dim, 7)
    qs = rows[np.arange(0, n, n // 16)[:16]] + np.float32(1e-3)
    all_s = [oracle.scores(rows, G.FLOAT32, G.L2, q)[0] for q in qs]
    radii = [radius_for_count(all_s[j], G.L2, (50, 1000, 12000)[j % 3]) for j in range(len(qs))]
    assert G.radius_route(G.FLOAT32, len(qs)) == 1  # the batched route; the ~12000-match queries overflow its candidates
    with G.GpuCorpus.from_array(rows) as c:
        res = c.search_radius(qs, np.array(radii, np.float32), m, G.L2)
        c.set_scan_path(1)
        ref = c.search_radius(qs, np.array(radii, np.float32), m, G.L2)
    assert (res.counts == ref.counts).all() and (res.indices == ref.indices).all(), "batched + repair != streaming"
    _check(oracle, res, rows, G.FLOAT32, G.L2, qs, radii, m, all_s=all_s)
    big = res.counts > G.RADIUS_LIST_CAP
    assert (res.overflowed == big).all() and big.sum() >= 1, "the ~12000-match queries overflow their lists and are repaired"
    for j in np.nonzero(res.counts > m)[0]:
        assert_float_topk(G.L2, res.scores[j], res.indices[j], all_s[j], rows, qs[j], m)


def test_find_within_radius_on_an_mvf_file(oracle, golden_dir):
    from metrovector_amd import MvfReader, find_within_radius
    r = MvfReader.open(os.path.join(golden_dir, "clusters_60x4_f32.mvf"))
    space = r.vector_space(r.vector_space_names()[0])
    rows = np.stack([space.get_vector(i).as_f32() for i in range(space.total_vectors())]).astype(np.float32)
    metric = int(space.distance_metric())
    q = rows[10] + np.float32(0.05)
    s = oracle.scores(rows, G.FLOAT32, metric, q)[0]
    radius = radius_for_count(s, metric, 7)
    hits = find_within_radius(space, q, radius)
    c, S, I, _ = oracle_radius(oracle, rows, G.FLOAT32, metric, q, radius, 60)
    assert [h.index for h in hits] == I[:c].astype(np.int64).tolist()
    np.testing.assert_allclose([h.score for h in hits], S[:c], rtol=1e-5, atol=1e-6)
    assert all((h.vector == rows[h.index]).all() for h in hits)
    assert len(find_within_radius(space, q, radius, max_results=3)) == min(3, c)
    assert find_within_radius(space, q, -1.0 if metric == 0 else 1e30) == []


CPP = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "mvf.hpp"
int main(int argc, char** argv) {
    if (argc < 7) return 2;
    auto reader = mvf::MvfReader::open(argv[1]);
    auto space = reader.vector_space(reader.vector_space_names()[0]);
    mvf::GpuVectorSpace gs(space);
    std::vector<float> q = {(float)atof(argv[2]), (float)atof(argv[3]), (float)atof(argv[4]), (float)atof(argv[5])};
    const float radius = (float)atof(argv[6]);
    for (const auto& h : gs.find_within_radius(q, radius, 100)) {
        uint32_t b;
        std::memcpy(&b, &h.score, 4);
        std::printf("%llu:%08x\n", (unsigned long long)h.index, b);
    }
    return 0;
}
'''


def test_cpp_find_within_radius(tmp_path, golden_dir):
    from metrovector_amd import MvfReader, find_within_radius
    src = tmp_path / "radius.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "radius_cpp")
    libdir = os.path.join(ROOT, "metrovector_amd")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                          "-L", libdir, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    path = os.path.join(golden_dir, "clusters_60x4_f32.mvf")
    q, radius = [1.0, 1.0, 1.0, 1.0], 2.5
    run = subprocess.run([exe, path] + [str(v) for v in q] + [str(radius)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [(int(a), int(b, 16)) for a, b in (l.split(":") for l in run.stdout.split())]
    r = MvfReader.open(path)
    want = find_within_radius(r.vector_space(r.vector_space_names()[0]), q, radius, max_results=100, with_vectors=False)
    assert got == [(h.index, int(np.float32(h.score).view(np.uint32))) for h in want]
    assert len(got) >= 1


@pytest.mark.parametrize("metric", METRICS)
def test_batched_route_equals_the_streaming_route(oracle, metric):
    """Float32, 200 queries: the batched route (tombstones, index_base, ids) returns the streaming route's counts, rows and
    score bits, and both agree with the oracle."""
    n, dim, nq = 50021, 96, 200
    rows = oracle.synth_rows(111, 0, n, dim, G.FLOAT32)
    qs = oracle.synth_queries(112, nq, dim, G.FLOAT32)
    dead = np.zeros(n, bool)
    dead[2::9] = True
    all_s = [oracle.scores(rows, G.FLOAT32, metric, q)[0] for q in qs]
    radii = np.array([radius_for_count(all_s[j], metric, (0, 10, 300, 5000)[j % 4], dead=dead) for j in range(nq)], np.float32)
    m = 400
    with G.GpuCorpus.from_array(rows, index_base=5) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        got = c.search_radius(qs, radii, m, metric)
        only = c.search_radius(qs, radii, 0, metric)
        c.set_scan_path(1)
        ref = c.search_radius(qs, radii, m, metric)
    assert (got.counts == ref.counts).all() and (only.counts == got.counts).all()
    assert (got.indices == ref.indices).all() and (got.scores.view(np.uint32) == ref.scores.view(np.uint32)).all()
    sub = G.RadiusResult(got.counts[::7], got.scores[::7], got.indices[::7], got.raw[::7])
    _check(oracle, sub, rows, G.FLOAT32, metric, qs[::7], radii[::7], m, all_s=all_s[::7], dead=dead, index_base=5)
