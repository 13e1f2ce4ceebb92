"""-m gpu tests of the partitioned search (DESIGN.md §3 "Partitioned search"): the index against numpy's group-by, and every
batch against both identities of the contract -- byte for byte the candidate search's row for the explicit list of the key's
rows, and the one-query filtered search's row through `column == key` -- and against the CPU oracle on the key's rows.
tests/_partitioned.py holds the layout: 8192 rows, partitions of 3000 .. 1 live rows scattered over all positions."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _partitioned as P
from _candidates import oracle_candidates
from _children import RUNNER
from _util import PAD, assert_float_topk
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "metrovector_amd")
L2, IP, COS = 0, 1, 2
CODE = {"f32": 0, "f16": 1, "i8": 2, "u8": 3}
INT = ("i8", "u8")

# (rows' type, dimension, metric): the handle's lane-group widths of one query -- 1 lane (dim 4), 32 (100), 64 (768) -- every
# type, and all three metrics on one float and one integer shape
CASES = [("f32", 4, L2), ("f32", 8, COS), ("f32", 100, L2), ("f32", 100, IP), ("f32", 100, COS), ("f32", 768, L2),
         ("f16", 128, IP), ("i8", 64, L2), ("i8", 64, IP), ("i8", 64, COS), ("u8", 200, L2)]


class World:
    """one corpus of the layout with its column and index, and the references the checks share"""

    def __init__(self, dt, dim, flavour, index_base=0, ids=None, n=P.N, lay=None):
        self.dt, self.dim, self.base, self.ids = dt, dim, index_base, ids
        self.lay = lay or P.layout(flavour)
        self.rows = P.make_rows(n, dim, dt)
        self.rows_f32 = self.rows.astype(np.float32) if dt not in INT else None
        self.c = G.GpuCorpus.from_array(self.rows, index_base=index_base)
        self.c.set_tombstones(np.packbits(self.lay["dead"], bitorder="little"))
        if ids is not None:
            self.c.set_vector_ids(ids)
            self.row_of_id = {int(v): r for r, v in enumerate(ids.tolist())}
        self.col = self.c.attach_column(self.lay["col"])
        self.part = self.c.make_partition(self.col)
        self._refs, self._filters = {}, {}

    def ref(self, key):
        key = int(key)
        if key not in self._refs:
            self._refs[key] = P.reference_rows(self.lay, key)
        return self._refs[key]

    def flt(self, key):
        key = int(key)
        if key not in self._filters:
            self._filters[key] = self.c.make_filter_where([(self.col, "==", key)])
        return self._filters[key]

    def entries(self, rows):
        return self.ids[rows] if self.ids is not None else rows.astype(np.uint64) + np.uint64(self.base)

    def local(self, idx):
        if self.ids is not None:
            return np.array([self.row_of_id[int(v)] for v in idx.tolist()], np.int64)
        return (idx - np.uint64(self.base)).astype(np.int64)

    def close(self):
        for f in self._filters.values():
            f.close()
        self.part.close()
        self.col.close()
        self.c.close()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(dt, dim, flavour):
        if (dt, dim, flavour) not in made:
            made[dt, dim, flavour] = World(dt, dim, flavour)
        return made[dt, dim, flavour]
    yield get
    for w in made.values():
        w.close()


def same_bytes(a, b, what):
    assert (a.indices == b.indices).all(), f"{what}: indices"
    assert (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all(), f"{what}: score bits"
    assert (a.raw == b.raw).all(), f"{what}: raw"


def check_batch(oracle, w, q, keys, k, metric, what):
    """one partitioned search against identity 1 (every query), identity 2 (at most 12 queries) and the oracle (every query)"""
    keys = np.asarray(keys, np.uint64)
    nq = q.shape[0]
    res = w.c.search_partitioned(q, keys, k, metric, w.part)
    assert res.scores.shape == res.indices.shape == res.raw.shape == (nq, k)
    refs = [w.ref(key) for key in keys]
    # 1. the candidate search's rows for the explicit lists
    cand = np.full((nq, max(1, max(r.size for r in refs))), PAD, np.uint64)
    for j, r in enumerate(refs):
        cand[j, :r.size] = w.entries(r)
    same_bytes(res, w.c.search_candidates(q, cand, k, metric), f"{what}: identity 1")
    # 2. one query through the filter of its key
    rng = np.random.default_rng(P._seed("sample", what))
    for j in sorted(rng.permutation(nq)[:12].tolist()):
        one = w.c.search_filtered(q[j:j + 1], k, metric, w.flt(keys[j]))
        assert (one.indices[0] == res.indices[j]).all() and (one.raw[0] == res.raw[j]).all() and \
            (one.scores[0].view(np.uint32) == res.scores[j].view(np.uint32)).all(), f"{what}: identity 2, query {j} (key {int(keys[j]):#x})"
    # the oracle on the key's rows
    code = CODE[w.dt]
    pad = np.inf if metric == L2 else -np.inf
    for j, r in enumerate(refs):
        real = min(k, r.size)
        assert (res.indices[j, real:] == PAD).all() and (res.scores[j, real:] == pad).all() and (res.raw[j, real:] == 0).all(), \
            f"{what}: padding of query {j}"
        assert (res.indices[j, :real] != PAD).all(), f"{what}: query {j} holds {r.size} rows"
        if r.size == 0:
            continue
        if w.dt in INT:
            _, s, i, rw = oracle_candidates(oracle, w.rows, code, metric, q[j], w.entries(r), k, index_base=w.base, ids=w.ids)
            assert (res.indices[j] == i).all() and (res.raw[j] == rw).all() and \
                (res.scores[j].view(np.uint32) == s.view(np.uint32)).all(), f"{what}: oracle, query {j}"
        else:
            loc = w.local(res.indices[j, :real])
            pos = np.searchsorted(r, loc)
            assert (pos < r.size).all() and (r[np.minimum(pos, r.size - 1)] == loc).all(), f"{what}: query {j} returned a row of another key"
            sub_idx = np.concatenate([pos.astype(np.uint64), res.indices[j, real:]])
            assert (res.raw[j] == 0).all()
            all_s = oracle.scores(w.rows[r], code, metric, q[j])[0]
            assert_float_topk(metric, res.scores[j], sub_idx, all_s, w.rows_f32[r], q[j], k)
    return res


def batches(w):
    """(name, queries' keys, k) of every batch of a shape"""
    lay = w.lay
    big, small64, small300 = lay["keys"][0], lay["keys"][5], lay["keys"][4]
    yield "q1_small", [small300], 10
    yield "q1_big", [big], 10
    yield "q7_one_key", [big] * 7, 10          # a group of four queries and a rest
    yield "q7_one_small_key", [lay["keys"][2]] * 7, 10
    yield "q64_mixed_k10", P.mixed_keys(lay, 64), 10
    yield "q64_mixed_k100", P.mixed_keys(lay, 64), 100   # pads on the small partitions
    yield "k1025", [small64, big], 1025        # beyond one pass: the large tier's dump ending


@pytest.mark.parametrize("flavour", ["u32", "u64"])
def test_the_index_is_the_columns_group_by_over_the_live_rows(worlds, flavour):
    w = worlds("i8", 64, flavour)
    lay = w.lay
    inf = w.part.info()
    keys, counts = P.group_by(lay)
    assert inf.key_type == (4 if flavour == "u32" else 5) and inf.rows == P.N
    assert inf.live_rows == int((~lay["dead"]).sum()) and inf.n_keys == keys.size and inf.largest == 3000
    assert inf.device_bytes == 4 * inf.live_rows + 8 * (2 * inf.n_keys + 1) and inf.host_bytes == 8 * (2 * inf.n_keys + 1)
    gk, gc = w.part.keys()
    assert (gk == keys).all() and (gc == counts).all()
    assert lay["dead_key"] not in gk.tolist(), "a key whose rows are all deleted is no key"
    ask = np.array(list(lay["all_keys"]) + [lay["dead_key"], lay["absent_key"], (1 << 64) - 2], np.uint64)
    want = np.array([P.reference_rows(lay, int(a)).size for a in ask], np.uint64)
    assert (w.part.lookup(ask) == want).all()
    if flavour == "u32":  # 64-bit comparison on the zero-extended value
        assert w.part.lookup([(1 << 32) | 7, 1 << 32]).tolist() == [0, 0]
    one = np.zeros(1, np.uint64)
    with pytest.raises(E.InvalidArgument, match="exceeds the partition's"):  # [first, first + count) must lie inside n_keys
        _lib.gpu_check(_lib.gpu().mvfgpu_partition_keys(w.part._h, inf.n_keys, 1, one.ctypes.data, one.ctypes.data))


# The pair sort over many tiles: 18 (36 000 live rows of 40 000) for every kind of tests/_partitioned.py's wide layouts, and
# the u64 keys of two differing digits with exactly 18 full tiles and one pair more
WIDE = [(kind, None) for kind in P.WIDE_KINDS] + [("u64_two_digits", 18 * P.SORT_TILE), ("u64_two_digits", 18 * P.SORT_TILE + 1)]


@pytest.mark.parametrize("kind,live", WIDE, ids=[f"{kind}-{live or 'tenth_dead'}" for kind, live in WIDE])
def test_an_index_over_many_sort_tiles_is_the_group_by_and_serves_the_candidate_searchs_bytes(kind, live):
    lay = P.wide_layout(kind, live=live)
    keys, counts = P.group_by(lay)
    n_live = int((~lay["dead"]).sum())
    assert n_live == (live or 36_000) and -(-n_live // P.SORT_TILE) >= 18
    if kind in ("u64_two_digits", "u32_random"):
        assert keys.size == P.WIDE_KEYS and 0.68 < counts.max() / n_live < 0.72
        differ = int(np.bitwise_or.reduce(keys) ^ np.bitwise_and.reduce(keys))
        digits = [d for d in range(8) if (differ >> (8 * d)) & 255]
        assert digits == ([0, 7] if kind == "u64_two_digits" else [0, 1, 2, 3]), "the digits the build sorts by"
    else:
        assert keys.size == (1 if kind == "one_key" else n_live)
    w = World("i8", 16, None, n=P.WIDE_N, lay=lay)
    try:
        inf = w.part.info()
        assert (inf.rows, inf.live_rows, inf.n_keys, inf.largest) == (P.WIDE_N, n_live, keys.size, int(counts.max()))
        gk, gc = w.part.keys()
        assert (gk == keys).all() and (gc == counts).all()
        ask = np.concatenate([keys[:2000], lay["col"][lay["dead"]][:200].astype(np.uint64), np.array([(1 << 64) - 2], np.uint64)])
        want = np.array([counts[i] if i < keys.size and keys[i] == a else 0 for a, i in zip(ask, np.searchsorted(keys, ask))], np.uint64)
        assert (w.part.lookup(ask) == want).all()
        picked = P.sample_keys(lay)
        assert lay["big"] is None or lay["big"] in picked
        q = P.make_queries(len(picked), 16, "i8")
        for j, key in enumerate(picked):
            r = w.ref(key)
            k = min(r.size, 1024)
            res = w.c.search_partitioned(q[j:j + 1], [key], k, L2, w.part)
            same_bytes(res, w.c.search_candidates(q[j:j + 1], w.entries(r)[None, :], k, L2), f"{kind}, key {key:#x} ({r.size} rows)")
            assert (res.indices[0] != PAD).all()
    finally:
        w.close()


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{dt}d{dim}m{m}" for dt, dim, m in CASES])
def test_every_batch_equals_the_candidate_search_the_filtered_search_and_the_oracle(oracle, worlds, case):
    dt, dim, metric = CASES[case]
    w = worlds(dt, dim, "u64" if case % 2 else "u32")
    for name, keys, k in batches(w):
        q = P.make_queries(len(keys), dim, dt)
        check_batch(oracle, w, q, keys, k, metric, f"{dt} x {dim}, metric {metric}, {name}")


def test_more_queries_than_one_window(oracle, worlds):
    w = worlds("f32", 8, "u32")
    lay = w.lay
    rng = np.random.default_rng(5)
    pool = np.array(list(lay["all_keys"]) + [lay["absent_key"], lay["dead_key"]], np.uint64)
    keys = pool[rng.integers(0, pool.size, 1500)]
    check_batch(oracle, w, P.make_queries(1500, 8, "f32"), keys, 10, L2, "1500 queries")


def test_a_host_window_beyond_the_pinned_mirrors_equals_its_pinned_slices(worlds):
    """256 queries at k = 300 are 256 x 300 x 16 B = 1.17 MiB of results: over the 1 MiB up to which a host window travels
    through the handle's pinned mirrors, so the call copies from and to the caller's buffers.  Slices of 32 queries (150 KiB)
    take the mirrors; a query's row does not depend on its batch, so every byte is the same."""
    w = worlds("f32", 8, "u32")
    nq, k = 256, 300
    assert nq * k * 16 > 1 << 20 >= 32 * (k * 16 + 8 * 4)
    q, keys = P.make_queries(nq, 8, "f32"), P.mixed_keys(w.lay, nq)
    assert w.lay["absent_key"] in keys.tolist()
    whole = w.c.search_partitioned(q, keys, k, L2, w.part)
    for j0 in range(0, nq, 32):
        part = w.c.search_partitioned(q[j0:j0 + 32], keys[j0:j0 + 32], k, L2, w.part)
        for name in ("scores", "indices", "raw"):
            assert getattr(whole, name)[j0:j0 + 32].tobytes() == getattr(part, name).tobytes(), f"{name} of queries from {j0}"


def test_vector_ids_and_index_base(oracle):
    ids = (np.random.default_rng(3).permutation(P.N).astype(np.uint64) * np.uint64(7) + np.uint64(5))
    w = World("i8", 64, "u64", index_base=1000, ids=ids)
    try:
        q = P.make_queries(64, 64, "i8")
        res = check_batch(oracle, w, q, P.mixed_keys(w.lay, 64), 10, L2, "ids")
        real = res.indices[res.indices != PAD]
        assert real.size and np.isin(real, ids).all(), "results carry vector ids"
    finally:
        w.close()
    w = World("f32", 100, "u32", index_base=1000)
    try:
        res = check_batch(oracle, w, P.make_queries(64, 100, "f32"), P.mixed_keys(w.lay, 64), 10, COS, "index_base")
        real = res.indices[res.indices != PAD]
        assert real.min() >= 1000 and real.max() < 1000 + P.N
    finally:
        w.close()


def test_a_query_beyond_the_lds_budget(oracle):
    """Float32 300 x 12296: the padded query takes more than 40 KiB, so both partitions are planned into the large tier"""
    n, dim = 300, 12296
    col = np.full(n, 9, np.uint32)
    col[np.random.default_rng(8).permutation(n)[:50]] = 4
    lay = dict(col=col, dead=np.zeros(n, bool))
    w = World("f32", dim, "u32", n=n, lay=lay)
    try:
        assert w.part.info().n_keys == 2 and w.part.info().largest == 250
        check_batch(oracle, w, P.make_queries(2, dim, "f32"), [4, 9], 10, L2, "wide query")
    finally:
        w.close()


def test_empty_indexes_answer_with_padding():
    rows = P.make_rows(100, 16, "i8")
    with G.GpuCorpus.from_array(rows) as c:
        c.set_tombstones(np.full(13, 0xFF, np.uint8))
        with c.attach_column(np.arange(100, dtype=np.uint32)) as col, c.make_partition(col) as part:
            inf = part.info()
            assert (inf.live_rows, inf.n_keys, inf.largest) == (0, 0, 0) and part.keys()[0].size == 0
            res = c.search_partitioned(P.make_queries(3, 16, "i8"), [0, 1, 2], 5, L2, part)
            assert (res.indices == PAD).all() and np.isposinf(res.scores).all() and (res.raw == 0).all()


def test_staleness_ownership_and_argument_checks(oracle):
    lay = P.layout("u32")
    rows = P.make_rows(P.N, 64, "i8")
    q = P.make_queries(4, 64, "i8")
    keys = [lay["keys"][0], lay["keys"][4], lay["keys"][5], lay["absent_key"]]
    with G.GpuCorpus.from_array(rows) as c, G.GpuCorpus.from_array(rows[:100]) as other:
        c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        before = c.search(q, 10, L2)
        with c.attach_column(lay["col"]) as col, other.attach_column(lay["col"][:100].copy()) as ocol:
            part = c.make_partition(col)
            opart = other.make_partition(ocol)
            first = c.search_partitioned(q, keys, 10, L2, part)
            with pytest.raises(E.InvalidArgument, match="another corpus handle"):
                c.make_partition(ocol)
            with pytest.raises(E.InvalidArgument, match="another corpus handle"):
                c.search_partitioned(q, keys, 10, L2, opart)
            with pytest.raises(E.DimensionMismatch):
                c.search_partitioned(q[:, :63], keys, 10, L2, part)
            with pytest.raises(E.BuildError):
                c.search_partitioned(q.astype(np.float32), keys, 10, L2, part)
            with pytest.raises(E.InvalidArgument):
                c.search_partitioned(q, keys[:3], 10, L2, part)
            # the handle's plain search answers as before
            again = c.search(q, 10, L2)
            same_bytes(before, again, "a plain search after partitioned ones")
            # new tombstones: the old index is stale, a new one excludes the newly deleted rows
            gone = P.reference_rows(lay, keys[1])[:7]
            dead2 = lay["dead"].copy()
            dead2[gone] = True
            c.set_tombstones(np.packbits(dead2, bitorder="little"))
            with pytest.raises(E.InvalidArgument, match="stale partition: mvfgpu_corpus_set_tombstones changed the handle's tombstones"):
                c.search_partitioned(q, keys, 10, L2, part)
            with c.make_partition(col) as part2:
                assert part2.info().live_rows == part.info().live_rows - 7 and part2.lookup([keys[1]])[0] == 300 - 7
                second = c.search_partitioned(q, keys, 10, L2, part2)
                assert not np.isin(second.indices, gone.astype(np.uint64)).any()
                same_bytes(G.SearchResult(first.scores[[0, 2, 3]], first.indices[[0, 2, 3]], first.raw[[0, 2, 3]]),
                           G.SearchResult(second.scores[[0, 2, 3]], second.indices[[0, 2, 3]], second.raw[[0, 2, 3]]), "untouched keys")
                lay2 = dict(lay, dead=dead2)
                _, s, i, rw = oracle_candidates(oracle, rows, 2, L2, q[1], P.reference_rows(lay2, keys[1]).astype(np.uint64), 10)
                assert (second.indices[1] == i).all() and (second.raw[1] == rw).all()
            part.close()
            opart.close()


def test_device_call_equals_the_host_call(worlds):
    import torch
    w = worlds("f32", 100, "u32")
    q = P.make_queries(64, 100, "f32")
    keys = P.mixed_keys(w.lay, 64)
    for k in (10, 1025):
        host = w.c.search_partitioned(q, keys, k, COS, w.part)
        dq = torch.from_numpy(q).cuda()
        ds = torch.empty((64, k), dtype=torch.float32, device="cuda")
        di = torch.empty((64, k), dtype=torch.int64, device="cuda")
        dr = torch.empty((64, k), dtype=torch.int32, device="cuda")
        w.c.search_partitioned_device(w.part, dq.data_ptr(), 0, 100, 64, keys, k, COS, ds.data_ptr(), di.data_ptr(), dr.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        same_bytes(host, G.SearchResult(ds.cpu().numpy(), di.cpu().numpy().view(np.uint64), dr.cpu().numpy()), f"device call, k {k}")


def test_a_fresh_process_gives_the_checked_answer_whatever_its_allocations_held(oracle, worlds, tmp_path):
    """the scenario of tests/_partitioned.py as the first device work of a child: twice plain, then with every allocation of
    the library filled with 0x00 and with 0xFF; one child at a time, none after a fault"""
    inp = P.fresh_inputs()
    w = worlds("f32", P.FP_DIM, "u32")
    assert (w.rows == inp["rows"]).all() and (w.lay["col"] == inp["lay"]["col"]).all()
    res = check_batch(oracle, w, inp["queries"], inp["keys"], P.FP_K, P.FP_METRIC, "fresh process, in this process")
    want = P.digest(res.scores, res.indices, res.raw)
    for tag, poison in (("plain1", None), ("plain2", None), ("poison00", 0), ("poisonFF", 255)):
        env = {k: v for k, v in os.environ.items() if k not in ("MVF_DEBUG_POISON", "MVF_FILTER_ROUTE", "MVF_LARGE_K")}
        if poison is not None:
            env["MVF_DEBUG_POISON"] = str(poison)
        path = str(tmp_path / f"{tag}.npz")
        out = RUNNER.run([sys.executable, os.path.join(HERE, "_partitioned.py"), path], env=env)
        assert out.returncode == 0, f"{tag}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
        with np.load(path) as z:
            assert z["poison"].tolist() == [-1 if poison is None else poison], f"{tag}: the child's poison byte"
            for call in ("host", "device"):
                got = P.digest(z[call + ".scores"], z[call + ".indices"], z[call + ".raw"])
                assert got == want, f"{tag}: the {call} call's answer differs from the checked one"


_CPP = r"""
#include "mvf.hpp"
#include <cstdio>
int main(int argc, char** argv) {
    using namespace mvf;
    if (argc < 2) return 2;
    try {
        std::vector<std::vector<float>> rows;
        std::vector<uint32_t> tenant;
        for (int i = 0; i < 60; i++) {
            rows.push_back({(float)i, 1.0f, 0.0f, 0.0f});
            tenant.push_back((uint32_t)(i % 5));
        }
        MvfBuilder b;
        b.add_vector_space("s", 4, VectorType::Dense, DistanceMetric::L2, DataType::Float32);
        b.add_vectors("s", rows);
        b.add_metadata_column("tenant", tenant);
        b.add_metadata_column("short", std::vector<uint32_t>(59, 0));
        b.build().save(argv[1]);
        MvfReader r = MvfReader::open(argv[1]);
        const GpuVectorSpace resident(r.vector_space("s"));
        const std::vector<float> queries = {21.0f, 1.0f, 0.0f, 0.0f, 3.0f, 1.0f, 0.0f, 0.0f, 3.0f, 1.0f, 0.0f, 0.0f};
        for (const auto& hits : resident.find_top_k_per_key(queries, {0, 3, 7}, 4, r.metadata_column("tenant"))) {
            for (const ScoredVector& v : hits) std::printf("%llu:%.1f ", (unsigned long long)v.index, v.score);
            std::printf("|\n");
        }
        std::printf("%zu\n", resident.find_top_k_per_key(queries, {1, 1, 1}, 40, r.metadata_column("tenant"))[2].size());
        try { resident.find_top_k_per_key(queries, {1, 1, 1}, 4, r.metadata_column("short")); } catch (const MvfError&) { std::printf("short column refused\n"); }
        try { resident.find_top_k_per_key(queries, {1, 1}, 4, r.metadata_column("tenant")); } catch (const MvfError&) { std::printf("two keys for three queries refused\n"); }
    } catch (const MvfError& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
"""


def test_cpp_find_top_k_per_key(tmp_path):
    src, exe = tmp_path / "per_key.cpp", str(tmp_path / "per_key_cpp")
    src.write_text(_CPP)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", LIBDIR, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = RUNNER.run([exe, str(tmp_path / "per_key.mvf")])
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ["20:1.0", "25:4.0", "15:6.0", "30:9.0", "|"]
    assert lines[1].split() == ["3:0.0", "8:5.0", "13:10.0", "18:15.0", "|"]
    assert lines[2].split() == ["|"], "no vector carries key 7"
    assert lines[3] == "12" and lines[4] == "short column refused" and lines[5] == "two keys for three queries refused"


def test_find_top_k_per_key_reads_the_files_column(tmp_path, oracle):
    import metrovector_amd as M
    n, dim = 700, 12
    rng = np.random.default_rng(10)
    rows = oracle.synth_rows(91, 0, n, dim, 0)
    q = oracle.synth_queries(92, 6, dim, 0)
    tenant = rng.integers(0, 5, n).astype(np.uint64) << np.uint64(31)
    dead = rng.random(n) < 0.2
    b = M.MvfBuilder()
    b.add_vector_space("s", dim, 0, 0, 0)
    b.add_vectors("s", rows)
    b.set_tombstones("s", 1, np.packbits(dead, bitorder="little").tobytes() + b"\0", int(dead.sum()))  # an odd block in front of the column
    b.add_metadata_column("tenant", 5, tenant.astype("<u8").tobytes())
    b.add_metadata_column("few", 4, np.zeros(n - 1, "<u4").tobytes())
    b.add_metadata_column("label", 6, b"x" * (4 * n))
    path = str(tmp_path / "per_key.mvf")
    b.build().save(path)
    keys = [0, 1 << 31, 4 << 31, 3 << 31, 9, 1 << 31]
    with M.MvfReader.open(path) as r:
        space = r.vector_space("s")
        got = M.find_top_k_per_key(space, q, keys, 15, column="tenant")
        for j, key in enumerate(keys):
            want = M.find_top_k_filtered(space, q[j], 15, tenant == np.uint64(key))
            real = got.indices[j] != PAD
            assert [(int(i), float(s)) for i, s in zip(got.indices[j][real], got.scores[j][real])] == [(v.index, v.score) for v in want]
            assert int(real.sum()) == (0 if key == 9 else 15)
        with M.upload_space(space, first=300, count=250) as c:  # a corpus that holds a row range reads its own part
            got = M.find_top_k_per_key(space, q[:2], keys[:2], 9, column="tenant", corpus=c)
            for j in range(2):
                want = M.find_top_k_filtered(space, q[j], 9, tenant == np.uint64(keys[j]), corpus=c)
                assert [(int(i), float(s)) for i, s in zip(got.indices[j], got.scores[j])] == [(v.index, v.score) for v in want]
        with pytest.raises(E.BuildError, match="holds 699 values"):
            M.find_top_k_per_key(space, q, keys, 3, column="few")
        with pytest.raises(E.BuildError, match="Unsupported metadata column data type"):
            M.find_top_k_per_key(space, q, keys, 3, column="label")
        with pytest.raises(E.VectorSpaceNotFound, match="Metadata column not found"):
            M.find_top_k_per_key(space, q, keys, 3, column="nope")
