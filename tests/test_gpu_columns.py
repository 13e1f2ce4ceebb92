"""Metadata columns and filters from predicates on the GPU (mvfgpu_column_*, mvfgpu_filter_create_where; DESIGN.md §3 "Column
filters", §5 "P0"): a where-filter is the same object as the bitmap filter of the restated predicate (tests/_columns.py) -- the
same info, the same admitted rows, byte-identical searches on both routes -- over the bit geometry of P0's words, both column
types, both column forms, extreme values, sets up to the cap, tombstones, base filters, the lifecycle, row-range shards, the
file-to-search path in Python and C++, and one multi-block case."""
import os
import subprocess
import threading

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

from _children import RUNNER
from _columns import OPS, TOP, U32, U64, edge_values, odd_address, where_mask
from _filtered import PAD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "metrovector_amd")
B = 32768  # rows one block of F0 / F1 covers
MASK, LIST = 1, 2
LO, HI = 1000, 2000
OPERAND = {"==": LO, "!=": HI, "<": LO, "<=": LO, ">": HI, ">=": HI, "between": (LO, HI),
           "in": [HI + 1, LO, 1500, LO, 1234, HI + 1], "not in": [LO - 1, HI, 1777, HI]}


def _force(monkeypatch, c, route):
    """MVF_FILTER_ROUTE is read into the handle's tuning; a filter takes it from the handle when it is created."""
    if route is None:
        monkeypatch.delenv("MVF_FILTER_ROUTE", raising=False)
    else:
        monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    c.reload_tuning()


def _same(a, b):
    return (a.indices == b.indices).all() and (a.raw == b.raw).all() and (a.scores.view(np.uint32) == b.scores.view(np.uint32)).all()


def _device_column(c, values):
    import torch
    t = torch.from_numpy(values.view(np.int32 if values.dtype == np.uint32 else np.int64)).cuda()
    col = c.attach_column_device(t.data_ptr(), U32 if values.dtype == np.uint32 else U64)
    torch.cuda.synchronize()
    return col


def _check_pair(c, q, metric, clauses, mask, any=False, base=None, index_base=0, what="", exact_rows=True):  # noqa: A002
    """A where-filter against the bitmap filter of the restated mask: info, admitted rows, byte-identical search."""
    with c.make_filter_where(clauses, any=any, base=base) as fw, c.make_filter(mask) as fb:
        iw, ib = fw.info(), fb.info()
        assert (iw.rows, iw.admitted, iw.has_row_list) == (ib.rows, ib.admitted, ib.has_row_list), what
        assert iw.admitted == int(mask.sum()), what
        k = int(ib.admitted) + 5
        rw, rb = c.search_filtered(q, k, metric, fw), c.search_filtered(q, k, metric, fb)
        assert _same(rw, rb), f"{what}: the where-filter's search differs from the bitmap filter's"
        if exact_rows:
            want = np.nonzero(mask)[0].astype(np.uint64) + np.uint64(index_base)
            got = rw.indices[0]
            assert (np.sort(got[:want.size]) == want).all(), f"{what}: the returned rows are not the admitted live rows"
            assert (got[want.size:] == PAD).all() and np.isinf(rw.scores[0][want.size:]).all(), f"{what}: padding"


# ---- the bit geometry of P0's words ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("data_type", [U32, U64])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025, 32767, 32768, 32769, 2 * B + 33])
def test_geometry_of_every_operator_form_and_combination(oracle, monkeypatch, n, data_type):
    rng = np.random.default_rng(n * 8 + data_type)
    rows = oracle.synth_rows(51, 0, n, 8, 0)
    q = oracle.synth_queries(52, 1, 8, 0)
    va = edge_values(n, data_type, rng)
    vb = edge_values(n, U32 + U64 - data_type, rng)   # the second column has the other type
    dead = np.zeros(n, bool)
    if n > 257:
        dead[rng.random(n) < 0.1] = True
    basem = rng.random(n) < 0.7
    padded = np.concatenate([rng.integers(0, 5000, 37).astype(va.dtype), va, rng.integers(0, 5000, 3).astype(va.dtype)])
    with G.GpuCorpus.from_array(rows, index_base=3) as c:
        if dead.any():
            c.set_tombstones(np.packbits(dead, bitorder="little"))
        forms = {}
        for fv in (0, 1, 37):  # the whole column from an odd byte address, the shard's rows from value fv on
            keep, addr = odd_address(padded[37 - fv:])
            forms[f"host first_value {fv}"] = c.attach_column_pointer(addr, data_type, fv, padded.size - (37 - fv))
            del keep  # the values were copied
        forms["device"] = _device_column(c, va)
        colb = c.attach_column(vb)
        try:
            for name, col in forms.items():
                inf = col.info()
                assert (inf.data_type, inf.rows, inf.device_bytes) == (data_type, n, n * va.itemsize), name
            for route in (MASK, LIST):
                _force(monkeypatch, c, route)
                with c.make_filter(basem) as fbase:
                    for i, op in enumerate(OPS):
                        one = (va, op, OPERAND[op])
                        for name, col in forms.items():
                            _check_pair(c, q, G.L2, [(col, op, OPERAND[op])], where_mask([one], dead=dead), index_base=3,
                                        what=f"route {route} n {n} {op} {name}")
                        # 2 and 8 clauses over both columns, the operators cycling from this one
                        cyc = [OPS[(i + j) % 9] for j in range(8)]
                        spec = [((va, forms["device"]) if j % 2 == 0 else (vb, colb), o, OPERAND[o]) for j, o in enumerate(cyc)]
                        for m in (2, 8):
                            for any_ in (False, True):
                                _check_pair(c, q, G.L2, [(cv[1], o, x) for cv, o, x in spec[:m]],
                                            where_mask([(cv[0], o, x) for cv, o, x in spec[:m]], any=any_, dead=dead), any=any_,
                                            index_base=3, what=f"route {route} n {n} {m} clauses from {op} any={any_}")
                        _check_pair(c, q, G.L2, [(cv[1], o, x) for cv, o, x in spec[:2]],
                                    where_mask([(cv[0], o, x) for cv, o, x in spec[:2]], base=basem, dead=dead), base=fbase,
                                    index_base=3, what=f"route {route} n {n} {op} with a base filter")
        finally:
            for col in list(forms.values()) + [colb]:
                col.close()


# ---- extreme values and operands, sets, empty and full predicates ---------------------------------------------------------

def test_extreme_values_operands_and_sets(oracle):
    n = 4200
    rng = np.random.default_rng(9)
    rows = oracle.synth_rows(53, 0, n, 8, 2)
    q = oracle.synth_queries(54, 1, 8, 2)
    ext = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, TOP - 1, TOP]
    v64 = np.array([ext[i % 7] for i in rng.permutation(n)], np.uint64)
    v32 = np.array([[0, 1, 2 ** 32 - 2, 2 ** 32 - 1][i % 4] for i in rng.permutation(n)], np.uint32)
    spread = rng.permutation(20000)[:n].astype(np.uint64)   # distinct values for the large sets
    with G.GpuCorpus.from_array(rows) as c, c.attach_column(v64) as c64, c.attach_column(v32) as c32, c.attach_column(spread) as csp:
        for vals, col in ((v64, c64), (v32, c32)):
            for op in OPS[:6]:
                for a in (0, 2 ** 32 - 1, 2 ** 32, TOP):
                    _check_pair(c, q, G.INNER_PRODUCT, [(col, op, a)], where_mask([(vals, op, a)]), what=f"{vals.dtype} {op} {a}")
            for a, b in ((0, TOP), (2 ** 32 - 1, 2 ** 32), (2 ** 32, TOP), (TOP, TOP), (TOP, 0), (5, 4), (0, 0)):
                _check_pair(c, q, G.INNER_PRODUCT, [(col, "between", (a, b))], where_mask([(vals, "between", (a, b))]),
                            what=f"{vals.dtype} between {a} {b}")
            for s in ([TOP], [2 ** 32, 0], [TOP, 0, 2 ** 32 - 1, 0, TOP, 2 ** 32], []):
                for op in ("in", "not in"):
                    _check_pair(c, q, G.INNER_PRODUCT, [(col, op, s)], where_mask([(vals, op, s)]), what=f"{vals.dtype} {op} {s}")
        # 4096 distinct values, unsorted and with repeats; one, two; the cap is the call's
        big = rng.permutation(20000)[:4096].astype(np.uint64)
        given = np.concatenate([big, big[:904]])[rng.permutation(5000)]
        for s in (given.tolist(), big[:1].tolist(), big[:2].tolist() * 3):
            for op in ("in", "not in"):
                _check_pair(c, q, G.INNER_PRODUCT, [(csp, op, s)], where_mask([(spread, op, s)]), what=f"{op} with {len(s)} values")
        # three sets in one call, 2048 + 1 + 2047 = the cap of 4096 exactly
        _check_pair(c, q, G.INNER_PRODUCT, [(csp, "in", big[:2048].tolist()), (c64, "not in", [0]), (csp, "in", big[2048:4095].tolist())],
                    where_mask([(spread, "in", big[:2048]), (v64, "not in", [0]), (spread, "in", big[2048:4095])], any=True), any=True,
                    what="three sets of 4096 values together in one call")
        with pytest.raises(E.InvalidArgument, match="4096"):   # ... and one more value is over it
            c.make_filter_where([(csp, "in", big[:2048].tolist()), (c64, "not in", [0]), (csp, "in", big[2048:].tolist())], any=True)
        with pytest.raises(E.InvalidArgument, match="4096"):
            c.make_filter_where([(csp, "in", list(range(4097)))])
        with pytest.raises(E.InvalidArgument, match="4096"):
            c.make_filter_where([(csp, "in", big.tolist()), (c64, "in", [1])])
        # everything and nothing
        with c.make_filter_where([(c64, ">=", 0)]) as f:
            assert f.admitted == n
        with c.make_filter_where([(c64, "<", 0), (c32, "in", [])], any=True) as f:
            assert f.admitted == 0
            res = c.search_filtered(q, 3, G.L2, f)
            assert (res.indices == PAD).all()


# ---- real searches on the route the rule chooses -------------------------------------------------------------------------------

N, DIM, K = 20_011, 96, 33
_CASES = {}


def _case(oracle, dtype):
    hit = _CASES.get(dtype)
    if hit is None:
        rng = np.random.default_rng(61)
        hit = _CASES[dtype] = (oracle.synth_rows(61, 0, N, DIM, dtype), oracle.synth_queries(62, 40, DIM, dtype),
                               rng.integers(0, 10, N).astype(np.uint32), rng.integers(0, 10 ** 12, N).astype(np.uint64),
                               rng.random(N) < 0.2)
    return hit


@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
def test_real_searches_equal_the_bitmap_filters(oracle, dtype):
    """Byte-identical to the bitmap filter's results, whose parity with the oracle tests/test_gpu_filtered.py proves."""
    rows, q, tenant, ts, dead = _case(oracle, dtype)
    with G.GpuCorpus.from_array(rows, index_base=7) as c, c.attach_column(tenant) as ct, c.attach_column(ts) as cs:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        for clauses, spec in (([(ct, "<=", 7), (cs, ">=", 5 * 10 ** 11)], [(tenant, "<=", 7), (ts, ">=", 5 * 10 ** 11)]),     # ~0.4
                              ([(ct, "==", 7), (cs, "<", 10 ** 11)], [(tenant, "==", 7), (ts, "<", 10 ** 11)])):            # ~0.01
            mask = where_mask(spec, dead=dead)
            with c.make_filter_where(clauses) as fw, c.make_filter(mask) as fb:
                assert fw.info().admitted == fb.info().admitted == int(mask.sum()) and fw.info().has_row_list == fb.info().has_row_list
                for metric in (G.L2, G.COSINE):
                    for nq in (1, 40):
                        rw, rb = c.search_filtered(q[:nq], K, metric, fw), c.search_filtered(q[:nq], K, metric, fb)
                        assert _same(rw, rb), f"dtype {dtype} metric {metric} nq {nq} density {mask.mean():.3f}"
                        live = rw.indices[rw.indices != PAD].astype(np.int64) - 7
                        assert mask[live].all()


# ---- lifecycle -----------------------------------------------------------------------------------------------------------------

def test_lifecycle_of_columns_and_where_filters(oracle):
    n = 3000
    rows = oracle.synth_rows(71, 0, n, 8, 0)
    q = oracle.synth_queries(72, 2, 8, 0)
    rng = np.random.default_rng(7)
    v = rng.integers(0, 100, n).astype(np.uint32)
    dead = rng.random(n) < 0.3
    with G.GpuCorpus.from_array(rows) as c, G.GpuCorpus.from_array(rows[:100]) as other:
        col = c.attach_column(v)
        with c.make_filter_where([(col, "<", 50)]) as before, c.make_filter(np.ones(n, bool)) as base_before:
            assert before.admitted == int((v < 50).sum())
            c.set_tombstones(np.packbits(dead, bitorder="little"))     # a new tombstone generation: the column stays valid
            with pytest.raises(E.InvalidArgument, match="stale filter"):
                c.search_filtered(q, 3, G.L2, before)
            with pytest.raises(E.InvalidArgument, match="stale filter"):
                c.make_filter_where([(col, "<", 50)], base=base_before)
            _check_pair(c, q[:1], G.L2, [(col, "<", 50)], (v < 50) & ~dead, what="after set_tombstones")
        # a column or a base of another handle
        with other.attach_column(v[:100].copy()) as ocol, other.make_filter(np.ones(100, bool)) as obase:
            with pytest.raises(E.InvalidArgument, match="another corpus handle"):
                c.make_filter_where([(col, "<", 50), (ocol, "<", 50)])
            with pytest.raises(E.InvalidArgument, match="another corpus handle"):
                c.make_filter_where([(col, "<", 50)], base=obase)
        with pytest.raises(E.InvalidArgument, match="fewer rows"):
            c.attach_column_pointer(v.ctypes.data, U32, 1, n)
        # the filter does not refer to the column after creation
        f = c.make_filter_where([(col, ">=", 90)])
        col.close()
        want = (v >= 90) & ~dead
        res = c.search_filtered(q, int(want.sum()) + 2, G.L2, f)
        assert (np.sort(res.indices[1][:int(want.sum())]) == np.nonzero(want)[0]).all() and (res.indices[:, int(want.sum()):] == PAD).all()
        f.close()
        # two threads, one handle, their own answers
        col = c.attach_column(v)
        got, errs = {}, []

        def work(t):
            try:
                for _ in range(20):
                    with c.make_filter_where([(col, "==", t)]) as ft:
                        got.setdefault(t, set()).add(int(ft.admitted))
            except Exception as e:  # noqa: BLE001 - reported below
                errs.append(e)

        ths = [threading.Thread(target=work, args=(t,)) for t in (3, 4)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        assert not errs, errs
        assert got == {t: {int(((v == t) & ~dead).sum())} for t in (3, 4)}
        col.close()


# ---- row-range shards ------------------------------------------------------------------------------------------------------

def test_two_shards_given_the_whole_column_merge_to_the_one_handle_answer(oracle):
    n, cut, k = 5003, 2777, 20
    rows = oracle.synth_rows(81, 0, n, 16, 2)
    q = oracle.synth_queries(82, 3, 16, 2)
    rng = np.random.default_rng(8)
    v = rng.integers(0, 50, n).astype(np.uint64)
    dead = rng.random(n) < 0.2
    tomb = np.packbits(dead, bitorder="little")
    clause = ("between", (10, 30))
    per = []
    for a, b in ((0, cut), (cut, n)):
        with G.GpuCorpus.from_array(rows[a:b], index_base=a) as c:
            c.set_tombstones(tomb, first_bit=a)
            with c.attach_column(v, first_value=a) as col, c.make_filter_where([(col,) + clause]) as f:
                assert f.admitted == int(where_mask([(v, *clause)], dead=dead)[a:b].sum())
                per.append(c.search_filtered(q, k, G.INNER_PRODUCT, f))
    merged = G.merge_topk_host(np.stack([p.scores for p in per]), np.stack([p.indices for p in per]), np.stack([p.raw for p in per]),
                               G.INNER_PRODUCT, 2)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_tombstones(tomb)
        with c.attach_column(v) as col, c.make_filter_where([(col,) + clause]) as f:
            assert _same(merged, c.search_filtered(q, k, G.INNER_PRODUCT, f))


# ---- from the file to the search ------------------------------------------------------------------------------------------------

def test_find_top_k_where_equals_find_top_k_filtered(tmp_path, oracle):
    n, dim = 700, 12
    rng = np.random.default_rng(10)
    rows = oracle.synth_rows(91, 0, n, dim, 0)
    q = oracle.synth_queries(92, 1, dim, 0)[0]
    tenant = rng.integers(0, 5, n).astype(np.uint32)
    ts = rng.integers(0, 1000, n).astype(np.uint64)
    dead = rng.random(n) < 0.2
    b = M.MvfBuilder()
    b.add_vector_space("s", dim, 0, 0, 0)
    b.add_vectors("s", rows)
    b.set_vector_ids("s", np.arange(n) * 3 + 11)
    b.set_tombstones("s", 1, np.packbits(dead, bitorder="little").tobytes() + b"\0", int(dead.sum()))  # an odd block in front of the columns
    b.add_metadata_column("tenant", U32, tenant.astype("<u4").tobytes())
    b.add_metadata_column("ts", U64, ts.astype("<u8").tobytes())
    b.add_metadata_column("few", U32, tenant[:n - 1].astype("<u4").tobytes())
    b.add_metadata_column("label", 6, b"x" * (4 * n))
    path = str(tmp_path / "where.mvf")
    b.build().save(path)
    with M.MvfReader.open(path) as r:
        space = r.vector_space("s")
        for where, any_, mask in (({"tenant": ("==", 3), "ts": (">=", 400)}, False, (tenant == 3) & (ts >= 400)),
                                  ({"tenant": ("in", [0, 4]), "ts": ("between", (100, 150))}, True, np.isin(tenant, [0, 4]) | ((ts >= 100) & (ts <= 150))),
                                  ({"ts": ("<", 0)}, False, np.zeros(n, bool))):
            got = M.find_top_k_where(space, q, 15, where, any=any_)
            want = M.find_top_k_filtered(space, q, 15, mask)
            assert [(g.index, g.score) for g in got] == [(w.index, w.score) for w in want] and len(got) == (15 if mask.any() else 0)
            assert all((g.vector == w.vector).all() for g, w in zip(got, want))
        # a corpus that holds a row range reads its own part of the columns
        with M.upload_space(space, first=300, count=250) as c:
            got = M.find_top_k_where(space, q, 9, {"tenant": ("!=", 2)}, corpus=c)
            want = M.find_top_k_filtered(space, q, 9, tenant != 2, corpus=c)
            assert [(g.index, g.score) for g in got] == [(w.index, w.score) for w in want] and len(got) == 9
        with pytest.raises(E.BuildError, match="holds 699 values"):
            M.find_top_k_where(space, q, 3, {"few": ("==", 1)})
        with pytest.raises(E.BuildError, match="Unsupported metadata column data type"):
            M.find_top_k_where(space, q, 3, {"label": ("==", 1)})
        with pytest.raises(E.VectorSpaceNotFound, match="Metadata column not found"):
            M.find_top_k_where(space, q, 3, {"nope": ("==", 1)})


_CPP = r"""
#include "mvf.hpp"
#include <cstdio>
int main(int argc, char** argv) {
    using namespace mvf;
    if (argc < 2) return 2;
    try {
        std::vector<std::vector<float>> rows;
        std::vector<uint32_t> tenant;
        std::vector<uint64_t> ts;
        for (int i = 0; i < 60; i++) {
            rows.push_back({(float)i, 1.0f, 0.0f, 0.0f});
            tenant.push_back((uint32_t)(i % 5));
            ts.push_back(1000ull + (uint64_t)i);
        }
        MvfBuilder b;
        b.add_vector_space("s", 4, VectorType::Dense, DistanceMetric::L2, DataType::Float32);
        b.add_vectors("s", rows);
        b.add_metadata_column("tenant", tenant).add_metadata_column("ts", ts);
        b.add_metadata_column("short", std::vector<uint32_t>(59, 0));
        b.build().save(argv[1]);
        MvfReader r = MvfReader::open(argv[1]);
        const GpuVectorSpace resident(r.vector_space("s"));
        WhereClause t{r.metadata_column("tenant"), MVFGPU_OP_EQ, 0, 0, {}};           // rows 0, 5, .., 55
        WhereClause late{r.metadata_column("ts"), MVFGPU_OP_GE, 1020, 0, {}};         // rows 20 ..
        for (const ScoredVector& v : resident.find_top_k_where({21.0f, 1.0f, 0.0f, 0.0f}, 4, {t, late})) std::printf("%llu:%.1f ", (unsigned long long)v.index, v.score);
        std::printf("\n");
        std::printf("%zu\n", resident.find_top_k_where({21.0f, 1.0f, 0.0f, 0.0f}, 40, {t, late}).size());
        WhereClause in{r.metadata_column("tenant"), MVFGPU_OP_IN, 0, 0, {4, 1, 4}};
        std::printf("%zu\n", resident.find_top_k_where({21.0f, 1.0f, 0.0f, 0.0f}, 60, {in, late}, true).size());
        try { resident.find_top_k_where({1, 1, 1, 1}, 1, {{r.metadata_column("short"), MVFGPU_OP_EQ, 0, 0, {}}}); } catch (const MvfError&) { std::printf("short column refused\n"); }
        try { r.metadata_column("nope"); } catch (const MvfError& e) { std::printf("%d\n", e.code()); }
    } catch (const MvfError& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
"""


def test_cpp_find_top_k_where(tmp_path):
    src, exe = tmp_path / "where.cpp", str(tmp_path / "where_cpp")
    src.write_text(_CPP)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", LIBDIR, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe, str(tmp_path / "where.mvf")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ["20:1.0", "25:4.0", "30:9.0", "35:14.0"]
    assert lines[1] == "8"                       # 20, 25, .., 55
    assert lines[2] == str(24 + 40 - 16)         # tenant in {1, 4}: 24 rows; ts >= 1020: 40 rows; both: 16
    assert lines[3] == "short column refused" and lines[4] == "4"


@pytest.mark.parametrize("poison", [None, 0x00, 0xFF])
def test_cpp_find_top_k_where_with_poisoned_allocations(tmp_path, poison):
    """The same executable, its process started with every allocation of the library filled with a byte before its first use
    (MVF_DEBUG_POISON): the answer does not depend on what the memory held."""
    src, exe = tmp_path / "where.cpp", str(tmp_path / "where_cpp")
    src.write_text(_CPP)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", LIBDIR, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    env = {k: v for k, v in os.environ.items() if k != "MVF_DEBUG_POISON"}
    if poison is not None:
        env["MVF_DEBUG_POISON"] = str(poison)
    out = RUNNER.run([exe, str(tmp_path / "where.mvf")], env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ["20:1.0", "25:4.0", "30:9.0", "35:14.0"]
    assert lines[1] == "8"                       # 20, 25, .., 55
    assert lines[2] == str(24 + 40 - 16)         # tenant in {1, 4}: 24 rows; ts >= 1020: 40 rows; both: 16
    assert lines[3] == "short column refused" and lines[4] == "4"


# ---- one larger case: several blocks of P0 and of F0 -----------------------------------------------------------------------------

def test_a_million_rows_three_clauses(oracle):
    n = 1_000_003
    rng = np.random.default_rng(12)
    rows = rng.integers(-128, 128, (n, 8), dtype=np.int8)
    q = oracle.synth_queries(93, 2, 8, 2)
    v = rng.integers(0, 2 ** 40, n).astype(np.uint64)
    w = rng.integers(0, 1000, n).astype(np.uint64)
    dead = rng.random(n) < 0.1
    with G.GpuCorpus.from_array(rows) as c, c.attach_column(v) as cv, c.attach_column(w) as cw:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        clauses = [(cv, ">=", 2 ** 39), (cw, "in", list(range(0, 1000, 7))), (cw, "!=", 21)]
        mask = where_mask([(v, ">=", 2 ** 39), (w, "in", list(range(0, 1000, 7))), (w, "!=", 21)], dead=dead)
        with c.make_filter_where(clauses) as fw, c.make_filter(mask) as fb:
            iw, ib = fw.info(), fb.info()
            assert (iw.rows, iw.admitted, iw.has_row_list) == (ib.rows, ib.admitted, ib.has_row_list) and iw.admitted == int(mask.sum())
            assert _same(c.search_filtered(q, 100, G.INNER_PRODUCT, fw), c.search_filtered(q, 100, G.INNER_PRODUCT, fb))
        with c.make_filter_where(clauses, any=True) as fw:
            assert fw.admitted == int(where_mask([(v, ">=", 2 ** 39), (w, "in", list(range(0, 1000, 7))), (w, "!=", 21)], any=True, dead=dead).sum())
