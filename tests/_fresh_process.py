"""Scenarios whose device calls are the FIRST device work of a process (tests/test_gpu_fresh_process.py starts this file as a
child: `python tests/_fresh_process.py <scenario> <out.npz>`).

Every other GPU test runs inside one long-lived Python process, where the library's scratch is recycled from its own earlier,
benign contents and where dozens of plain searches precede every filter, candidate, radius or join call.  A scenario here
builds its inputs from fixed numpy seeds, performs its calls in a fixed order and saves every output array -- together with
mvfgpu_selftest_poison(), so that the parent can tell that a child really ran with MVF_DEBUG_POISON set (DESIGN.md §2,
"Poisoned allocations").  The parent imports this module too: the inputs and the order of the calls are stated once, here.

Imports metrovector_amd and numpy only (and the standard library); as a child it also keeps the binding from loading torch, so the library binds to the
platform's HIP runtime as a C or C++ consumer's process does.
"""
import os
import sys
import zlib

import numpy as np

DT = {"f32": (np.float32, 0), "f16": (np.float16, 1), "i8": (np.int8, 2), "u8": (np.uint8, 3)}
L2, IP, COS = 0, 1, 2
METRICS = (L2, IP, COS)
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)

# rows of exactly one 16-byte pitch, and rows shorter than their pitch (the padding bytes matter)
EXACT_FIT = (("f32", 4), ("f16", 8), ("i8", 16), ("u8", 16))
SHORT = (("f32", 3), ("f16", 5), ("i8", 9))
S2_SHAPES = EXACT_FIT + SHORT
S2_ROWS, S2_BASE = 97, 3


def shape_name(dt, dim):
    return f"{dt}d{dim}"


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def make_rows(tag, n, dim, dt):
    """n x dim rows of `dt`: small integers for the integer types (ties happen), unit normals for the float types."""
    rng = np.random.default_rng(_seed("rows", tag, n, dim, dt))
    if dt == "i8":
        return rng.integers(-128, 128, (n, dim)).astype(np.int8)
    if dt == "u8":
        return rng.integers(0, 256, (n, dim)).astype(np.uint8)
    return rng.standard_normal((n, dim)).astype(DT[dt][0])


def make_queries(tag, nq, dim, dt):
    """Float32 queries for the float spaces, the space's own type for the integer ones."""
    rng = np.random.default_rng(_seed("queries", tag, nq, dim, dt))
    if dt == "i8":
        return rng.integers(-128, 128, (nq, dim)).astype(np.int8)
    if dt == "u8":
        return rng.integers(0, 256, (nq, dim)).astype(np.uint8)
    return rng.standard_normal((nq, dim)).astype(np.float32)


def exactly(tag, n, count):
    """bool[n] with exactly `count` rows set"""
    rng = np.random.default_rng(_seed("mask", tag, n, count))
    m = np.zeros(n, bool)
    m[rng.permutation(n)[:count]] = True
    return m


# ---- S1: the failing C++ consumer's shape -------------------------------------------------------------------------------------
S1_KS = (4, 40, 60)


def s1_inputs():
    rows = np.zeros((60, 4), np.float32)
    rows[:, 0] = np.arange(60)
    rows[:, 1] = 1.0
    allow = np.zeros(60, bool)
    allow[::5] = True
    return dict(rows=rows, query=np.array([[21.0, 1.0, 0.0, 0.0]], np.float32), allow=allow,
                column=(np.arange(60) % 5).astype(np.uint32))


# ---- S2 / S3: 97 rows, 10 % deleted, 30 % allowed, index_base 3 ------------------------------------------------------------
def s2_inputs(dt, dim):
    n = S2_ROWS
    dead = exactly(("dead", dt, dim), n, 10)
    allow = exactly(("allow", dt, dim), n, 29)
    return dict(rows=make_rows("s2", n, dim, dt), dead=dead, allow=allow, admit=allow & ~dead,
                queries=make_queries("s2", 5, dim, dt))


def s2_calls(inp):
    adm = int(inp["admit"].sum())
    for metric in METRICS:
        for nq in (1, 5):
            for k in (adm - 1, adm + 5):
                yield f"m{metric}_q{nq}_k{k}", metric, nq, k


S3_M, S3_K, S3_NQ = 37, 100, 3


def s3_inputs(dt, dim):
    inp = s2_inputs(dt, dim)
    n = S2_ROWS
    rng = np.random.default_rng(_seed("cand", dt, dim))
    cand = (rng.integers(0, n, (S3_NQ, S3_M)).astype(np.uint64) + np.uint64(S2_BASE))
    dead_rows = np.nonzero(inp["dead"])[0]
    for q in range(S3_NQ):
        cand[q, 1] = cand[q, 0]                          # a repeat
        cand[q, 5] = PAD                                 # padding in the middle of the list
        cand[q, 9] = np.uint64(S2_BASE + n + q)          # behind the shard
        cand[q, 13] = np.uint64(q)                       # in front of it (index_base is 3)
        cand[q, 17] = np.uint64(S2_BASE + dead_rows[q])  # a deleted row
        cand[q, 36] = cand[q, 20]                        # a repeat far from its twin
    inp["cand"] = cand
    inp["queries"] = inp["queries"][:S3_NQ]
    return inp


# ---- S4: plain K1 -----------------------------------------------------------------------------------------------------------
S4_ROWS = (97, 10_007)


def s4_inputs(dt, dim):
    return {n: dict(rows=make_rows("s4", n, dim, dt), queries=make_queries("s4", 4, dim, dt)) for n in S4_ROWS}


def s4_calls():
    for n in S4_ROWS:
        for metric in METRICS:
            for nq in (1, 4):
                for k in (10, n + 5):
                    yield f"n{n}_m{metric}_q{nq}_k{k}", n, metric, nq, k


# ---- S5: a batch on the MFMA route ------------------------------------------------------------------------------------------
S5_ROWS, S5_DIM, S5_NQ, S5_K = 20_011, 96, 300, 33
S5_CASES = {"f32cos": ("f32", COS), "f16l2": ("f16", L2), "i8ip": ("i8", IP)}


def s5_inputs(case):
    dt, metric = S5_CASES[case]
    return dict(rows=make_rows("s5", S5_ROWS, S5_DIM, dt), queries=make_queries("s5", S5_NQ, S5_DIM, dt), metric=metric, dt=dt)


# ---- S6: ONE Float32 query over the int8 / the 6-bit shadow --------------------------------------------------------------------
S6_ROWS, S6_DIM, S6_KS = 40_001, 64, (1, 100)
S6_PATHS = {"i8": 6, "6b": 7}


def s6_inputs():
    return dict(rows=make_rows("s6", S6_ROWS, S6_DIM, "f32"), queries=make_queries("s6", 1, S6_DIM, "f32"))


# ---- S7: large k ------------------------------------------------------------------------------------------------------------
S7_ROWS, S7_DIM = 10_007, 16
S7_KS = (2048, S7_ROWS + 5)


def s7_inputs():
    return dict(rows=make_rows("s7", S7_ROWS, S7_DIM, "i8"), queries=make_queries("s7", 3, S7_DIM, "i8"))


def s7_calls():
    for metric in (L2, IP):
        for nq in (1, 3):
            for k in S7_KS:
                yield f"m{metric}_q{nq}_k{k}", metric, nq, k


# ---- S8: radius -------------------------------------------------------------------------------------------------------------
S8_ROWS, S8_MAX = 10_007, 50
S8_SHAPES = {"i8": 16, "f32": 8}
S8_WANT = (9000, 7, 0)  # matches: beyond the 8192-entry device list (finished by top-k), a handful, none


def s8_inputs(dt):
    dim = S8_SHAPES[dt]
    rows, q = make_rows("s8", S8_ROWS, dim, dt), make_queries("s8", 3, dim, dt)
    radii = np.zeros(3, np.float32)
    for j, want in enumerate(S8_WANT):  # L2; the distance of the want-th nearest row, in float64
        d = np.sort(np.sqrt(((rows.astype(np.float64) - q[j].astype(np.float64)) ** 2).sum(1)))
        radii[j] = np.float32(d[want - 1]) if want else np.float32(-1.0)
    return dict(rows=rows, queries=q, radii=radii)


# ---- S9: self-join over two windows -------------------------------------------------------------------------------------------
S9_ROWS, S9_DIM, S9_K = 1_500, 16, 5


def s9_inputs():
    return dict(rows=make_rows("s9", S9_ROWS, S9_DIM, "i8"), dead=exactly("s9", S9_ROWS, 40))


# ---- S10: a shard set of two row ranges -----------------------------------------------------------------------------------------
S10_SHARD, S10_NQ, S10_K = 5_000, 3, 10
S10_SHAPES = {"i8": 16, "f32": 8}


def s10_inputs(dt):
    dim = S10_SHAPES[dt]
    return dict(rows=make_rows("s10", 2 * S10_SHARD, dim, dt), queries=make_queries("s10", S10_NQ, dim, dt))


def scenarios():
    """name -> (does DESIGN.md §3 define the route's bits?)  Integer spaces, K1 (up to four queries on small corpora), the
    filter's list route, candidates, the streaming radius kernel and the join are bit-defined: two runs must agree byte for
    byte.  Elsewhere two unpoisoned runs are the yardstick."""
    out = {"s1_bitmap": True, "s1_where": True}
    for dt, dim in S2_SHAPES:
        out[f"s2_r2_{shape_name(dt, dim)}"] = True
        out[f"s2_r1_{shape_name(dt, dim)}"] = dt in ("i8", "u8")
        out[f"s3_{shape_name(dt, dim)}"] = True
    for dt, dim in EXACT_FIT:
        out[f"s4_{shape_name(dt, dim)}"] = True
    for case, (dt, _) in S5_CASES.items():
        out[f"s5_{case}"] = dt == "i8"
    for name in S6_PATHS:
        out[f"s6_{name}"] = False
    out["s7_lk1"] = out["s7_lk2"] = True
    out["s8_i8"] = out["s8_f32"] = True
    out["s9"] = True
    out["s10_i8"] = True
    out["s10_f32"] = False
    return out


def parse_shape(s):
    for dt, dim in S2_SHAPES:
        if s == shape_name(dt, dim):
            return dt, dim
    raise SystemExit(f"unknown shape {s}")


# ===== the child ===================================================================================================================
def _put(out, key, res, vectors=None):
    out[key + ".scores"], out[key + ".indices"], out[key + ".raw"] = res.scores, res.indices, res.raw
    if hasattr(res, "counts"):
        out[key + ".counts"] = res.counts
    if vectors is not None:
        out[key + ".vectors"] = vectors


def _put_info(out, key, flt):
    inf = flt.info()
    out[key + ".filter_info"] = np.array([inf.has_row_list, inf.rows, inf.admitted, inf.device_bytes], np.uint64)


def run(name, G):
    out = {}
    fam, _, rest = name.partition("_")
    if fam == "s1":
        inp = s1_inputs()
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            for k in S1_KS:  # one filter per call, created and destroyed around it, as include/mvf.hpp does
                if rest == "bitmap":
                    with c.make_filter(np.packbits(inp["allow"], bitorder="little")) as f:
                        _put_info(out, f"k{k}", f)
                        _put(out, f"k{k}", c.search_filtered(inp["query"], k, L2, f))
                else:
                    with c.attach_column(inp["column"]) as col, c.make_filter_where([(col, "==", 0)]) as f:
                        _put_info(out, f"k{k}", f)
                        _put(out, f"k{k}", c.search_filtered(inp["query"], k, L2, f))
    elif fam == "s2":
        route, _, shape = rest.partition("_")
        os.environ["MVF_FILTER_ROUTE"] = route[1:]  # read when the handle is created
        inp = s2_inputs(*parse_shape(shape))
        with G.GpuCorpus.from_array(inp["rows"], index_base=S2_BASE) as c:
            c.set_tombstones(np.packbits(inp["dead"], bitorder="little"))
            with c.make_filter(inp["allow"]) as f:
                _put_info(out, "filter", f)
                for key, metric, nq, k in s2_calls(inp):
                    _put(out, key, c.search_filtered(inp["queries"][:nq], k, metric, f))
    elif fam == "s3":
        inp = s3_inputs(*parse_shape(rest))
        with G.GpuCorpus.from_array(inp["rows"], index_base=S2_BASE) as c:
            c.set_tombstones(np.packbits(inp["dead"], bitorder="little"))
            for metric in METRICS:
                _put(out, f"m{metric}", c.search_candidates(inp["queries"], inp["cand"], S3_K, metric))
    elif fam == "s4":
        dt, dim = parse_shape(rest)
        inp = s4_inputs(dt, dim)
        handles = {n: G.GpuCorpus.from_array(inp[n]["rows"]) for n in S4_ROWS}
        for key, n, metric, nq, k in s4_calls():
            _put(out, key, handles[n].search(inp[n]["queries"][:nq], k, metric))
        for metric in METRICS:  # the payload rows fused into the final select
            res, vec = handles[97].search_fetch(inp[97]["queries"][:1], 10, metric)
            _put(out, f"fetch_m{metric}", res, vec)
        for h in handles.values():
            h.close()
    elif fam == "s5":
        inp = s5_inputs(rest)
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            _put(out, "batch", c.search(inp["queries"], S5_K, inp["metric"]))
            out["selection_state"] = np.array([c.info().selection_state, c.info().shadows], np.uint32)
    elif fam == "s6":
        inp = s6_inputs()
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            c.set_profiling(True)
            c.set_scan_path(S6_PATHS[rest])
            for k in S6_KS:
                for metric in METRICS:
                    _put(out, f"m{metric}_k{k}", c.search(inp["queries"], k, metric))
                    t = c.last_timing()
                    out[f"m{metric}_k{k}.scan"] = np.array([t.scan_kernel, t.scan_bytes, t.repaired_queries], np.uint64)
    elif fam == "s7":
        os.environ["MVF_LARGE_K"] = rest[2:]
        inp = s7_inputs()
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            for key, metric, nq, k in s7_calls():
                _put(out, key, c.search(inp["queries"][:nq], k, metric))
    elif fam == "s8":
        inp = s8_inputs(rest)
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            res = c.search_radius(inp["queries"], inp["radii"], S8_MAX, L2)
            _put(out, "lists", res)
            out["counts_only.counts"] = c.search_radius(inp["queries"], inp["radii"], 0, L2).counts
    elif fam == "s9":
        inp = s9_inputs()
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            c.set_tombstones(np.packbits(inp["dead"], bitorder="little"))
            for metric in (L2, IP):
                _put(out, f"m{metric}", c.knn_join(S9_K, metric))
    elif fam == "s10":
        inp = s10_inputs(rest)
        shards = [G.GpuCorpus.from_array(inp["rows"][a:a + S10_SHARD], index_base=a) for a in (0, S10_SHARD)]
        with G.ShardSet(shards) as ss:
            for metric in METRICS:
                _put(out, f"m{metric}", ss.search(inp["queries"], S10_K, metric))
        for s in shards:
            s.close()
    else:
        raise SystemExit(f"unknown scenario {name}")
    return out


def main(argv):
    if len(argv) != 3 or argv[1] not in scenarios():
        print("usage: _fresh_process.py <scenario> <out.npz>; scenarios: " + " ".join(scenarios()), file=sys.stderr)
        return 2
    sys.modules.setdefault("torch", None)  # the binding would load torch's HIP runtime first where torch is installed
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from metrovector_amd import gpu as G
    out = run(argv[1], G)
    out["poison"] = np.array([G.selftest_poison()], np.int32)
    np.savez(argv[2], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
