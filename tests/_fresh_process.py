"""Scenarios whose device calls are the FIRST device work of a process (tests/test_gpu_fresh_process.py starts this file as a
child: `python tests/_fresh_process.py <scenario> <out.npz>`).

Every other GPU test runs inside one long-lived Python process, where the library's scratch is recycled from its own earlier,
benign contents and where dozens of plain searches precede every filter, candidate, radius or join call.  A scenario here
builds its inputs from fixed numpy seeds, performs its calls in a fixed order and saves every output array -- together with
mvfgpu_selftest_poison(), so that the parent can tell that a child really ran with MVF_DEBUG_POISON set (DESIGN.md §2,
"Poisoned allocations").  The parent imports this module too: the inputs and the order of the calls are stated once, here.

S11 .. S17 are the routes over a partition index (partitioned, grouped, multi-vector on both routes, candidate keys, diversified
re-ranking) and S17 the call order of include/mvf.hpp's helpers: one handle, and for every step a column and an index of its
own that are closed before the next step -- what examples/cpp/rerank_documents.cpp does.  Their host calls are repeated as
device calls on buffers of the HIP runtime the library is bound to; the parent holds both to the same bytes.

Imports metrovector_amd, numpy and the numpy-only helper modules beside it (and the standard library); as a child it also keeps
the binding from loading torch, so the library binds to the platform's HIP runtime as a C or C++ consumer's process does.
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

import _maxsim_candidates as MC
import _mmr as MM
import _partitioned as P

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


# ---- S11 .. S17: the routes over a partition index ----------------------------------------------------------------------------
# One layout for S11 .. S15 (tests/_partitioned.py's `layout`, tests/_maxsim.py's form sizes): 2048 rows, every 10th dead; keys
# of 300, 129, 128, 127, 64, 2 and 1 live rows and 20 further keys of about 55; one key whose rows are all deleted and one no
# row carries.  27 keys hold rows.
FI_N, FI_SIZES, FI_FURTHER = 2048, (300, 129, 128, 127, 64, 2, 1), 20


def fi_layout():
    return P.layout("u32", FI_N, FI_SIZES, FI_FURTHER)


def fi_rows(tag, dt, dim):
    return make_rows(tag, FI_N, dim, dt)


def any_shape(s):
    dt, _, dim = s.partition("d")
    if dt not in DT or not dim.isdigit():
        raise SystemExit(f"unknown shape {s}")
    return dt, int(dim)


# S11: partitioned.  Query j's key: 300 rows, one row, wholly deleted, absent, two rows; k below and above every key's rows
S11_SHAPES = (("i8", 16), ("f32", 3))
S11_KS = (2, 400)


def s11_inputs(dt, dim):
    lay = fi_layout()
    keys = np.array([lay["keys"][0], lay["keys"][6], lay["dead_key"], lay["absent_key"], lay["keys"][5]], np.uint64)
    return dict(lay=lay, rows=fi_rows("s11", dt, dim), queries=make_queries("s11", 5, dim, dt), keys=keys)


def s11_calls():
    for metric in METRICS:
        for nq in (1, 5):
            for k in S11_KS:
                yield f"m{metric}_q{nq}_k{k}", metric, nq, k


# S12: grouped.  27 keys hold rows: k = 10 fills under both caps, k = 100 exceeds what per_key 3 can give (25 x 3 + 2 + 1)
S12_SHAPES = (("i8", 16), ("f32", 4))
S12_PER_KEYS, S12_KS, S12_NQ = (1, 3), (10, 100), 5


def s12_inputs(dt, dim):
    return dict(lay=fi_layout(), rows=fi_rows("s12", dt, dim), queries=make_queries("s12", S12_NQ, dim, dt))


def s12_calls():
    for metric in METRICS:
        for per_key in S12_PER_KEYS:
            for k in S12_KS:
                yield f"m{metric}_p{per_key}_k{k}", metric, per_key, k, (1 if (per_key, k) == (1, 10) else S12_NQ)


# S13 / S14: multi-vector search, route 1 and route 2.  T = 33: eight token groups of four and a last one of one token
S13_SHAPES = (("i8", 16), ("f32", 8), ("f16", 8))
S14_CASES = {"f32ip": ("f32", 8, IP), "f16cos": ("f16", 8, COS)}
MS_TS, MS_NQS, MS_KS, MS_POOL = (3, 33), (1, 3), (5, 40), (3, 33)   # 27 keys: k = 5 below, k = 40 above


def ms_inputs(tag, dt, dim):
    nq, T = MS_POOL
    return dict(lay=fi_layout(), rows=fi_rows(tag, dt, dim), pool=make_queries(tag, nq * T, dim, dt).reshape(nq, T, dim))


def ms_sets(inp, nq, T):
    """the leading nq sets of T tokens of the pool: one reference serves every (nq, T)"""
    return np.ascontiguousarray(inp["pool"][:nq, :T])


def ms_calls(metrics=METRICS):
    for metric in metrics:
        for T in MS_TS:
            for nq in MS_NQS:
                for k in MS_KS:
                    yield f"m{metric}_t{T}_q{nq}_k{k}", metric, T, nq, k


# S15: candidate keys.  Three mixed lists (repeats, pads, the absent and the wholly deleted key), then one list whose keys hold
# exactly 128 rows -- its part of the concatenated list ends at a block -- and one of 129: a block and one position
S15_SHAPES = (("i8", 16), ("f32", 8))
S15_M, S15_T, S15_KS, S15_MIXED = 16, 3, (1, 20), 3   # k = 20 exceeds m: above every list's held count


def s15_inputs(dt, dim):
    lay = fi_layout()
    held, counts = P.group_by(lay)
    skipped = [lay["absent_key"], lay["dead_key"], int(PAD)]
    lists = [MC.mixed_lists(held, S15_MIXED + 1, S15_M, skipped, "s15")[1:]]   # its first list holds m keys and nothing else
    for target in (MC.BLOCK, MC.BLOCK + 1):
        rng = np.random.default_rng(_seed("s15 edge", target))
        small = np.isin(counts, (127, 2, 1))   # two segments: the keys of 128 and 129 rows alone would be one
        mine = MC.rows_ending_at(held[small], counts[small], target, rng)
        assert mine is not None and 2 <= mine.size < S15_M, f"no keys of {target} rows in all"
        row = np.full(S15_M, PAD, np.uint64)
        row[:mine.size] = mine
        row[mine.size] = np.uint64(lay["dead_key"])
        lists.append(row[rng.permutation(S15_M)][None, :])
    lists = np.concatenate(lists)
    nq = lists.shape[0]
    return dict(lay=lay, rows=fi_rows("s15", dt, dim), lists=lists,
                sets=make_queries("s15", nq * S15_T, dim, dt).reshape(nq, S15_T, dim))


# S16: diversified re-ranking over tests/_mmr.py's planted world, cut down
S16_N, S16_DIM, S16_M, S16_K, S16_LAMBDAS = 2000, 32, 64, 16, (0.5, 1.0)


def s16_inputs():
    rows, q, lst, where = MM.planted_world(seed=77, n=S16_N, dim=S16_DIM, m=S16_M, copies=8)
    rng = np.random.default_rng(_seed("s16"))
    second = rng.integers(0, S16_N + 50, S16_M).astype(np.uint64)   # a random list: repeats, rows behind the corpus, pads
    second[::9] = PAD
    return dict(rows=rows, queries=np.stack([q, make_queries("s16", 1, S16_DIM, "f32")[0]]), lists=np.stack([lst, second]),
                copies=where)


# S17: the documents example (examples/cpp/rerank_documents.cpp and its test) on ONE handle, every step with a column and an
# index of its own, both closed before the next step -- include/mvf.hpp's call order
S17_N, S17_DIM, S17_DOCS, S17_UNIT, S17_T, S17_K, S17_SEED = 600, 8, 30, 1000003, 3, 6, 21
S17_STEPS = {"cpp": ("full", "cand", "empty"), "mixed": ("cand", "perkey", "grouped", "full", "cand")}


def s17_inputs():
    rng = np.random.default_rng(S17_SEED)
    rows = rng.standard_normal((S17_N, S17_DIM)).astype(np.float32)
    doc = rng.integers(0, S17_DOCS, S17_N).astype(np.uint64) * np.uint64(S17_UNIT)
    cand = np.array([int(v) for v in (np.array([4, 9, 9, 77, 0, 13, 4, 21], np.uint64) * np.uint64(S17_UNIT))] + [(1 << 64) - 1], np.uint64)
    return dict(rows=rows, doc=doc, cand=cand, query=np.ascontiguousarray(rows[:S17_T]))


def scenarios():
    """name -> (does DESIGN.md §3 define the route's bits?)  Integer spaces, K1 (up to four queries on small corpora), the
    filter's list route, candidates, the streaming radius kernel and the join are bit-defined: two runs must agree byte for
    byte.  Elsewhere two unpoisoned runs are the yardstick.  The routes over a partition index (S11 .. S17) are bit-defined in
    every space: the partitioned and the grouped search are the candidate search's bytes, the multi-vector searches sum K1's
    one-query bits in token order on either route, the diversified re-ranking is its recipe's bytes."""
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
    for dt, dim in S11_SHAPES:
        out[f"s11_{shape_name(dt, dim)}"] = True
    for dt, dim in S12_SHAPES:
        out[f"s12_{shape_name(dt, dim)}"] = True
    for dt, dim in S13_SHAPES:
        out[f"s13_{shape_name(dt, dim)}"] = True
    for case in S14_CASES:
        out[f"s14_{case}"] = True
    for dt, dim in S15_SHAPES:
        out[f"s15_{shape_name(dt, dim)}"] = True
    out["s16"] = True
    for variant in S17_STEPS:
        out[f"s17_{variant}"] = True
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


def _put_ms(out, key, res):
    out[key + ".scores"], out[key + ".keys"], out[key + ".counts"] = res.scores, res.keys, res.counts


class _Device:
    """device buffers of the HIP runtime the library is bound to (tests/_partitioned.py's way): what the device calls take"""

    def __init__(self):
        self.hip = P._hip_runtime()
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.held = []

    def empty(self, nbytes):
        p = C.c_void_p()
        P._check(self.hip.hipMalloc(C.byref(p), max(nbytes, 16)), "hipMalloc")
        self.held.append(p)
        return p.value

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.empty(a.nbytes)
        P._check(self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1), "hipMemcpy H2D")
        return p

    def get(self, p, shape, dtype):
        """waits for the device first"""
        P._check(self.hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
        a = np.empty(shape, dtype)
        P._check(self.hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2), "hipMemcpy D2H")
        return a

    def release(self):
        for p in self.held:
            P._check(self.hip.hipFree(p), "hipFree")
        self.held = []


def _indexed(c, lay):
    """tombstones, then a column and an index over it (closed by the caller's `with`)"""
    c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
    col = c.attach_column(lay["col"])
    return col, c.make_partition(col)


def _maxsim_calls(out, G, c, part, inp, dt, dim, calls):
    """every call of `calls` as the host call and as the device call"""
    dev = _Device()
    for key, metric, T, nq, k in calls:
        sets = ms_sets(inp, nq, T)
        _put_ms(out, key, c.search_maxsim(sets, k, metric, part))
        dq, ds, dk, dc = dev.put(sets), dev.empty(nq * k * 4), dev.empty(nq * k * 8), dev.empty(nq * 4)
        c.search_maxsim_device(part, dq, DT[dt][1] if dt in ("i8", "u8") else 0, dim, nq, T, k, metric, ds, dk, dc)
        _put_ms(out, key + "@device", G.MaxSimResult(dev.get(ds, (nq, k), np.float32), dev.get(dk, (nq, k), np.uint64),
                                                      dev.get(dc, (nq,), np.uint32)))
        dev.release()
    return dev


def _s17_step(out, c, inp, step, tag):
    """one helper of include/mvf.hpp: its own column and index around one search"""
    q, doc = inp["query"], inp["doc"]
    with c.attach_column(doc) as col, c.make_partition(col) as part:
        if step == "full":
            _put_ms(out, tag, c.search_maxsim(q, S17_DOCS + 2, L2, part))   # every document: what the candidates are filtered from
            _put_ms(out, tag + "_k", c.search_maxsim(q, S17_K, L2, part))
        elif step == "cand":
            _put_ms(out, tag, c.search_maxsim_candidates(q, inp["cand"], S17_K, L2, part))
        elif step == "empty":
            _put_ms(out, tag, c.search_maxsim_candidates(q, np.zeros(0, np.uint64), S17_K, L2, part))
        elif step == "perkey":
            _put(out, tag, c.search_partitioned(q, inp["cand"][[0, 3, 4]], S17_K, L2, part))
        elif step == "grouped":
            _put(out, tag, c.search_grouped(q, S17_K, 1, L2, part))
        else:
            raise SystemExit(f"unknown step {step}")


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
    elif fam == "s11":
        dt, dim = any_shape(rest)
        inp = s11_inputs(dt, dim)
        qcode = DT[dt][1] if dt in ("i8", "u8") else 0
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            col, part = _indexed(c, inp["lay"])
            with col, part:
                dev = _Device()
                for key, metric, nq, k in s11_calls():
                    q, keys = inp["queries"][:nq], inp["keys"][:nq]
                    _put(out, key, c.search_partitioned(q, keys, k, metric, part))
                    dq, ds, di, dr = dev.put(q), dev.empty(nq * k * 4), dev.empty(nq * k * 8), dev.empty(nq * k * 4)
                    c.search_partitioned_device(part, dq, qcode, dim, nq, keys, k, metric, ds, di, dr)
                    _put(out, key + "@device", G.SearchResult(dev.get(ds, (nq, k), np.float32), dev.get(di, (nq, k), np.uint64),
                                                              dev.get(dr, (nq, k), np.int32)))
                    dev.release()
    elif fam == "s12":
        dt, dim = any_shape(rest)
        inp = s12_inputs(dt, dim)
        qcode = DT[dt][1] if dt in ("i8", "u8") else 0
        live = np.nonzero(~inp["lay"]["dead"])[0].astype(np.uint64)
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            col, part = _indexed(c, inp["lay"])
            with col, part:
                dev = _Device()
                for key, metric, per_key, k, nq in s12_calls():
                    q = inp["queries"][:nq]
                    _put(out, key, c.search_grouped(q, k, per_key, metric, part))
                    dq, ds, di, dr = dev.put(q), dev.empty(nq * k * 4), dev.empty(nq * k * 8), dev.empty(nq * k * 4)
                    c.search_grouped_device(part, dq, qcode, dim, nq, k, per_key, metric, ds, di, dr)
                    _put(out, key + "@device", G.SearchResult(dev.get(ds, (nq, k), np.float32), dev.get(di, (nq, k), np.uint64),
                                                              dev.get(dr, (nq, k), np.int32)))
                    dev.release()
                for metric in METRICS:  # the ranking of every held row the walk is taken over (identity 1)
                    _put(out, f"rank_m{metric}", c.search_candidates(inp["queries"], np.repeat(live[None, :], S12_NQ, axis=0), live.size, metric))
    elif fam == "s13":
        dt, dim = any_shape(rest)
        inp = ms_inputs("s13", dt, dim)
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            col, part = _indexed(c, inp["lay"])
            with col, part:
                c.set_maxsim_route(1)
                _maxsim_calls(out, G, c, part, inp, dt, dim, ms_calls())
    elif fam == "s14":
        dt, dim, metric = S14_CASES[rest]
        inp = ms_inputs("s14", dt, dim)
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            col, part = _indexed(c, inp["lay"])
            with col, part:
                c.set_maxsim_route(2)
                dev = _maxsim_calls(out, G, c, part, inp, dt, dim, ms_calls((metric,)))
                # the handle really selects: the stage timer of one of the searches counts candidates and blocks
                nq, T, k = MS_NQS[-1], MS_TS[-1], MS_KS[0]
                dq, ds, dk = dev.put(ms_sets(inp, nq, T)), dev.empty(nq * k * 4), dev.empty(nq * k * 8)
                _, cand, blocks = c.maxsim_mfma_stage_ms(part, dq, 0, dim, nq, T, k, metric, ds, dk)
                out["candidates"], out["blocks"] = cand, blocks
                dev.release()
    elif fam == "s15":
        dt, dim = any_shape(rest)
        inp = s15_inputs(dt, dim)
        sets, lists = inp["sets"], inp["lists"]
        nq = sets.shape[0]
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            col, part = _indexed(c, inp["lay"])
            with col, part:
                dev = _Device()
                for metric in METRICS:
                    for k in S15_KS:
                        key = f"m{metric}_k{k}"
                        _put_ms(out, key, c.search_maxsim_candidates(sets, lists, k, metric, part))   # the child's first search
                        dq, ds, dk, dc = dev.put(sets), dev.empty(nq * k * 4), dev.empty(nq * k * 8), dev.empty(nq * 4)
                        c.search_maxsim_candidates_device(part, dq, DT[dt][1] if dt == "i8" else 0, dim, nq, S15_T, lists, k, metric, ds, dk, dc)
                        _put_ms(out, key + "@device", G.MaxSimResult(dev.get(ds, (nq, k), np.float32), dev.get(dk, (nq, k), np.uint64),
                                                                      dev.get(dc, (nq,), np.uint32)))
                        dev.release()
                    _put_ms(out, f"full_m{metric}", c.search_maxsim(sets, int(part.info().n_keys), metric, part))
    elif fam == "s16":
        inp = s16_inputs()
        q, lists = inp["queries"], inp["lists"]
        nq, m, k = q.shape[0], S16_M, S16_K
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            dev = _Device()
            for lam in S16_LAMBDAS:
                for metric in (COS, L2):
                    key = f"l{lam}_m{metric}"
                    res = c.search_mmr(q, lists, k, lam, metric)   # the child's first search
                    _put(out, key, res)
                    out[key + ".objective"] = res.objective
                    dq, dl = dev.put(q), dev.put(lists)
                    ds, di, dr, do, dc = dev.empty(nq * k * 4), dev.empty(nq * k * 8), dev.empty(nq * k * 4), dev.empty(nq * k * 4), dev.empty(nq * 8)
                    c.search_mmr_device(dq, 0, S16_DIM, nq, dl, m, k, lam, metric, ds, di, dr, do, dc)
                    dres = G.MmrResult(dev.get(ds, (nq, k), np.float32), dev.get(di, (nq, k), np.uint64), dev.get(dr, (nq, k), np.int32),
                                       dev.get(dc, (nq,), np.uint64), dev.get(do, (nq, k), np.float32))
                    _put(out, key + "@device", dres)
                    out[key + "@device.objective"] = dres.objective
                    dev.release()
            # what the recipe is made of (tests/_mmr.py `recipe`): the candidate searches of the queries and of the listed rows
            for metric in (COS, L2):
                for j in range(nq):
                    R = c.search_candidates(q[j:j + 1], lists[j:j + 1], m, metric)
                    _put(out, f"rel_m{metric}_q{j}", R)
                    cnt = int(R.counts[0])
                    pos = np.sort(R.indices[0][:cnt])
                    _put(out, f"sim_m{metric}_q{j}", c.search_candidates(c.gather_rows(pos), np.repeat(lists[j:j + 1], cnt, axis=0), m, metric))
    elif fam == "s17":
        inp = s17_inputs()
        with G.GpuCorpus.from_array(inp["rows"]) as c:
            for i, step in enumerate(S17_STEPS[rest]):
                _s17_step(out, c, inp, step, f"step{i}_{step}")
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
