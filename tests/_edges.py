"""Corpora and queries at the edges of the float formats, with expectations that need no tolerance (DESIGN.md §2 "Format
edges", §3 "Values at the edges").

Scaling by a power of two commutes with every f32 rounding while nothing underflows or overflows, so a corpus and its scaled
TWIN have the same index lists and, after `ldexp`, the same score bits on any route whose arithmetic is f32:

* Float16: integers m from [-1023, 1023]; H = m 2^-10 (normal or zero), S = m 2^-24 (every non-zero value SUBNORMAL),
  T = m 2^5 (up to 32736; 2^15 times H), R = row r of H times 2^-(7 r mod 15) (normal to fully subnormal rows side by side).
* Float32: F = the synthetic corpus, its twins ldexp(F, -40) and ldexp(F, +40).
* InnerProduct(twin, q) = ldexp(InnerProduct(base, q), e); Cosine(twin, q) = Cosine(base, q);
  L2(twin, ldexp(q, e)) = ldexp(L2(base, q), e).  For R only the cosine identity holds.

Edge queries (NaN, +Inf, 2^64 q, 2^-130 q, zeros, 2^+-40 q) have their answer from the rule of §3's table, written here in
numpy from its words.  Everything here is numpy on the CPU; the library is never called."""
from __future__ import annotations

import numpy as np

import _wide as W
from _util import PAD

F32, F16 = 0, 1
L2, IP, COS = 0, 1, 2
METRICS = (L2, IP, COS)
NP_OF = {F32: np.float32, F16: np.float16}

# twin -> the power of two between it and its base corpus
SHIFT = {"H": 0, "S": -14, "T": 15, "R": None, "F": 0, "Fdn": -40, "Fup": 40}
# the scale of the queries under L2: the corpus' own; R's is that of its smallest, fully subnormal rows -- with queries of H's
# scale every small row lies at |q| (1 +- 1e-6), inside the boundary band of all the others, and nothing is decided
L2_QUERY_SHIFT = dict(SHIFT, R=-14)
BASE_OF = {F16: "H", F32: "F"}
TWINS_OF = {F16: ("S", "T", "R"), F32: ("Fdn", "Fup")}
R_PERIOD = 15           # row r of R is H's row times 2^-(7 r mod 15)
F16_MIN_NORMAL = 2.0 ** -14

POOL, NQ = 80, 64       # queries generated per case; the first NQ of them with a thin boundary band are used
KS = (10, 100)

# name -> (seed, rows, dimension, tombstones on 20 % of the rows).  The batched routes' shapes are those of
# tests/test_gpu_float_ties.py (several phases); K1's are one per lane-group class of choose_group for the type (Float16 /
# Float32 row bytes): one lane, 4, 8, 16, 32 and 64 lanes and a row of at least 3 KiB.
BATCHED = {"n20k_d200": (1200, 20_000, 200, True), "n40k_d96": (1096, 40_000, 96, False)}
K1_SHAPES = {
    F16: {"d4": (2004, 4000, 4, False), "d16": (2016, 4000, 16, True), "d48": (2048, 4000, 48, False), "d96": (2096, 4000, 96, True),
          "d200": (2200, 3000, 200, False), "d776": (2776, 3000, 776, True), "d1536": (3536, 3000, 1536, False)},
    F32: {"d4": (4004, 4000, 4, True), "d16": (4016, 4000, 16, False), "d32": (4032, 4000, 32, True), "d48": (4048, 4000, 48, False),
          "d100": (4100, 4000, 100, True), "d200": (4200, 3000, 200, False), "d776": (4776, 3000, 776, True)},
}
ZERO_ROWS = (5, 77, -3)   # rows whose element in the +Inf column is planted as 0 (and one at the middle of the corpus)


def shape_of(name, dtype):
    return BATCHED[name] if name in BATCHED else K1_SHAPES[dtype][name]


class Case:
    """One shape of one type: the base corpus, its twins, the live rows, the 64 thin-band queries and the base edge query.
    Built once, shared, never changed."""

    def __init__(self, oracle, name, dtype):
        self.name, self.dtype = name, dtype
        self.seed, self.n, self.dim, self.tomb = shape_of(name, dtype)
        n, dim = self.n, self.dim
        rng = np.random.default_rng(self.seed)
        self.col = dim // 3                                  # the column of the NaN / +Inf element
        zero_rows = [r % n for r in ZERO_ROWS] + [n // 2]
        self.corpora = {}
        if dtype == F16:
            m = rng.integers(-1023, 1024, (n, dim)).astype(np.int64)
            m[zero_rows, self.col] = 0
            self.m = m
            mf = m.astype(np.float64)
            self.rshift = -((7 * np.arange(n)) % R_PERIOD)
            self.exact = {"H": mf * 2.0 ** -10, "S": mf * 2.0 ** -24, "T": mf * 2.0 ** 5,
                          "R": np.ldexp(mf * 2.0 ** -10, self.rshift[:, None])}
        else:
            f = np.array(oracle.synth_rows(self.seed, 0, n, dim, F32))
            f[zero_rows, self.col] = 0.0
            f64 = f.astype(np.float64)
            self.exact = {"F": f64, "Fdn": np.ldexp(f64, -40), "Fup": np.ldexp(f64, 40)}
        for kind, x in self.exact.items():
            self.corpora[kind] = np.ascontiguousarray(x.astype(NP_OF[dtype]))
        self.dead = None
        if self.tomb:
            self.dead = np.zeros(n, bool)
            self.dead[rng.choice(n, n // 5, replace=False)] = True
        self.live = np.ones(n, bool) if self.dead is None else ~self.dead
        self.livepos = np.nonzero(self.live)[0]
        self.pool = np.array(oracle.synth_queries(self.seed + 1, POOL, dim, F32))
        self._ref, self._rows32, self._thin = {}, {}, None
        self.tag = f"{name} dtype {dtype}{' (tombstones)' if self.tomb else ''}"

    # -- rows and queries ---------------------------------------------------------------------------------------------
    def rows(self, kind):
        return self.corpora[kind]

    def rows32_live(self, kind):
        """The live rows widened to f32 (exact for every corpus here), cached: `assert_float_topk` caches norms per array."""
        if kind not in self._rows32:
            self._rows32[kind] = self.corpora[kind][self.livepos].astype(np.float32)
        return self._rows32[kind]

    def query_shift(self, kind, metric):
        """Under L2 the queries live at the corpus' scale."""
        return L2_QUERY_SHIFT[kind] if metric == L2 else 0

    def queries_for(self, kind, metric, q=None):
        q = self.q if q is None else q
        return np.ldexp(q, self.query_shift(kind, metric)).astype(np.float32)

    def ref64(self, kind, pool=False):
        """{metric: f64 [nq, live rows]} of the case's queries (or the whole pool) against the corpus actually searched."""
        key = (kind, pool)
        if key not in self._ref:
            q = self.pool if pool else self.q
            rows = self.corpora[kind][self.livepos]
            out = W.f64_scores_all(rows, q)
            e = self.query_shift(kind, L2)
            if e:
                out[L2] = W.f64_scores_all(rows, np.ldexp(q, e).astype(np.float32))[L2]
            self._ref[key] = out
        return self._ref[key]

    # -- the thin-band queries ----------------------------------------------------------------------------------------
    def thin(self):
        """Indices into the pool of the first 64 queries that `thin_band_queries` accepts on the base corpus AND on R (the
        exact twins have the base's band: every score and the band's width scale alike)."""
        if self._thin is None:
            kinds = ("H", "R") if self.dtype == F16 else ("F",)
            keep = None
            for kind in kinds:
                ref = self.ref64(kind, pool=True)
                ok = W.thin_band_queries(ref, self.rows32_live(kind), self.pool, KS, want=POOL)
                keep = set(ok.tolist()) if keep is None else keep & set(ok.tolist())
            self._thin = np.array(sorted(keep), np.int64)[:NQ]
        return self._thin

    @property
    def q(self):
        return self.pool[self.thin()]

    def batch(self, nq):
        """[nq, dim]: the thin queries first (the ones compared), the rest of the pool behind them, repeated as needed."""
        t = self.thin()
        rest = np.setdiff1d(np.arange(POOL), t)
        order = np.concatenate([t, rest])
        return self.pool[np.resize(order, nq)] if nq > len(order) else self.pool[order[:nq]]

    # -- edge queries -------------------------------------------------------------------------------------------------
    def edge_base(self):
        """The base query of the edge table: the first of the pool with sum q^2 >= 2, so that 2^64 q overflows sum q^2 in
        any summation order while its elements stay finite."""
        for q in self.pool:
            if float((q.astype(np.float64) ** 2).sum()) >= 2.0 and q[self.col] != 0:
                return q
        raise AssertionError("no query of the pool with sum q^2 >= 2")

    def edge_queries(self):
        q = self.edge_base()
        nan, inf = q.copy(), q.copy()
        nan[self.col], inf[self.col] = np.nan, np.inf
        return {"nan": nan, "inf": inf, "2^64": np.ldexp(q, 64).astype(np.float32), "2^-130": np.ldexp(q, -130).astype(np.float32),
                "zeros": np.zeros(self.dim, np.float32), "-zeros": np.full(self.dim, -0.0, np.float32)}


_CASES = {}


def get_case(oracle, name, dtype):
    key = (name, dtype)
    if key not in _CASES:
        _CASES[key] = Case(oracle, name, dtype)
    return _CASES[key]


def all_cases():
    """(name, dtype) of every case the GPU file uses; tests/test_format_edges_cpu.py holds each to its conditions."""
    return [(n, d) for d in (F16, F32) for n in list(BATCHED) + list(K1_SHAPES[d])]


# ---- the twin identity ---------------------------------------------------------------------------------------------------

def score_bits(sc):
    """u32 bits of f32 scores, -0.0 folded into +0.0 and every NaN into one."""
    sc = np.asarray(sc, np.float32)
    return np.where(np.isnan(sc), np.uint32(0x7FC00000), np.where(sc == 0, np.float32(0), sc).view(np.uint32))


def twin_shift(kind, metric):
    """The exponent between a twin's scores and its base's: Cosine 0, InnerProduct and L2 the corpus' shift; None where no
    identity holds (R under InnerProduct and L2)."""
    if SHIFT[kind] is None:
        return 0 if metric == COS else None
    return 0 if metric == COS else SHIFT[kind]


def twin_difference(base_scores, base_idx, twin_scores, twin_idx, e):
    """One query: None where the lists agree -- indices equal, score bits equal after ldexp(base, e) -- else a message."""
    base_idx, twin_idx = np.asarray(base_idx), np.asarray(twin_idx)
    d = np.nonzero(base_idx != twin_idx)[0]
    if d.size:
        r = int(d[0])
        return f"indices differ first at rank {r}: base row {base_idx[r]}, twin row {twin_idx[r]}"
    want = np.ldexp(np.asarray(base_scores, np.float32), e).astype(np.float32)
    d = np.nonzero(score_bits(want) != score_bits(twin_scores))[0]
    if d.size:
        r = int(d[0])
        return (f"score bits differ first at rank {r} (row {twin_idx[r]}): ldexp(base, {e}) = {want[r]!r} "
                f"(0x{score_bits(want)[r]:08x}), twin {np.asarray(twin_scores)[r]!r} (0x{score_bits(twin_scores)[r]:08x})")
    return None


# ---- the rule of §3's edge-query table -----------------------------------------------------------------------------------

ORDINARY = "ordinary"   # finite scores in the ordinary order: judged by float64 within §3's tolerance
UNASSERTED = None       # InnerProduct with the 2^-130 query: every product is subnormal, there is no criterion


def edge_expectation(qname, metric, x_col, livepos, k):
    """The answer the table DEFINES for one edge query -> ORDINARY, UNASSERTED or (indices u64 [k], classes [k]) with a class
    per entry out of "nan", "+inf", "-inf", "zero" (either sign), "pad".  x_col: the corpus' element in the NaN / +Inf column
    of every row (only its sign matters)."""
    first = {("nan", L2): "nan", ("nan", IP): "nan", ("nan", COS): "zero",
             ("inf", L2): "+inf", ("inf", COS): "nan",
             ("2^64", L2): "+inf", ("2^64", COS): "zero",
             ("2^-130", COS): "zero",
             ("zeros", IP): "zero", ("zeros", COS): "zero", ("-zeros", IP): "zero", ("-zeros", COS): "zero"}
    real = min(k, livepos.size)
    idx = np.full(k, PAD, np.uint64)
    cls = np.full(k, "pad", object)
    if (qname, metric) in first:
        idx[:real] = livepos[:real].astype(np.uint64)
        cls[:real] = first[(qname, metric)]
        return idx, cls
    if (qname, metric) == ("inf", IP):
        xc = np.asarray(x_col, np.float64)[livepos]
        order = np.concatenate([livepos[xc > 0], livepos[xc < 0], livepos[xc == 0]])
        names = np.concatenate([np.full(int((xc > 0).sum()), "+inf", object), np.full(int((xc < 0).sum()), "-inf", object),
                                np.full(int((xc == 0).sum()), "nan", object)])
        idx[:real], cls[:real] = order[:real].astype(np.uint64), names[:real]
        return idx, cls
    if (qname, metric) == ("2^-130", IP):
        return UNASSERTED
    return ORDINARY


def class_of(scores):
    sc = np.asarray(scores, np.float32)
    out = np.full(sc.shape, "finite", object)
    out[np.isnan(sc)] = "nan"
    out[np.isposinf(sc)] = "+inf"
    out[np.isneginf(sc)] = "-inf"
    out[sc == 0] = "zero"
    return out


def assert_edge(case, kind, qname, metric, query, scores, indices, k, what="", pos=None):
    """One edge query's result list against the table (indices are positions; pos: the admitted live rows, default all)."""
    from _util import assert_float_topk
    livepos = case.livepos if pos is None else pos
    want = edge_expectation(qname, metric, case.exact[kind][:, case.col], livepos, k)
    if want is UNASSERTED:
        return
    indices, scores = np.asarray(indices, np.uint64), np.asarray(scores, np.float32)
    if want is ORDINARY:
        rows = case.rows(kind)[livepos]
        ref = W.f64_scores_all(rows, query[None, :])[metric][0]
        real = min(k, livepos.size)
        at = np.minimum(np.searchsorted(livepos, indices[:real].astype(np.int64)), livepos.size - 1)
        assert (livepos[at] == indices[:real].astype(np.int64)).all(), f"{what}: a deleted or unadmitted row was returned"
        rows32 = case.rows32_live(kind) if pos is None else rows.astype(np.float32)
        assert_float_topk(metric, scores, np.concatenate([at.astype(np.uint64), indices[real:]]), ref, rows32, query, k)
        return
    idx, cls = want
    real = cls != "pad"
    d = np.nonzero(indices != idx)[0]
    assert d.size == 0, (f"{what}: the index list is fixed by the rule and differs first at rank {d[0]}: got row {indices[d[0]]} "
                         f"(score {scores[d[0]]!r}), expected row {idx[d[0]]} ({cls[d[0]]})")
    got = class_of(scores)
    d = np.nonzero(got[real] != cls[real])[0]
    assert d.size == 0, f"{what}: rank {d[0]} (row {idx[d[0]]}) has score {scores[d[0]]!r}, expected {cls[d[0]]}"
    assert (scores[~real] == (np.inf if metric == L2 else -np.inf)).all(), f"{what}: padding scores"


# ---- the model of a kernel that flushes f16 subnormals ---------------------------------------------------------------------

def flushed(rows16):
    """What a kernel that flushes Float16 subnormals to zero would see."""
    x = rows16.astype(np.float64)
    return np.where(np.abs(x) < F16_MIN_NORMAL, 0.0, x)


def topk_of_scores(metric, scores64, k):
    """(scores f32 [k], local indices u64 [k]) of ONE query's float64 scores: best first, ties by position, NaN last."""
    key = scores64 if metric == L2 else -scores64
    key = np.where(np.isnan(key), np.inf, key)
    order = np.argsort(key, kind="stable")[:k]
    sc = np.full(k, np.inf if metric == L2 else -np.inf, np.float32)
    idx = np.full(k, PAD, np.uint64)
    sc[:order.size], idx[:order.size] = scores64[order].astype(np.float32), order.astype(np.uint64)
    return sc, idx
