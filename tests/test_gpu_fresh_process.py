"""Answers must not depend on what a process finds in memory the library allocated and has not written yet, nor on which
device call comes first in a process (tests/_fresh_process.py holds the scenarios; DESIGN.md §2, "Poisoned allocations").

Every scenario runs as a child process four times, one after the other: twice as it is, then with every allocation of the
library filled with 0x00 and with 0xFF before its first use (MVF_DEBUG_POISON).  Every run must match the CPU reference --
integer spaces bit for bit, float spaces by tests/_util.py's criterion with DESIGN.md §3's tolerance; the poisoned children
must report the byte they were given; where the two plain runs agree byte for byte, both poisoned runs must equal them byte
for byte; and on the routes whose bits DESIGN.md §3 defines the two plain runs must agree to begin with.

One child at a time, each under tests/_children.py's limit; after a child that faults no further process is started."""
import os
import sys

import numpy as np
import pytest

import _fresh_process as F
import _grouped as GR
import _maxsim as MS
import _maxsim_candidates as MC
import _mmr as MM
import _partitioned as P
from _candidates import candidate_rows
from _children import RUNNER
from _filtered import assert_float_filtered, oracle_filtered
from _radius import assert_float_radius, oracle_radius
from _util import PAD, TOL
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INT = ("i8", "u8")


class Got:
    """the arrays one call left in a child's .npz"""

    def __init__(self, out, key):
        self.scores, self.indices, self.raw = out[key + ".scores"], out[key + ".indices"], out[key + ".raw"]
        self.counts = out.get(key + ".counts")
        self.vectors = out.get(key + ".vectors")


def _check_topk(oracle, rows, dt, metric, queries, k, admit, got, index_base=0, what=""):
    """`got` is the top-k of every query among rows[admit]: integer spaces bit for bit, float spaces within the tolerance"""
    code = F.DT[dt][1]
    assert got.scores.shape == got.indices.shape == got.raw.shape == (len(queries), k), what
    if dt in INT:
        sc, idx, raw = oracle_filtered(oracle, rows, code, metric, queries, k, admit, index_base=index_base)
        assert (got.indices == idx).all(), f"{what}: indices"
        assert (got.raw == raw).all(), f"{what}: raw"
        assert (got.scores.view(np.uint32) == sc.view(np.uint32)).all(), f"{what}: score bits"
        return
    assert (got.raw == 0).all(), f"{what}: raw of a float space"
    for j, q in enumerate(queries):
        assert_float_filtered(oracle, rows, code, metric, q, k, admit, got.scores[j], got.indices[j], index_base=index_base)


def _check_filter_info(info, n, admitted):
    assert info[1] == n and info[2] == admitted and info[0] in (0, 1) and info[3] >= ((n + 31) // 32 + 1) * 4


def expect_s1(oracle, name):
    inp = F.s1_inputs()

    def check(out):
        for k in F.S1_KS:
            got = Got(out, f"k{k}")
            _check_filter_info(out[f"k{k}.filter_info"], 60, 12)
            _check_topk(oracle, inp["rows"], "f32", F.L2, inp["query"], k, inp["allow"], got, what=f"k {k}")
            real = min(k, 12)
            assert (got.indices[0, :real] != PAD).all() and (got.indices[0, real:] == PAD).all(), f"k {k}: 12 rows are admitted"
            assert got.indices[0, :4].tolist() == [20, 25, 15, 30], f"k {k}"
            assert np.round(got.scores[0, :4].astype(np.float64), 1).tolist() == [1.0, 4.0, 6.0, 9.0], f"k {k}"
    return check


def expect_s2(oracle, name):
    route, shape = name.split("_")[1:]
    dt, dim = F.parse_shape(shape)
    inp = F.s2_inputs(dt, dim)
    adm = int(inp["admit"].sum())
    assert adm - 1 >= 1

    def check(out):
        _check_filter_info(out["filter.filter_info"], F.S2_ROWS, adm)
        if route == "r2":
            assert out["filter.filter_info"][0] == 1, "the forced list route builds the list"
        for key, metric, nq, k in F.s2_calls(inp):
            _check_topk(oracle, inp["rows"], dt, metric, inp["queries"][:nq], k, inp["admit"], Got(out, key), F.S2_BASE, key)
    return check


def expect_s3(oracle, name):
    dt, dim = F.parse_shape(name.split("_")[1])
    inp = F.s3_inputs(dt, dim)
    sels = [candidate_rows(inp["cand"][q], F.S2_ROWS, index_base=F.S2_BASE, dead=inp["dead"]) for q in range(F.S3_NQ)]
    assert all(1 <= s.size < F.S3_M for s in sels)

    def check(out):
        for metric in F.METRICS:
            got = Got(out, f"m{metric}")
            assert got.counts.tolist() == [s.size for s in sels], f"metric {metric}: counts"
            for q in range(F.S3_NQ):
                admit = np.zeros(F.S2_ROWS, bool)
                admit[sels[q]] = True
                one = Got({"x.scores": got.scores[q:q + 1], "x.indices": got.indices[q:q + 1], "x.raw": got.raw[q:q + 1]}, "x")
                _check_topk(oracle, inp["rows"], dt, metric, inp["queries"][q:q + 1], F.S3_K, admit, one, F.S2_BASE,
                            f"metric {metric} query {q}")
    return check


def expect_s4(oracle, name):
    dt, dim = F.parse_shape(name.split("_")[1])
    inp = F.s4_inputs(dt, dim)

    def check(out):
        for key, n, metric, nq, k in F.s4_calls():
            _check_topk(oracle, inp[n]["rows"], dt, metric, inp[n]["queries"][:nq], k, np.ones(n, bool), Got(out, key), what=key)
        for metric in F.METRICS:
            got = Got(out, f"fetch_m{metric}")
            _check_topk(oracle, inp[97]["rows"], dt, metric, inp[97]["queries"][:1], 10, np.ones(97, bool), got, what="fetch")
            assert (got.vectors[0] == inp[97]["rows"][got.indices[0].astype(np.int64)]).all(), "the fused payload rows"
    return check


def expect_s5(oracle, name):
    inp = F.s5_inputs(name.split("_")[1])

    def check(out):
        _check_topk(oracle, inp["rows"], inp["dt"], inp["metric"], inp["queries"], F.S5_K, np.ones(F.S5_ROWS, bool), Got(out, "batch"),
                    what=name)
    return check


def expect_s6(oracle, name):
    which = name.split("_")[1]
    inp = F.s6_inputs()
    nbytes = G.shadow6_bytes(F.S6_ROWS, F.S6_DIM) if which == "6b" else F.S6_ROWS * F.S6_DIM

    def check(out):
        for k in F.S6_KS:
            for metric in F.METRICS:
                key = f"m{metric}_k{k}"
                assert out[key + ".scan"].tolist()[:2] == [7, nbytes], f"{key}: the scan streamed the shadow"
                _check_topk(oracle, inp["rows"], "f32", metric, inp["queries"], k, np.ones(F.S6_ROWS, bool), Got(out, key), what=key)
    return check


def expect_s7(oracle, name):
    inp = F.s7_inputs()

    def check(out):
        for key, metric, nq, k in F.s7_calls():
            _check_topk(oracle, inp["rows"], "i8", metric, inp["queries"][:nq], k, np.ones(F.S7_ROWS, bool), Got(out, key), what=key)
    return check


def expect_s8(oracle, name):
    dt = name.split("_")[1]
    code = F.DT[dt][1]
    inp = F.s8_inputs(dt)
    rows, qs, radii = inp["rows"], inp["queries"], inp["radii"]
    want = [oracle_radius(oracle, rows, code, F.L2, qs[j], radii[j], F.S8_MAX) for j in range(3)]
    all_s = [oracle.scores(rows, code, F.L2, qs[j])[0] for j in range(3)]
    assert want[0][0] > G.RADIUS_LIST_CAP and 1 <= want[1][0] <= F.S8_MAX and want[2][0] == 0, [w[0] for w in want]

    def check(out):
        got = Got(out, "lists")
        only = out["counts_only.counts"]
        for j in range(3):
            if dt in INT:
                cnt, sc, idx, raw = want[j]
                assert got.counts[j] == cnt == only[j], f"query {j}: count"
                assert (got.indices[j] == idx).all() and (got.raw[j] == raw).all(), f"query {j}"
                assert (got.scores[j].view(np.uint32) == sc.view(np.uint32)).all(), f"query {j}: score bits"
            else:
                assert got.counts[j] == only[j], f"query {j}: the counts-only call"
                assert_float_radius(F.L2, int(got.counts[j]), got.scores[j], got.indices[j], all_s[j], rows.astype(np.float32),
                                    qs[j], float(radii[j]), F.S8_MAX)
    return check


def expect_s9(oracle, name):
    inp = F.s9_inputs()
    rows, dead = inp["rows"], inp["dead"]
    n, k = F.S9_ROWS, F.S9_K
    want = {}
    for metric in (F.L2, F.IP):
        S = np.full((n, k), np.inf if metric == F.L2 else -np.inf, np.float32)
        I = np.full((n, k), PAD, np.uint64)
        R = np.zeros((n, k), np.int32)
        for i in np.nonzero(~dead)[0]:  # a deleted query row is all padding
            sc, keys, raw = oracle.scores(rows, 2, metric, rows[i])
            comp = (keys.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
            comp[dead] = PAD
            comp[i] = PAD  # never its own neighbour, by position
            pos = (np.sort(np.partition(comp, k - 1)[:k]) & np.uint64(0xFFFFFFFF)).astype(np.int64)
            S[i], I[i], R[i] = sc[pos], pos.astype(np.uint64), raw[pos]
        want[metric] = (S, I, R)

    def check(out):
        for metric in (F.L2, F.IP):
            got = Got(out, f"m{metric}")
            S, I, R = want[metric]
            assert (got.indices == I).all() and (got.raw == R).all(), f"metric {metric}"
            assert (got.scores.view(np.uint32) == S.view(np.uint32)).all(), f"metric {metric}: score bits"
    return check


def expect_s10(oracle, name):
    dt = name.split("_")[1]
    inp = F.s10_inputs(dt)

    def check(out):
        for metric in F.METRICS:
            _check_topk(oracle, inp["rows"], dt, metric, inp["queries"], F.S10_K, np.ones(2 * F.S10_SHARD, bool),
                        Got(out, f"m{metric}"), what=f"metric {metric}")
    return check


# ---- S11 .. S17: the routes over a partition index ------------------------------------------------------------------------------
def _same_call(out, key, fields):
    """the device call left the host call's bytes"""
    for f in fields:
        a, b = out[f"{key}.{f}"], out[f"{key}@device.{f}"]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{key}: the device call's {f} differ from the host call's"


def _row(got, j):
    return Got({"x.scores": got.scores[j:j + 1], "x.indices": got.indices[j:j + 1], "x.raw": got.raw[j:j + 1]}, "x")


def expect_s11(oracle, name):
    dt, dim = F.any_shape(name.split("_")[1])
    inp = F.s11_inputs(dt, dim)
    lay = inp["lay"]
    admits = [np.zeros(F.FI_N, bool) for _ in inp["keys"]]
    for a, key in zip(admits, inp["keys"]):
        a[P.reference_rows(lay, key)] = True
    held = [int(a.sum()) for a in admits]
    assert held == [300, 1, 0, 0, 2] and min(F.S11_KS) < 300 < max(F.S11_KS)

    def check(out):
        for key, metric, nq, k in F.s11_calls():
            got = Got(out, key)
            _same_call(out, key, ("scores", "indices", "raw"))
            for j in range(nq):
                _check_topk(oracle, inp["rows"], dt, metric, inp["queries"][j:j + 1], k, admits[j], _row(got, j), what=f"{key} query {j}")
                assert (got.indices[j, min(k, held[j]):] == PAD).all(), f"{key} query {j}: padding behind the key's {held[j]} rows"
    return check


def expect_s12(oracle, name):
    dt, dim = F.any_shape(name.split("_")[1])
    code = F.DT[dt][1]
    inp = F.s12_inputs(dt, dim)
    lay, rows, q = inp["lay"], inp["rows"], inp["queries"]
    live = GR.live_rows(lay)
    admit = ~lay["dead"]
    ranked = {}
    if dt in INT:  # the oracle's ranking of every held row
        for metric in F.METRICS:
            sc, idx, raw = oracle.search(rows[live], code, metric, q, live.size)
            ranked[metric] = (sc, live[idx.astype(np.int64)].astype(np.uint64), raw)

    def check(out):
        for metric in F.METRICS:
            rk = Got(out, f"rank_m{metric}")
            # the candidate search over every held row is the exact ranking (the oracle's bytes, or its scores within the tolerance)
            _check_topk(oracle, rows, dt, metric, q, live.size, admit, rk, what=f"ranking, metric {metric}")
        for key, metric, per_key, k, nq in F.s12_calls():
            got = Got(out, key)
            _same_call(out, key, ("scores", "indices", "raw"))
            assert got.scores.shape == got.indices.shape == got.raw.shape == (nq, k), key
            rk = ranked[metric] if dt in INT else (out[f"rank_m{metric}.scores"], out[f"rank_m{metric}.indices"], out[f"rank_m{metric}.raw"])
            for j in range(nq):
                places = GR.grouped_walk(rk[1][j].astype(np.int64), lay["col"], per_key, k)
                s, i, r = GR.expected(rk[0][j], rk[1][j], rk[2][j], places, k, metric)
                assert (got.indices[j] == i).all() and (got.raw[j] == r).all(), f"{key} query {j}: the walk's rows"
                assert (got.scores[j].view(np.uint32) == s.view(np.uint32)).all(), f"{key} query {j}: score bits"
    return check


def _float_sets_reference(inp):
    """{metric: (b, tol)} of every token of the pool, float64 (tests/_maxsim.py f64_key_bests; DESIGN.md §3's tolerance)"""
    nq, T, dim = inp["pool"].shape
    return MS.f64_key_bests(inp["rows"], inp["lay"], inp["pool"].reshape(nq * T, dim), TOL)


def _check_maxsim_float(got, f64, key_values, metric, nq, T, k, pool_T, what):
    nk = key_values.size
    kk = min(k, nk)
    b, tol = f64[metric]
    assert got.counts.tolist() == [kk] * nq, f"{what}: counts"
    assert (got.keys[:, kk:] == PAD).all() and (got.scores[:, kk:] == (np.inf if metric == F.L2 else -np.inf)).all(), f"{what}: padding"
    for j in range(nq):
        sl = slice(j * pool_T, j * pool_T + T)
        MS.assert_f64_contract(got.scores[j, :kk], got.keys[j, :kk], key_values, b[sl].sum(0), tol[sl].sum(0), metric, kk)


class GotMs:
    def __init__(self, out, key):
        self.scores, self.keys, self.counts = out[key + ".scores"], out[key + ".keys"], out[key + ".counts"]


def _maxsim_expect(inp, dt, dim, calls):
    """check(out) of a multi-vector scenario: Int8 the exact reference byte for byte, floats the float64 contract; the device
    call the host call's bytes"""
    lay = inp["lay"]
    key_values = MS.key_order(lay)[3]
    pool_T = inp["pool"].shape[1]
    assert min(F.MS_KS) < key_values.size < max(F.MS_KS), "k below and above the keys that hold rows"
    f64 = None if dt in INT else _float_sets_reference(inp)
    want = {}
    if dt in INT:
        for key, metric, T, nq, k in calls:
            want[key] = MS.int_reference(inp["rows"], lay, F.ms_sets(inp, nq, T), metric, k)

    def check(out):
        for key, metric, T, nq, k in calls:
            got = GotMs(out, key)
            _same_call(out, key, ("scores", "keys", "counts"))
            assert got.scores.shape == got.keys.shape == (nq, k) and got.counts.shape == (nq,), key
            if dt in INT:
                sc, ky, cnt = want[key]
                assert (got.keys == ky).all() and (got.counts == cnt).all(), f"{key}: keys"
                assert (got.scores.view(np.uint32) == sc.view(np.uint32)).all(), f"{key}: score bits"
            else:
                _check_maxsim_float(got, f64, key_values, metric, nq, T, k, pool_T, key)
    return check


def expect_s13(oracle, name):
    dt, dim = F.any_shape(name.split("_")[1])
    return _maxsim_expect(F.ms_inputs("s13", dt, dim), dt, dim, list(F.ms_calls()))


def expect_s14(oracle, name):
    dt, dim, metric = F.S14_CASES[name.split("_")[1]]
    inp = F.ms_inputs("s14", dt, dim)
    calls = list(F.ms_calls((metric,)))
    contract = _maxsim_expect(inp, dt, dim, calls)
    route1 = {}  # route 2's answer is route 1's bytes -- route 1 on a handle of this process
    with G.GpuCorpus.from_array(inp["rows"]) as c:
        c.set_tombstones(np.packbits(inp["lay"]["dead"], bitorder="little"))
        with c.attach_column(inp["lay"]["col"]) as col, c.make_partition(col) as part:
            c.set_maxsim_route(1)
            for key, m, T, nq, k in calls:
                route1[key] = c.search_maxsim(F.ms_sets(inp, nq, T), k, m, part)

    def check(out):
        contract(out)
        assert (out["candidates"] >= F.MS_KS[0]).all() and (out["blocks"] >= 1).all(), "the child's handle selected by the MFMA route"
        for key, *_ in calls:
            got, want = GotMs(out, key), route1[key]
            assert (got.keys == want.keys).all() and (got.counts == want.counts).all(), f"{key}: route 1's keys"
            assert (got.scores.view(np.uint32) == want.scores.view(np.uint32)).all(), f"{key}: route 1's score bits"
    return check


def s15_held(inp):
    """per list the distinct candidates that hold rows, from the layout alone"""
    held = P.group_by(inp["lay"])[0]
    return held, [MC.held_distinct(l, held) for l in inp["lists"]]


def expect_s15(oracle, name):
    dt, dim = F.any_shape(name.split("_")[1])
    inp = F.s15_inputs(dt, dim)
    lay, sets, lists = inp["lay"], inp["sets"], inp["lists"]
    nq, T = sets.shape[:2]
    held, mine = s15_held(inp)
    nk = held.size
    assert all(1 <= m.size < F.S15_M for m in mine) and max(F.S15_KS) > F.S15_M
    if dt in INT:
        full_ref = {metric: MS.int_reference(inp["rows"], lay, sets, metric, nk) for metric in F.METRICS}
    else:
        f64 = MS.f64_key_bests(inp["rows"], lay, sets.reshape(nq * T, dim), TOL)

    def check(out):
        for metric in F.METRICS:
            full = GotMs(out, f"full_m{metric}")
            if dt in INT:
                sc, ky, cnt = full_ref[metric]
                assert (full.keys == ky).all() and (full.scores.view(np.uint32) == sc.view(np.uint32)).all(), f"metric {metric}: the full search"
            for k in F.S15_KS:
                key = f"m{metric}_k{k}"
                got = GotMs(out, key)
                _same_call(out, key, ("scores", "keys", "counts"))
                sc, ky, cnt = MC.filter_full(full.scores, full.keys, nk, lists, held, k, metric)
                assert (got.counts == cnt).all() and got.counts.tolist() == [min(k, m.size) for m in mine], f"{key}: counts"
                assert (got.keys == ky).all(), f"{key}: the full search's keys, filtered"
                assert (got.scores.view(np.uint32) == sc.view(np.uint32)).all(), f"{key}: the full search's score bits, filtered"
                if dt not in INT:  # and the float64 contract among the list's own keys
                    b, tol = f64[metric]
                    for j in range(nq):
                        at = np.searchsorted(held, mine[j])
                        kk = min(k, mine[j].size)
                        sl = slice(j * T, (j + 1) * T)
                        MS.assert_f64_contract(got.scores[j, :kk], got.keys[j, :kk], mine[j], b[sl].sum(0)[at], tol[sl].sum(0)[at], metric, kk)
    return check


class _Replay:
    """tests/_mmr.py `recipe` asks a corpus for three things; this one answers from what the child saved"""

    def __init__(self, out, metric, j, rows):
        self.out, self.metric, self.j, self.rows, self.asked = out, metric, j, rows, 0

    def search_candidates(self, q, entries, m, metric):
        assert metric == self.metric
        key = ("rel" if self.asked == 0 else "sim") + f"_m{metric}_q{self.j}"
        self.asked += 1
        return G.CandidateResult(self.out[key + ".scores"], self.out[key + ".indices"], self.out[key + ".raw"], self.out[key + ".counts"])

    def gather_rows(self, pos):
        return self.rows[np.asarray(pos).astype(np.int64)]


def expect_s16(oracle, name):
    inp = F.s16_inputs()
    rows, q, lists = inp["rows"], inp["queries"], inp["lists"]
    nq = q.shape[0]
    sels = [candidate_rows(lists[j], F.S16_N) for j in range(nq)]
    assert sels[0].size == F.S16_M and 1 <= sels[1].size < F.S16_M

    def check(out):
        for metric in (F.COS, F.L2):
            for j in range(nq):  # the recipe's ingredients are the exact candidate searches
                rel = Got(out, f"rel_m{metric}_q{j}")
                admit = np.zeros(F.S16_N, bool)
                admit[sels[j]] = True
                assert rel.counts.tolist() == [sels[j].size]
                _check_topk(oracle, rows, "f32", metric, q[j:j + 1], F.S16_M, admit, rel, what=f"relevance, metric {metric}, query {j}")
                sim = Got(out, f"sim_m{metric}_q{j}")
                for s in (0, sels[j].size - 1):
                    _check_topk(oracle, rows, "f32", metric, rows[sels[j][s]][None, :], F.S16_M, admit, _row(sim, s),
                                what=f"similarity, metric {metric}, query {j}, row {s}")
            for lam in F.S16_LAMBDAS:
                key = f"l{lam}_m{metric}"
                _same_call(out, key, ("scores", "indices", "raw", "objective", "counts"))
                got = G.MmrResult(out[key + ".scores"], out[key + ".indices"], out[key + ".raw"], out[key + ".counts"], out[key + ".objective"])
                for j in range(nq):
                    MM.assert_rows_equal(got, MM.recipe(_Replay(out, metric, j, rows), metric, q[j], lists[j], F.S16_K, lam), j, key)
                if metric == F.COS:  # the planted world: relevance alone takes the eight copies first, lambda 0.5 takes one
                    picked = np.isin(got.indices[0][:8], inp["copies"])
                    assert picked.all() if lam == 1.0 else picked.sum() == 1, f"{key}: the copies among the first eight picks"
    return check


def s17_reference():
    """(documents ascending, float64 sums, tolerances, the candidate documents that hold rows): the float64 contract of the
    documents example, in numpy"""
    inp = F.s17_inputs()
    rows, doc, q = inp["rows"].astype(np.float64), inp["doc"], inp["query"].astype(np.float64)
    d = np.sqrt(((rows[None, :, :] - q[:, None, :]) ** 2).sum(2))   # [T, n] L2
    docs = np.unique(doc)
    b = np.stack([d[:, doc == g].min(1) for g in docs], axis=1)      # [T, documents]
    return docs, b.sum(0), (TOL * np.abs(b)).sum(0), MC.held_distinct(inp["cand"], docs)


def check_s17_answer(full_scores, full_keys, cand_scores, cand_keys, ref=None):
    """the documents line (k = S17_K) and the re-ranked line of one process against the float64 contract"""
    docs, S, tol, held = ref or s17_reference()
    MS.assert_f64_contract(full_scores, full_keys, docs, S, tol, F.L2, F.S17_K)
    at = np.searchsorted(docs, held)
    assert len(cand_keys) == min(F.S17_K, held.size), "the candidates that hold rows"
    MS.assert_f64_contract(cand_scores, cand_keys, held, S[at], tol[at], F.L2, len(cand_keys))


def expect_s17(oracle, name):
    steps = F.S17_STEPS[name.split("_")[1]]
    inp = F.s17_inputs()
    ref = s17_reference()
    docs, S, tol, held = ref
    assert docs.size == F.S17_DOCS and held.size == 5, "4, 9, 0, 13, 21: the repeats, 77 and the pad are skipped"

    def check(out):
        tags = [f"step{i}_{s}" for i, s in enumerate(steps)]
        full = GotMs(out, next(t for t, s in zip(tags, steps) if s == "full"))
        assert full.counts.tolist() == [F.S17_DOCS] and (np.sort(full.keys[0, :F.S17_DOCS]) == docs).all()
        MS.assert_f64_contract(full.scores[0, :F.S17_DOCS], full.keys[0, :F.S17_DOCS], docs, S, tol, F.L2, F.S17_DOCS)
        want = MC.filter_full(full.scores, full.keys, F.S17_DOCS, inp["cand"][None, :], docs, F.S17_K, F.L2)
        cands = []
        for tag, step in zip(tags, steps):
            if step == "full":
                top = GotMs(out, tag + "_k")
                assert top.counts.tolist() == [F.S17_K] and (top.keys[0] == full.keys[0, :F.S17_K]).all()
                assert (top.scores[0].view(np.uint32) == full.scores[0, :F.S17_K].view(np.uint32)).all(), f"{tag}: k = {F.S17_K} is the head of the full list"
            elif step == "cand":
                got = GotMs(out, tag)
                cands.append(got)
                check_s17_answer(full.scores[0, :F.S17_K], full.keys[0, :F.S17_K], got.scores[0, :5], got.keys[0, :5], ref)
                assert got.counts.tolist() == [5] and (got.keys == want[1]).all(), f"{tag}: the same child's full answer, filtered"
                assert (got.scores.view(np.uint32) == want[0].view(np.uint32)).all(), f"{tag}: the same child's full answer's score bits, filtered"
            elif step == "empty":
                got = GotMs(out, tag)
                assert got.counts.tolist() == [0] and (got.keys == PAD).all() and np.isposinf(got.scores).all(), f"{tag}: no candidates"
            elif step == "perkey":
                got = Got(out, tag)
                for j, key in enumerate(inp["cand"][[0, 3, 4]]):
                    _check_topk(oracle, inp["rows"], "f32", F.L2, inp["query"][j:j + 1], F.S17_K, inp["doc"] == key, _row(got, j), what=f"{tag} query {j}")
            elif step == "grouped":
                got = Got(out, tag)
                for j in range(F.S17_T):  # one row per document: every hit the best row of its document, documents in the order of those
                    hit = got.indices[j].astype(np.int64)
                    assert np.unique(inp["doc"][hit]).size == F.S17_K, f"{tag} query {j}: one row per document"
                    d = np.sqrt(((inp["rows"].astype(np.float64) - inp["query"][j].astype(np.float64)) ** 2).sum(1))
                    best = np.array([d[inp["doc"] == g].min() for g in docs])
                    assert np.allclose(got.scores[j], np.sort(best)[:F.S17_K], rtol=TOL, atol=0), f"{tag} query {j}: the documents' best rows"
                    assert np.allclose(got.scores[j], d[hit], rtol=TOL, atol=0), f"{tag} query {j}: the hits' own distances"
        for later in cands[1:]:
            for f in ("scores", "keys", "counts"):
                assert getattr(later, f).tobytes() == getattr(cands[0], f).tobytes(), f"the second candidate call's {f} differ from the first's"
    return check


EXPECT = dict(s1=expect_s1, s2=expect_s2, s3=expect_s3, s4=expect_s4, s5=expect_s5, s6=expect_s6, s7=expect_s7, s8=expect_s8,
              s9=expect_s9, s10=expect_s10, s11=expect_s11, s12=expect_s12, s13=expect_s13, s14=expect_s14, s15=expect_s15,
              s16=expect_s16, s17=expect_s17)


def _child(name, tag, poison, tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("MVF_DEBUG_POISON", "MVF_FILTER_ROUTE", "MVF_LARGE_K", "MVF_MAXSIM_ROUTE", "MVF_MAXSIM_SCRATCH_BYTES")}
    if poison is not None:
        env["MVF_DEBUG_POISON"] = str(poison)
    path = str(tmp_path / f"{tag}.npz")
    out = RUNNER.run([sys.executable, os.path.join(HERE, "_fresh_process.py"), name, path], env=env)
    assert out.returncode == 0, f"{name} ({tag}): exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    assert arrays["poison"].tolist() == [-1 if poison is None else poison], f"{name} ({tag}): the child's poison byte"
    return arrays


def _differences(a, b):
    """the arrays of two runs that differ in shape, type or bytes (the poison byte itself aside)"""
    keys = sorted((set(a) | set(b)) - {"poison"})
    return [k for k in keys if k not in a or k not in b or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
            or a[k].tobytes() != b[k].tobytes()]


@pytest.mark.parametrize("name", list(F.scenarios()))
def test_fresh_process_answers_do_not_depend_on_stale_memory(oracle, tmp_path, name):
    bit_defined = F.scenarios()[name]
    check = EXPECT[name.split("_")[0]](oracle, name)
    first = _child(name, "plain1", None, tmp_path)
    second = _child(name, "plain2", None, tmp_path)
    check(first)
    plain_differ = _differences(first, second)
    if plain_differ:  # (a run that equals a checked one byte for byte has been checked)
        check(second)
    print(f"{name}: plain runs differ in {plain_differ or 'nothing'}")
    if bit_defined:
        assert not plain_differ, f"two plain runs of a bit-defined route differ in {plain_differ}"
    for tag, byte in (("poison00", 0x00), ("poisonFF", 0xFF)):  # 0x00 first: what it shows is diagnosed before 0xFF runs
        run = _child(name, tag, byte, tmp_path)
        diff = _differences(first, run)
        print(f"{name}: {tag} differs from the plain run in {diff or 'nothing'}")
        if not plain_differ:
            assert not diff, f"allocations filled with {byte:#04x} change {diff}"
        if diff:
            check(run)
