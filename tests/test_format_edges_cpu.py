"""The format-edge corpora of tests/_edges.py without a GPU: the corpora are exactly what they claim, every twin identity holds
on the oracle bit for bit (the expectation of tests/test_gpu_format_edges.py, proven without the library), the oracle lies
within a quarter of §3's tolerance of float64 on them, every case yields its 64 thin-band queries, the edge-query table of
DESIGN.md §3 is what the oracle returns, and a numpy model of a kernel that flushes Float16 subnormals is rejected."""
import numpy as np
import pytest

import _edges as E
import _wide as W
from _util import PAD, assert_float_topk

CASES = E.all_cases()
IDS = [f"{n}-{'f16' if d == E.F16 else 'f32'}" for n, d in CASES]
F16_CASES = [c for c in CASES if c[1] == E.F16]
ORACLE_FRACTION = 0.25   # of §3's tolerance; measured: at most 0.117, at 3000 x 1536 Float16 (DESIGN.md §2 "Format edges")


def oracle_live(oracle, case, kind, metric, q, k):
    """oracle.search over the live rows of one corpus, mapped back to positions."""
    pos = case.livepos
    sc, idx, _ = oracle.search(np.ascontiguousarray(case.rows(kind)[pos]), case.dtype, metric, q, k)
    real = idx != PAD
    out = np.full(idx.shape, PAD, np.uint64)
    out[real] = pos[idx[real].astype(np.int64)].astype(np.uint64)
    return sc, out


@pytest.mark.parametrize("name,dtype", CASES, ids=IDS)
def test_corpora_are_exactly_representable(oracle, name, dtype):
    case = E.get_case(oracle, name, dtype)
    for kind, exact in case.exact.items():
        assert (case.rows(kind).astype(np.float64) == exact).all(), f"{kind} is not exact in its storage type"
        assert np.isfinite(case.rows(kind).astype(np.float64)).all()
        assert (np.sqrt((exact[case.livepos] ** 2).sum(1)) > 0).all(), f"{kind}: an all-zero live row"
    assert (case.exact[E.BASE_OF[dtype]][:, case.col] == 0).sum() >= 4, "rows with a zero in the +Inf column are planted"
    if dtype == E.F16:
        m = case.m
        assert m.min() == -1023 and m.max() == 1023
        s, t, h, r = (case.rows(kd).astype(np.float64) for kd in "STHR")
        assert (s == m * 2.0 ** -24).all() and (np.abs(s[s != 0]) < E.F16_MIN_NORMAL).all(), "S: every non-zero element is subnormal"
        assert (np.abs(h[h != 0]) >= E.F16_MIN_NORMAL).all(), "H: normal or zero"
        assert np.abs(t).max() == 32736.0 and np.abs(t).max() < 65504
        sub = (np.abs(r) < E.F16_MIN_NORMAL) & (r != 0)
        assert not sub[case.rshift >= -4].any() and (np.abs(r[case.rshift == -14]) < E.F16_MIN_NORMAL).all(), "R: fully normal to fully subnormal"
        assert len(np.unique(case.rshift)) == E.R_PERIOD
    else:
        f = case.exact["F"]
        assert np.abs(f[f != 0]).min() >= 2.0 ** -23 and np.abs(f).max() <= 1.0
    assert (case.dead is not None) == case.tomb and (not case.tomb or abs(case.dead.mean() - 0.2) < 1e-3)


def test_half_of_the_cases_carry_tombstones():
    for group in (list(E.BATCHED.values()), *[list(E.K1_SHAPES[d].values()) for d in (E.F16, E.F32)]):
        share = np.mean([s[3] for s in group])
        assert 0.4 <= share <= 0.6, share


@pytest.mark.parametrize("name,dtype", CASES, ids=IDS)
def test_every_case_yields_its_thin_band_queries(oracle, name, dtype):
    """A condition on the inputs, from the float64 reference alone: 64 of the pool's 80 queries have at most k // 10 rows
    beside the k-th inside the boundary band for every metric and k -- on the base corpus and on R (the exact twins have the
    base's band).  A case that fails changes its seed."""
    case = E.get_case(oracle, name, dtype)
    assert len(case.thin()) == E.NQ, f"{case.tag}: only {len(case.thin())} thin-band queries in a pool of {E.POOL}"
    for kind in E.TWINS_OF[dtype]:   # the band of a twin, recounted on the twin itself
        ref = case.ref64(kind)
        for metric in E.METRICS:
            q = case.queries_for(kind, metric)
            for k in E.KS:
                for j in range(0, E.NQ, 9):
                    assert W.band_count(metric, ref[metric][j], case.rows32_live(kind), q[j], k) <= k // 10


@pytest.mark.parametrize("name,dtype", CASES, ids=IDS)
def test_twin_identities_hold_on_the_oracle_bit_for_bit(oracle, name, dtype):
    case = E.get_case(oracle, name, dtype)
    base, k = E.BASE_OF[dtype], max(E.KS)
    for metric in E.METRICS:
        bsc, bidx = oracle_live(oracle, case, base, metric, case.q, k)
        for kind in E.TWINS_OF[dtype]:
            e = E.twin_shift(kind, metric)
            if e is None:
                continue
            tsc, tidx = oracle_live(oracle, case, kind, metric, case.queries_for(kind, metric), k)
            for j in range(E.NQ):
                d = E.twin_difference(bsc[j], bidx[j], tsc[j], tidx[j], e)
                assert d is None, f"{case.tag} {kind} vs {base} metric {metric} query {j}: {d}"


@pytest.mark.parametrize("name,dtype", CASES, ids=IDS)
def test_scaled_queries_on_fixed_rows_on_the_oracle(oracle, name, dtype):
    """ldexp(q, +-40): InnerProduct scales exactly, Cosine is identical."""
    case = E.get_case(oracle, name, dtype)
    kind = "S" if dtype == E.F16 else "F"
    q = case.q[:16]
    for metric in (E.IP, E.COS):
        bsc, bidx = oracle_live(oracle, case, kind, metric, q, 100)
        for e in (-40, 40):
            tsc, tidx = oracle_live(oracle, case, kind, metric, np.ldexp(q, e).astype(np.float32), 100)
            for j in range(len(q)):
                d = E.twin_difference(bsc[j], bidx[j], tsc[j], tidx[j], e if metric == E.IP else 0)
                assert d is None, f"{case.tag} {kind} query 2^{e} metric {metric} query {j}: {d}"


@pytest.mark.parametrize("name,dtype", CASES, ids=IDS)
def test_the_oracle_agrees_with_float64_on_the_twins(oracle, name, dtype):
    """The oracle is the thing measured here: its strict-order f32 rounding in units of §3's tolerance."""
    case = E.get_case(oracle, name, dtype)
    worst = 0.0
    for kind in E.TWINS_OF[dtype]:
        ref = case.ref64(kind)
        rows = np.ascontiguousarray(case.rows(kind)[case.livepos])
        for metric in E.METRICS:
            q = case.queries_for(kind, metric)
            for j in range(0, E.NQ, 8):
                got = oracle.scores(rows, dtype, metric, q[j])[0]
                frac = W.tolerance_fraction(metric, got, ref[metric][j], rows, q[j])
                worst = max(worst, frac)
                assert frac <= ORACLE_FRACTION, f"{case.tag} {kind} metric {metric} query {j}: {frac:.3f} of the tolerance"
    print(f"{case.tag}: oracle vs float64 at most {worst:.3f} of the tolerance")


@pytest.mark.parametrize("name,dtype", CASES, ids=IDS)
def test_the_edge_query_table_holds_on_the_oracle(oracle, name, dtype):
    case = E.get_case(oracle, name, dtype)
    kinds = ("S", "R") if dtype == E.F16 else ("F", "Fdn")
    base = case.edge_base()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(np.sum(np.ldexp(base, 64).astype(np.float32) ** 2, dtype=np.float32)))
    assert np.sum(np.ldexp(base, -130).astype(np.float32) ** 2, dtype=np.float32) == 0 and (np.ldexp(base, -130).astype(np.float32) != 0).any()
    full = name in ("d4", "d200")   # k = every live row: all three classes of the +Inf query and both boundaries in one list
    for kind in kinds:
        for qname, q in case.edge_queries().items():
            for metric in E.METRICS:
                for k in (10, case.livepos.size + 3) if full else (10,):
                    sc, idx = oracle_live(oracle, case, kind, metric, q[None, :], k)
                    E.assert_edge(case, kind, qname, metric, q, sc[0], idx[0], k, what=f"{case.tag} {kind} query {qname} metric {metric} k {k}")
        if full:
            _, cls = E.edge_expectation("inf", E.IP, case.exact[kind][:, case.col], case.livepos, case.livepos.size)
            assert {"+inf", "-inf", "nan"} <= set(cls.tolist())


def test_the_edge_checker_rejects_wrong_answers(oracle):
    case = E.get_case(oracle, "d16", E.F16)
    q = case.edge_queries()
    sc, idx = oracle_live(oracle, case, "S", E.COS, q["2^-130"][None, :], 10)
    E.assert_edge(case, "S", "2^-130", E.COS, q["2^-130"], sc[0], idx[0], 10)
    with pytest.raises(AssertionError, match="fixed by the rule"):
        E.assert_edge(case, "S", "2^-130", E.COS, q["2^-130"], sc[0], idx[0][::-1], 10)
    with pytest.raises(AssertionError, match="expected zero"):
        E.assert_edge(case, "S", "2^-130", E.COS, q["2^-130"], sc[0] + np.float32(1e-3), idx[0], 10)
    sc, idx = oracle_live(oracle, case, "S", E.IP, q["inf"][None, :], 10)
    with pytest.raises(AssertionError, match="expected \\+inf"):
        E.assert_edge(case, "S", "inf", E.IP, q["inf"], np.full(10, np.nan, np.float32), idx[0], 10)
    a = oracle_live(oracle, case, "H", E.IP, case.q[:1], 10)
    assert E.twin_difference(a[0][0], a[1][0], np.ldexp(a[0][0], -14), a[1][0], -14) is None
    assert "score bits" in E.twin_difference(a[0][0], a[1][0], np.nextafter(np.ldexp(a[0][0], -14), np.float32(9)), a[1][0], -14)


# ---- teeth: a kernel that flushes Float16 subnormals to zero ---------------------------------------------------------------

@pytest.mark.parametrize("name,dtype", F16_CASES, ids=[i for i, c in zip(IDS, CASES) if c[1] == E.F16])
def test_a_kernel_that_flushes_f16_subnormals_is_rejected(oracle, name, dtype):
    """Elements with |x| < 2^-14 become 0, the scores are float64 of what is left, the lists are its top-k.  On S the flushed
    corpus is all zeros: every metric's answer must fall, by `assert_float_topk` against float64 AND by the twin comparison
    with the oracle's answer on H.  On R the rows scaled below 2^-4 lose elements.  Under Cosine every scale is equally likely
    to hold a best row: both checks again.  Under L2 the queries sit at 2^-14, so the nearest rows are the fully subnormal
    ones, which the flush turns into zeros: `assert_float_topk` must reject it (R has no L2 twin identity).  At least 90 % of
    the 64 queries of every case.  R under InnerProduct is the one combination WITHOUT teeth and is not asserted: a row's
    score grows with its scale, so the best rows are the large, unflushed ones and the flushed answer is the right one (the
    last lines count it: no query may be rejected, or this sentence is wrong).  InnerProduct's teeth are S's."""
    case = E.get_case(oracle, name, dtype)
    for kind, metrics in (("S", E.METRICS), ("R", (E.L2, E.COS))):
        fl = E.flushed(case.rows(kind)[case.livepos])
        if kind == "S":
            assert (fl == 0).all()
        else:
            lost = (fl != case.exact[kind][case.livepos]).any(1)
            rs = case.rshift[case.livepos]
            assert lost[rs == -14].all() and lost[rs < -4].any() and not lost[rs >= -4].any()
        ref = case.ref64(kind)
        for metric in metrics:
            q = case.queries_for(kind, metric)
            wrong = W.f64_scores_all(fl, q)[metric]
            e = E.twin_shift(kind, metric)
            for k in E.KS:
                bsc, bidx = oracle_live(oracle, case, "H", metric, case.q, k)
                by_topk = by_twin = 0
                for j in range(E.NQ):
                    sc, local = E.topk_of_scores(metric, wrong[j], k)
                    try:
                        assert_float_topk(metric, sc, local, ref[metric][j], case.rows32_live(kind), q[j], k)
                    except AssertionError:
                        by_topk += 1
                    real = local != PAD
                    pos = np.full(k, PAD, np.uint64)
                    pos[real] = case.livepos[local[real].astype(np.int64)].astype(np.uint64)
                    by_twin += e is not None and E.twin_difference(bsc[j], bidx[j], sc, pos, e) is not None
                what = f"{case.tag} {kind} metric {metric} k {k}"
                assert by_topk >= 0.9 * E.NQ, f"{what}: assert_float_topk rejects only {by_topk} of {E.NQ} flushed answers"
                assert e is None or by_twin >= 0.9 * E.NQ, f"{what}: the twin comparison rejects only {by_twin} of {E.NQ} flushed answers"
    fl = E.flushed(case.rows("R")[case.livepos])
    wrong = W.f64_scores_all(fl, case.q)[E.IP]
    for k in E.KS:
        rejected = 0
        for j in range(E.NQ):
            sc, local = E.topk_of_scores(E.IP, wrong[j], k)
            try:
                assert_float_topk(E.IP, sc, local, case.ref64("R")[E.IP][j], case.rows32_live("R"), case.q[j], k)
            except AssertionError:
                rejected += 1
        assert rejected == 0, f"{case.tag} R InnerProduct k {k}: {rejected} flushed answers rejected -- it has teeth after all, assert them"
