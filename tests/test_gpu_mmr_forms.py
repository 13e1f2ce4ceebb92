"""-m gpu tests of the diversified re-ranking on every form of its walk kernel D0 (DESIGN.md §5 "D0"): the six lane widths of
each data type, both sides of the switch between the picked row staged in LDS and read back through the cache, the widest
integer rows, and the widths only MVF_K1_G reaches.  The table of cases is tests/_mmr.py's FORM_CELLS / FORCED_CELLS;
mvfgpu_selftest_mmr_form says which instantiation a case runs, and every test asserts it before it searches.  Two yardsticks
per case and metric: the recipe of candidate searches (byte for byte) and a reference independent of every kernel -- exact
integers for Int8 / UInt8 (byte for byte), the walk in float64 held along the kernel's own path for the float types (the pick
within the band of the float64 maximum and equal to it at a clear step, objective and score within a tolerance derived from
§3's).  Lists of 65 / 257 / 1000 / 1024 rows (65 / 257 from 10240 dimensions on, over 300 rows), k = m, 3 (8 through the
cache) and 32, one and three queries.  Behind them: duplicate rows whose tied copies straddle every ownership edge of the
block, and Float16 corpora of subnormal values with their power-of-two twins.
Run time on an MI355X: the 47 tests take 20 s together, the slowest 2 s (the first: it also pays the first use of the device;
every other one at most 0.75 s).  Nothing was cut: every case runs every metric.  The largest float error measured is 0.035
of the tolerance (printed per case and metric before it is asserted); 12 of the 66 float walks met one unclear step of 32 on
the kernel's path, none more.  Device code of D0 unchanged by the self-test: the tests pass on the kernel as it was."""
import numpy as np
import pytest

import _dups as D
import _edges as E
import _mmr as MM
from _candidates import candidate_rows
from _util import TOL
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
METRICS = (L2, IP, COS)
FORM_IDS = [f"{dt}d{dim}" for dt, dim in MM.FORM_CASES]
FORCED_IDS = [f"{dt}d{dim}g{w}" for dt, dim, w in MM.FORCED_CASES]


def assert_cell(dt, dim, forced=0):
    """the instantiation the case is listed for is the one the launch takes"""
    cell = MM.FORCED_CELLS[dt, dim, forced] if forced else MM.FORM_CELLS[dt, dim]
    f = G.mmr_form(MM.DTYPE[dt], dim, forced)
    assert tuple(f) == cell, f"{dt} x {dim}, forced width {forced}: listed as {cell}, the library says {f}"
    return f


def run_case(c, rows, qs, dt, dim, ci, qlds):
    """every call of a case on the handle c, against both yardsticks"""
    n = rows.shape[0]
    f64 = None
    for mi, metric in enumerate(METRICS):
        calls = MM.form_calls(ci, mi, dim, qlds)
        for ti, (m, k, lam, nq) in enumerate(calls):
            what = f"{dt} x {dim}, metric {metric}, m {m}, k {k}, lambda {lam}, nq {nq}"
            follow = ti == len(calls) - 1          # the call the float64 check follows
            lists = MM.f64_list(dt, dim, n, m)[None, :] if follow else MM.form_lists(dt, dim, (metric, ti), n, nq, m)
            if not qlds:
                assert m >= 65 and k >= 8, "through the cache: every wave scores, in more than one pass, over several rewrites"
            got = c.search_mmr(qs[:nq], lists, k, lam, metric)
            assert int(got.counts[0]) == m
            for j in range(nq):
                MM.assert_rows_equal(got, MM.recipe(c, metric, qs[j], lists[j], k, lam), j, what + ": the recipe")
                if MM.is_int(dt):
                    MM.assert_rows_equal(got, MM.int_reference(rows, lists[j], qs[j], metric, lam, k), j, what + ": exact")
            if follow and not MM.is_int(dt):
                sel = candidate_rows(lists[0], n)
                if f64 is None:
                    f64 = MM.f64_terms(rows[sel], qs[0], TOL)
                picks = np.searchsorted(sel, got.indices[0][:k].astype(np.int64))
                unclear, frac = MM.f64_walk(metric, lam, f64[metric], k, picks, got.objective[0], got.scores[0])
                print(f"{what}: {frac:.3f} of the tolerance, {unclear} unclear steps of {k}")
                assert unclear <= MM.F64_DEVICE_UNCLEAR_MAX, f"{what}: {unclear} unclear steps on the kernel's path"


@pytest.mark.parametrize("case", range(len(MM.FORM_CASES)), ids=FORM_IDS)
def test_every_form_is_the_recipe_and_the_independent_reference(case):
    """a / b. every case and metric, the calls of MM.form_calls: search_mmr is the recipe byte for byte, and the exact integer
    reference byte for byte (Int8 / UInt8) or within the float64 walk's band and tolerances (Float32 / Float16)"""
    dt, dim = MM.FORM_CASES[case]
    f = assert_cell(dt, dim)
    rows, qs = MM.form_world(dt, dim)
    with G.GpuCorpus.from_array(rows) as c:
        run_case(c, rows, qs, dt, dim, case, f.qlds)


@pytest.mark.parametrize("case", range(len(MM.FORCED_CASES)), ids=FORCED_IDS)
def test_forced_widths(case, monkeypatch):
    """MVF_K1_G, read when the handle is created: 64 lanes on rows of 5 vectors, and 16 lanes at dimension 10241 -- the one
    way to the through-the-cache form with fewer than 64 lanes per row"""
    dt, dim, width = MM.FORCED_CASES[case]
    f = assert_cell(dt, dim, width)
    rows, qs = MM.form_world(dt, dim)
    monkeypatch.setenv("MVF_K1_G", str(width))
    c = G.GpuCorpus.from_array(rows)
    monkeypatch.delenv("MVF_K1_G")
    try:
        run_case(c, rows, qs, dt, dim, len(MM.FORM_CASES) + case, f.qlds)
    finally:
        c.close()


def same_bytes(a, b, what):
    for name in ("scores", "indices", "raw", "counts", "objective"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), f"{what}: {name}"


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", [G.FLOAT32, G.FLOAT16])
def test_tied_copies_at_the_ownership_edges(dtype, metric):
    """24 distinct vectors in skewed copy counts, 1024 listed positions, every one picked: untaken copies of a vector hold
    bit-equal objectives at every step, between positions of different waves, of different 256-strides and of one thread's two
    strides -- the recipe's bytes, the copies of each vector in ascending position, and identity 3"""
    cp = D.corpus_b(MM.DUP_SEED + dtype, MM.DUP_N, MM.DUP_DIM, dtype)
    lst = MM.dup_list()
    m = lst.size
    groups = cp.group_of[lst.astype(np.int64)]
    assert m == 1024 and np.unique(lst).size == m and MM.tie_edges(groups) == (True, True, True)
    q = D.gaussian_queries(MM.DUP_SEED + 7, 1, MM.DUP_DIM)
    rng = np.random.default_rng(MM.DUP_SEED + metric)
    with G.GpuCorpus.from_array(cp.rows) as c:
        for lam in (0.3, 1.0):
            what = f"dtype {dtype}, metric {metric}, lambda {lam}"
            got = c.search_mmr(q, lst[None, :], m, lam, metric)
            MM.assert_rows_equal(got, MM.recipe(c, metric, q[0], lst, m, lam), 0, what)
            picks = np.searchsorted(lst, got.indices[0])
            assert np.sort(picks).tolist() == list(range(m)), f"{what}: every position is picked once"
            bad = MM.first_descending_copy(picks, groups)
            assert bad is None, f"{what}: copies of one vector at ranks {bad} come in descending position"
            same_bytes(c.search_mmr(q, lst[rng.permutation(m)][None, :], m, lam, metric), got, what + ": permuted")
            few = lst[:900]
            repeated = np.concatenate([few, few[rng.integers(0, 900, m - 900)]])[rng.permutation(m)]
            same_bytes(c.search_mmr(q, repeated[None, :], m, lam, metric),
                       c.search_mmr(q, np.concatenate([few, np.full(m - 900, MM.PAD)])[None, :], m, lam, metric), what + ": repeats")


@pytest.mark.parametrize("metric", METRICS)
def test_float16_format_edges(oracle, metric):
    """tests/_edges.py's Float16 corpora at dimension 200 (32 lanes): S (every value subnormal), R (normal to fully subnormal
    rows side by side), T and their base H against the recipe, which widens on the host; and the twin identities that hold
    exactly under power-of-two scaling -- Cosine: R gives H's picks, score bits and objective bits; L2 with the queries scaled
    like the corpus: S gives H's picks, scores and objectives after ldexp.  A walk kernel that flushed Float16 subnormals
    differs from all of them (tests/test_mmr_cpu.py)."""
    case = E.get_case(oracle, MM.EDGE_SHAPE, E.F16)
    assert_cell("f16", case.dim)
    lists = MM.edge_lists(case)
    k, lam = MM.EDGE_K, MM.EDGE_LAMBDA
    res = {}
    for kind in ("H", "S", "R", "T"):
        qs = case.queries_for(kind, metric, case.pool[:2])
        with G.GpuCorpus.from_array(case.rows(kind)) as c:
            res[kind] = c.search_mmr(qs, lists, k, lam, metric)
            for j in range(2):
                MM.assert_rows_equal(res[kind], MM.recipe(c, metric, qs[j], lists[j], k, lam), j, f"{kind}, metric {metric}")
    if metric == COS:
        same_bytes(res["R"], res["H"], "Cosine: R against its unscaled twin H")
    if metric == L2:
        e = E.SHIFT["S"]
        assert res["S"].indices.tobytes() == res["H"].indices.tobytes(), "L2: S picks H's rows"
        for name in ("scores", "objective"):
            want = np.ldexp(getattr(res["H"], name), e).astype(np.float32)
            assert getattr(res["S"], name).tobytes() == want.tobytes(), f"L2: S's {name} are H's after ldexp"
