"""-m gpu tests of the multi-vector search on every form of its scoring kernel M0 (DESIGN.md §5 "M0 / M1"): the 34 cells of
data type x lanes per row x (rows in registers | rows re-read | tokens through the cache) the library's own rule reaches, both
sides of the three switches between them, the widths only MVF_K1_G reaches, and integer rows whose sums lie next to 2^31.  The
table of cases is tests/_maxsim.py's FORM_CASES; mvfgpu_selftest_maxsim_form says which instantiation a case runs, and every
test asserts it before it searches.  Two yardsticks per case: the recipe of grouped searches the call replaces (byte for byte)
and a reference independent of every kernel -- exact integers for Int8 / UInt8 (byte for byte), float64 with §3's tolerance
scaled by the tokens for the float types.  The candidate form runs on the same worlds against the filtered full search.
2048 rows over seven sized keys and 20 further ones; 1024 rows from 10240 dimensions on.
Run time on an MI355X: the 99 tests take 9 s together, the slowest 2 s (the first: it also pays the first use of the device;
every other one at most 0.25 s).  Nothing was cut: every case runs every metric.  The largest float error measured is 0.03 of
the tolerance (printed per result row before it is asserted).  Device code of M0 unchanged by the self-test: the tests pass on
the kernels as they were."""
import numpy as np
import pytest

import _maxsim as MS
import _maxsim_candidates as MC
import test_gpu_maxsim_candidates as TC
from _maxsim_world import expected, recipe, same_bytes
from _util import PAD, TOL
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
METRICS = (L2, IP, COS)
NQS = (1, 3)
CASE_IDS = [f"{dt}d{dim}" for dt, dim in MS.FORM_CASES]


def tokens_of(dim):
    """T = 5: a full token group and a short one; T = 33: chunked by 32 or by the LDS share"""
    return (1, 5, 33) if dim <= 4112 else (1, 5)


def is_int(dt):
    return dt in ("i8", "u8")


def assert_cell(dt, dim, forced=0, cell=None):
    """the instantiation the case is listed for is the one the launch takes"""
    f = G.maxsim_form(MS.DTYPE[dt], dim, forced)
    cell = MS.FORM_CELLS[dt, dim] if cell is None else cell
    assert (f.G, f.J, f.form) == cell, f"{dt} x {dim}, forced width {forced}: listed as {cell}, the library says {f}"
    return f


def make_world(dt, dim, lay=None, rows=None):
    lay = MS.form_layout(MS.form_rows(dim)) if lay is None else lay
    assert MS.spans_block_edge(lay), "a key's rows lie on both sides of a block of 128 list positions"
    return TC.World(dt, dim, lay, rows=rows)


def result(t):
    return G.MaxSimResult(*t)


def assert_f64(w, got, nq, k, S, tol, metric, what):
    """every result row against the float64 sums; padding behind the keys"""
    kk = min(k, w.nk)
    assert (got.counts == kk).all() and (got.keys[:, kk:] == PAD).all(), f"{what}: counts and padding"
    assert (got.scores[:, kk:] == (np.inf if metric == L2 else -np.inf)).all(), f"{what}: padding scores"
    for j in range(nq):
        frac = MS.f64_fraction(got.scores[j, :kk], got.keys[j, :kk], w.keys, S[j], tol[j])
        print(f"{what}, set {j}: {frac:.3f} of the tolerance")
        MS.assert_f64_contract(got.scores[j, :kk], got.keys[j, :kk], w.keys, S[j], tol[j], metric, kk)


@pytest.mark.parametrize("case", range(len(MS.FORM_CASES)), ids=CASE_IDS)
def test_every_form_is_the_recipe_and_the_independent_reference(case):
    """a. every case, metric, T, nq and k: search_maxsim is the recipe of search_grouped calls byte for byte, and the exact
    integer reference byte for byte (Int8 / UInt8) or the float64 contract within TOL (Float32 / Float16)"""
    dt, dim = MS.FORM_CASES[case]
    assert_cell(dt, dim)
    w = make_world(dt, dim)
    try:
        Ts = tokens_of(dim)
        pool = MS.token_pool(dt, dim, max(NQS), max(Ts))   # set j, token t of every (nq, T): pool[j, t]
        flat = pool.reshape(-1, dim)
        if is_int(dt):
            raw = MS.int_raw(w.rows, w.lay, flat)
        else:
            f64 = MS.f64_key_bests(w.rows, w.lay, flat, TOL)
        for metric in METRICS:
            if is_int(dt):
                sc, _, row_keys = MS.int_row_scores(w.rows, w.lay, flat, metric, raw)
            else:
                b, tol = (a.reshape(max(NQS), max(Ts), w.nk) for a in f64[metric])
            for T in Ts:
                for nq in NQS:
                    sets = np.ascontiguousarray(pool[:nq, :T])
                    best = recipe(w, sets, metric)
                    for k in (1, 10, w.nk, w.nk + 3):
                        what = f"{dt} x {dim}, metric {metric}, T {T}, nq {nq}, k {k}"
                        got = w.c.search_maxsim(sets, k, metric, w.part)
                        same_bytes(got, expected(w, best, metric, k), what + ": the recipe")
                        if is_int(dt):
                            same_bytes(got, result(MS.rank_sets(sc, row_keys, nq, T, metric, k, stride=max(Ts))), what + ": exact")
                        else:
                            assert_f64(w, got, nq, k, b[:nq, :T].sum(1), tol[:nq, :T].sum(1), metric, what)
    finally:
        w.close()


@pytest.mark.parametrize("case", range(len(MS.FORM_CASES)), ids=CASE_IDS)
def test_the_candidate_form_on_every_form(case):
    """b. one call per case and metric, T = 5, nq = 3: held, unheld, repeated and PAD entries, another number of held candidates
    per set, against the filtered full search; and a list of every key is search_maxsim"""
    dt, dim = MS.FORM_CASES[case]
    assert_cell(dt, dim)
    w = make_world(dt, dim)
    try:
        sets = np.ascontiguousarray(MS.token_pool(dt, dim, 3, 5))
        every = np.ascontiguousarray(np.broadcast_to(w.keys, (3, w.nk)))
        for metric in METRICS:
            lists = MC.mixed_lists(w.keys, 3, 40, w.unheld + [int(PAD)], ("forms", case, metric))
            assert len(set(TC.distinct_counts(w, lists))) == 3
            TC.check(w, sets, lists, metric, f"{dt} x {dim}, metric {metric}")
            for k in (10, w.nk + 3):
                TC.same_bytes(w.c.search_maxsim_candidates(sets, every, k, metric, w.part), w.c.search_maxsim(sets, k, metric, w.part),
                              f"{dt} x {dim}, metric {metric}, k {k}: every key listed")
    finally:
        w.close()


SATURATED = [(dt, dim, cell) for dt in ("i8", "u8") for dim, cell in ((1024, (16, 4, MS.REG)), (2048, (16, 8, MS.REREAD)),
                                                                       (33025, (64, 33, MS.REREAD)))]


@pytest.mark.parametrize("dt,dim,cell", SATURATED, ids=[f"{dt}d{dim}" for dt, dim, _ in SATURATED])
def test_saturated_integer_rows_are_exact(dt, dim, cell):
    """c. all-min, all-max, alternating and near-max rows, each under a key of its own, against all-min, all-max, alternating
    and zero tokens: raw values up to 65025 x 33025 = INT32_MAX - 33022.  The full and the candidate call, every metric,
    T = 5, nq = 2, byte for byte against the exact reference"""
    assert_cell(dt, dim, cell=cell)
    rows, lay, _ = MS.saturated_world(dt, dim)
    w = make_world(dt, dim, lay, rows)
    try:
        sets = MS.saturated_sets(dt, dim)
        nq, T = sets.shape[:2]
        planted = np.array([MS.SAT_OWN_KEY0 + i for i in range(10)] + [MS.SAT_TIE_KEY], np.uint64)
        assert np.isin(planted, w.keys).all()
        raw = MS.int_raw(rows, lay, sets.reshape(nq * T, dim))
        for metric in METRICS:
            sc, _, row_keys = MS.int_row_scores(rows, lay, sets.reshape(nq * T, dim), metric, raw)
            full = MS.rank_sets(sc, row_keys, nq, T, metric, w.nk + 1)
            for k in (1, 10, w.nk + 3):
                same_bytes(w.c.search_maxsim(sets, k, metric, w.part), result(MS.rank_sets(sc, row_keys, nq, T, metric, k)),
                           f"saturated {dt} x {dim}, metric {metric}, k {k}")
            lists = MC.mixed_lists(w.keys, nq, 40, w.unheld + [int(PAD)], ("saturated", dt, dim, metric))
            lists[0, :planted.size] = planted           # every planted key among set 0's candidates, half of them among set 1's
            lists[1, :planted.size // 2] = planted[::2][:planted.size // 2]
            d = TC.distinct_counts(w, lists)
            for k in (1, 10, max(d) + 3):
                want = result(MC.filter_full(full[0], full[1], w.nk, lists, w.keys, k, metric))
                TC.same_bytes(w.c.search_maxsim_candidates(sets, lists, k, metric, w.part), want,
                              f"saturated {dt} x {dim}, metric {metric}, k {k}: candidates")
    finally:
        w.close()


FORCED_CELLS = {1: (1, 50, MS.REREAD), 4: (4, 13, MS.REREAD), 8: (8, 7, MS.REREAD), 16: (16, 4, MS.REG), 32: (32, 2, MS.REG),
                64: (64, 1, MS.REG)}


@pytest.mark.parametrize("dt,dim", MS.FORCED_SHAPES, ids=[f"{dt}d{dim}" for dt, dim in MS.FORCED_SHAPES])
def test_forced_widths(dt, dim, monkeypatch):
    """d. MVF_K1_G, read when the handle is created: rows of 50 vectors under each of the six widths -- 1, 4 and 8 lanes take
    the re-read form with 16, 4 and 2 sums kept per lane, which no shape reaches by the library's own rule.  Integer results are
    the exact reference's bytes under every width; float results pass the float64 contract; T = 33 in at least 3 chunks and
    2 windows gives the unchunked bytes of the same width."""
    lay = MS.form_layout(2048)
    T, nq = 5, 3
    pool = MS.token_pool(dt, dim, nq, 33)
    sets, long_sets = np.ascontiguousarray(pool[:, :T]), np.ascontiguousarray(pool)
    rows, first = None, {}
    for width in MS.FORCED_WIDTHS:
        assert_cell(dt, dim, width, FORCED_CELLS[width])
        monkeypatch.setenv("MVF_K1_G", str(width))
        w = make_world(dt, dim, lay, rows)
        budget = w.nk * (8 * 4 + MS.KEY_BYTES)
        chunk, window = G.maxsim_plan(w.nk, 33, nq, G.maxsim_form(MS.DTYPE[dt], dim, width).token_bytes, budget)
        assert -(-33 // chunk) >= 3 and -(-nq // window) >= 2
        monkeypatch.setenv("MVF_MAXSIM_SCRATCH_BYTES", str(budget))
        small = make_world(dt, dim, lay, w.rows)
        monkeypatch.delenv("MVF_MAXSIM_SCRATCH_BYTES")
        monkeypatch.delenv("MVF_K1_G")
        try:
            if rows is None:
                rows = w.rows
                if is_int(dt):
                    raw = MS.int_raw(rows, lay, sets.reshape(nq * T, dim))
                else:
                    f64 = MS.f64_key_bests(rows, lay, sets.reshape(nq * T, dim), TOL)
            for metric in METRICS:
                for k in (1, 10, w.nk + 3):
                    what = f"{dt} x {dim}, {width} lanes, metric {metric}, k {k}"
                    got = w.c.search_maxsim(sets, k, metric, w.part)
                    if is_int(dt):
                        sc, _, row_keys = MS.int_row_scores(rows, lay, sets.reshape(nq * T, dim), metric, raw)
                        same_bytes(got, result(MS.rank_sets(sc, row_keys, nq, T, metric, k)), what + ": exact")
                        same_bytes(got, first.setdefault((metric, k), got), what + ": the first width's bytes")
                    else:
                        b, tol = (a.reshape(nq, T, w.nk) for a in f64[metric])
                        assert_f64(w, got, nq, k, b.sum(1), tol.sum(1), metric, what)
            metric = (L2, IP, COS)[MS.FORCED_WIDTHS.index(width) % 3]
            for k in (10, w.nk + 3):
                same_bytes(small.c.search_maxsim(long_sets, k, metric, small.part), w.c.search_maxsim(long_sets, k, metric, w.part),
                           f"{dt} x {dim}, {width} lanes, metric {metric}, k {k}: chunked against unchunked")
        finally:
            small.close()
            w.close()
