"""Float tie order on every search route (DESIGN.md §3 "Order": best first, ties by ascending row POSITION, NaN last), pinned
with corpora of exactly duplicated rows (tests/_dups.py).

All copies of a vector carry one score, so a route that sorts unstably, whose candidate budget drops the earlier copy of a row
at the k-th rank, or whose phase / pass / range / shard merge orders equal keys by arrival returns a list that the
tolerance-aware helper accepts and that these checks do not: on every query the three properties of
`_dups.assert_dup_properties` (one score per vector bit for bit, strictly ascending (order key, position), prefix-closed),
on every CLEAR query of corpus B the exact index list, and `assert_float_topk` against the oracle's scores as everywhere else.
tests/test_float_ties_cpu.py proves the expectation against the oracle and asserts the clear share of the cases used here."""
import contextlib

import numpy as np
import pytest

from metrovector_amd import gpu as G

import _dups as D
from _util import PAD, assert_float_topk

pytestmark = pytest.mark.gpu

DTYPES, METRICS = (0, 1), (0, 1, 2)
K_PASS = D.K_PASS
_REFS = {}


class Ref:
    """One corpus with one set of live rows: everything the checks need, built once, shared, never changed."""

    def __init__(self, oracle, kind, name, dtype, live_kind):
        self.cp = D.get_b(name, dtype) if kind == "b" else D.get_a(oracle, name, dtype)
        self.name, self.kind, self.dtype, self.live_kind = name, kind, dtype, live_kind
        self.q = D.get_queries(name)
        self.live = D.get_live(name, live_kind, self.cp)
        self.dead = D.get_dead(name) if "dead" in live_kind or live_kind == "tombstones" else None
        self.allow = D.get_allow(name, self.cp) if "allow" in live_kind else None
        self.livepos = np.nonzero(self.live)[0]
        self.rows32_live = self.cp.rows[self.livepos].astype(np.float32)
        self.tag = f"corpus {kind.upper()} {name} dtype {dtype} ({live_kind})"

    def oracle_scores(self, oracle, metric, q):
        """The oracle's f32 score of every live row (corpus B: of the distinct vectors, a row's score is a function of its bytes)."""
        cp = self.cp
        if cp.vectors is not None:
            return oracle.scores(cp.vectors, cp.dtype, metric, q)[0][cp.group_of[self.livepos]]
        return oracle.scores(cp.rows, cp.dtype, metric, q)[0][self.livepos]


def get_ref(oracle, kind, name, dtype, live_kind="all"):
    key = (kind, name, dtype, live_kind)
    if key not in _REFS:
        _REFS[key] = Ref(oracle, kind, name, dtype, live_kind)
    return _REFS[key]


@contextlib.contextmanager
def open_corpus(ref, ids=None, path=None):
    with G.GpuCorpus.from_array(ref.cp.rows) as c:
        if ref.dead is not None:
            c.set_tombstones(np.packbits(ref.dead, bitorder="little"))
        if ids is not None:
            c.set_vector_ids(ids)
        if path is not None:
            c.set_scan_path(path)
        c.set_profiling(True)
        yield c


def check(oracle, ref, what, metric, q, labels, k, scores, indices, ids=None, extra="", live=None, exact=True, dups=True):
    """Every check of one result [nq, k]; -> the number of clear queries compared with the exact list."""
    cp = ref.cp
    live = ref.live if live is None else live
    idx = D.positions_of_ids(ids, indices) if ids is not None else np.asarray(indices, np.uint64)
    nq = len(q)
    for j in range(nq if dups else 0):
        D.assert_dup_properties(metric, scores[j], idx[j], cp.group_of, live, k, what=f"{what} k {k} query {labels[j]}{extra}")
    ncl = 0
    if cp.vectors is not None and exact:
        want = D.expected_topk(cp, metric, q, k, live)
        clear = D.clear_queries(cp, metric, q, k, live)
        for j in np.nonzero(clear)[0]:
            r = D.first_difference(idx[j], want[j])
            assert r is None, (f"{what} k {k} query {labels[j]}: the list differs from the exact answer first at rank {r}: got row "
                               f"{idx[j][r]} (score {scores[j][r]!r}), expected row {want[j][r]}{extra}")
        ncl = int(clear.sum())
    if live is ref.live:
        kk = min(k, ref.livepos.size)
        for j in (range(nq) if nq <= 8 else sorted(set(np.linspace(0, nq - 1, 8).astype(int).tolist()))):
            local = np.concatenate([np.searchsorted(ref.livepos, idx[j][:kk].astype(np.int64)).astype(np.uint64), idx[j][kk:]])
            assert_float_topk(metric, scores[j], local, ref.oracle_scores(oracle, metric, q[j]), ref.rows32_live, q[j], k)
    return ncl


def starts(nq):
    """One- to five-query cases run over consecutive slices of the first ten queries (one of them is clear), batches once."""
    return range(0, 10 - nq + 1, nq) if nq <= 5 else (0,)


def run_route(oracle, ref, route, metric, path, nqs, ks, kernels=None, ids=None, kernel_kmax=409):
    ncl = 0
    with open_corpus(ref, ids, path) as c:
        for nq in nqs:
            for k in ks:
                assert ref.kind != "b" or D.listed(ref.name, ref.live_kind, k), "a case whose clear share no CPU test asserts"
                for s in starts(nq):
                    lab = np.arange(s, s + nq)
                    res = c.search(ref.q[lab], k, metric)
                    t = c.last_timing()
                    what = f"{route} (scan path {path}) {ref.tag} metric {metric} nq {nq}"
                    # (asserted as the routes' own tests assert it; beyond 409 a shadow route may hand the search on)
                    assert kernels is None or k > kernel_kmax or t.scan_kernel in kernels, f"{what} k {k}: scan_kernel {t.scan_kernel}, expected {kernels}"
                    ncl += check(oracle, ref, what, metric, ref.q[lab], lab, k, res.scores, res.indices, ids,
                                 extra=f" [scan_kernel {t.scan_kernel}, repaired_queries {t.repaired_queries}]")
    assert ref.kind != "b" or ncl > 0, "no clear query was compared with the exact list"


def variant_ids(ref):
    return D.permuted_ids(D.B_SHAPES[ref.name][0] + 4000, ref.cp.n)


# ---- K1: the streaming scan on the stored rows ---------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(D.B_SHAPES))
def test_k1(oracle, name, dtype, metric):
    """nq 1, 4 and 5 (two passes) at every lane-group class: one lane (dim 4), 4, 8, 16, 32 and 64 lanes, 3104-byte rows."""
    run_route(oracle, get_ref(oracle, "b", name, dtype), "K1", metric, 1, (1, 4, 5), K_PASS, kernels=(1,))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_k1_many_small_groups(oracle, dtype, metric):
    run_route(oracle, get_ref(oracle, "a", "n20k_d200", dtype), "K1", metric, 1, (1, 5), (7, 1000), kernels=(1,))
    run_route(oracle, get_ref(oracle, "a", "n40k_d96", dtype, "tombstones"), "K1", metric, 1, (4,), (100,), kernels=(1,))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_k1_ids_and_tombstones(oracle, dtype, metric):
    """Ties follow position, never id."""
    ref = get_ref(oracle, "b", "n40k_d96", dtype, "tombstones")
    run_route(oracle, ref, "K1 with ids", metric, 1, (1, 5), K_PASS, kernels=(1,), ids=variant_ids(ref))


# ---- K2 on the stored rows -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["n90k_d48", "n20k_d200"])
def test_k2_exact_f32_mfma(oracle, name, metric):
    """InnerProduct / Cosine keys are final, L2 is re-scored."""
    run_route(oracle, get_ref(oracle, "b", name, 0), "K2 f32", metric, 2, (130,), K_PASS, kernels=(2,))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [200, 40])
@pytest.mark.parametrize("name", ["n90k_d48", "n20k_d200"])
def test_k2_f16_rows(oracle, name, nq, metric):
    """200 queries: the ping-pong kernel; 40: the streaming MFMA kernel."""
    run_route(oracle, get_ref(oracle, "b", name, 1), "K2 f16", metric, 2, (nq,), K_PASS, kernels=(3,))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_k2_many_small_groups(oracle, dtype, metric):
    run_route(oracle, get_ref(oracle, "a", "n40k_d96", dtype), "K2", metric, 2, (130,), (7, 1000))


# ---- selection shadows ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["n90k_d48", "n20k_d200"])
def test_f16_shadow_batched(oracle, name, metric):
    run_route(oracle, get_ref(oracle, "b", name, 0), "f16 shadow", metric, 3, (130,), K_PASS, kernels=(4,))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["n90k_d48", "n40k_d96"])
def test_f16_shadow_streamed(oracle, name, metric):
    run_route(oracle, get_ref(oracle, "b", name, 0), "f16 shadow stream", metric, 4, (1, 2), K_PASS, kernels=(5, 1))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["n90k_d48", "n20k_d200"])
def test_int8_shadow_batched(oracle, name, dtype, metric):
    run_route(oracle, get_ref(oracle, "b", name, dtype), "int8 shadow", metric, 5, (40, 200), (1, 7, 100, 409), kernels=(6,))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_int8_shadow_ids_and_tombstones_and_small_groups(oracle, dtype, metric):
    ref = get_ref(oracle, "b", "n90k_d48", dtype, "tombstones")
    run_route(oracle, ref, "int8 shadow with ids", metric, 5, (40,), (1, 7, 100, 409), kernels=(6,), ids=variant_ids(ref))
    run_route(oracle, get_ref(oracle, "a", "n40k_d96", dtype), "int8 shadow", metric, 5, (200,), (7, 409), kernels=(6,))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["n90k_d48", "n40k_d96"])
def test_int8_shadow_streamed(oracle, name, dtype, metric):
    run_route(oracle, get_ref(oracle, "b", name, dtype), "int8 shadow stream", metric, 6, (1, 4), (1, 7, 100), kernels=(7, 1))
    if name == "n40k_d96":
        run_route(oracle, get_ref(oracle, "a", name, dtype), "int8 shadow stream", metric, 6, (1, 4), (7, 100), kernels=(7, 1))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["n90k_d48", "n40k_d96"])
def test_6bit_shadow_streamed(oracle, name, metric):
    run_route(oracle, get_ref(oracle, "b", name, 0), "6-bit shadow stream", metric, 7, (1,), (1, 7, 100), kernels=(7,))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["n90k_d48", "n20k_d200"])
def test_default_path(oracle, name, dtype, metric):
    run_route(oracle, get_ref(oracle, "b", name, dtype), "default", metric, 0, (1, 40, 200), K_PASS)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_default_path_many_small_groups(oracle, dtype, metric):
    run_route(oracle, get_ref(oracle, "a", "n40k_d96", dtype), "default", metric, 0, (1, 40, 200), (7, 1000))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_int8_shadow_two_ranges_merge_in_position_order(oracle, monkeypatch, dtype, metric):
    """The shadowed prefix ends inside every large group: its copies come out of both ranges' lists and merge by position."""
    ref = get_ref(oracle, "b", "n90k_d48", dtype)
    prefix = 65536
    g = ref.cp.group_of
    big = int(np.argmax(ref.cp.sizes()))
    assert (g[:prefix] == big).any() and (g[prefix:] == big).any()
    monkeypatch.setenv("MVF_I8_SHADOW_ROWS", str(prefix))
    ncl = 0
    with open_corpus(ref, path=0) as c:
        for k in (1, 7, 100, 409):
            res = c.search(ref.q, k, metric)
            t = c.last_timing()
            assert c.info().shadows & 4, "MVF_I8_SHADOW_ROWS shadows a prefix only"
            ncl += check(oracle, ref, f"partial int8 shadow ({prefix} rows) {ref.tag} metric {metric} nq {D.NQ_SET}", metric, ref.q,
                         np.arange(D.NQ_SET), k, res.scores, res.indices,
                         extra=f" [scan_kernel {t.scan_kernel}, repaired_queries {t.repaired_queries}]")
    assert ncl > 0


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path,nq", [(5, 40), (6, 1)])
def test_repair_with_the_largest_group_at_the_kth_rank(oracle, path, nq, dtype, metric):
    """Queries next to the vector of the n / 6 group: its 15 000 tied copies hold the k-th rank and exceed every candidate
    budget, the streaming kernel redoes the query (no count is promised: repaired_queries is reported)."""
    ref = get_ref(oracle, "b", "n90k_d48", dtype)
    cp = ref.cp
    big = int(np.argmax(cp.sizes()))
    rng = np.random.default_rng(31)
    near = (cp.vectors[big].astype(np.float32)[None, :] + 0.05 * rng.standard_normal((8, cp.rows.shape[1]))).astype(np.float32)
    k, ncl, inside = 100, 0, 0
    with open_corpus(ref, path=path) as c:
        batches = [np.concatenate([near, ref.q[:nq - 8]])] if nq > 8 else [near[i:i + 1] for i in range(4)]
        for b, q in enumerate(batches):
            res = c.search(q, k, metric)
            t = c.last_timing()
            inside += int((cp.group_of[D.expected_topk(cp, metric, q[:1], k)[0].astype(np.int64)] == big).all())
            ncl += check(oracle, ref, f"repair (scan path {path}) {ref.tag} metric {metric} nq {nq}", metric, q, np.arange(len(q)) + b,
                         k, res.scores, res.indices, extra=f" [scan_kernel {t.scan_kernel}, repaired_queries {t.repaired_queries}]")
    assert ncl > 0 and inside > 0, "the largest group does not hold the k-th rank of any query"


# ---- k beyond one pass ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("variant", [False, True])
def test_large_k(oracle, monkeypatch, variant, mode, dtype, metric):
    """k = 1025 and 3000 by passes (1) and by the whole-shard sort (2)."""
    monkeypatch.setenv("MVF_LARGE_K", str(mode))
    ref = get_ref(oracle, "b", "n40k_d96", dtype, "tombstones" if variant else "all")
    run_route(oracle, ref, f"large k (MVF_LARGE_K={mode})", metric, 0, (1, 5), (1025, 3000), kernels=((1,) if mode == 1 else (8,)),
              ids=variant_ids(ref) if variant else None, kernel_kmax=3000)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2])
def test_large_k_many_small_groups(oracle, monkeypatch, mode, dtype):
    monkeypatch.setenv("MVF_LARGE_K", str(mode))
    for metric in METRICS:
        run_route(oracle, get_ref(oracle, "a", "n40k_d96", dtype), f"large k (MVF_LARGE_K={mode})", metric, 0, (5,), (3000,))


# ---- filtered search -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,path,nqs", [(1, 1, (1, 5)), (1, 0, (40,)), (2, 0, (1, 5, 40))])
@pytest.mark.parametrize("live_kind", ["allow", "allow & ~dead"])
def test_filtered(oracle, monkeypatch, live_kind, route, path, nqs, dtype, metric):
    """The allow mask admits a seeded half of every group: the expectation is rebuilt with live = allow & ~dead."""
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    ref = get_ref(oracle, "b", "n40k_d96", dtype, live_kind)
    ncl = 0
    with open_corpus(ref, path=path) as c, c.make_filter(ref.allow) as f:
        assert f.admitted == ref.livepos.size
        for nq in nqs:
            for k in K_PASS:
                assert D.listed(ref.name, live_kind, k)
                for s in starts(nq):
                    lab = np.arange(s, s + nq)
                    res = c.search_filtered(ref.q[lab], k, metric, f)
                    ncl += check(oracle, ref, f"filtered (MVF_FILTER_ROUTE={route}, scan path {path}) {ref.tag} metric {metric} nq {nq}",
                                 metric, ref.q[lab], lab, k, res.scores, res.indices)
    assert ncl > 0


# ---- candidates --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("live_kind", ["all", "tombstones"])
def test_candidates_every_row_listed_in_shuffled_order(oracle, live_kind, dtype, metric):
    ref = get_ref(oracle, "b", "n40k_d96", dtype, live_kind)
    n, nq = ref.cp.n, 3
    rng = np.random.default_rng(41)
    cand = np.stack([rng.permutation(np.concatenate([np.arange(n), rng.choice(n, 500)])) for _ in range(nq)]).astype(np.uint64)
    ncl = 0
    with open_corpus(ref) as c:
        for k in (7, 1000):
            res = c.search_candidates(ref.q[:nq], cand, k, metric)
            assert (res.counts == ref.livepos.size).all(), f"counts {res.counts} for {ref.livepos.size} live rows"
            ncl += check(oracle, ref, f"candidates {ref.tag} metric {metric} nq {nq}", metric, ref.q[:nq], np.arange(nq), k,
                         res.scores, res.indices)
    assert ncl > 0


# ---- radius ------------------------------------------------------------------------------------------------------------------

def _radius_case(ref, metric, want_queries):
    """Fully clear queries and, per query, two radii midway (float64) between the scores of adjacent vectors: one with at
    least 30 matches that ends behind a group of at least 4 live copies, one with more than MVFGPU_RADIUS_LIST_CAP matches."""
    cp = ref.cp
    nlive = np.array([m.size for m in D.members_of(cp, ref.live)])
    s, tol = D.vector_scores(metric, cp.vectors, ref.q)
    out = []
    for i in range(D.NQ_SET):
        order, clear = D.clear_pairs(metric, s[i], tol[i], nlive > 0)
        if not clear.all():
            continue
        cum = np.cumsum(nlive[order])
        small = [j for j in range(len(order) - 1) if 30 <= cum[j] <= G.RADIUS_LIST_CAP and nlive[order[j]] >= 4]
        large = [j for j in range(len(order) - 1) if cum[j] > G.RADIUS_LIST_CAP]
        if small and large:
            mid = lambda j: np.float32((s[i][order[j]] + s[i][order[j + 1]]) / 2)  # noqa: E731
            out.append((i, mid(small[0]), int(cum[small[0]]), int(nlive[order[small[0]]]), mid(large[0]), int(cum[large[0]])))
        if len(out) == want_queries:
            break
    assert len(out) == want_queries
    return out


def _check_radius(oracle, ref, what, metric, lab, res, counts, m):
    assert (res.counts == np.asarray(counts, np.uint64)).all(), f"{what}: counts {res.counts}, expected exactly {counts}"
    q = ref.q[lab]
    want = D.expected_topk(ref.cp, metric, q, m, ref.live) if m else None
    for j in range(len(lab)):
        real = min(int(counts[j]), m)
        r = D.first_difference(res.indices[j][:real], want[j][:real])
        assert r is None, f"{what} query {lab[j]}: first difference at rank {r}: got row {res.indices[j][r]}, expected {want[j][r]}"
        assert (res.indices[j][real:] == PAD).all(), f"{what} query {lab[j]}: padding"
        D.assert_dup_properties(metric, res.scores[j], res.indices[j], ref.cp.group_of, ref.live, real, what=f"{what} query {lab[j]}")
        if real == m:  # the identity of §3 "Radius search": the top-m of the search
            local = np.searchsorted(ref.livepos, res.indices[j].astype(np.int64)).astype(np.uint64)
            assert_float_topk(metric, res.scores[j], local, ref.oracle_scores(oracle, metric, q[j]), ref.rows32_live, q[j], m)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_between_two_vectors_counts_exactly_the_live_copies_inside(oracle, dtype, metric):
    ref = get_ref(oracle, "b", "n40k_d96", dtype, "tombstones")
    cases = _radius_case(ref, metric, 20)
    what = f"radius {ref.tag} metric {metric}"
    with open_corpus(ref) as c:
        for i, r_small, n_small, last_group, r_large, n_large in cases[:4]:
            m = n_small - last_group // 2  # max_per_query cuts the list inside the last group within the radius
            res = c.search_radius(ref.q[i:i + 1], r_small, m, metric)
            _check_radius(oracle, ref, f"{what} nq 1 max_per_query {m} inside a group", metric, [i], res, [n_small], m)
            res = c.search_radius(ref.q[i:i + 1], r_small, n_small + 9, metric)
            _check_radius(oracle, ref, f"{what} nq 1 max_per_query {n_small + 9}", metric, [i], res, [n_small], n_small + 9)
        lab = [cs[0] for cs in cases[:4]]
        res = c.search_radius(ref.q[lab], np.array([cs[4] for cs in cases[:4]], np.float32), 300, metric)
        assert res.overflowed.all()
        _check_radius(oracle, ref, f"{what} nq 4 beyond the list cap (the top-k finish)", metric, lab, res, [cs[5] for cs in cases[:4]], 300)
        lab = [cs[0] for cs in cases]  # 20 queries: Float32 rows take the thresholded batched pass
        res = c.search_radius(ref.q[lab], np.array([cs[1] for cs in cases], np.float32), 64, metric)
        _check_radius(oracle, ref, f"{what} nq 20", metric, lab, res, [cs[2] for cs in cases], 64)
        res = c.search_radius(ref.q[lab], np.array([cs[1] for cs in cases], np.float32), 0, metric)
        assert (res.counts == np.array([cs[2] for cs in cases], np.uint64)).all(), f"{what} nq 20, counts only"


# ---- join --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("count", [D.JOIN_COUNT, 5])
def test_self_join_over_a_window_of_duplicated_rows(oracle, count, exclude, dtype):
    """L2: a row's copies are its neighbours at distance 0 in ascending position; with the flag a row with more than k copies
    at lower positions loses its last entry and no duplicate; beyond the group the vector-to-vector order decides."""
    ref = get_ref(oracle, "b", "n20k_d200", dtype)
    cp, first = ref.cp, D.JOIN_FIRST
    window = cp.rows[first:first + count].astype(np.float32)
    mem = D.members_of(cp, ref.live)
    ncl = below = 0
    with open_corpus(ref, path=0) as c:
        for k in D.JOIN_KS:
            res = c.knn_join(k, G.L2, first, count, exclude_self=exclude)
            k1 = k + 1 if exclude else k
            full = D.expected_topk(cp, 0, window, k1, ref.live)
            clear = D.clear_queries(cp, 0, window, k1, ref.live)
            for i in range(count):
                p = first + i
                what = f"join (exclude_self {exclude}) {ref.tag} window {first}+{count} k {k} query row {p}"
                live = ref.live
                if exclude:
                    live = ref.live.copy()
                    live[p] = False
                D.assert_dup_properties(0, res.scores[i], res.indices[i], cp.group_of, live, k, what=what)
                others = mem[cp.group_of[p]]
                others = others[others != p] if exclude else others
                if others.size >= k:  # k below the group size: needs no separation
                    below += 1
                    assert (res.indices[i] == others[:k].astype(np.uint64)).all(), f"{what}: not the first k copies in ascending position"
                    assert (res.scores[i] == 0).all(), f"{what}: a copy at a distance other than 0"
                elif clear[i]:
                    ncl += 1
                    want = full[i][full[i] != np.uint64(p)][:k] if exclude else full[i]
                    r = D.first_difference(res.indices[i], want)
                    assert r is None, f"{what}: first difference at rank {r}: got row {res.indices[i][r]}, expected {want[r]}"
                    assert (res.scores[i][:others.size] == 0).all(), f"{what}: a copy at a distance other than 0"
            for i in sorted(set(np.linspace(0, count - 1, 6).astype(int).tolist())):
                sc = ref.oracle_scores(oracle, 0, window[i])
                if exclude:
                    sc = sc.copy()
                    sc[first + i] = np.nan  # self is never reported
                assert_float_topk(0, res.scores[i], res.indices[i], sc, ref.rows32_live, window[i], k)
    assert below > 0 and (ncl > 0 or count < D.JOIN_COUNT)


# ---- shard set ---------------------------------------------------------------------------------------------------------------

def _check_batched_shards(oracle, ref, what, metric, q, lab, k, res, ids, shard_of):
    """A batch on the shard set: every shard re-scores its candidates with the batched route's kernels or, where a query
    overflowed ITS candidate budget, redoes that query with K1 -- two summation orders, chosen per (handle, query), both within
    §3's tolerance (DESIGN.md §3 "Cross-shard merge order").  So the copies of one vector carry one score PER SHARD: the three
    properties hold with (vector, shard) as the group, every score lies within the tolerance of the float64 score, and the
    exact list is determined -- and compared -- wherever the shards' bits agree."""
    cp = ref.cp
    idx = D.positions_of_ids(ids, res.indices) if ids is not None else res.indices
    per_shard = cp.group_of * (int(shard_of.max()) + 1) + shard_of
    s64, tol = D.vector_scores(metric, cp.vectors, q)
    want = D.expected_topk(cp, metric, q, k, ref.live)
    clear = D.clear_queries(cp, metric, q, k, ref.live)
    ncl = 0
    for j in range(len(q)):
        w = f"{what} k {k} query {lab[j]}"
        D.assert_dup_properties(metric, res.scores[j], idx[j], per_shard, ref.live, k, what=w)
        pos = idx[j][idx[j] != PAD].astype(np.int64)
        g = cp.group_of[pos]
        err = np.abs(res.scores[j][:pos.size].astype(np.float64) - s64[j][g])
        assert (err <= tol[j][g]).all(), f"{w}: a score beyond the tolerance of its float64 score ({err.max()})"
        if clear[j] and D.first_bit_difference(res.scores[j][:pos.size], pos, cp.group_of) is None:
            r = D.first_difference(idx[j], want[j])
            assert r is None, f"{w}: first difference at rank {r}: got row {idx[j][r]}, expected row {want[j][r]}"
            ncl += 1
    check(oracle, ref, what, metric, q, lab, k, res.scores, res.indices, ids, exact=False, dups=False)
    return ncl


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", [False, True])
def test_shard_set_cut_inside_large_groups(oracle, variant, dtype, metric):
    """Three row-range shards whose cut points lie inside the two largest groups: the merge is by global position.  One query
    (K1 in every shard) and k = 3000 (passes / the sort) carry K1's bits in every shard: the unsharded expectation, exactly."""
    ref = get_ref(oracle, "b", "n40k_d96", dtype, "tombstones" if variant else "all")
    cp = ref.cp
    ids = variant_ids(ref) if variant else None
    cuts = D.shard_cuts(cp)
    shard_of = np.searchsorted(cuts, np.arange(cp.n), side="right") - 1
    shards, ncl, nbatched = [], 0, 0
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            c = G.GpuCorpus.from_array(np.ascontiguousarray(cp.rows[a:b]), index_base=a)
            shards.append(c)
            if variant:
                c.set_tombstones(np.packbits(ref.dead[a:b], bitorder="little"))
                c.set_vector_ids(ids[a:b])
        with G.ShardSet(shards) as ss:
            for nq in (1, 40):
                for k in (7, 1000, 3000):
                    assert D.listed(ref.name, ref.live_kind, k)
                    for s in starts(nq):
                        lab = np.arange(s, s + nq)
                        res = ss.search(ref.q[lab], k, metric)
                        what = f"shard set (cuts {cuts}) {ref.tag} metric {metric} nq {nq}"
                        if nq > 4 and k <= 1024:
                            repaired = [c.last_timing().repaired_queries for c in shards]
                            nbatched += _check_batched_shards(oracle, ref, f"{what} [repaired_queries per shard {repaired}]", metric,
                                                              ref.q[lab], lab, k, res, ids, shard_of)
                        else:
                            ncl += check(oracle, ref, what, metric, ref.q[lab], lab, k, res.scores, res.indices, ids)
    finally:
        for c in shards:
            c.close()
    assert ncl > 0 and nbatched > 0
