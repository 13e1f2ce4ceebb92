"""Float routes at the edges of their formats (DESIGN.md §2 "Format edges", §3 "Values at the edges"): corpora of SUBNORMAL
Float16 rows, rows next to the top of Float16, rows of every scale side by side, Float32 rows at 2^-40 and 2^+40, and queries
that are NaN, +Inf, 2^64 q, 2^-130 q, zeros or 2^+-40 q (tests/_edges.py).

Every ordinary answer is held to two things: `assert_float_topk` against the float64 scores of the corpus actually searched,
and the TWIN identity against the same route's answer on the base corpus from the same process, scan path, batch and k --
indices equal, score bits equal after `ldexp`.  A kernel that flushes subnormals, mis-widens them or builds a shadow or a
norm from flushed values fails both (tests/test_format_edges_cpu.py proves the expectation on the oracle and that a model of
such a kernel is rejected).  The edge queries are compared with the rule of §3's table, never with another route.  One handle
per (corpus, test): a route's edge queries run on the handle that answered its ordinary ones."""
import contextlib
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import pytest

from metrovector_amd import gpu as G

import _edges as E
import _wide as W
from _util import PAD, assert_float_topk

pytestmark = pytest.mark.gpu

L2, IP, COS = E.L2, E.IP, E.COS
F16, F32 = E.F16, E.F32
EDGE_NAMES = ("nan", "inf", "2^64", "2^-130", "zeros", "-zeros")
BAD_NAMES = ("nan", "inf", "2^64")


class Handle:
    """An opened corpus as a route's `call` sees it: what is searched (a corpus or a shard set), which corpus it holds, what
    was made from it (a partition) and the timing of every corpus behind it (one, or each shard of a set)."""

    def __init__(self, searched, kind, corpora=None, part=None):
        self.searched, self.kind, self.part = searched, kind, part
        self.corpora = [searched] if corpora is None else corpora

    def kernels(self):
        return tuple(sorted({c.last_timing().scan_kernel for c in self.corpora}))

    def repaired(self):
        return sum(c.last_timing().repaired_queries for c in self.corpora)

    def scan_bytes(self):
        return [c.last_timing().scan_bytes for c in self.corpora]

    def info(self):
        return f" [scan_kernel {'/'.join(map(str, self.kernels()))}, repaired_queries {self.repaired()}]"


@contextlib.contextmanager
def open_corpus(case, kind, path=None):
    with G.GpuCorpus.from_array(case.rows(kind)) as c:
        if case.dead is not None:
            c.set_tombstones(np.packbits(case.dead, bitorder="little"))
        if path is not None:
            c.set_scan_path(path)
        c.set_profiling(True)
        yield Handle(c, kind)


def search(h, q, k, metric):
    res = h.searched.search(q, k, metric)
    return res.scores, res.indices


@dataclass(frozen=True)
class Route:
    name: str
    path: Optional[int] = None        # set_scan_path
    kernel: Optional[int] = None      # the scan_kernel every search of up to 1024 results must report (None: the library's rule)
    large_k: bool = False             # ... and every search beyond 1024 results too (else the passes or the sort take those)
    call: Callable = search           # (handle, queries, k, metric) -> (scores, indices)
    opened: Callable = open_corpus    # (case, kind, path) -> a context manager of a Handle
    pos: Optional[np.ndarray] = None  # the rows the route admits (default: the live rows)
    six_bit: bool = False             # every search must have streamed the 6-bit shadow
    repairs_bad: bool = False         # a shadow route: the NaN, +Inf and 2^64 queries must report repaired_queries >= 1

    def __str__(self):
        return f"{self.name} (scan path {self.path})"


def ask(h, route, case, q, k, metric, what):
    """One search on one handle -> (scores, indices, what + the timing): the route that was meant is the route that ran."""
    sc, idx = route.call(h, q, k, metric)
    what += h.info()
    if route.kernel is not None and (k <= 1024 or route.large_k):
        assert h.kernels() == (route.kernel,), f"{what}: expected scan_kernel {route.kernel}"
    if route.six_bit:   # scan_kernel is 7 on the int8 stream too: the bytes scanned tell the two apart
        assert h.scan_bytes() == [G.shadow6_bytes(case.n, case.dim)], \
            f"{what}: {h.scan_bytes()} bytes scanned, the 6-bit shadow has {G.shadow6_bytes(case.n, case.dim)}"
    return sc, idx, what


def check_f64(case, kind, metric, q, k, scores, indices, what, ref=None, pos=None):
    """`assert_float_topk` of every query of one result against float64 over the admitted rows `pos` (default: the live rows)."""
    pos = case.livepos if pos is None else pos
    rows32 = case.rows32_live(kind) if pos is case.livepos else case.rows(kind)[pos].astype(np.float32)
    if ref is None:
        ref = W.f64_scores_all(case.rows(kind)[pos], q)[metric]
    real = min(k, pos.size)
    for j in range(len(q)):
        idx = np.asarray(indices[j], np.uint64)
        at = np.searchsorted(pos, idx[:real].astype(np.int64))
        assert (at < pos.size).all() and (pos[np.minimum(at, pos.size - 1)] == idx[:real].astype(np.int64)).all(), \
            f"{what} query {j}: a row outside the admitted set was returned"
        try:
            assert_float_topk(metric, scores[j], np.concatenate([at.astype(np.uint64), idx[real:]]), ref[j], rows32, q[j], k)
        except AssertionError as err:
            raise AssertionError(f"{what} query {j} against float64: {err}") from None


def check_twin(base, twin, e, what):
    for j in range(len(base[0])):
        d = E.twin_difference(base[0][j], base[1][j], twin[0][j], twin[1][j], e)
        assert d is None, f"{what} query {j}: twin identity: {d}"


def batches(case, kind, metric, nq, slices):
    """The ordinary queries of one batch size -> (labels of the thin-band queries compared, the queries sent).  Up to five
    queries: consecutive slices of the first `slices` thin-band queries; up to 64: the first nq; more: all 64, filled from the
    rest of the pool."""
    if nq > E.NQ:
        yield np.arange(E.NQ), case.queries_for(kind, metric, case.batch(nq))
    elif nq > 5:
        yield np.arange(nq), case.queries_for(kind, metric)[:nq]
    else:
        for s in range(0, slices or (12 if nq == 1 else 20), nq):
            lab = np.arange(s, min(s + nq, E.NQ))
            yield lab, case.queries_for(kind, metric)[lab]


def run_route(case, route, ks, nqs, slices=None, same_repairs=False, edges=None):
    """The two checks of the module's docstring for one route, on the base corpus and then on every twin, one handle per corpus.
    edges: {corpus: (batch size, ks)} -- §3's edge-query table on that corpus' handle, behind its ordinary queries.
    same_repairs: an exact twin overflows the candidate budgets of exactly as many queries as the base corpus -- a selection
    that lost the twin's values keys every row alike and is repaired query by query, which the answers alone would not show."""
    base = E.BASE_OF[case.dtype]
    answers, seen = {}, set()
    for kind in (base,) + E.TWINS_OF[case.dtype]:
        with route.opened(case, kind, route.path) as h:
            for metric in E.METRICS:
                e = E.twin_shift(kind, metric)
                ref = case.ref64(kind)[metric] if route.pos is None else None
                for nq in nqs:
                    for k in ks:
                        for lab, q in batches(case, kind, metric, nq, slices):
                            what = f"{route} {case.tag} corpus {kind} metric {metric} nq {nq} k {k} queries {lab[0]}.."
                            sc, idx, what = ask(h, route, case, q, k, metric, what)
                            sc, idx, q = sc[:len(lab)], idx[:len(lab)], q[:len(lab)]
                            seen.add((kind, h.kernels(), "repaired" if h.repaired() else "-"))
                            key = (metric, nq, k, lab[0])
                            if kind == base:
                                answers[key] = (sc, idx, h.repaired())
                                continue
                            check_f64(case, kind, metric, q, k, sc, idx, what, None if ref is None else ref[lab], route.pos)
                            if e is not None:
                                check_twin(answers[key], (sc, idx), e, what + f" vs corpus {base}")
                            if same_repairs and E.SHIFT[kind] is not None:
                                assert h.repaired() == answers[key][2], f"{what}: the base corpus repaired {answers[key][2]} queries"
            if edges and kind in edges:
                run_edges(h, case, route, *edges[kind])
    print(f"{route} {case.tag}: (corpus, scan_kernel, repairs) {sorted(seen)}")


SIX_BIT_PAD = 8   # ordinary searches in front of every edge search on the 6-bit route


def run_edges(h, case, route, nq, ks=(10,)):
    """§3's edge-query table on one handle.  A batch of 32 or more carries the edge queries between ordinary ones; smaller
    batches hold edge queries only, nq at a time.

    The 6-bit route keeps count of its repairs per handle and goes back to the int8 shadow once four searches were repaired
    and more than one in eight (`feedback_consume`); the NaN, +Inf, 2^64 and zero queries ARE repaired, by design.  So there
    each edge search follows SIX_BIT_PAD ordinary ones -- one repair in nine, whatever the handle has seen before -- and
    `ask` holds every one of them to the 6-bit shadow's bytes."""
    kind = h.kind
    eq = case.edge_queries()
    base = case.edge_base()
    for metric in E.METRICS:
        fill = case.queries_for(kind, metric, case.batch(max(nq, len(EDGE_NAMES), SIX_BIT_PAD)))
        what0 = f"{route} {case.tag} corpus {kind} metric {metric} nq {nq}"

        def padded(q, k, what):
            if route.six_bit:
                for j in range(SIX_BIT_PAD):
                    ask(h, route, case, fill[j:j + 1], k, metric, f"{what0} k {k} ordinary query {j} in front of an edge query")
            return ask(h, route, case, q, k, metric, what)

        if nq >= 32:
            sent = [(fill[:nq].copy(), {name: 3 + 5 * i for i, name in enumerate(EDGE_NAMES)})]
        else:
            sent = [(fill[:nq].copy(), {name: i for i, name in enumerate(EDGE_NAMES[s:s + nq])}) for s in range(0, len(EDGE_NAMES), nq)]
        for q, at in sent:
            for name, i in at.items():
                q[i] = eq[name]
        for k in ks:
            for q, at in sent:
                sc, idx, what = padded(q, k, f"{what0} k {k}")
                for name, i in at.items():
                    E.assert_edge(case, kind, name, metric, eq[name], sc[i], idx[i], k, what=f"{what} query {name} at {i}", pos=route.pos)
                bad = sorted(set(at) & set(BAD_NAMES))
                if route.repairs_bad and bad and k <= 1024:
                    assert h.repaired() >= 1, f"{what}: the documented `bad` branch flags {bad} for repair"
                if nq == 1:
                    print(f"{what}: query {next(iter(at))}")
            # ldexp(q, +-40) on fixed rows: InnerProduct scales exactly, Cosine is identical
            if metric != L2:
                b = ask(h, route, case, np.concatenate([base[None, :], fill[1:nq]]), k, metric, f"{what0} k {k} query q")
                for e in (-40, 40):
                    t = padded(np.concatenate([np.ldexp(base, e).astype(np.float32)[None, :], fill[1:nq]]), k, f"{what0} k {k} query 2^{e} q")
                    d = E.twin_difference(b[0][0], b[1][0], t[0][0], t[1][0], e if metric == IP else 0)
                    assert d is None, f"{t[2]}: {d}"


def both_edge_corpora(dtype, nq, ks=(10,)):
    """The edge queries on the corpus at the bottom of the format and on the second-hardest one."""
    return {("S" if dtype == F16 else "F"): (nq, ks), ("R" if dtype == F16 else "Fdn"): (nq, ks)}


def one_edge_corpus(dtype, nq, ks=(10,)):
    return {("S" if dtype == F16 else "F"): (nq, ks)}


# ---- K1 ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(E.K1_SHAPES[F16]))
def test_k1_f16(oracle, name):
    """nq 1, 4 and 5 (two passes) at every lane-group class; at two of them the edge queries with k = every live row + 3."""
    case = E.get_case(oracle, name, F16)
    ks = (10, case.livepos.size + 3) if name in ("d4", "d200") else (10,)
    run_route(case, Route("K1", path=1, kernel=1), E.KS, (1, 4, 5), edges={"S": (1, ks), "R": (4, (10,))})


@pytest.mark.parametrize("name", sorted(E.K1_SHAPES[F32]))
def test_k1_f32(oracle, name):
    case = E.get_case(oracle, name, F32)
    ks = (10, case.livepos.size + 3) if name in ("d4", "d200") else (10,)
    run_route(case, Route("K1", path=1, kernel=1), E.KS, (1, 4, 5), edges={"F": (1, ks), "Fdn": (4, (10,))})


# ---- batched routes ----------------------------------------------------------------------------------------------------------

# The batched kernels select by approximate keys within a proven margin and re-score the survivors exactly, so every answer is
# held to float64; their final scores come from the batched re-scoring (another summation order than K1's, the same for a
# corpus and its twin), so the twin identity is asserted there too.

@pytest.mark.parametrize("nq,pp", [(200, "1"), (200, "0"), (100, None), (40, None), (16, None)])
@pytest.mark.parametrize("name", sorted(E.BATCHED))
def test_k2_f16_rows(oracle, monkeypatch, name, nq, pp):
    """The three f16 MFMA kernels on STORED Float16 rows: 200 queries (256-query tiles) on the ping-pong kernel -- forced with
    MVF_K2_PP=1, these corpora have too few row tiles for it to be chosen -- and on the LDS-DMA kernel (MVF_K2_PP=0), 100 queries
    on the LDS-DMA kernel's 128-query tiles, 40 and 16 on the small-batch kernel's per-wave rings.  Subnormal A/B inputs of the
    f16 MFMA are ordinary values or the route is wrong."""
    if pp is not None:
        monkeypatch.setenv("MVF_K2_PP", pp)   # read when the handle is created
    case = E.get_case(oracle, name, F16)
    run_route(case, Route(f"K2 f16 (MVF_K2_PP={pp})", path=2, kernel=3), E.KS, (nq,), same_repairs=True,
              edges=one_edge_corpus(F16, nq) if nq in (200, 40) else None)


@pytest.mark.parametrize("name", sorted(E.BATCHED))
def test_k2_exact_f32_mfma(oracle, name):
    case = E.get_case(oracle, name, F32)
    run_route(case, Route("K2 f32", path=2, kernel=2), E.KS, (130,), edges=one_edge_corpus(F32, 130))


@pytest.mark.parametrize("path,nqs,kernel", [(3, (130,), 4), (4, (1, 2), 5)])
@pytest.mark.parametrize("name", sorted(E.BATCHED))
def test_f16_shadow_of_f32_rows(oracle, name, path, nqs, kernel):
    """Rows at 2^-40 are far below Float16's range and rows at 2^+40 far above it: the shadow must carry its own scale or the
    route must hand the search on.  The edge queries reach the route's own query preparation (its guard against a query
    that does not fit Float16)."""
    case = E.get_case(oracle, name, F32)
    run_route(case, Route("f16 shadow", path=path, kernel=kernel), E.KS, nqs, slices=4, edges=one_edge_corpus(F32, nqs[0]))


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("name", sorted(E.BATCHED))
def test_int8_shadow_batched(oracle, name, dtype):
    case = E.get_case(oracle, name, dtype)
    run_route(case, Route("int8 shadow", path=5, kernel=6, repairs_bad=True), (10, 100, 409), (40, 200), edges=one_edge_corpus(dtype, 40))


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("name", sorted(E.BATCHED))
def test_int8_shadow_streamed(oracle, name, dtype):
    case = E.get_case(oracle, name, dtype)
    run_route(case, Route("int8 shadow stream", path=6, kernel=7, repairs_bad=True), E.KS, (1, 2, 3, 4), slices=8,
              edges=both_edge_corpora(dtype, 1))


@pytest.mark.parametrize("name", sorted(E.BATCHED))
def test_6bit_shadow_streamed(oracle, name):
    """Every search here, ordinary or edge, is held to the 6-bit shadow's bytes (`ask`, `run_edges`)."""
    case = E.get_case(oracle, name, F32)
    run_route(case, Route("6-bit shadow stream", path=7, kernel=7, six_bit=True, repairs_bad=True), E.KS, (1,),
              edges={"F": (1, (10,)), "Fup": (1, (10,))})


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("name", sorted(E.BATCHED))
def test_default_path(oracle, name, dtype):
    """Whatever the library's own rule chooses at these sizes."""
    case = E.get_case(oracle, name, dtype)
    run_route(case, Route("default", path=0), E.KS, (1, 40, 200), slices=4, edges=one_edge_corpus(dtype, 1))


# ---- k beyond one pass -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 2])
def test_large_k_f16(oracle, monkeypatch, mode):
    """k = 1025 and 3000 by passes (1) and by the whole-shard sort (2); the edge queries at k = 1025."""
    monkeypatch.setenv("MVF_LARGE_K", str(mode))
    case = E.get_case(oracle, "n20k_d200", F16)
    run_route(case, Route(f"large k (MVF_LARGE_K={mode})", path=0, kernel=1 if mode == 1 else 8, large_k=True), (1025, 3000), (1, 5),
              slices=5, edges={"S": (1, (1025,))})


# ---- radius ------------------------------------------------------------------------------------------------------------------

def _radii(case, kind, metric, lab, lo=20, hi=60):
    """Per query a radius midway (float64) between two adjacent scores of ranks lo..hi, where their gap is the widest, and the
    number of live rows inside; the gap must exceed 8 tolerances at that score (a condition on the inputs)."""
    ref = case.ref64(kind)[metric][lab]
    q = case.queries_for(kind, metric)[lab]
    radii, counts = [], []
    xmax = float(np.sqrt((case.rows(kind)[case.livepos].astype(np.float64) ** 2).sum(1)).max())
    for j in range(len(lab)):
        key = np.sort(ref[j] if metric == L2 else -ref[j])[:hi + 1]
        r = lo + int(np.argmax(np.diff(key[lo - 1:hi + 1])))
        mid = (key[r - 1] + key[r]) / 2
        tol = 1e-5 * (abs(mid) if metric == L2 else 1.0 if metric == COS else
                      float(np.linalg.norm(q[j].astype(np.float64))) * xmax)
        assert key[r] - key[r - 1] > 8 * tol, "no clear gap between two scores of ranks 20..60"
        mid32 = np.float32(mid if metric == L2 else -mid)
        assert (key[r - 1] < (mid32 if metric == L2 else -np.float64(mid32)) < key[r])
        radii.append(mid32)
        counts.append(r)
    return np.array(radii, np.float32), np.array(counts, np.uint64)


def _radius_edges(c, case, kind, nq, what):
    """§3's table through `search_radius` with the radius that admits every score (+inf under L2, -inf otherwise).  A row
    matches iff it is live and its score is not NaN (§3 "Match rule"), so wherever the table fixes the list the count is the
    number of its entries that are not NaN and the list its first max_per_query such entries; a query whose every score is
    NaN matches nothing.  The table's ordinary and unasserted entries have no fixed list and are left to the searches above."""
    eq = case.edge_queries()
    m = 64
    for metric in E.METRICS:
        q = case.queries_for(kind, metric, case.batch(max(nq, len(EDGE_NAMES))))
        at = {name: i * (len(q) // len(EDGE_NAMES)) for i, name in enumerate(EDGE_NAMES)}   # between ordinary queries
        for name, i in at.items():
            q[i] = eq[name]
        res = c.search_radius(q, np.float32(np.inf if metric == L2 else -np.inf), m, metric)
        for name, i in at.items():
            want = E.edge_expectation(name, metric, case.exact[kind][:, case.col], case.livepos, case.livepos.size)
            if want is E.ORDINARY or want is E.UNASSERTED:
                continue
            idx, cls = want
            match = cls != "nan"
            w = f"{what} metric {metric} edge query {name} at {i}"
            assert res.counts[i] == match.sum(), f"{w}: count {res.counts[i]}, expected {match.sum()}"
            n = min(m, int(match.sum()))
            assert (res.indices[i][:n] == idx[match][:n]).all() and (res.indices[i][n:] == PAD).all(), f"{w}: indices {res.indices[i]}"
            assert (E.class_of(res.scores[i][:n]) == cls[match][:n]).all(), f"{w}: scores {res.scores[i]}"


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("path,nq", [(0, 4), (0, 20), (1, 20), (2, 4)])
def test_radius(oracle, dtype, path, nq):
    """Radii placed between two float64 scores: the counts are exact, the lists the top of the search.  A radius search
    reports no kernel in its timing; the route is an input here -- scan path 1 forces the streaming kernel R1, scan path 2
    the batched pass on Float32 rows, scan path 0 streams below 16 queries (`mvfgpu_selftest_radius_route` is that rule;
    Float16 rows always stream) -- and the score bits of R1 are pinned by the twin identity."""
    case = E.get_case(oracle, "n20k_d200", dtype)
    route = G.radius_route(dtype, nq, path)
    assert route == (1 if dtype == F32 and (path == 2 or (path == 0 and nq >= 16)) else 0)
    lab = np.arange(nq)
    got = {}
    for kind in (E.BASE_OF[dtype],) + E.TWINS_OF[dtype]:
        with open_corpus(case, kind, path) as h:
            c = h.searched
            what = f"radius (scan path {path}, route {route}) {case.tag} corpus {kind} nq {nq}"
            for metric in E.METRICS:
                radii, counts = _radii(case, kind, metric, lab)
                q = case.queries_for(kind, metric)[lab]
                res = c.search_radius(q, radii, 64, metric)
                w = f"{what} metric {metric}"
                assert (res.counts == counts).all(), f"{w}: counts {res.counts}, expected exactly {counts}"
                for j in range(nq):
                    n = int(counts[j])
                    assert (res.indices[j][n:] == PAD).all(), f"{w} query {j}: padding"
                    check_f64(case, kind, metric, q[j:j + 1], n, res.scores[j:j + 1, :n], res.indices[j:j + 1, :n], w,
                              case.ref64(kind)[metric][lab[j:j + 1]])
                got[(kind, metric)] = (res.scores, res.indices)
                e = E.twin_shift(kind, metric)
                if kind != E.BASE_OF[dtype] and e is not None and route == 0:
                    check_twin(got[(E.BASE_OF[dtype], metric)], got[(kind, metric)], e, w)
            if kind in ("S", "F"):
                _radius_edges(c, case, kind, nq, what)


# ---- candidates, filters, partitions ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("half", [False, True])
def test_candidates(oracle, dtype, half):
    """A candidate list of every row, and a shuffled half."""
    case = E.get_case(oracle, "n40k_d96", dtype)
    rng = np.random.default_rng(51)
    rows = rng.permutation(case.n)[:case.n // 2] if half else np.arange(case.n)
    admitted = np.zeros(case.n, bool)
    admitted[rows] = True
    pos = np.nonzero(admitted & case.live)[0] if half else None

    def call(h, q, k, metric):
        cand = np.ascontiguousarray(np.broadcast_to(rows.astype(np.uint64), (len(q), rows.size)))
        res = h.searched.search_candidates(q, cand, k, metric)
        return res.scores, res.indices

    run_route(case, Route("candidates", call=call, pos=pos), E.KS, (3,), slices=6, edges=one_edge_corpus(dtype, 1))


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("route", [1, 2])
def test_filtered(oracle, monkeypatch, dtype, route):
    """The filtered mask route (1) and list route (2) over a seeded half of the rows."""
    monkeypatch.setenv("MVF_FILTER_ROUTE", str(route))
    case = E.get_case(oracle, "n20k_d200", dtype)
    allow = np.random.default_rng(52).random(case.n) < 0.5
    pos = np.nonzero(allow & case.live)[0]

    def call(h, q, k, metric):
        with h.searched.make_filter(allow) as f:
            res = h.searched.search_filtered(q, k, metric, f)
        return res.scores, res.indices

    run_route(case, Route(f"filtered (MVF_FILTER_ROUTE={route})", path=0, call=call, pos=pos), E.KS, (1, 40), slices=3,
              edges=one_edge_corpus(dtype, 1))


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("tier", [1, 2])
def test_partitioned(oracle, dtype, tier):
    """One key per query: key 1 holds ~600 rows (the small tier), key 2 the rest (the large tier)."""
    case = E.get_case(oracle, "n20k_d200", dtype)
    keys = np.where(np.random.default_rng(53).random(case.n) < 0.03, 1, 2).astype(np.uint32)
    pos = np.nonzero((keys == tier) & case.live)[0]
    assert (G.partition_plan(np.full(6, pos.size), np.full(6, tier), 100)[0] == tier).all()

    @contextlib.contextmanager
    def opened(case, kind, path):
        with open_corpus(case, kind, path) as h, h.searched.attach_column(keys) as col, h.searched.make_partition(col) as part:
            yield Handle(h.searched, kind, part=part)

    def call(h, q, k, metric):
        res = h.searched.search_partitioned(q, np.full(len(q), tier, np.uint32), k, metric, h.part)
        return res.scores, res.indices

    run_route(case, Route(f"partitioned (tier {tier})", call=call, opened=opened, pos=pos), E.KS, (6,), edges=one_edge_corpus(dtype, 1))


# ---- self-join, shard set, fetch ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("exclude", [True, False])
def test_self_join_of_subnormal_rows(oracle, exclude):
    """A 1024-row window: the queries are widened subnormal rows.  Both sides scale, so InnerProduct scales by the square."""
    case = E.get_case(oracle, "n20k_d200", F16)
    first, count, k = 777, G.JOIN_WINDOW, 10
    live_in_window = np.nonzero(case.live[first:first + count])[0]   # (a deleted query row gets a row of padding)
    some = live_in_window[np.linspace(0, live_in_window.size - 1, 12).astype(int)]
    got = {}
    for kind in ("H", "S", "T", "R"):
        window = case.rows(kind)[first:first + count].astype(np.float32)
        ref = W.f64_scores_all(case.rows(kind)[case.livepos], window[some])
        with open_corpus(case, kind, 0) as h:
            for metric in E.METRICS:
                res = h.searched.knn_join(k, metric, first, count, exclude_self=exclude)
                what = f"join (exclude_self {exclude}) {case.tag} corpus {kind} metric {metric} window {first}+{count}{h.info()}"
                got[(kind, metric)] = (res.scores, res.indices)
                assert (res.indices[~case.live[first:first + count]] == PAD).all(), f"{what}: deleted query rows get padding"
                for j, i in enumerate(some):
                    sc = ref[metric][j:j + 1].copy()
                    if exclude:
                        assert first + i not in res.indices[i].tolist(), f"{what} query row {first + i}: self was reported"
                        sc[0, np.searchsorted(case.livepos, first + i)] = np.nan  # self is never reported
                    check_f64(case, kind, metric, window[i:i + 1], k, res.scores[i:i + 1], res.indices[i:i + 1], f"{what} query row {first + i}", sc)
                if kind != "H":
                    e = E.twin_shift(kind, metric)
                    if e is not None:
                        check_twin(got[("H", metric)], got[(kind, metric)], 2 * e if metric == IP else e, what + " vs corpus H")


@pytest.mark.parametrize("dtype", [F16, F32])
def test_shard_set(oracle, dtype):
    """Three row-range shards; every message carries the kernels and the repairs of all three."""
    case = E.get_case(oracle, "n20k_d200", dtype)
    cuts = [0, 6001, 13002, case.n]

    @contextlib.contextmanager
    def opened(case, kind, path):
        shards = []
        try:
            for a, b in zip(cuts[:-1], cuts[1:]):
                c = G.GpuCorpus.from_array(np.ascontiguousarray(case.rows(kind)[a:b]), index_base=a)
                shards.append(c)
                c.set_tombstones(np.packbits(case.dead[a:b], bitorder="little"))
                c.set_profiling(True)
            with G.ShardSet(shards) as ss:
                yield Handle(ss, kind, corpora=shards)
        finally:
            for c in shards:
                c.close()

    run_route(case, Route("shard set", opened=opened), E.KS, (1, 40), slices=3, edges=one_edge_corpus(dtype, 1))


def test_search_fetch_returns_the_stored_bytes(oracle):
    """`search_fetch` on every Float16 corpus, ordinary and edge queries: the list is the search's, and the rows returned
    with it are the stored bytes of the rows it names (zero rows behind a short list)."""
    case = E.get_case(oracle, "n40k_d96", F16)

    def call(h, q, k, metric):
        res, vec = h.searched.search_fetch(q, k, metric)
        real = res.indices != PAD
        want = case.rows(h.kind)[res.indices[real].astype(np.int64)]
        assert (vec[real].view(np.uint16) == want.view(np.uint16)).all(), f"search_fetch corpus {h.kind} metric {metric}: not the stored bytes"
        assert (vec[~real].view(np.uint16) == 0).all()
        assert h.kind != "S" or ((np.abs(vec[real].astype(np.float64)) < E.F16_MIN_NORMAL) & (vec[real] != 0)).mean() > 0.99
        return res.scores, res.indices

    run_route(case, Route("search_fetch", path=0, call=call), (10,), (5,), slices=10, edges=one_edge_corpus(F16, 1))
