"""-m gpu tests of the PREMISE of the multi-vector search's MFMA selection route (DESIGN.md §3 "Multi-vector search: the MFMA
route", §5 "A0 / P0"): for every query set and every key the approximate sum S~ that A0 and M1 produce lies within Delta
(maxsim_margin, scan_maxsim.h) of route 1's sum S.  tests/test_gpu_maxsim_mfma.py holds the route's ANSWER to route 1's bytes,
which passes whenever the exact top k falls among the candidates; this file reads the selection itself out of the device
(mvfgpu_selftest_maxsim_mfma_selection: S~ as P0 read it, A0's forced keys, the candidates, Delta, theta, xxmax) and holds
  (a) |S~ - S| <= Delta for every key of every set, S route 1's f32 sum (search_maxsim on route 1 with k = n_keys, mapped back
      by key) and S a float64 recomputation on the host (tests/_maxsim_mfma.py f64_sums: the stored rows, the f32 tokens, the
      per-token maximum over each key's live rows, the float64 sum over the tokens; Cosine with float64 norms and K1's zero rule);
      Delta itself against maxsim_margin of the host's token norms;
  (b) P0's rule, recomputed in NumPy from the read-out alone (tests/_maxsim_mfma.py p0_rule, theta_of), bit for bit; the
      candidate count against the stage timer's; route 1's top k among the candidates.
The worlds are tests/test_gpu_maxsim_mfma.py's.  The only pass condition of the measured share max |S~ - S| / Delta is <= 1, the
header's claim; the shares measured on an MI355X stand in DESIGN.md §5 "A0 / P0".
Run time on an MI355X: see DESIGN.md §8; every case takes two seconds at the most."""
import numpy as np
import pytest

import _edges as ED
import _maxsim as MS
import _maxsim_mfma as MM
import _partitioned as P
from _maxsim_world import World
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
SHAPES = [("f32", 3), ("f32", 100), ("f32", 129), ("f32", 768), ("f16", 8), ("f16", 20), ("f16", 200), ("f16", 768)]
TOKENS = (1, 5, 32, 33, 70)
NQS = (1, 3)
KS = (1, 10)
U = 2.0 ** -23
SHARES = {}   # (kind of world, dtype, metric) -> the largest |S~ - S| / Delta seen: the measurement, printed when the module ends
OUTSIDE = {}  # (subnormal corpus, metric) -> the (set, key) pairs the bound did not cover there (forced, S~ or Delta not finite)


def code_of(dt):
    return MS.DTYPE[dt]


def selection(w, sets, metric, k):
    """the read-out of one search by route 2 -> (MaxSimSelection, its result (scores, keys))"""
    import torch
    nq, T, dim = sets.shape
    dq = torch.from_numpy(np.ascontiguousarray(sets)).cuda()
    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    dk = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    sel = w.c.maxsim_mfma_selection(w.part, dq.data_ptr(), 0, dim, nq, T, k, metric, ds.data_ptr(), dk.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert sel.sums.shape == (nq, w.nk) and sel.forced.shape == (nq, w.nk) and sel.candidates.shape == (nq, w.nk)
    return sel, (ds.cpu().numpy(), dk.cpu().numpy().view(np.uint64))


def stage_candidates(w, sets, metric, k):
    import torch
    nq, T, dim = sets.shape
    dq = torch.from_numpy(np.ascontiguousarray(sets)).cuda()
    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    dk = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    return w.c.maxsim_mfma_stage_ms(w.part, dq.data_ptr(), 0, dim, nq, T, k, metric, ds.data_ptr(), dk.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)[1]


def route1(w, sets, metric):
    """route 1 with k = n_keys -> (S f32 [nq, n_keys] by key ordinal, the ordinals best first [nq, n_keys], the result)"""
    w.c.set_maxsim_route(1)
    try:
        res = w.c.search_maxsim(sets, w.nk, metric, w.part)
    finally:
        w.c.set_maxsim_route(0)
    assert (res.counts == w.nk).all()
    at = np.searchsorted(w.keys, res.keys)
    assert (w.keys[at] == res.keys).all()
    S = np.empty((sets.shape[0], w.nk), np.float32)
    np.put_along_axis(S, at, res.scores, 1)
    return S, at, res


def reference(w, sets, metric):
    """tests/_maxsim_mfma.py f64_sums over the world's live rows in the index's order"""
    live, _, starts, values = MS.key_order(w.lay)
    assert (values == w.keys).all()
    return MM.f64_sums(w.rows[live], starts, sets, metric)


def check_delta(w, sel, sets, metric):
    """Delta as the device computed it against maxsim_margin of the host's f32 token norms and the read-out xxmax: exactly under
    Cosine (the formula does not read norms there), within (dim + 16) 2^-23 relative under InnerProduct -- the project's bound of
    two f32 sums of squares taken in different orders; xxmax itself within the same of the float64 maximum over the stored rows"""
    tol = (w.dim + 16) * U
    x64 = w.rows.astype(np.float64)
    assert sel.xxmax == pytest.approx(float((x64 * x64).sum(1).max()), rel=tol), "xxmax"
    for q, tokens in enumerate(sets):
        want = G.maxsim_margin(code_of(w.dt), metric, w.dim, np.sqrt((tokens * tokens).sum(1, dtype=np.float32)), sel.xxmax)
        if metric == COS:
            assert sel.delta[q] == want, f"set {q}: Delta {sel.delta[q]} is not the margin {want}"
        else:
            assert sel.delta[q] == pytest.approx(want, rel=tol), f"set {q}: Delta {sel.delta[q]} against the margin {want}"


def check_bound(sel, S1, S64, inside, what):
    """(a) for the (set, key) pairs of `inside` -> the largest |S~ - S| / Delta among them"""
    assert np.isfinite(sel.sums[inside]).all(), f"{what}: a sum the bound covers is not finite"
    if not inside.any():
        return 0.0
    at = np.argwhere(inside)
    delta = np.broadcast_to(sel.delta[:, None], inside.shape)[inside]   # the covered pairs only: their Delta is finite
    worst = 0.0
    for name, S in (("route 1", S1.astype(np.float64)), ("float64", S64)):
        err = np.abs(sel.sums.astype(np.float64)[inside] - S[inside])
        share = np.where(err == 0, 0.0, err / np.where(delta > 0, delta, np.inf))
        share = np.where((err > 0) & ~(delta > 0), np.inf, share)       # an error against a Delta of 0
        worst = max(worst, float(share.max()))
        assert (err <= delta).all(), (f"{what}: |S~ - S| above Delta against {name}: {float(share.max())} of Delta at (set, key) "
                                      f"{at[int(np.argmax(share))].tolist()}, Delta {sel.delta}")
    return worst


def check_rule(w, sel, sets, metric, k, top1, result, what):
    """(b): P0's rule from the read-out alone, theta, the stage timer's count, route 1's top k, and the search's own result"""
    kk = min(k, w.nk)
    theta, nan = MM.theta_of(sel.sums, sel.forced, kk)
    assert (sel.theta_nan == nan).all() and (sel.theta[~nan] == theta[~nan]).all() and np.isnan(sel.theta[nan]).all(), \
        f"{what}: theta {sel.theta} / {sel.theta_nan}, from the sums {theta} / {nan}"
    want = MM.p0_rule(sel.sums, sel.forced, sel.delta, sel.theta, sel.theta_nan)
    assert (sel.candidates == want).all(), f"{what}: the candidates are not the rule's at (set, key) {np.argwhere(sel.candidates != want)[:5].tolist()}"
    assert (sel.candidates.sum(1) == stage_candidates(w, sets, metric, k)).all(), f"{what}: the stage timer counts other candidates"
    assert np.take_along_axis(sel.candidates, top1[:, :kk], 1).all(), f"{what}: a key of route 1's top {kk} is no candidate"
    assert (result[1] == w.keys[top1[:, :k]]).all(), f"{what}: the read-out's search is not route 1's"


def note(kind, w, metric, share):
    key = (kind, w.dt, "IP" if metric == IP else "Cosine")
    SHARES[key] = max(SHARES.get(key, 0.0), share)


def check_finite_world(w, sets, metric, ks, kind, what, ref=None, first=None):
    """(a) for every key and (b) on a world of finite values -> the share of Delta.  ref / first: f64_sums / route1 of a pool the
    sets lead, where a caller keeps them"""
    nq, T, _ = sets.shape
    S64, fails = MM.key_sums(reference(w, sets, metric) if ref is None else ref, nq, T)
    S1, top1, _ = route1(w, sets, metric) if first is None else first
    assert not fails.any()
    worst = 0.0
    for k in ks:
        sel, result = selection(w, sets, metric, k)
        assert sel.forced.sum() == 0 and np.isfinite(sel.sums).all(), f"{what}, k {k}: a finite world forces no key"
        check_delta(w, sel, sets, metric)
        worst = max(worst, check_bound(sel, S1, S64, np.ones(S1.shape, bool), f"{what}, k {k}"))
        check_rule(w, sel, sets, metric, k, top1, result, f"{what}, k {k}")
    note(kind, w, metric, worst)
    return worst


def assert_far_from_the_edges(ref, what):
    """the condition under which no key of a finite world may be forced: every dot product and denominator seven decades and
    more inside the premises' edges 1e37 and 1e-30 (tests/test_maxsim_mfma_cpu.py holds the same on the CPU alone)"""
    assert ref["dot_max"] < 1e30 and ref["den_max"] < 1e30 and ref["den_min"] > 1e-20, (what, ref["dot_max"], ref["den_min"], ref["den_max"])


@pytest.fixture(scope="module")
def world_a():
    made = {}

    def get(dt, dim):
        if (dt, dim) not in made:
            made[dt, dim] = World(dt, dim, MS.form_layout(2048))
        return made[dt, dim]
    yield get
    for w in made.values():
        w.close()
    for key in sorted(SHARES):
        print(f"max |S~ - S| / Delta, {key[0]} world, {key[1]} rows, {key[2]}: {SHARES[key]:.4f}")
    for key in sorted(OUTSIDE):
        print(f"subnormal corpus {key[0]}, metric {key[1]}: {OUTSIDE[key]} (set, key) pairs outside the bound")


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=[f"{dt}d{dim}" for dt, dim in SHAPES])
def test_the_bound_holds_for_every_key_and_the_rule_is_the_headers(world_a, case):
    """World A at every shape (odd and even V, a step count that is and is not a multiple of PB, a row of one vector), 1 to 7
    tiles of query rows (every MT instantiation, a partial last tile, a second trip of the tile loop that ends early), both
    metrics, k 1 and 10: (a) and (b) for EVERY key -- no key is forced and every S~ is finite, which the inputs guarantee: the
    float64 reference alone shows every dot product below 1e30 and every Cosine denominator inside (1e-20, 1e30), decades from
    the premises' edges 1e37 and 1e-30 (asserted here and, without a GPU, in tests/test_maxsim_mfma_cpu.py)."""
    dt, dim = SHAPES[case]
    w = world_a(dt, dim)
    assert MS.spans_block_edge(w.lay)
    pool = MS.token_pool(dt, dim, 3, 70)
    for metric in (IP, COS):
        ref = reference(w, pool, metric)
        assert_far_from_the_edges(ref, f"{dt} x {dim}")
        for T in TOKENS:
            S1, top1, res = route1(w, pool[:, :T], metric)
            for nq in NQS:
                share = check_finite_world(w, pool[:nq, :T], metric, KS, "random", f"{dt} x {dim}, metric {metric}, T {T}, nq {nq}",
                                           ref=ref, first=(S1[:nq], top1[:nq], res))
                assert share <= 1.0


@pytest.mark.parametrize("dt,dim", [("f32", 768), ("f16", 768)])
def test_one_signed_rows_and_tokens(dt, dim):
    """|World A's rows| against |tokens|: no cancellation, the accumulation's worst case; (a) and (b)"""
    lay = MS.form_layout(2048)
    w = World(dt, dim, lay, rows=np.abs(P.make_rows(2048, dim, dt)))
    try:
        sets = np.abs(MS.make_sets(3, 33, dim, dt))
        for metric in (IP, COS):
            ref = reference(w, sets, metric)
            assert_far_from_the_edges(ref, f"one-signed {dt}")
            assert check_finite_world(w, sets, metric, KS, "one-signed", f"one-signed {dt}, metric {metric}", ref=ref) <= 1.0
    finally:
        w.close()


@pytest.mark.parametrize("dt,dim", [("f32", 100), ("f16", 200)])
def test_a_ladder_of_keys_a_quarter_of_delta_apart(dt, dim):
    """The rule's 2 Delta itself.  A rule that subtracts one Delta differs only on keys whose S~ lies between theta - 2 Delta
    and theta - Delta, where random worlds put a key by chance alone.  Here key g holds one positive row scaled by 1 - g c under InnerProduct with
    positive tokens, c a quarter of Delta / S: the sums descend in steps of Delta / 4 (the rows' own rounding moves a sum by far
    less: one element's half ulp, averaged over the dimension), so at k = 1 keys lie inside that band, which the test first
    asserts from the read-out -- a condition of the world, not of the rule -- and then holds (a) and (b) as everywhere."""
    lay = MS.form_layout(2048)
    live, keys, starts, values = MS.key_order(lay)
    v = np.abs(P.make_rows(1, dim, dt)[0].astype(np.float64)) + 0.5
    sets = np.abs(MS.make_sets(3, 5, dim, dt)) + np.float32(0.5)
    norms = np.sqrt((sets[0] * sets[0]).sum(1, dtype=np.float32))
    delta = G.maxsim_margin(code_of(dt), IP, dim, norms, float((v * v).sum()))
    c = delta / 4.0 / float((sets[0].astype(np.float64) @ v).sum())
    rows = np.broadcast_to(v.astype(P.make_rows(1, dim, dt).dtype), (2048, dim)).copy()   # the tombstoned rows too: xxmax is |v|^2
    ordinal = np.searchsorted(values, lay["col"][live])
    rows[live] = (v[None, :] * (1.0 - ordinal * c)[:, None]).astype(rows.dtype)
    w = World(dt, dim, lay, rows=rows)
    try:
        sel, _ = selection(w, sets, IP, 1)
        band = (sel.sums >= (sel.theta - 2.0 * sel.delta)[:, None]) & (sel.sums < (sel.theta - sel.delta)[:, None])
        assert band[0].sum() >= 2, f"the ladder puts keys between theta - 2 Delta and theta - Delta: {band.sum(1)}"
        assert check_finite_world(w, sets, IP, KS, "ladder", f"ladder {dt}") <= 1.0
    finally:
        w.close()


def test_a_small_scratch_budget_the_selection_of_chunks_and_windows(world_a, monkeypatch):
    """The world of test_a_small_scratch_budget_gives_several_windows_and_chunks (t0 > 0, several windows with w0 > 0), nq 3 x
    T 33: the read-out satisfies (a) and (b), (a) also against the unchunked handle's route 1 -- and S~ equals the unchunked
    handle's S~ bit for bit: a (token, row) score of A0 does not depend on the tile or the chunk it is computed in (the steps of
    a row accumulate in one order whatever MT and PB are), and M1 adds the chunks' bests to the running f32 sum in token order,
    the same chain."""
    for dt, dim, metric in (("f32", 100, COS), ("f16", 200, IP)):
        w = world_a(dt, dim)
        budget = w.nk * (8 * 4 + MS.KEY_BYTES)
        chunk, window = G.maxsim_plan(w.nk, 33, 3, 16, budget)
        assert -(-33 // chunk) >= 3 and -(-3 // window) >= 2
        # route 2's own plan (maxsim_mfma_plan, scan_maxsim.h): A0's chunk is the plan of tokens that take no LDS (token_bytes 0),
        # its window at most the shorter of the two plans' -- so A0 runs with t0 > 0 and the call has windows with w0 > 0
        achunk, awindow = G.maxsim_plan(w.nk, 33, 3, 0, budget)
        assert -(-33 // achunk) >= 2 and -(-3 // min(window, awindow)) >= 2, (achunk, awindow)
        monkeypatch.setenv("MVF_MAXSIM_SCRATCH_BYTES", str(budget))
        small = World(dt, dim, w.lay)
        monkeypatch.delenv("MVF_MAXSIM_SCRATCH_BYTES")
        try:
            sets = MS.make_sets(3, 33, dim, dt)
            ref = reference(w, sets, metric)
            whole1 = route1(w, sets, metric)
            check_finite_world(small, sets, metric, KS, "random", f"{dt}: small budget", ref=ref)
            check_finite_world(small, sets, metric, KS, "random", f"{dt}: small budget against the unchunked route 1", ref=ref, first=whole1)
            for k in KS:
                a, b = selection(small, sets, metric, k)[0], selection(w, sets, metric, k)[0]
                assert (a.sums.view(np.uint32) == b.sums.view(np.uint32)).all(), f"{dt}, k {k}: chunked S~ against unchunked S~"
                assert (a.candidates == b.candidates).all() and (a.delta == b.delta).all() and (a.theta == b.theta).all()
        finally:
            small.close()


def token_edges(dim, dt):
    base = MS.make_sets(3, 5, dim, dt)
    for name in ("ordinary", "nan", "zero", "inf", "huge"):
        sets = base.copy()
        if name == "inf":
            sets[1, 2, 0] = np.inf
        elif name == "huge":
            sets[1, 2] *= np.float32(1e30)
            sets[2, 0] *= np.float32(1e-30)
        elif name != "ordinary":
            token = np.full(dim, np.nan, np.float32) if name == "nan" else np.zeros(dim, np.float32)
            sets[0, 1], sets[2, 4] = token, token
        yield name, sets


@pytest.mark.parametrize("dt,dim", [("f32", 100), ("f16", 200)])
def test_forced_keys_cover_every_failed_premise(dt, dim):
    """The planted world of test_non_finite_huge_and_zero_values with its token edges.  The host finds, in float64, the (set, key)
    pairs where a premise fails for some token and live row: forced | S~ not finite is asserted to be a SUPERSET of them -- the
    f32 kernel may force more (a norm whose f32 sum of squares overflows where the float64 one does not, values at an edge in
    f32 only), which is not pinned.  Every pair outside the superset meets (a) where Delta is finite, and (b) holds as it stands.
    An all-zero key under Cosine is not forced and has S~ exactly 0 for every set whose tokens are all finite (0 x NaN and
    0 x Inf are no numbers: such a token's dot product fails the premise for every row, zero rows included).  A tombstoned row
    never contributes: the key whose only non-finite row is tombstoned is not forced by sets of ordinary tokens."""
    rows, lay, tomb_key, zero_key = MM.planted_world(dt, dim)
    w = World(dt, dim, lay, rows=rows)
    try:
        for name, sets in token_edges(dim, dt):
            ordinary = np.array([np.isfinite(s).all() and np.abs(s).max() < 1e3 and (np.abs(s).max(1) > 1e-3).all() for s in sets])
            for metric in (IP, COS):
                S64, fails = MM.key_sums(reference(w, sets, metric), 3, 5)
                S1, top1, _ = route1(w, sets, metric)
                for k in KS:
                    what = f"edges {dt}, {name} tokens, metric {metric}, k {k}"
                    sel, result = selection(w, sets, metric, k)
                    covered = sel.forced | ~np.isfinite(sel.sums)
                    assert covered[fails].all(), f"{what}: a failed premise left unforced at (set, key) {np.argwhere(fails & ~covered)[:5].tolist()}"
                    inside = ~covered & np.isfinite(sel.delta)[:, None]
                    note("planted", w, metric, check_bound(sel, S1, S64, inside, what))
                    check_rule(w, sel, sets, metric, k, top1, result, what)
                    assert not sel.forced[ordinary, tomb_key].any(), f"{what}: a tombstoned NaN row forced its key"
                    if metric == COS:
                        finite = np.isfinite(sets).all((1, 2))
                        assert not sel.forced[finite, zero_key].any() and (sel.sums[finite, zero_key] == 0).all(), f"{what}: the all-zero key"
            if name == "ordinary":
                assert fails.any() and not fails.all() and not fails[:, tomb_key].any()
    finally:
        w.close()


@pytest.mark.parametrize("kind", ["S", "R", "T"])
def test_subnormal_f16_rows_stay_inside_delta(oracle, kind):
    """tests/_edges.py's Float16 corpora at d96 (S every non-zero value subnormal, R normal to fully subnormal rows side by side,
    T values up to 32736) with test_subnormal_f16_rows' three token scalings: (a) and (b) for every (set, key) outside forced |
    S~ not finite; with the tokens as they are and scaled down, where nothing comes near a premise's edge, every pair must be
    covered (asserted).  MEASURED on an MI355X: the matrix unit's handling of subnormal f16 inputs stays inside Delta.  Every (set,
    key) pair of the three corpora was covered -- none forced, every S~ and Delta finite -- and the largest |S~ - S| was 0.057 of
    Delta (DESIGN.md §5 "A0 / P0"): the unit does not flush subnormal inputs; a flushed row of corpus S would lose its whole
    score, hundreds of Delta."""
    case = ED.get_case(oracle, "d96", ED.F16)
    rows = case.rows(kind)
    n = rows.shape[0]
    dead = case.dead if case.dead is not None else np.zeros(n, bool)
    col = ((np.arange(n) * 2654435761) % 211).astype(np.uint32)
    w = World("f16", case.dim, dict(col=col, dead=dead), rows=rows)
    try:
        pool = case.pool[:15].reshape(3, 5, case.dim).astype(np.float32)
        for metric in (IP, COS):
            for scale, sets in ((0, pool), (-20, np.ldexp(pool, -20).astype(np.float32)), (20, np.ldexp(pool, 20).astype(np.float32))):
                S64, fails = MM.key_sums(reference(w, sets, metric), 3, 5)
                S1, top1, _ = route1(w, sets, metric)
                for k in KS:
                    what = f"f16 corpus {kind}, tokens x 2^{scale}, metric {metric}, k {k}"
                    sel, result = selection(w, sets, metric, k)
                    covered = sel.forced | ~np.isfinite(sel.sums)
                    assert covered[fails].all(), what
                    inside = ~covered & np.isfinite(sel.delta)[:, None]
                    note(f"subnormal {kind}", w, metric, check_bound(sel, S1, S64, inside, what))
                    OUTSIDE[kind, metric] = OUTSIDE.get((kind, metric), 0) + int((~inside).sum())
                    if scale <= 0:   # every value lies decades inside the premises: an A0 that forced these rows would hold (a) vacuously
                        assert not fails.any() and inside.all(), f"{what}: {int((~inside).sum())} pairs left the bound"
                    check_rule(w, sel, sets, metric, k, top1, result, what)
    finally:
        w.close()


def test_refusals_of_the_read_out(world_a):
    """what the stage timer refuses: an ineligible handle or metric; no device error is left behind"""
    import torch
    f = world_a("f32", 100)
    sets = MS.make_sets(3, 5, 100, "f32")
    dq = torch.from_numpy(sets).cuda()
    ds, dk = torch.empty((3, 10), dtype=torch.float32, device="cuda"), torch.empty((3, 10), dtype=torch.int64, device="cuda")
    with pytest.raises(E.InvalidArgument, match="Float32 / Float16 rows under InnerProduct / Cosine"):
        f.c.maxsim_mfma_selection(f.part, dq.data_ptr(), 0, 100, 3, 5, 10, L2, ds.data_ptr(), dk.data_ptr())
    with pytest.raises(E.InvalidArgument):
        f.c.maxsim_mfma_selection(f.part, dq.data_ptr(), 0, 100, 3, 0, 10, IP, ds.data_ptr(), dk.data_ptr())
    # every NULL output, on a call that is otherwise the search's own
    import ctypes as C
    from metrovector_amd import _lib
    bufs = [np.zeros(3 * f.nk, t) for t in (np.float32, np.uint8, np.uint8)] + [np.zeros(3, t) for t in (np.float64, np.float32, np.uint8)] + [np.zeros(1, np.float32)]
    for missing in range(len(bufs)):
        outs = [None if i == missing else b.ctypes.data_as(C.c_void_p) for i, b in enumerate(bufs)]
        rc = _lib.gpu().mvfgpu_selftest_maxsim_mfma_selection(f.c._h, f.part._h, IP, C.c_void_p(dq.data_ptr()), 0, 100, 3, 5, 10,
                                                              C.c_void_p(ds.data_ptr()), C.c_void_p(dk.data_ptr()), None, *outs)
        assert rc == E.InvalidArgument.status, f"output {missing} NULL"
    assert all(not b.any() for b in bufs), "a refused call writes nothing"
    w = World("i8", 64, MS.form_layout(2048))
    try:
        d8 = torch.from_numpy(MS.make_sets(3, 5, 64, "i8")).cuda()
        with pytest.raises(E.InvalidArgument, match="Float32 / Float16 rows under InnerProduct / Cosine"):
            w.c.maxsim_mfma_selection(w.part, d8.data_ptr(), 2, 64, 3, 5, 10, IP, ds.data_ptr(), dk.data_ptr())
    finally:
        w.close()
    torch.cuda.synchronize()
