"""No-GPU tests of the multi-vector search's MFMA selection route (DESIGN.md §3 "Multi-vector search: the MFMA route", §5
"A0 / P0"): the route rule, the bound Delta against a restatement of its formula, the formula against the arithmetic by
emulation -- the selection's scores as a sequential f32 chain (the tokens rounded to f16 on Float16 rows) against a blocked f32
product and float64 --, adversarial rows and tokens, the yardsticks tests/test_gpu_maxsim_mfma_bound.py holds the selection's
read-out to (P0's rule restated, the float64 sums; the distance of its finite worlds from the bound's premises), and the
refusals of the new entry points.
Run time: 16 s together on one core, of which the yardsticks' tests take 1 s; the slowest case (768 dimensions) takes 4 s."""
import ctypes as C

import numpy as np
import pytest

import _partitioned as P
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G
import metrovector_amd as M

F32, F16, I8, U8 = 0, 1, 2, 3
L2, IP, COS = 0, 1, 2
U = 2.0 ** -23


def margin(dtype, metric, dim, norms, xxmax):
    """the header's formula, restated"""
    eps = (max(dim, 64) + 16) * U + (2.0 ** -11 * 1.001 if dtype == F16 else 0.0)
    xm = float(np.sqrt(np.float64(np.float32(xxmax))))
    total = 0.0
    for n in np.asarray(norms, np.float32):
        u = 1.0 if metric == COS else float(n) * xm
        if not (u == 0.0 or 1e-24 <= u < 1e37):
            return float("inf")
        total += u
    if not total < 1e37:
        return float("inf")
    return 1.001 * (eps + (len(norms) - 1) * U) * total


# ---- the route rule
def test_an_ineligible_type_or_metric_takes_route_1_whatever_is_forced():
    for dtype in (F32, F16, I8, U8):
        for metric in (L2, IP, COS):
            eligible = dtype in (F32, F16) and metric in (IP, COS)
            for forced in (0, 1, 2):
                got = G.maxsim_route(10 ** 7, 10 ** 5, 128, dtype, metric, 1, 32, 100, forced)
                assert got == (2 if eligible and forced != 1 else 1), (dtype, metric, forced)
                small = G.maxsim_route(10 ** 4, 10 ** 2, 128, dtype, metric, 1, 32, 10, forced)
                assert small == (2 if eligible and forced == 2 else 1), (dtype, metric, forced)


def test_forced_routes_are_honoured_where_eligible_and_automatic_is_monotone():
    """the automatic rule of scan_maxsim.h, from the crossover profiles/r18_maxsim_mfma.txt measured"""
    for dtype, dim in ((F32, 768), (F16, 128)):
        for metric in (IP, COS):
            assert M.maxsim_route(5 * 10 ** 7, 10 ** 6, dim, dtype, metric, 1, 32, 100, 1) == 1
            assert M.maxsim_route(5 * 10 ** 7, 10 ** 6, dim, dtype, metric, 1, 32, 100, 2) == 2
            assert M.maxsim_route(1, 1, dim, dtype, metric, 1, 1, 1, 2) == 2
            # automatic: monotone in the held rows at every token count and in the tokens at every row count -- never back to
            # route 1 --, route 2 from the measured crossover on (2M rows x 32 tokens), route 1 for a call that fills no tile of
            # 32 query rows, for k above half the keys and for small corpora
            grid_rows, grid_T = (1, 10 ** 3, 10 ** 5, 2 * 10 ** 6, 10 ** 7, 10 ** 9, 2 ** 32 - 1), (1, 4, 31, 32, 128, 1024)
            auto = {(r, t): G.maxsim_route(r, max(r // 50, 1), dim, dtype, metric, 1, t, 100, 0) for r in grid_rows for t in grid_T}
            assert set(auto.values()) == {1, 2}
            for t in grid_T:
                seen = [auto[r, t] for r in grid_rows]
                assert seen == sorted(seen), f"T {t}: {seen}"
            for r in grid_rows:
                seen = [auto[r, t] for t in grid_T]
                assert seen == sorted(seen), f"rows {r}: {seen}"
            assert auto[2 * 10 ** 6, 32] == 2 and auto[10 ** 5, 32] == 1 and auto[10 ** 9, 31] == 1 and auto[10 ** 9, 4] == 1
            assert G.maxsim_route(10 ** 9, 10 ** 7, dim, dtype, metric, 8, 4, 100, 0) == 2, "eight sets of four tokens fill a tile"
            assert G.maxsim_route(10 ** 7, 10 ** 5, dim, dtype, metric, 1, 32, 50001, 0) == 1
            assert G.maxsim_route(10 ** 7, 10 ** 5, dim, dtype, metric, 1, 32, 50000, 0) == 2
            assert G.maxsim_route(8192, 100, dim, dtype, metric, 3, 33, 10, 0) == 1, "the test worlds stay on route 1"


# ---- the bound against its formula
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("metric", [IP, COS])
def test_the_margin_is_the_formula(dtype, metric):
    rng = np.random.default_rng(P._seed("margin", dtype, metric))
    for dim in (1, 3, 64, 100, 768, 4100):
        for T in (1, 5, 33, 1024):
            norms = np.abs(rng.standard_normal(T)).astype(np.float32) * np.float32(10.0)
            for xxmax in (0.0, 1.0, 131.5, 3e10):
                want, got = margin(dtype, metric, dim, norms, xxmax), M.maxsim_margin(dtype, metric, dim, norms, xxmax)
                assert got == pytest.approx(want, rel=1e-12), (dim, T, xxmax)
    one = np.ones(4, np.float32)
    assert G.maxsim_margin(dtype, COS, 128, one, np.inf) < 1.0, "Cosine does not read the rows' norms"
    for norms, xxmax in ((one, np.inf), (one, np.nan), (one * np.float32(np.nan), 1.0), (one * np.float32(1e-30), 1.0),
                         (one * np.float32(1e30), 1e20), (np.array([1, 1, np.inf, 1], np.float32), 1.0)):
        assert G.maxsim_margin(dtype, IP, 128, norms, xxmax) == float("inf"), (norms, xxmax)
    zero = np.array([0, 1, 0, 1], np.float32)
    assert np.isfinite(G.maxsim_margin(dtype, IP, 128, zero, 4.0)), "a zero token is exact: it stays inside the premises"
    assert G.maxsim_margin(dtype, IP, 128, zero, 4.0) == pytest.approx(margin(dtype, IP, 128, zero, 4.0), rel=1e-12)


# ---- the formula against the arithmetic
def chain_f32(q, x):
    """[T, n] f32: the dot products as ONE sequential f32 chain over the dimension, each product rounded, then each sum"""
    acc = np.zeros((q.shape[0], x.shape[0]), np.float32)
    xt = np.ascontiguousarray(x.T.astype(np.float32))
    for d in range(x.shape[1]):
        acc += q[:, d, None] * xt[d][None, :]
    return acc


def selection_scores(q, x, dtype):
    """the selection's dot products: Float16 rows meet the token as f16(q 2^e), max|q| 2^e in [2^14, 2^15), undone in f32"""
    if dtype == F32:
        return chain_f32(q, x)
    mx = np.abs(q).max(1)
    e = np.where((mx > 0) & np.isfinite(mx), 15 - np.frexp(mx)[1], 0)
    up = np.ldexp(np.float32(1.0), e).astype(np.float32)
    q16 = (q * up[:, None]).astype(np.float16).astype(np.float32)
    return chain_f32(q16, x) * np.ldexp(np.float32(1.0), -e).astype(np.float32)[:, None]


def to_scores(dot, q, x, metric, f64=False):
    if metric == IP:
        return dot
    t = np.float64 if f64 else np.float32
    qn = np.sqrt((q.astype(t) ** 2).sum(1, dtype=t))
    xn = np.sqrt((x.astype(t) ** 2).sum(1, dtype=t))
    den = qn[:, None] * xn[None, :]
    with np.errstate(all="ignore"):
        return np.where(den > 0, dot / den, 0).astype(t)


def key_sums(scores, per_key, f64=False):
    """[n_keys]: the per-token best over each key's per_key consecutive rows, summed over the tokens in order"""
    best = scores.reshape(scores.shape[0], -1, per_key).max(2)
    S = best[0].copy()
    for t in range(1, best.shape[0]):
        S = S + best[t] if f64 else (S + best[t]).astype(np.float32)
    return S


def emulate(q, x, dtype, metric, per_key):
    """(S~ f32, S f32 from a blocked f32 product, S float64, Delta) of every key for ONE set of tokens q [T, dim]"""
    xf = x.astype(np.float32)
    approx = key_sums(to_scores(selection_scores(q, xf, dtype), q, xf, metric), per_key)
    exact = key_sums(to_scores(q @ xf.T, q, xf, metric), per_key)
    s64 = key_sums(to_scores(q.astype(np.float64) @ x.astype(np.float64).T, q, x, metric, f64=True), per_key, f64=True)
    norms = np.sqrt((q * q).sum(1, dtype=np.float32))
    xxmax = (xf * xf).sum(1, dtype=np.float32).max()
    return approx, exact, s64, G.maxsim_margin(dtype, metric, x.shape[1], norms, xxmax)


def candidates(approx, delta, k):
    theta = np.sort(approx.astype(np.float64))[::-1][k - 1]
    return approx.astype(np.float64) >= theta - 2.0 * delta


def held(approx, exact, s64, delta, k, what):
    assert np.isfinite(delta) and delta > 0, what
    worst = max(np.abs(approx.astype(np.float64) - exact).max(), np.abs(approx.astype(np.float64) - s64).max())
    assert worst <= delta, f"{what}: |S~ - S| {worst} above Delta {delta}"
    cand = candidates(approx, delta, k)
    for S in (exact.astype(np.float64), s64):
        top = np.lexsort((np.arange(S.size), -S))[:k]
        assert cand[top].all(), f"{what}: a key of the exact top {k} is no candidate"
    return worst / delta, int(cand.sum())


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", [128, 768])
def test_the_formula_holds_the_arithmetic(dtype, dim):
    """2000 keys x 8 rows, T = 5 and 33, both metrics: |S~ - S| <= Delta for every key, the exact top 10 inside the rule"""
    rng = np.random.default_rng(P._seed("mfma emulation", dtype, dim))
    x = rng.standard_normal((16000, dim)).astype(np.float16 if dtype == F16 else np.float32)
    q = rng.standard_normal((33, dim)).astype(np.float32)
    for T in (5, 33):
        for metric in (IP, COS):
            frac, n = held(*emulate(q[:T], x, dtype, metric, 8), 10, f"dim {dim}, T {T}, metric {metric}")
            assert frac < 0.5 and 10 <= n <= 1000, f"the bound is loose but selects: {frac} of Delta, {n} candidates"


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("metric", [IP, COS])
def test_adversarial_rows_and_tokens(dtype, metric):
    dim, T = 128, 5
    rng = np.random.default_rng(P._seed("mfma adversarial", dtype, metric))
    q = rng.standard_normal((T, dim)).astype(np.float32)
    rt = np.float16 if dtype == F16 else np.float32
    # all rows equal: every sum ties up to the chain's rounding, every key is a candidate
    x = np.broadcast_to(rng.standard_normal(dim).astype(rt), (800, dim)).copy()
    approx, exact, s64, delta = emulate(q, x, dtype, metric, 8)
    held(approx, exact, s64, delta, 10, "equal rows")
    assert candidates(approx, delta, 10).all()
    # one-signed rows and tokens: no cancellation, the accumulation's worst case
    x = np.abs(rng.standard_normal((1600, dim))).astype(rt)
    held(*emulate(np.abs(q), x, dtype, metric, 8), 10, "one-signed")
    # tokens of norm 1e-20 and 1e20 among ordinary ones.  1e-20 and 1e15 stay inside the premises: the bound holds as it stands.
    # A token of norm 1e20 has no f32 sum of squares (1e40): its norm is +inf on the device as here, so under InnerProduct Delta
    # is +inf -- every key a candidate, the rule holds trivially -- and under Cosine the token's denominators are not finite,
    # which forces every key it meets (tests/test_gpu_maxsim_mfma.py holds the identity there).
    x = rng.standard_normal((1600, dim)).astype(rt)
    for scale in (1e-20, 1e15, 1e20):
        qs = q.copy()
        qs[1] *= np.float32(scale / np.linalg.norm(q[1]))
        qs[3] *= np.float32(scale / np.linalg.norm(q[3]))
        if scale < 1e20:
            held(*emulate(qs, x, dtype, metric, 8), 10, f"token norm {scale}")
            continue
        with np.errstate(over="ignore"):
            approx, exact, s64, delta = emulate(qs, x, dtype, metric, 8)
            norms = np.sqrt((qs * qs).sum(1, dtype=np.float32))
        assert np.isinf(norms[[1, 3]]).all() and np.isfinite(norms[[0, 2, 4]]).all()
        if metric == IP:
            assert delta == float("inf") and candidates(approx, delta, 10).all()


@pytest.mark.parametrize("dt,dim", [("f32", 100), ("f16", 200)])
def test_the_reference_alone_selects_on_the_gpu_tests_world(dt, dim):
    """tests/test_gpu_maxsim_mfma.py asserts 10 <= candidates <= n_keys / 2 on its world B at k = 10: the emulation stays inside
    those caps on the same rows and tokens, so they are conditions of the rule, not of one kernel"""
    import _maxsim as MS
    import _maxsim_mfma as MM
    lay = MM.world_b()
    live, keys, starts, values = MS.key_order(lay)
    x = P.make_rows(P.N, dim, dt)[live]
    sets = MS.make_sets(3, 5, dim, dt)
    code = F16 if dt == "f16" else F32
    for metric in (IP, COS):
        for q in sets:
            xf = x.astype(np.float32)
            sc = to_scores(selection_scores(q, xf, code), q, xf, metric)
            best = np.maximum.reduceat(sc, starts, axis=1)
            S = best[0].copy()
            for t in range(1, 5):
                S = (S + best[t]).astype(np.float32)
            delta = G.maxsim_margin(code, metric, dim, np.sqrt((q * q).sum(1, dtype=np.float32)), (xf * xf).sum(1, dtype=np.float32).max())
            n = int(candidates(S, delta, 10).sum())
            assert values.size >= 1000 and 10 <= n <= values.size // 4, f"{dt}, metric {metric}: {n} candidates of {values.size} keys"


# ---- the yardsticks of tests/test_gpu_maxsim_mfma_bound.py, themselves tested
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_the_restated_rule_is_the_emulations_on_the_emulations_worlds(dtype):
    """tests/_maxsim_mfma.py p0_rule / theta_of -- what the GPU tests recompute P0 with -- against candidates() on the worlds of
    test_the_formula_holds_the_arithmetic and the one-signed world, then the clauses the emulation's worlds never reach"""
    import _maxsim_mfma as MM
    dim = 128
    rng = np.random.default_rng(P._seed("mfma rule", dtype))
    rt = np.float16 if dtype == F16 else np.float32
    q = rng.standard_normal((33, dim)).astype(np.float32)
    worlds = [(q, rng.standard_normal((16000, dim)).astype(rt)), (np.abs(q), np.abs(rng.standard_normal((1600, dim))).astype(rt))]
    for qs, x in worlds:
        for T in (5, 33):
            for metric in (IP, COS):
                approx, exact, s64, delta = emulate(qs[:T], x, dtype, metric, 8)
                for k in (1, 10, approx.size):
                    theta, nan = MM.theta_of(approx[None], np.zeros((1, approx.size), bool), k)
                    assert not nan[0] and theta[0] == np.sort(approx)[::-1][k - 1]
                    got = MM.p0_rule(approx[None], np.zeros((1, approx.size), bool), np.array([delta]), theta, nan)[0]
                    want = candidates(approx, delta, k)
                    assert (got == want).all() and want.sum() >= k, (T, metric, k)
    # the other clauses: a forced key and a sum that is not finite are candidates and do not count towards theta; theta the NaN
    # entry, theta or Delta not finite: every key; a sum exactly on the threshold is inside (the threshold rounds downwards)
    S = np.array([[5.0, 4.0, np.nan, 3.0, np.inf, 1.0]], np.float32)
    forced = np.array([[True, False, False, False, False, False]])
    theta, nan = MM.theta_of(S, forced, 2)
    assert theta[0] == 3.0 and not nan[0]
    assert MM.p0_rule(S, forced, np.array([0.25]), theta, nan)[0].tolist() == [True, True, True, True, True, False]
    assert MM.p0_rule(S, forced, np.array([1.0]), theta, nan)[0].tolist() == [True, True, True, True, True, True], "1.0 >= 3 - 2 x 1"
    theta, nan = MM.theta_of(S, forced, 4)
    assert nan[0] and np.isnan(theta[0]) and MM.p0_rule(S, forced, np.array([0.25]), theta, nan).all()
    for delta, th in ((np.inf, 3.0), (np.nan, 3.0), (0.25, np.inf), (0.25, -np.inf)):
        assert MM.p0_rule(S, forced, np.array([delta]), np.array([th], np.float32), np.array([False])).all(), (delta, th)
    edge = np.array([[1.0, np.float32(1.0) - np.float32(2.0 ** -10), 0.5]], np.float32)
    got = MM.p0_rule(edge, np.zeros((1, 3), bool), np.array([2.0 ** -11]), np.array([1.0], np.float32), np.array([False]))
    assert got[0].tolist() == [True, True, False]


def test_the_float64_yardstick_and_the_finite_worlds_distance_from_the_premises():
    """tests/_maxsim_mfma.py f64_sums on a world small enough to state by hand, and the condition under which
    tests/test_gpu_maxsim_mfma_bound.py asserts that NO key is forced: on its finite worlds (World A's rows at every shape with
    the token pool, their absolute values at 768 dimensions) every dot product stays below 1e30 and every Cosine denominator
    inside (1e-20, 1e30) -- seven decades and more from the premises' edges 1e37 and 1e-30, from the float64 reference alone"""
    import _maxsim as MS
    import _maxsim_mfma as MM
    x = np.array([[1, 0], [0, 2], [3, 4], [0, 0], [np.nan, 1]], np.float32)
    starts = np.array([0, 2, 3, 4])
    sets = np.array([[[1, 1], [1, -1]], [[0, 0], [2, 0]]], np.float32)
    S, fails = MM.key_sums(MM.f64_sums(x, starts, sets, IP), 2, 2)
    assert S[:, :3].tolist() == [[2 + 1, 7 - 1, 0], [0 + 2, 0 + 6, 0]] and np.isnan(S[:, 3]).all()
    assert fails.tolist() == [[False, False, False, True]] * 2
    S, fails = MM.key_sums(MM.f64_sums(x, starts, sets, COS), 2, 2)
    r = np.sqrt(0.5)
    assert S[0, :3] == pytest.approx([r + r, 7 / 5 * r - 1 / 5 * r, 0]) and S[1, :3] == pytest.approx([1.0, 0.6, 0.0])
    assert fails.tolist() == [[False, False, False, True]] * 2, "a zero row and a zero token score 0: no premise fails"
    tiny = MM.f64_sums(x[:3], starts[:2], np.full((1, 1, 2), 1e-30, np.float32), COS)
    assert (tiny["best"] == 0).all() and not tiny["bad"].any(), "a token whose f32 sum of squares is 0 has norm 0: K1's rule"
    huge = MM.f64_sums(x[:3], starts[:2], np.full((1, 1, 2), 1e30, np.float32), COS)
    assert huge["bad"].all(), "a token whose f32 sum of squares is not finite: the denominator leaves the premises"
    lay = MS.form_layout(2048)
    live, _, starts, _ = MS.key_order(lay)
    for dt, dim in [("f32", 3), ("f32", 100), ("f32", 129), ("f32", 768), ("f16", 8), ("f16", 20), ("f16", 200), ("f16", 768)]:
        rows, pool = P.make_rows(2048, dim, dt), MS.token_pool(dt, dim, 3, 70)
        worlds = [(rows, pool)] + ([(np.abs(rows), np.abs(MS.make_sets(3, 33, dim, dt)))] if dim == 768 else [])
        for r, sets in worlds:
            ref = MM.f64_sums(r[live], starts, sets, COS)
            assert ref["dot_max"] < 1e30 and 1e-20 < ref["den_min"] and ref["den_max"] < 1e30 and not ref["bad"].any(), (dt, dim)
            assert not MM.f64_sums(r[live], starts, sets, IP)["bad"].any()


# ---- the route's header
def test_the_routes_header_is_classed_exported_and_plain_c(tmp_path):
    """include/mvf_gpu_maxsim_route.h: every function it declares has a stream class in tests/_maxsim_mfma.py in the words of
    tests/_streams.py, the aid times a device-call route that table lists, the library exports them all, and a C compiler
    takes the header"""
    import os
    import re
    import shutil
    import subprocess
    import _maxsim_mfma as MM
    import _streams as S
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mvf_gpu_maxsim_route.h")) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    fns = set(re.findall(r"\b(mvfgpu_\w+)\s*\(", text))
    assert fns == set(MM.ENTRY_CLASS) and len(fns) == 5
    assert set(MM.ENTRY_CLASS.values()) <= {S.NO_HANDLE, S.NO_DEVICE_WORK, S.DEVICE_CALL}
    assert not fns & set(S.ENTRY_CLASS), "declared once"
    for aid, form in MM.TIMED_FORM_OF.items():
        assert MM.ENTRY_CLASS[aid] == S.DEVICE_CALL and S.ENTRY_CLASS[form] == S.DEVICE_CALL and form in S.entries_named()
    assert {f for f, c in MM.ENTRY_CLASS.items() if c == S.DEVICE_CALL} == set(MM.TIMED_FORM_OF)
    lib = _lib.gpu()
    for f in fns:
        assert getattr(lib, f) is not None
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:
        src = tmp_path / "t.c"
        src.write_text('#include "mvf_gpu_maxsim_route.h"\nint main(void){return mvfgpu_set_maxsim_route(0, 0) == 0;}\n')
        out = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(root, "include"), str(src)],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr


# ---- refusals
def test_refusals_of_the_new_entry_points():
    lib = _lib.gpu()
    out, d = C.c_uint32(7), C.c_double(7.0)
    norms = (C.c_float * 4)(1, 1, 1, 1)
    assert lib.mvfgpu_set_maxsim_route(None, 1) == E.InvalidArgument.status
    for bad in (lambda: lib.mvfgpu_selftest_maxsim_route(10, 2, 8, F32, IP, 1, 4, 1, 0, None),
                lambda: lib.mvfgpu_selftest_maxsim_route(10, 2, 8, 9, IP, 1, 4, 1, 0, C.byref(out)),
                lambda: lib.mvfgpu_selftest_maxsim_route(10, 2, 8, F32, 3, 1, 4, 1, 0, C.byref(out)),
                lambda: lib.mvfgpu_selftest_maxsim_route(10, 2, 0, F32, IP, 1, 4, 1, 0, C.byref(out)),
                lambda: lib.mvfgpu_selftest_maxsim_route(10, 2, 8, F32, IP, 1, 0, 1, 0, C.byref(out)),
                lambda: lib.mvfgpu_selftest_maxsim_route(10, 2, 8, F32, IP, 1, 1025, 1, 0, C.byref(out)),
                lambda: lib.mvfgpu_selftest_maxsim_route(10, 2, 8, F32, IP, 1, 4, 1, 3, C.byref(out)),
                lambda: lib.mvfgpu_selftest_maxsim_route(10, 2, 8, F32, IP, 1, 4, 1, -1, C.byref(out)),
                lambda: lib.mvfgpu_selftest_maxsim_margin(F32, IP, 8, None, 4, 1.0, C.byref(d)),
                lambda: lib.mvfgpu_selftest_maxsim_margin(F32, IP, 8, norms, 4, 1.0, None),
                lambda: lib.mvfgpu_selftest_maxsim_margin(I8, IP, 8, norms, 4, 1.0, C.byref(d)),
                lambda: lib.mvfgpu_selftest_maxsim_margin(F32, L2, 8, norms, 4, 1.0, C.byref(d)),
                lambda: lib.mvfgpu_selftest_maxsim_margin(F32, IP, 0, norms, 4, 1.0, C.byref(d)),
                lambda: lib.mvfgpu_selftest_maxsim_margin(F32, IP, 8, norms, 0, 1.0, C.byref(d)),
                lambda: lib.mvfgpu_selftest_maxsim_margin(F32, IP, 8, norms, 1025, 1.0, C.byref(d)),
                lambda: lib.mvfgpu_selftest_maxsim_mfma_stage_ms(None, None, IP, None, 0, 8, 1, 4, 1, None, None, None, None, None, None)):
        assert bad() == E.InvalidArgument.status
    assert out.value == 7 and d.value == 7.0, "a refused call writes nothing"
    # the selection's read-out: NULL outputs, each alone and all together, and -- every output given -- the search's own refusal of
    # a NULL handle (an ineligible type or metric needs a handle: tests/test_gpu_maxsim_mfma_bound.py)
    bufs = [np.full(4, 7, t) for t in (np.float32, np.uint8, np.uint8, np.float64, np.float32, np.uint8, np.float32)]
    given = [b.ctypes.data_as(C.c_void_p) for b in bufs]
    for outs in [[None] * 7, given] + [[None if i == j else g for i, g in enumerate(given)] for j in range(7)]:
        assert lib.mvfgpu_selftest_maxsim_mfma_selection(None, None, IP, None, 0, 8, 1, 4, 1, None, None, None, *outs) == E.InvalidArgument.status
    assert all((b == 7).all() for b in bufs), "a refused call writes nothing"
    with pytest.raises(E.InvalidArgument, match="route must be 0, 1 or 2, got 3"):
        G.maxsim_route(10, 2, 8, F32, IP, 1, 4, 1, 3)
    with pytest.raises(E.InvalidArgument, match="Float32 / Float16 rows under InnerProduct / Cosine"):
        G.maxsim_margin(U8, COS, 8, [1.0], 1.0)
