"""Wide rows, CPU tier: what tests/test_gpu_wide_rows.py leans on, checked without a GPU.

* the integer reference of tests/_wide.py equals the C oracle bit for bit on saturated rows at dimension 33025, where the
  L2 raw value reaches 65025 * 33025 = INT32_MAX - 33022;
* the float64 reference is accurate to a small fraction of DESIGN.md section 3's tolerance (against correctly rounded
  sums), and the strict-order f32 oracle is not: its own rounding is measured in units of that tolerance;
* every float case of the GPU tier keeps few rows inside the boundary band of assert_float_topk;
* the radius -> i32 bound conversion at the top of the i32 range;
* the route self-tests at the dimension switches, pinned."""
import ctypes as C
import math

import numpy as np
import pytest

from metrovector_amd import gpu as G

import _wide as W
from _wide import COS, F16, F32, I8, IP, L2, U8

INT32_MAX, INT32_MIN = 2**31 - 1, -2**31


# ---------------------------------------------------------------------------------------------------------------------
# the integer reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [I8, U8])
def test_integer_reference_equals_the_oracle_on_saturated_rows(oracle, dtype):
    n, dim, nq, k = 9000, W.MAX_INT_DIM, 16, 100
    rows, pos = W.saturated_rows(oracle, 0x5A7 + dtype, n, dim, dtype)
    q = W.saturated_queries(oracle, 0x5A8 + dtype, nq, dim, dtype)
    dot, qq, xx = W.int_raw(rows, q)
    l2 = qq[:, None] + xx[None, :] - 2 * dot
    assert int(l2.max()) == W.L2_RAW_MAX == 2_147_450_625 == INT32_MAX - 33_022
    assert int(l2[0, pos[1]]) == W.L2_RAW_MAX and int(l2[1, pos[0]]) == W.L2_RAW_MAX  # all-min against all-max, both ways
    if dtype == U8:
        assert int(dot.max()) == W.L2_RAW_MAX and int(xx.max()) == W.L2_RAW_MAX and int(qq.max()) == W.L2_RAW_MAX
    else:
        assert int(dot.max()) == 128 * 128 * dim and int(dot.min()) == -128 * 127 * dim
    assert (rows[pos[4]] == rows[pos[5]]).all()  # the planted tie
    for metric in (L2, IP, COS):
        sc, idx, raw = W.int_topk(metric, dot, qq, xx, k)
        osc, oidx, oraw = oracle.search(rows, dtype, metric, q, k)
        assert (idx == oidx).all(), metric
        assert (raw == oraw).all(), metric
        assert (sc.view(np.uint32) == osc.view(np.uint32)).all(), metric
    # the planted rows are in play: the all-max query's best dot products are planted rows, in position order on the tie
    best = W.int_topk(IP, dot, qq, xx, 4)[1][1].astype(np.int64).tolist()
    assert set(best) <= set(pos) and best[0] == pos[1]


def test_integer_reference_with_deletions_and_ids(oracle):
    n, dim = 8200, 8193
    rows, pos = W.saturated_rows(oracle, 77, n, dim, U8)
    q = W.saturated_queries(oracle, 78, 6, dim, U8)
    dead = np.zeros(n, bool)
    dead[pos[::2]] = True
    ids = np.random.default_rng(5).permutation(np.arange(50_000, 50_000 + n)).astype(np.uint64)
    dot, qq, xx = W.int_raw(rows, q)
    live = np.nonzero(~dead)[0]
    for metric in (L2, IP, COS):
        sc, idx, raw = W.int_topk(metric, dot, qq, xx, 50, dead=dead, labels=ids)
        osc, oidx, oraw = oracle.search(rows[live], U8, metric, q, 50)
        assert (idx == ids[live[oidx.astype(np.int64)]]).all() and (raw == oraw).all()
        assert (sc.view(np.uint32) == osc.view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------------------------------
# the float reference
# ---------------------------------------------------------------------------------------------------------------------
def _exact_scores(x, q):
    """(l2, dot, cosine) of one row from correctly rounded sums: math.fsum over float64 terms.  The products of two
    f32 / f16 values are exact in float64; (q - x)^2 rounds once per term (2^-53 relative)."""
    x, q = x.astype(np.float64), q.astype(np.float64)
    dot, qq, xx = math.fsum((q * x).tolist()), math.fsum((q * q).tolist()), math.fsum((x * x).tolist())
    l2 = math.sqrt(math.fsum(((q - x) ** 2).tolist()))
    den = math.sqrt(qq) * math.sqrt(xx)
    return {L2: l2, IP: dot, COS: dot / den if den > 0 else 0.0}


@pytest.mark.parametrize("dtype,dim,kind", [(F32, 36000, "synthetic"), (F32, 36000, "nonneg"), (F16, 33000, "planted")])
def test_float64_reference_against_correctly_rounded_sums(oracle, dtype, dim, kind):
    """The yardstick's own error, in units of the tolerance it is used to check: below 1e-3 (observed ~1e-8).  With the
    oracle's scores in place of f64_scores_all's this fails at these dimensions: see the test below."""
    rows, q = W.float_inputs(oracle, 11, 64, dim, dtype, 4, kind)
    ref = W.f64_scores_all(rows, q)
    for metric in (L2, IP, COS):
        for qi in range(4):
            exact = np.array([_exact_scores(rows[r], q[qi])[metric] for r in range(0, 64, 8)])
            frac = W.tolerance_fraction(metric, ref[metric][qi, 0:64:8], exact, rows[0:64:8], q[qi])
            assert frac < 1e-3, f"float64 reference off by {frac} of the tolerance (metric {metric}, query {qi})"


def test_strict_order_f32_oracle_is_no_yardstick_for_wide_rows(oracle):
    """The oracle-to-float64 error as a fraction of DESIGN.md section 3's tolerance, synthetic Float32 rows (n = 3000, 8
    queries; L2 on the generator's rows, cosine on their absolute values), next to a pairwise f32 sum of the same rows.
    Measured: L2 0.08 at dimension 768, 0.28 at 8192, 0.49 at 20000, 0.64-0.79 at 33025-36000; cosine on non-negative
    rows 0.29 / 0.64 / 0.90 at 8192 / 20000 / 36000; pairwise 0.01-0.03.  Asserted: what justifies a float64 reference --
    negligible at 768, more than half the tolerance at 36000 -- and that the pairwise sum stays an order below."""
    n, nq = 3000, 8
    seen = {}
    for dim in (768, 8192, 20000, 36000):
        rows, q = W.float_inputs(oracle, 21, n, dim, F32, nq, "synthetic")
        ref = W.f64_scores(rows, q, L2)
        seen[("l2", dim)] = max(W.tolerance_fraction(L2, oracle.scores(rows, F32, L2, q[i])[0], ref[i], rows, q[i]) for i in range(nq))
        seen[("l2 pairwise", dim)] = max(W.tolerance_fraction(L2, W.pairwise_f32_scores(rows, q[i], L2), ref[i], rows, q[i]) for i in range(2))
        np.abs(rows, out=rows)
        np.abs(q, out=q)
        ref = W.f64_scores(rows, q, COS)
        seen[("cos nonneg", dim)] = max(W.tolerance_fraction(COS, oracle.scores(rows, F32, COS, q[i])[0], ref[i], rows, q[i]) for i in range(nq))
    report = ", ".join(f"{name} @ {dim}: {v:.3f}" for (name, dim), v in seen.items())
    assert seen[("l2", 768)] < 0.1, report
    assert seen[("l2", 36000)] > 0.5, report
    assert seen[("l2", 768)] < seen[("l2", 8192)] < seen[("l2", 36000)], report
    assert seen[("cos nonneg", 36000)] > 0.5, report
    assert all(seen[("l2 pairwise", dim)] < 0.1 for dim in (768, 8192, 20000, 36000)), report


@pytest.mark.parametrize("dtype,dim,kind,ks", W.float_cases())
def test_float_cases_keep_the_boundary_band_thin(oracle, dtype, dim, kind, ks):
    """For every float case of the GPU tier, every query it uses, every metric and k: the rows beside the k-th best whose
    float64 score lies inside assert_float_topk's band around it are at most 10 % of k (measured over the whole pools: <= 8
    at k = 100, <= 20 at k = 1000, and 0-2 at k = 10).  Rows inside the band may be ranked either way by a correct kernel,
    so a query with a crowded band checks little: the GPU tier takes the first 130 queries of a pool of 170 that hold the
    condition (tests/_wide.py thin_band_queries).  Here: the pool suffices with room to spare (at most a fifth of the
    queries in front of the last one used is passed over -- a change of shapes that crowds the boundary fails this), and
    the chosen queries hold the condition."""
    rows, q = W.float_inputs(oracle, W.float_case_seed(dtype, dim, kind), W.FLOAT_N, dim, dtype, W.FLOAT_POOL, kind)
    ref = W.f64_scores_all(rows, q)
    rows32 = rows if dtype == F32 else rows.astype(np.float32)
    use = W.thin_band_queries(ref, rows32, q, ks)
    assert len(use) == W.FLOAT_NQ, f"only {len(use)} of {W.FLOAT_POOL} queries keep the band thin"
    assert int(use[-1]) + 1 - W.FLOAT_NQ <= (int(use[-1]) + 1) // 5, f"{int(use[-1]) + 1 - W.FLOAT_NQ} queries passed over"
    if kind == "planted":
        assert np.count_nonzero(use % 2 == 0) >= W.FLOAT_NQ // 3  # planted and free queries both stay in
    worst = {(m, k): max(W.band_count(m, ref[m][qi], rows32, q[qi], k) for qi in use) for m in (L2, IP, COS) for k in ks}
    for (metric, k), c in worst.items():
        assert c <= k // 10, f"{c} rows in the band at k = {k}, metric {metric}: all cases {worst}"


# ---------------------------------------------------------------------------------------------------------------------
# radius -> i32 bound at the top of the range
# ---------------------------------------------------------------------------------------------------------------------
def _l2_bound_brute(r, window=4096):
    """largest R in [0, INT32_MAX] with sqrtf((float)R) <= r, over the integers around r^2 (numpy's f32 sqrt is
    correctly rounded)"""
    r = np.float32(r)
    if r < 0:
        return -1
    if np.isinf(r) or np.sqrt(np.float32(INT32_MAX)) <= r:
        return INT32_MAX
    c = int(float(r) * float(r))
    R = np.arange(max(0, c - window), min(INT32_MAX, c + window) + 1, dtype=np.int64)
    ok = np.sqrt(R.astype(np.float32)) <= r
    assert ok[0] and not ok[-1]
    return int(R[ok].max())


def _ip_bound_brute(r, window=4096):
    """smallest R with (float)R >= r; INT32_MAX when no i32 reaches r"""
    r = np.float32(r)
    if r == -np.inf:
        return INT32_MIN
    if r > np.float32(INT32_MAX):
        return INT32_MAX
    c = int(math.floor(float(r)))
    R = np.arange(max(INT32_MIN, c - window), min(INT32_MAX, c + window) + 1, dtype=np.int64)
    ok = R.astype(np.float32) >= r
    return int(R[ok].min()) if ok.any() else INT32_MAX


@pytest.mark.parametrize("dtype", [I8, U8])
def test_l2_radius_bound_at_the_largest_raw_value(dtype):
    top = np.sqrt(np.float32(float(W.L2_RAW_MAX)))
    below, above = np.nextafter(top, np.float32(0)), np.nextafter(top, np.float32(np.inf))
    f = lambda r: G.radius_bound(dtype, G.L2, float(r))  # noqa: E731
    for r in (top, below, above):
        key, raw = f(r)
        assert raw == _l2_bound_brute(r), float(r)
        assert key == (raw ^ 0x80000000)
    # f32 keeps 24 bits: 128 integers share sqrtf's argument up there, and the radius that IS the largest row's score has to
    # admit the largest raw value, the one below it must not
    assert f(top)[1] >= W.L2_RAW_MAX > f(below)[1]
    assert f(above)[1] > f(top)[1]
    assert f(math.inf)[1] == INT32_MAX
    assert f(np.sqrt(np.float32(INT32_MAX)))[1] == INT32_MAX
    assert f(np.nextafter(np.sqrt(np.float32(INT32_MAX)), np.float32(0)))[1] == _l2_bound_brute(np.nextafter(np.sqrt(np.float32(INT32_MAX)), np.float32(0)))


@pytest.mark.parametrize("dtype", [I8, U8])
def test_inner_product_radius_bound_at_the_largest_and_smallest_dot(dtype):
    dim = W.MAX_INT_DIM
    hi = 255 * 255 * dim if dtype == U8 else 128 * 128 * dim
    lo = 0 if dtype == U8 else -128 * 127 * dim
    f = lambda r: G.radius_bound(dtype, G.INNER_PRODUCT, float(r))  # noqa: E731
    for v in (hi, lo):
        at = np.float32(v)
        for r in (at, np.nextafter(at, np.float32(np.inf)), np.nextafter(at, np.float32(-np.inf))):
            key, raw = f(r)
            assert raw == _ip_bound_brute(r), float(r)
            assert key == (~(raw ^ 0x80000000) & 0xFFFFFFFF)
    # a radius rounded UP from the largest dot no longer admits it; one rounded down does
    if np.float32(hi) > hi:
        assert f(np.float32(hi))[1] > hi
    assert f(np.nextafter(np.float32(hi), np.float32(0)))[1] <= hi
    # (float)R rounds to nearest: every R from 2^31 - 64 on becomes 2^31, every R from 2^31 - 191 on at least 2^31 - 128
    assert f(2147483648.0)[1] == 2147483584 == _ip_bound_brute(2147483648.0)
    assert f(2147483520.0)[1] == 2147483457 == _ip_bound_brute(2147483520.0)
    assert f(np.nextafter(np.float32(2147483648.0), np.float32(np.inf)))[1] == INT32_MAX  # no i32 reaches it: nothing matches
    assert f(-2147483648.0)[1] == INT32_MIN


# ---------------------------------------------------------------------------------------------------------------------
# routes at the dimension switches
# ---------------------------------------------------------------------------------------------------------------------
def _route(rows, dim, dtype, metric, nq, k):
    out = C.c_uint32(99)
    G._lib.gpu_check(G._lib.gpu().mvfgpu_selftest_route(rows, dim, dtype, metric, nq, k, C.byref(out)))
    return out.value


K1, BATCHED = 0, 1


def test_routes_at_the_dimension_switches_are_pinned():
    """`mvfgpu_selftest_route` / `_stream_rows` for the shapes of tests/test_gpu_wide_rows.py (default tuning, scan path 0, no
    history).  The self-test sees: the re-scoring kernels' LDS limit (Float32 L2 and every Float16 batch leave the batched
    route above dimension 12288), the limit of the exact f32 MFMA kernel's final keys (Float32 InnerProduct / Cosine leave
    it above 16384) and, through the "shadowed" thresholds, the end of the int8-shadow selection above 8192.
    It does NOT see which kernel the batched route then runs (6 / 4 / 3 / 2: the GPU tier asserts `scan_kernel`), nor the
    LDS fallbacks of the streaming kernel -- four-query passes giving way to one-query passes above 150 KiB, the refusal
    above 160 KiB: both are decided per launch from scan_lds_bytes and are restated in tests/_wide.py, where the GPU tier
    (groups B, F and G) holds the restatement against the library's behaviour."""
    n = W.FLOAT_N
    for dim in (8192, 8200, 12288):
        for dtype in (F32, F16):
            for metric in (L2, IP, COS):
                assert _route(n, dim, dtype, metric, 1, 10) == K1
                assert _route(n, dim, dtype, metric, 40, 10) == BATCHED
                assert _route(n, dim, dtype, metric, 130, 100) == BATCHED
    # three queries: with a shadow to select on, corpora of <= 512 MB stay on K1; Float16 rows beyond the int8 shadow's
    # limit have none and take the batched route from two queries, Float32 rows there still have the f16 shadow
    assert _route(n, 8192, F32, L2, 3, 10) == K1 and _route(n, 8192, F16, L2, 3, 10) == K1
    assert _route(n, 8200, F32, L2, 3, 10) == K1 and _route(n, 8200, F16, L2, 3, 10) == BATCHED
    assert _route(n, 12288, F32, COS, 3, 10) == K1 and _route(n, 12288, F16, COS, 3, 10) == BATCHED
    for dim in (12296, 16384, 16392, 20000, 33000, 38400):
        for nq in (1, 3, 40, 130):
            for metric in (L2, IP, COS):
                assert _route(n, dim, F16, metric, nq, 10) == K1          # no re-scoring kernel for such rows
            assert _route(n, dim, F32, L2, nq, 10) == K1
        for metric in (IP, COS):
            # the exact f32 MFMA kernel carries final keys (no re-scoring) -- up to dimension 16384: on wider rows its one long
            # chain per sum no longer holds the tolerance on one-signed data (GPU tier, group D) and K1 takes every batch
            want = [K1, K1, K1, BATCHED, BATCHED, BATCHED] if dim <= 16384 else [K1] * 6
            assert [_route(n, dim, F32, metric, nq, 10) for nq in (1, 3, 31, 32, 40, 130)] == want, (dim, metric)
            assert _route(10_000_000, dim, F32, metric, 1024, 100) == (BATCHED if dim <= 16384 else K1)  # whatever the size
    # Int8 / UInt8 rows: no switch in the route itself (the batched kernels' epilogue changes at 8192: GPU tier, group A)
    for dtype in (I8, U8):
        for dim in (8192, 8193, 33025):
            for metric in (L2, IP, COS):
                assert [_route(9000, dim, dtype, metric, nq, 10) for nq in (1, 3)] == [K1, K1]
                assert [_route(9000, dim, dtype, metric, nq, 100) for nq in (40, 128, 257)] == [BATCHED] * 3
        assert _route(9000, 33025, dtype, L2, 1, 2048) in (2, 3)  # beyond one pass: passes or the whole-shard sort
    # which rows ONE Float32 query streams: the int8 shadow from 512 MiB of rows on, up to dimension 8192
    for metric in (L2, IP, COS):
        assert G.stream_rows(16_400, 8192, F32, metric, 1, 100) == 1
        assert G.stream_rows(16_383, 8192, F32, metric, 1, 100) == 0   # below 512 MiB
        assert G.stream_rows(16_400, 8200, F32, metric, 1, 100) == 0
        assert G.stream_rows(16_400, 12288, F32, metric, 1, 100) == 0
        assert G.stream_rows(16_400, 12296, F32, metric, 1, 100) == 0
        assert G.stream_rows(16_400, 33025, F32, metric, 1, 100) == 0
        assert G.stream_rows(16_400, 8192, F16, metric, 1, 100) == 0 and G.stream_rows(16_400, 8192, F32, metric, 2, 100) == 0


def test_k1_lds_restatement_gives_the_documented_limits():
    """tests/_wide.py restates scan_lds_bytes; the numbers DESIGN.md section 3 quotes come out of it."""
    assert W.k1_max_dim(F32, 10) == W.k1_max_dim(F32, 512) == 38656
    assert W.k1_max_dim(F16, 100) == 38400
    assert W.k1_max_dim(F32, 1000) == W.k1_max_dim(F32, 2048) == 36608 and W.k1_max_dim(F16, 1000) == 36352
    assert W.k1_max_dim(I8, 1024) > W.MAX_INT_DIM       # integer rows never reach the refusal
    assert W.k1_four_query_pass(I8, 29696, 100) and not W.k1_four_query_pass(I8, 29697, 100)
    assert W.k1_four_query_pass(I8, 28000, 512) and not W.k1_four_query_pass(I8, 28000, 1024)  # the lists grow with k
    assert not W.k1_four_query_pass(F32, 8192, 10) and not W.k1_four_query_pass(F16, 8192, 10)
