"""References and inputs for rows of thousands of dimensions (tests/test_wide_cpu.py, tests/test_gpu_wide_rows.py).

Plain numpy, no GPU.  Two references, both independent of the C oracle:

* float rows: float64 scores of every row from the exactly widened inputs.  From dimension ~8k on the strict-order f32
  oracle's own rounding is a sizeable fraction of DESIGN.md section 3's tolerance (test_wide_cpu.py measures it), so a kernel
  compared with the oracle there would be passed or failed by the oracle's rounding; float64 is ~1e-9 of that tolerance.
* Int8 / UInt8 rows: exact int64 raw values, order (raw, position), scores restated in numpy f32 as DESIGN.md section 3
  writes them.  Bit-exact.

Inputs: integer rows with SATURATED rows planted (sums next to 2^31: uniform random bytes sit three orders of magnitude
below the range the arithmetic is declared exact for), and wide float rows in three kinds (synthetic, the same made
non-negative, and queries planted next to a stored row)."""
import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
F32, F16, I8, U8 = 0, 1, 2, 3
L2, IP, COS = 0, 1, 2
MAX_INT_DIM = 33025            # include/mvf_gpu.h MVFGPU_MAX_INT_DIM: dim * 255^2 < 2^31
L2_RAW_MAX = 65025 * 33025     # 2 147 450 625 = INT32_MAX - 33 022: all-min against all-max at the largest dimension


# ---------------------------------------------------------------------------------------------------------------------
# K1's LDS rule, restated (metrovector_amd/csrc/scan_stream.h scan_lds_bytes + api.hip choose_group, wide rows only)
# ---------------------------------------------------------------------------------------------------------------------
ELEM = {F32: 4, F16: 2, I8: 1, U8: 1}
K1_FOUR_QUERY_LDS = 150 * 1024   # above it 2..4 queries run as one-query passes
K1_MAX_LDS = 160 * 1024          # above it the search is refused (MVF_ERR_BUILD)


def next_pow2(x):
    p = 1
    while p < x:
        p *= 2
    return p


def k1_lds_bytes(dtype, dim, nqv, k):
    """scan_lds_bytes(dtype, G, J, nqv, next_pow2(k + scan_chunk_safe(G))) for rows of >= 512 16-byte vectors, where
    choose_group takes G = 64 lanes per row for one and for four queries per pass (scan_chunk_safe(64) = 512)."""
    V = (dim * ELEM[dtype] + 15) // 16
    assert V >= 512, "the restatement covers wide rows only"
    G = 64
    J = (V + G - 1) // G
    qb = 32 if dtype == F16 else 16          # LDS bytes per 16-byte vector of the row type (f16 queries are kept widened)
    q = (nqv * J * G * qb + 15) & ~15
    pmax = next_pow2(min(k, 1024) + 512)     # beyond MVFGPU_K_PER_PASS the kernel's lists stay at one pass' size
    return q + nqv * pmax * 8 + nqv * 32


def k1_four_query_pass(dtype, dim, k):
    """True where two to four queries share one pass over the rows (the 150-KiB rule)."""
    return k1_lds_bytes(dtype, dim, 4, k) <= K1_FOUR_QUERY_LDS


def k1_max_dim(dtype, k):
    """The largest dimension the streaming kernel takes at this k (the 160-KiB rule at one query per pass)."""
    lo, hi = 512 * 16 // ELEM[dtype], 1 << 20
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if k1_lds_bytes(dtype, mid, 1, k) <= K1_MAX_LDS:
            lo = mid
        else:
            hi = mid - 1
    return lo


def radius_lds_bytes(dtype, dim, nqv):
    """radius_scan_lds_bytes (scan_radius.hip): the streaming radius kernel keeps the queries in LDS and no candidate
    lists, so its limits lie above K1's."""
    V = (dim * ELEM[dtype] + 15) // 16
    assert V >= 512
    J = (V + 63) // 64
    return ((nqv * J * 64 * (32 if dtype == F16 else 16) + 15) & ~15) + nqv * 16


def radius_max_dim(dtype):
    """The largest dimension the streaming radius kernel takes (160 KiB at one query per pass)."""
    lo, hi = 512 * 16 // ELEM[dtype], 1 << 20
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if radius_lds_bytes(dtype, mid, 1) <= K1_MAX_LDS:
            lo = mid
        else:
            hi = mid - 1
    return lo


# ---------------------------------------------------------------------------------------------------------------------
# float reference
# ---------------------------------------------------------------------------------------------------------------------
def f64_scores_all(rows, queries, chunk_bytes=1 << 29):
    """float64 score of every row for every query, every metric from one pass over the rows -> {metric: f64[nq, n]}
    (row qi of an array is what assert_float_topk takes as all_scores).

    The inputs are widened exactly (f16 / f32 -> f64); rows in chunks so the f64 copy stays under chunk_bytes.  Dot
    products by a float64 GEMM; L2 as sqrt(qq + xx - 2 dot) in float64: its cancellation error is ~dim^0.5 * 2^-53 *
    (qq + xx), 1e-9 relative even for a planted query at 1 % of the row's norm -- four orders below the 1e-5 under test
    (test_wide_cpu.py checks the whole function against correctly rounded sums).  Cosine is 0 where the denominator is
    not > 0."""
    q = np.atleast_2d(queries).astype(np.float64)
    n, dim = rows.shape
    out = {m: np.empty((q.shape[0], n), np.float64) for m in (L2, IP, COS)}
    qq = np.einsum("ij,ij->i", q, q)
    step = max(1, chunk_bytes // (dim * 8))
    for r0 in range(0, n, step):
        x = rows[r0:r0 + step].astype(np.float64)
        dot = q @ x.T
        xx = np.einsum("ij,ij->i", x, x)
        out[IP][:, r0:r0 + step] = dot
        out[L2][:, r0:r0 + step] = np.sqrt(np.maximum(qq[:, None] + xx[None, :] - 2.0 * dot, 0.0))
        den = np.sqrt(qq)[:, None] * np.sqrt(xx)[None, :]
        out[COS][:, r0:r0 + step] = np.where(den > 0, dot / np.where(den > 0, den, 1.0), 0.0)
    return out


def f64_scores(rows, queries, metric, chunk_bytes=1 << 29):
    return f64_scores_all(rows, queries, chunk_bytes)[metric]


def pairwise_f32_scores(rows, query, metric):
    """The same scores summed in float32 by numpy's pairwise reduction (what a tree-shaped f32 sum achieves; test_wide_cpu.py
    sets it beside the strict-order oracle) -> f32[n]."""
    x = rows.astype(np.float32)
    q = np.asarray(query, np.float32)
    if metric == L2:
        d = x - q
        return np.sqrt(np.sum(d * d, axis=1, dtype=np.float32))
    dot = np.sum(x * q, axis=1, dtype=np.float32)
    if metric == IP:
        return dot
    den = np.sqrt(np.sum(q * q, dtype=np.float32)) * np.sqrt(np.sum(x * x, axis=1, dtype=np.float32))
    return np.where(den > 0, dot / np.where(den > 0, den, np.float32(1)), np.float32(0)).astype(np.float32)


def tolerance_fraction(metric, got, ref64, rows, query):
    """max over rows of |got - ref64| in units of DESIGN.md section 3's tolerance (1e-5 relative for L2, 1e-5 absolute for
    cosine, 1e-5 |q||x| for dot)."""
    err = np.abs(got.astype(np.float64) - ref64)
    if metric == L2:
        tol = 1e-5 * np.maximum(np.abs(ref64), 1e-30)
    elif metric == COS:
        tol = 1e-5
    else:
        x = rows.astype(np.float64)
        tol = 1e-5 * np.sqrt(np.einsum("ij,ij->i", x, x)) * float(np.linalg.norm(np.asarray(query, np.float64)))
    return float(np.max(err / tol))


def band_count(metric, all_scores, rows_f32, q_f32, k):
    """Rows other than the top-k's own whose reference score lies inside assert_float_topk's boundary band around the k-th
    best: the rows the criterion lets a kernel rank either way.  A case is only worth running while they are few."""
    from _util import boundary_band
    kk = min(k, len(all_scores))
    key, kth, btol = boundary_band(metric, all_scores, rows_f32, q_f32, kk)
    return int(np.count_nonzero(np.abs(key - kth) <= btol)) - 1


# ---------------------------------------------------------------------------------------------------------------------
# integer reference
# ---------------------------------------------------------------------------------------------------------------------
def int_raw(rows, queries, chunk=1000):
    """Exact (dot, qq, xx) as int64: dot[nq, n], qq[nq], xx[n].  A float64 GEMM per `chunk` rows is exact here: every
    product is below 2^16 and every sum below 2^31 (dimension <= 33025), far inside the 2^53 float64 counts exactly."""
    assert rows.shape[1] <= MAX_INT_DIM
    q = np.atleast_2d(queries).astype(np.float64)
    n = rows.shape[0]
    dot = np.empty((q.shape[0], n), np.int64)
    xx = np.empty(n, np.int64)
    for r0 in range(0, n, chunk):
        x = rows[r0:r0 + chunk].astype(np.float64)
        dot[:, r0:r0 + chunk] = np.rint(q @ x.T).astype(np.int64)
        xx[r0:r0 + chunk] = np.rint(np.einsum("ij,ij->i", x, x)).astype(np.int64)
    qq = np.rint(np.einsum("ij,ij->i", q, q)).astype(np.int64)
    return dot, qq, xx


def int_scores(metric, dot, qq, xx):
    """(scores f32[nq, n], keys i64-or-f64[nq, n] ascending = best first, raw i32[nq, n]) from the exact integers, as
    DESIGN.md section 3 writes them: sqrtf((float)raw), (float)raw, (float)dot / (sqrtf((float)qq) * sqrtf((float)xx)) and
    0 when the denominator is not > 0; cosine reports raw = 0."""
    if metric == L2:
        raw = qq[:, None] + xx[None, :] - 2 * dot
        assert raw.min() >= 0 and raw.max() <= 2**31 - 1
        return np.sqrt(raw.astype(np.float32)), raw, raw.astype(np.int32)
    if metric == IP:
        assert dot.min() >= -2**31 and dot.max() <= 2**31 - 1
        return dot.astype(np.float32), -dot, dot.astype(np.int32)
    den = np.sqrt(qq.astype(np.float32))[:, None] * np.sqrt(xx.astype(np.float32))[None, :]
    ok = den > 0
    sc = np.where(ok, dot.astype(np.float32) / np.where(ok, den, np.float32(1)), np.float32(0)).astype(np.float32)
    sc = sc + np.float32(0)  # -0.0 -> +0.0
    return sc, -sc.astype(np.float64), np.zeros(dot.shape, np.int32)


def int_topk(metric, dot, qq, xx, k, dead=None, labels=None):
    """Top-k of every query: best first, ties by ascending POSITION, deleted rows left out, the library's padding behind.
    labels: what a result carries for row r (vector ids, or index_base + r); default the position.
    -> (scores f32[nq, k], indices u64[nq, k], raw i32[nq, k])"""
    sc, key, raw = int_scores(metric, dot, qq, xx)
    nq, n = sc.shape
    live = np.arange(n) if dead is None else np.nonzero(~dead)[0]
    out_s = np.full((nq, k), np.inf if metric == L2 else -np.inf, np.float32)
    out_i = np.full((nq, k), PAD, np.uint64)
    out_r = np.zeros((nq, k), np.int32)
    for qi in range(nq):
        take = live[np.argsort(key[qi, live], kind="stable")[:k]]
        out_s[qi, :take.size] = sc[qi, take]
        out_i[qi, :take.size] = take.astype(np.uint64) if labels is None else labels[take]
        out_r[qi, :take.size] = raw[qi, take]
    return out_s, out_i, out_r


class IntScores:
    """The integer reference behind the interface tests/_radius.py and tests/_candidates.py expect of the oracle
    (`scores(rows, dtype, metric, query) -> (scores, order keys, raw)`), for ONE corpus and its queries: the values
    come from the exact int64 sums, looked up by the query's bytes."""

    def __init__(self, rows, queries):
        self.rows, self.queries = rows, np.atleast_2d(queries)
        self.dot, self.qq, self.xx = int_raw(rows, self.queries)

    def scores(self, rows, dtype, metric, query):
        assert rows is self.rows
        hit = np.nonzero((self.queries == np.asarray(query)[None, :]).all(axis=1))[0]
        assert hit.size, "not one of this reference's queries"
        qi = int(hit[0])
        sc, key, raw = int_scores(metric, self.dot[qi:qi + 1], self.qq[qi:qi + 1], self.xx)
        # order keys: ascending = best first, dense ranks so that they are integers whatever the metric
        keys = np.unique(key[0], return_inverse=True)[1].astype(np.uint32)
        return sc[0], keys, raw[0]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
INT_RANGE = {I8: (-128, 127), U8: (0, 255)}


def planted_positions(n):
    """Rows that fall into different tiles and phases of the batched kernels and different chunks of the streaming one:
    the first row, both sides of a 256-row tile and of a 4096-row boundary, and the tail."""
    assert n >= 8200
    pos = [0, 255, 256, 4095, 4096, 4097, n - 1]
    pos += [n - 2, n - 130, n - 257, n - 700, 2000, 4100, 6000, 6001, n - 1000, n - 1001, 8191, 8192, 100, 101, 7000]
    assert len(set(pos)) == len(pos)
    return pos


def saturated_rows(oracle, seed, n, dim, dtype):
    """Synthetic Int8 / UInt8 rows with saturated rows planted -> (rows, planted positions).  In order: all-min, all-max,
    alternating min / max, all-max with one element at min, then all-max rows with one to three elements lowered by one
    (ties and near-ties at the top of the range; two of them are equal rows at different positions)."""
    lo, hi = INT_RANGE[dtype]
    rows = oracle.synth_rows(seed, 0, n, dim, dtype)
    pos = planted_positions(n)
    t = rows.dtype.type
    rows[pos[0]] = t(lo)
    rows[pos[1]] = t(hi)
    rows[pos[2], 0::2] = t(lo)
    rows[pos[2], 1::2] = t(hi)
    rows[pos[3]] = t(hi)
    rows[pos[3], dim // 2] = t(lo)
    rng = np.random.default_rng(seed)
    for i, p in enumerate(pos[4:]):
        rows[p] = t(hi)
        if i == 1:                       # the same row as the one before it, elsewhere: a tie broken by position
            rows[p] = rows[pos[4]]
            continue
        for j in rng.choice(dim, 1 + i % 3, replace=False):
            rows[p, j] = t(hi - 1)
    return rows, pos


def saturated_queries(oracle, seed, nq, dim, dtype):
    """Queries: all-min, all-max, alternating min / max, all-zero, the rest synthetic."""
    lo, hi = INT_RANGE[dtype]
    q = oracle.synth_queries(seed, nq, dim, dtype)
    t = q.dtype.type
    special = [np.full(dim, lo), np.full(dim, hi), np.where(np.arange(dim) % 2 == 0, lo, hi), np.zeros(dim, np.int64)]
    for i, s in enumerate(special[:nq]):
        q[i] = s.astype(t)
    return q


FLOAT_KINDS = ("synthetic", "nonneg", "planted")


def float_inputs(oracle, seed, n, dim, dtype, nq, kind):
    """Wide Float32 / Float16 rows and f32 queries.  "synthetic": the generator's rows; "nonneg": their absolute values,
    the tail of each row at a quarter of its weight (every product has one sign: sums grow and a summation order's rounding
    shows, nothing cancels); "planted": synthetic
    rows, and every other query is a stored row plus noise of 1 % of its norm, so the head of its list is a clear winner."""
    rows = oracle.synth_rows(seed, 0, n, dim, dtype)
    q = oracle.synth_queries(seed + 1, nq, dim, dtype)
    if kind == "nonneg":
        np.abs(rows, out=rows)
        np.abs(q, out=q)
        # absolute values alone all point the same way (every cosine within 0.0015 of 0.75 at dimension 38656: a third of
        # the queries find several rows inside 2e-5 of their 10th best); a quarter-weight tail of a length that differs
        # from row to row spreads cosines over 0.6 .. 0.75 and distances and dot products likewise (x 0.25 is exact)
        cut = (dim * np.random.default_rng(seed).uniform(0.2, 1.0, n)).astype(np.int64)
        for r in range(n):
            rows[r, cut[r]:] *= rows.dtype.type(0.25)
    elif kind == "planted":
        rng = np.random.default_rng(seed)
        for qi in range(0, nq, 2):
            x = rows[int(rng.integers(0, n))].astype(np.float32)
            noise = rng.standard_normal(dim).astype(np.float32)
            noise *= np.float32(0.01 * np.linalg.norm(x.astype(np.float64)) / np.linalg.norm(noise.astype(np.float64)))
            q[qi] = x + noise
    else:
        assert kind == "synthetic"
    return rows, q


# The float cases of the GPU tier (group D of tests/test_gpu_wide_rows.py); test_wide_cpu.py holds each of them to the
# boundary-band condition without a GPU.  One corpus per case, every metric, the batches and k below on the one handle.
# Dimensions: both sides of the int8-shadow switch (8192 | 8200), of the f16-shadow / re-scoring switch (12288 | 12296) and
# of the exact f32 MFMA kernel's limit for final InnerProduct / Cosine keys (16384 | 16392), 20000, 33000, and the largest
# dimension K1 takes at the case's k (k1_max_dim).  The three kinds rotate over the dimensions (each type sees each kind on
# either side of a switch somewhere), non-negative rows -- the hard ones for a long f32 chain -- sit on both sides of the
# 16384 switch, and all three kinds run at the largest dimension.
FLOAT_BATCHES = (1, 3, 40, 130)
FLOAT_KS = (10, 100)
FLOAT_N = 3000
FLOAT_NQ = 130
FLOAT_POOL = 170   # queries generated per case; the first FLOAT_NQ of them with a thin boundary band are used


def thin_band_queries(ref, rows_f32, queries, ks, want=FLOAT_NQ):
    """Indices of the first `want` queries of the pool whose boundary band holds at most 10 % of k rows beside the k-th,
    for every metric and every k of the case -- decided from the float64 reference alone.  In thousands of dimensions the
    scores of random rows concentrate (L2 distances within ~1 % of each other, cosines within ~0.01), so at k = 10 about
    one query in ten finds a second row within 2e-5 of its 10th best; either order of those two is a correct answer, so
    such a query checks nothing at its boundary and the next query of the pool takes its place."""
    keep = []
    for qi in range(len(queries)):
        if all(band_count(m, ref[m][qi], rows_f32, queries[qi], k) <= k // 10 for m in (L2, IP, COS) for k in ks):
            keep.append(qi)
            if len(keep) == want:
                break
    return np.array(keep, np.int64)


def float_cases():
    """[(dtype, dim, kind, ks)]"""
    out = []
    for dtype in (F32, F16):
        dims = [8192, 8200, 12288, 12296, 20000, 33000]
        for i, dim in enumerate(dims):
            out.append((dtype, dim, FLOAT_KINDS[(i + dtype) % 3], FLOAT_KS))
        out += [(dtype, 16384, "nonneg", FLOAT_KS), (dtype, 16392, "nonneg", FLOAT_KS)]
        for kind in FLOAT_KINDS:
            out.append((dtype, k1_max_dim(dtype, max(FLOAT_KS)), kind, FLOAT_KS))
        out.append((dtype, k1_max_dim(dtype, 1000), "synthetic", (1000,)))   # the one k = 1000 case: its own, lower, limit
    return out


def float_case_seed(dtype, dim, kind):
    return 0x57494445 + 1000 * dtype + dim + 7 * FLOAT_KINDS.index(kind)
