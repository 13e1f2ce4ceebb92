"""The multi-vector search tests' numpy references (DESIGN.md §3 "Multi-vector search"), and -- run as a program,
`python tests/_maxsim.py <out.npz>` -- the scenario tests/test_gpu_maxsim.py starts as a child process whose FIRST device work
it is.

The reference is the contract written out with dicts: per token, the best row score of every key in the search's order (best
first, NaN last, -0.0 == +0.0), reconstructed from its order key; the sum over tokens in f32, in token order; the keys ranked by
(order key of the sum, key value); padding.  It takes the row scores as given -- the library's (the identity tests) or float64
ones rounded to f32 (the CPU tests) -- so it states the SELECTION and the SUM, not the arithmetic of a row score.

Behind it, for the tests of the scoring kernel's forms (DESIGN.md §5 "M0 / M1"; tests/test_gpu_maxsim_forms.py): the table of
(type, dimension) cases with the cell each holds, and two references that DO state a row score's arithmetic, independent of
every kernel -- float64 sums with §3's tolerance per token, and exact integers for Int8 / UInt8 rows --, the saturated integer
world and two wrong kernels as models.

Imports numpy and the standard library only; as a child it keeps the binding from loading torch.
"""
import ctypes as C
import os
import sys

import numpy as np

import _partitioned as P

PAD = P.PAD
NAN_BITS = np.uint32(0x7FC00000)   # the NaN every result carries
NAN_KEY = np.uint32(0xFFFFFFFF)
MAX_TOKENS, CHUNK_MAX, TOKEN_GROUP, LDS_TOKEN_BYTES, KEY_BYTES, WINDOW_MAX = 1024, 32, 4, 40 * 1024, 20, 1024


def order_key(scores, metric):
    """the library's u32 order key of f32 scores (mvf_common.h: key_from_score): ascending = best first, NaN = 0xFFFFFFFF"""
    s = np.asarray(scores, np.float32)
    x = (s if metric == 0 else -s) + np.float32(0.0)
    b = x.view(np.uint32)
    k = np.where(b >> np.uint32(31), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(s), NAN_KEY, k)


def score_of_key(keys, metric):
    """the score a result reports for an order key (score_from_key): +0.0 for +-0.0, one NaN"""
    k = np.asarray(keys, np.uint32)
    b = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    s = b.view(np.float32)
    s = s if metric == 0 else -s + np.float32(0.0)
    return np.where(k == NAN_KEY, NAN_BITS.view(np.float32), s).astype(np.float32)


def canonical(scores):
    """f32 scores with every NaN the library's"""
    s = np.array(scores, np.float32)
    s[np.isnan(s)] = NAN_BITS.view(np.float32)
    return s


def pad_rows(nq, k, metric):
    return np.full((nq, k), np.inf if metric == 0 else -np.inf, np.float32), np.full((nq, k), PAD, np.uint64)


def by_dict(row_scores, row_keys, metric, k, best="min_key", total="f32", tie="ascending"):
    """One query set.  row_scores f32 [T, m]: token t's score of held row i; row_keys [m]: the rows' column values.
    -> (scores f32 [k], keys u64 [k], count).  best / total / tie select the contract's rule or one of the wrong models the
    CPU tests must tell from it: best "nan_first" (a max that prefers NaN), total "f64" (the sum in float64, rounded once),
    tie "descending" (equal sums by descending key)."""
    T, m = row_scores.shape
    okeys = order_key(row_scores, metric)
    sums = {}
    for t in range(T):
        bests = {}
        for i in range(m):
            g, key = int(row_keys[i]), int(okeys[t, i])
            if best == "nan_first":
                key = -1 if key == int(NAN_KEY) else key
            if g not in bests or key < bests[g]:
                bests[g] = key
        for g, key in bests.items():
            b = score_of_key(np.array([NAN_KEY if key < 0 else key], np.uint32), metric)[0]
            if total == "f64":
                sums[g] = float(b) if t == 0 else sums[g] + float(b)
            else:
                sums[g] = b if t == 0 else np.float32(sums[g] + b)
    entries = [(int(order_key(np.float32(S), metric)), g if tie == "ascending" else -g, np.float32(S), g) for g, S in sums.items()]
    entries.sort(key=lambda e: e[:2])
    sc, ky = pad_rows(1, k, metric)
    for i, e in enumerate(entries[:k]):
        sc[0, i], ky[0, i] = e[2], e[3]
    return canonical(sc[0]), ky[0], min(k, len(entries))


def vectorised(row_scores, row_keys, metric, k):
    """by_dict's contract rule without the loops"""
    T, m = row_scores.shape
    sc, ky = pad_rows(1, k, metric)
    if m == 0:
        return sc[0], ky[0], 0
    order = np.argsort(np.asarray(row_keys, np.uint64), kind="stable")
    ks = np.asarray(row_keys, np.uint64)[order]
    starts = np.nonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))[0]
    best = np.minimum.reduceat(order_key(row_scores, metric)[:, order], starts, axis=1)   # [T, n_keys]
    return rank_keys(score_of_key(best, metric), ks[starts], metric, k)


def rank_keys(per_token_best, key_values, metric, k):
    """(scores, keys, count) from b(t, g) f32 [T, n_keys] and the keys' values: the f32 sum in token order, the ranking, padding"""
    S = per_token_best[0].astype(np.float32)
    for t in range(1, per_token_best.shape[0]):
        S = (S + per_token_best[t]).astype(np.float32)
    S = canonical(S)
    order = np.lexsort((np.asarray(key_values, np.uint64), order_key(S, metric)))[:k]
    sc, ky = pad_rows(1, k, metric)
    sc[0, :order.size], ky[0, :order.size] = S[order], np.asarray(key_values, np.uint64)[order]
    return sc[0], ky[0], int(order.size)


def plan(n_keys, n_tokens, nq, token_bytes, budget):
    """the header's plan rule (mvfgpu_selftest_maxsim_plan), restated"""
    in_lds = CHUNK_MAX if token_bytes == 0 or token_bytes > LDS_TOKEN_BYTES else LDS_TOKEN_BYTES // token_bytes
    cap = min(n_tokens, CHUNK_MAX, in_lds)
    least = min(cap, TOKEN_GROUP)
    per_key = budget // max(n_keys, 1)
    fit = (per_key - KEY_BYTES) // 4 if per_key > KEY_BYTES else 0
    chunk = min(max(fit, least), cap)
    per_set = max(n_keys, 1) * (chunk * 4 + KEY_BYTES)
    return chunk, max(1, min(budget // per_set, nq, WINDOW_MAX))


def make_sets(nq, n_tokens, dim, dt):
    return P.make_queries(nq * n_tokens, dim, dt).reshape(nq, n_tokens, dim)


# ---- the scoring kernel's forms (DESIGN.md §5 "M0 / M1"; tests/test_gpu_maxsim_forms.py, tests/test_maxsim_cpu.py)
DTYPE = {"f32": 0, "f16": 1, "i8": 2, "u8": 3}
REG, REREAD, CACHE = 0, 1, 2
REG_STEPS = 4      # kMaxsimRegSteps: rows of up to this many steps per lane stay in registers
FORM_LAYOUT = (300, 129, 128, 127, 64, 2, 1), 20   # P.layout's sizes and further keys, on 2048 or 1024 rows

# (type, dimension) -> the cell it holds: (lanes per row G, steps per lane J, form), worked out by hand from the rules of
# choose_group (api.hip) and maxsim_form (scan_maxsim.h); mvfgpu_selftest_maxsim_form is the authority the tests hold it to.
FORM_CELLS = {
    ("f32", 3): (1, 1, REG), ("f32", 16): (4, 1, REG), ("f32", 32): (8, 1, REG), ("f32", 64): (16, 1, REG), ("f32", 100): (32, 1, REG),
    ("f32", 128): (16, 2, REG), ("f32", 256): (16, 4, REG), ("f32", 288): (16, 5, REREAD), ("f32", 384): (16, 6, REREAD),
    ("f32", 736): (16, 12, REREAD), ("f32", 1024): (64, 4, REG), ("f32", 1028): (64, 5, REREAD), ("f32", 10240): (64, 40, REREAD),
    ("f32", 10241): (64, 41, CACHE),
    ("f16", 8): (1, 1, REG), ("f16", 20): (4, 1, REG), ("f16", 64): (8, 1, REG), ("f16", 128): (16, 1, REG), ("f16", 200): (32, 1, REG),
    ("f16", 512): (16, 4, REG), ("f16", 768): (16, 6, REREAD), ("f16", 1024): (16, 8, REREAD), ("f16", 2048): (64, 4, REG),
    ("f16", 2056): (64, 5, REREAD), ("f16", 10240): (64, 20, REREAD), ("f16", 10248): (64, 21, CACHE),
    ("i8", 16): (1, 1, REG), ("i8", 64): (4, 1, REG), ("i8", 128): (8, 1, REG), ("i8", 400): (32, 1, REG), ("i8", 768): (16, 3, REG),
    ("i8", 1000): (64, 1, REG), ("i8", 1536): (16, 6, REREAD), ("i8", 4096): (64, 4, REG), ("i8", 4112): (64, 5, REREAD),
    ("i8", 33025): (64, 33, REREAD),
    ("u8", 5): (1, 1, REG), ("u8", 64): (4, 1, REG), ("u8", 100): (8, 1, REG), ("u8", 256): (16, 1, REG), ("u8", 300): (32, 1, REG),
    ("u8", 1024): (16, 4, REG), ("u8", 2048): (16, 8, REREAD), ("u8", 3000): (64, 3, REG), ("u8", 33025): (64, 33, REREAD),
}
FORM_CASES = list(FORM_CELLS)
# the three switches, (type, last dimension on the near side, first on the far side): J 4 -> 5 at 16 lanes, at 64 lanes, LDS -> cache
FORM_SWITCHES = {"reg to reread, G 16": [("f32", 256, 288)],
                 "reg to reread, G 64": [("f32", 1024, 1028), ("f16", 2048, 2056), ("i8", 4096, 4112)],
                 "LDS to cache": [("f32", 10240, 10241), ("f16", 10240, 10248)]}
FORCED_WIDTHS = (1, 4, 8, 16, 32, 64)
FORCED_SHAPES = [("f32", 200), ("f16", 400), ("i8", 800)]   # V = 50 vectors of 16 bytes


def form_rows(dim):
    """rows of a form case's world: 2048; 1024 for the widest rows (the layout keeps a key across a 128-position block edge)"""
    return 1024 if dim >= 10240 else 2048


def form_layout(n):
    return P.layout("u32", n, *FORM_LAYOUT)


def key_order(lay):
    """(live rows in the index's order -- ascending key value, then position --, their keys, the first list position of every
    key, the keys' values)"""
    live = np.nonzero(~lay["dead"])[0]
    keys = lay["col"][live].astype(np.uint64)
    order = np.argsort(keys, kind="stable")
    live, keys = live[order], keys[order]
    starts = np.nonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))[0]
    return live, keys, starts, keys[starts]


def spans_block_edge(lay, block=128):
    """a key's rows lie on both sides of a multiple of `block` list positions"""
    _, keys, starts, _ = key_order(lay)
    ends = np.concatenate([starts[1:], [keys.size]])
    return bool(((starts // block) != ((ends - 1) // block)).any())


def token_pool(dt, dim, nq=3, T=33):
    """[nq, T, dim]: the query sets of a form case are its leading [:nq, :T], so one reference serves every (nq, T)"""
    return P.make_queries(nq * T, dim, dt).reshape(nq, T, dim)


# -- floats: the float64 contract (DESIGN.md §3 "Tolerance")
def f64_key_bests(rows, lay, tokens, tol_unit):
    """{metric: (b [T, n_keys] float64 -- token t's best score among key g's live rows --, tol [T, n_keys]: §3's tolerance of
    that row score: tol_unit relative under L2, absolute under Cosine, x |q| max|x| of the key under InnerProduct)},
    independent of every kernel"""
    import _wide as W
    live, _, starts, _ = key_order(lay)
    x = rows[live]
    all64 = W.f64_scores_all(x, tokens)
    xn = np.sqrt(np.einsum("ij,ij->i", x.astype(np.float64), x.astype(np.float64)))
    qn = np.linalg.norm(tokens.astype(np.float64), axis=1)
    out = {}
    for metric in (0, 1, 2):
        sign = 1.0 if metric == 0 else -1.0
        b = sign * np.minimum.reduceat(sign * all64[metric], starts, axis=1)
        if metric == 0:
            tol = tol_unit * np.abs(b)
        elif metric == 2:
            tol = np.full(b.shape, tol_unit)
        else:
            tol = tol_unit * np.maximum.reduceat(xn, starts)[None, :] * qn[:, None]
        out[metric] = (b, tol)
    return out


def assert_f64_contract(scores, keys, key_values, S, tol, metric, k):
    """One result row against float64 sums S [n_keys] with their tolerances tol [n_keys] (each the sum over the tokens of a row
    score's): k distinct keys of the partition, every returned sum within its tolerance, the list in (order key, key value)
    order, and the set of keys right up to sums within two such tolerances of the k-th -- boundary ties only at the k-th rank."""
    at = np.searchsorted(key_values, keys)
    assert (key_values[at] == keys).all() and np.unique(at).size == k, "k distinct keys of the partition"
    assert (np.abs(scores.astype(np.float64) - S[at]) <= tol[at]).all(), f"k {k}: a sum outside its tolerance"
    okey = order_key(scores, metric).astype(np.int64)
    assert ((okey[1:] > okey[:-1]) | ((okey[1:] == okey[:-1]) & (keys[1:] > keys[:-1]))).all(), "order"
    key = (1.0 if metric == 0 else -1.0) * S
    kth, band = np.partition(key, k - 1)[k - 1], 2 * tol.max()
    assert set(np.nonzero(key < kth - band)[0].tolist()) <= set(at.tolist()), "a clear winner is missing"
    assert set(at.tolist()) <= set(np.nonzero(key <= kth + band)[0].tolist()), "a clear loser was returned"


def f64_fraction(scores, keys, key_values, S, tol):
    """the largest |returned sum - float64 sum| of a result row in units of its tolerance"""
    at = np.searchsorted(key_values, keys)
    return float(np.max(np.abs(scores.astype(np.float64) - S[at]) / tol[at]))


# -- Int8 / UInt8: exact
def int_raw(rows, lay, tokens):
    """the exact integers of every (token, live row): W.int_raw's (dot, qq, xx) over the live rows in the index's order"""
    import _wide as W
    return W.int_raw(rows[key_order(lay)[0]], tokens)


def int_row_scores(rows, lay, tokens, metric, raw=None):
    """(f32 scores [T, live] of the live rows in the index's order, their exact raw integers, their keys): W.int_raw ->
    W.int_scores; raw: int_raw's result where a caller keeps it over the metrics"""
    import _wide as W
    sc, _, r = W.int_scores(metric, *(int_raw(rows, lay, tokens) if raw is None else raw))
    return sc, r, key_order(lay)[1]


def rank_sets(scores, keys, nq, T, metric, k, stride=None):
    """(scores [nq, k], keys [nq, k], counts [nq]): `vectorised` over set j's token rows scores[j * stride : j * stride + T]"""
    stride = T if stride is None else stride
    res = [vectorised(scores[j * stride:j * stride + T], keys, metric, k) for j in range(nq)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.uint32)


def int_reference(rows, lay, sets, metric, k):
    """(scores [nq, k], keys [nq, k], counts [nq]) of search_maxsim over Int8 / UInt8 rows, exact: every byte must match"""
    nq, T, dim = sets.shape
    sc, _, keys = int_row_scores(rows, lay, sets.reshape(nq * T, dim), metric)
    return rank_sets(sc, keys, nq, T, metric, k)


# -- saturated integer rows: sums next to 2^31 (tests/_wide.py's saturated_rows, on this file's layout)
INT_RANGE = {"i8": (-128, 127), "u8": (0, 255)}
SAT_OWN_KEY0, SAT_TIE_KEY = 0x70000000, 0x70000100   # the planted rows' keys: values the layout does not draw


def saturated_positions(n):
    """13 live positions (none a multiple of 10): the first rows, both sides of 128, 256 and the middle, the tail"""
    pos = [1, 2, 127, 128, 129, 255, 257, n // 2 - 1, n // 2 + 1, n - 1, n - 2, n - 3, n - 5]
    assert len(set(pos)) == len(pos) and all(p % 10 for p in pos)
    return pos


def saturated_world(dt, dim, n=None):
    """-> (rows [n, dim], layout, planted positions).  Random rows with saturated ones planted.  Planted rows 0..9 carry a key of
    their own each -- their score is that key's best whatever the metric --: all-min, all-max, alternating min / max, all-max with
    one element at min, then six all-max rows with one to three elements lowered by one, the second of them equal to the first
    (two keys with equal rows: bit-equal sums).  Planted rows 10..12 share one further key: two equal near-max rows and a third
    (a tie inside a key)."""
    n = form_rows(dim) if n is None else n
    lo, hi = INT_RANGE[dt]
    lay = form_layout(n)
    rows = P.make_rows(n, dim, dt)
    pos = saturated_positions(n)
    assert not lay["dead"][pos].any()
    t = rows.dtype.type
    rows[pos[0]] = t(lo)
    rows[pos[1]] = t(hi)
    rows[pos[2], 0::2] = t(lo)
    rows[pos[2], 1::2] = t(hi)
    rows[pos[3]] = t(hi)
    rows[pos[3], dim // 2] = t(lo)
    rng = np.random.default_rng(P._seed("saturated", dt, dim, n))
    for i, p in enumerate(pos[4:]):
        rows[p] = t(hi)
        if i in (1, 7):                  # the same row as the one before it, elsewhere
            rows[p] = rows[pos[4 + i - 1]]
            continue
        for j in rng.choice(dim, 1 + i % 3, replace=False):
            rows[p, j] = t(hi - 1)
    col = lay["col"].copy()
    own = [SAT_OWN_KEY0 + i for i in range(10)]
    assert not np.isin(col, np.array(own + [SAT_TIE_KEY], col.dtype)).any()
    col[pos[:10]] = np.array(own, col.dtype)
    col[pos[10:]] = SAT_TIE_KEY
    return rows, dict(lay, col=col), pos


def saturated_sets(dt, dim, nq=2, T=5):
    """[nq, T, dim]: tests/_wide.py saturated_queries' four special tokens -- all-min, all-max, alternating, all-zero -- among
    random ones, at other places in every set"""
    lo, hi = INT_RANGE[dt]
    sets = make_sets(nq, T, dim, dt)
    special = [np.full(dim, lo), np.full(dim, hi), np.where(np.arange(dim) % 2 == 0, lo, hi), np.zeros(dim, np.int64)]
    assert T > len(special)
    for j in range(nq):
        for i, s in enumerate(special):
            sets[j, (i + j) % T if j % 2 == 0 else T - 1 - i] = s.astype(sets.dtype)
    return sets


# -- two wrong kernels the exact reference must tell from the right one
def model_drops_last_step(rows, tokens, G, J, elems_per_vector=16):
    """(rows, tokens) as a kernel sees them that never runs the row's last step j = J - 1: the vectors (J - 1) G .. are zero"""
    cut = (J - 1) * G * elems_per_vector
    r, q = rows.copy(), tokens.copy()
    r[:, cut:], q[:, cut:] = 0, 0
    return r, q


def model_swaps_row_pairs(n_live, G, block=128):
    """the list position whose score a kernel attributes to position i when it takes row u of a step for row u ^ 1: rows of a
    step are neighbouring groups of 64 / G positions of the block; a partner behind the list's end leaves the position its own"""
    rpg = 64 // G
    i = np.arange(n_live)
    inb, b0 = i % block, i - i % block
    partner = b0 + ((inb // rpg) ^ 1) * rpg + inb % rpg
    return np.where(partner < n_live, partner, i)


# ---- the fresh-process scenario: Float32 8192 x 100, the stock layout, 3 sets of 5 tokens, host call and device call
FP_DIM, FP_K, FP_METRIC, FP_NQ, FP_T = 100, 10, 2, 3, 5


def fresh_inputs():
    import _grouped as GR
    return dict(lay=GR.stock("u32"), rows=P.make_rows(P.N, FP_DIM, "f32"), queries=make_sets(FP_NQ, FP_T, FP_DIM, "f32"))


def main(argv):
    if len(argv) != 2:
        print("usage: _maxsim.py <out.npz>", file=sys.stderr)
        return 2
    sys.modules.setdefault("torch", None)  # the binding would load torch's HIP runtime first where torch is installed
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from metrovector_amd import gpu as G
    inp = fresh_inputs()
    lay, q = inp["lay"], inp["queries"]
    out = {}
    with G.GpuCorpus.from_array(inp["rows"]) as c:
        c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        with c.attach_column(lay["col"]) as col, c.make_partition(col) as part:
            res = c.search_maxsim(q, FP_K, FP_METRIC, part)   # the child's first search
            out["host.scores"], out["host.keys"], out["host.counts"] = res.scores, res.keys, res.counts
            hip = P._hip_runtime()
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            nres = FP_NQ * FP_K
            sizes = [q.nbytes, nres * 4, nres * 8, FP_NQ * 4]
            ptrs = [C.c_void_p() for _ in sizes]
            for p, size in zip(ptrs, sizes):
                P._check(hip.hipMalloc(C.byref(p), size), "hipMalloc")
            P._check(hip.hipMemcpy(ptrs[0], q.ctypes.data_as(C.c_void_p), q.nbytes, 1), "hipMemcpy H2D")
            c.search_maxsim_device(part, ptrs[0].value, 0, FP_DIM, FP_NQ, FP_T, FP_K, FP_METRIC, ptrs[1].value, ptrs[2].value, ptrs[3].value)
            P._check(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
            got = [np.empty((FP_NQ, FP_K), np.float32), np.empty((FP_NQ, FP_K), np.uint64), np.empty(FP_NQ, np.uint32)]
            for a, p in zip(got, ptrs[1:]):
                P._check(hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2), "hipMemcpy D2H")
            for p in ptrs:
                P._check(hip.hipFree(p), "hipFree")
            out["device.scores"], out["device.keys"], out["device.counts"] = got
    out["poison"] = np.array([G.selftest_poison()], np.int32)
    np.savez(argv[1], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
