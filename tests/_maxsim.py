"""The multi-vector search tests' numpy references (DESIGN.md §3 "Multi-vector search"), and -- run as a program,
`python tests/_maxsim.py <out.npz>` -- the scenario tests/test_gpu_maxsim.py starts as a child process whose FIRST device work
it is.

The reference is the contract written out with dicts: per token, the best row score of every key in the search's order (best
first, NaN last, -0.0 == +0.0), reconstructed from its order key; the sum over tokens in f32, in token order; the keys ranked by
(order key of the sum, key value); padding.  It takes the row scores as given -- the library's (the identity tests) or float64
ones rounded to f32 (the CPU tests) -- so it states the SELECTION and the SUM, not the arithmetic of a row score.

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
