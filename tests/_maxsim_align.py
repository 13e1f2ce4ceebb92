"""The MaxSim alignment tests' numpy references (DESIGN.md §3 "Alignments"), and -- run as a program,
`python tests/_maxsim_align.py <out.npz>` -- the scenario tests/test_gpu_maxsim_align.py starts as a child process whose FIRST
device work it is.

The reference is the contract's words: per (entry, token) the first row in the search's order -- smallest order key, ties by
ascending position, NaN last -- among the live rows that carry the entry's key, in list order; padding where no live row does.
It takes the row scores as given, so it states the SELECTION, not the arithmetic of a row score.  The plan's reference restates
the header's rule.

Imports numpy and the standard library only; as a child it keeps the binding from loading torch.
"""
import ctypes as C
import os
import sys

import numpy as np

import _maxsim as MS
import _maxsim_candidates as MC
import _partitioned as P

PAD = P.PAD
MIN_BYTES = 8   # a minimum of M0-arg: (order key << 32) | local row


def plan(n_keys, n_tokens, nq, token_bytes, budget):
    """the header's plan rule (mvfgpu_selftest_maxsim_align_plan), restated: maxsim_plan's chunk rules with chunk x n_keys x 8
    bytes per set of a window and nothing else"""
    in_lds = MS.CHUNK_MAX if token_bytes == 0 or token_bytes > MS.LDS_TOKEN_BYTES else MS.LDS_TOKEN_BYTES // token_bytes
    cap = min(n_tokens, MS.CHUNK_MAX, in_lds)
    least = min(cap, MS.TOKEN_GROUP)
    nk = max(n_keys, 1)
    chunk = min(max(budget // nk // MIN_BYTES, least), cap)
    return chunk, max(1, min(budget // (nk * chunk * MIN_BYTES), nq, MS.WINDOW_MAX))


def pad_outputs(nq, m, T, metric):
    return (np.full((nq, m, T), PAD, np.uint64), np.full((nq, m, T), np.inf if metric == 0 else -np.inf, np.float32),
            np.zeros((nq, m, T), np.int32))


def by_contract(row_scores, row_keys, row_names, keys, metric, row_raw=None):
    """One query set.  row_scores f32 [T, n]: token t's score of live row i, the rows in ascending position; row_keys [n] their
    column values; row_names [n] what a search reports for them (index_base + row, or the id); keys [m] the list.
    -> (rows u64 [m, T], scores f32 [m, T], raw i32 [m, T])"""
    T, n = row_scores.shape
    keys = np.asarray(keys, np.uint64).reshape(-1)
    rows, scores, raw = (a[0] for a in pad_outputs(1, keys.size, T, metric))
    okeys = MS.order_key(row_scores, metric)
    for i, key in enumerate(keys):
        mine = np.nonzero(np.asarray(row_keys, np.uint64) == key)[0]   # ascending position
        if mine.size == 0:
            continue
        for t in range(T):
            at = mine[np.argmin(okeys[t, mine])]   # argmin: the first of equal keys, the lowest position
            rows[i, t] = row_names[at]
            scores[i, t] = MS.score_of_key(okeys[t, at:at + 1], metric)[0]
            if row_raw is not None:
                raw[i, t] = row_raw[t, at]
    return rows, scores, raw


def token_sum(scores):
    """((s0 + s1) + ...) in plain f32 along the last axis, every NaN the library's: identity 2's left-hand side"""
    S = scores[..., 0].astype(np.float32)
    for t in range(1, scores.shape[-1]):
        S = (S + scores[..., t]).astype(np.float32)
    return MS.canonical(S)


def partitioned_pairs(sets, lists):
    """the nq * m * T one-query searches of identity 1 as ONE partitioned batch: (queries [nq m T, dim], keys [nq m T]), element
    (q, i, t) at ((q m) + i) T + t"""
    nq, T, dim = sets.shape
    lists = np.asarray(lists, np.uint64).reshape(nq, -1)
    m = lists.shape[1]
    queries = np.ascontiguousarray(np.broadcast_to(sets[:, None, :, :], (nq, m, T, dim))).reshape(nq * m * T, dim)
    return queries, np.repeat(lists.reshape(-1), T)


def varied_lists(held_keys, counts, m, skipped, seed):
    """[len(counts), m]: set q lists counts[q] distinct held keys, a repeat of one of them where there is room, then `skipped`
    entries, shuffled"""
    rng = np.random.default_rng(P._seed("align lists", seed, tuple(counts), m))
    held_keys, skipped = np.asarray(held_keys, np.uint64), np.asarray(skipped, np.uint64)
    out = np.empty((len(counts), m), np.uint64)
    for q, n in enumerate(counts):
        mine = rng.choice(held_keys, n, replace=False)
        rest = m - n
        extra = np.concatenate([mine[:1].repeat(min(rest, 1)), rng.choice(skipped, max(rest - 1, 0))]) if n else rng.choice(skipped, rest)
        out[q] = rng.permutation(np.concatenate([mine, extra]))
    return out


# ---- the fresh-process scenario: tests/_maxsim_candidates.py's inputs -- Float32 8192 x 100, the stock layout, 3 sets of 5 tokens,
# lists of 40 -- through the host call and the device call
FP_DIM, FP_METRIC, FP_NQ, FP_T, FP_M = MC.FP_DIM, MC.FP_METRIC, MC.FP_NQ, MC.FP_T, MC.FP_M


def main(argv):
    if len(argv) != 2:
        print("usage: _maxsim_align.py <out.npz>", file=sys.stderr)
        return 2
    sys.modules.setdefault("torch", None)  # the binding would load torch's HIP runtime first where torch is installed
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from metrovector_amd import gpu as G
    inp = MC.fresh_inputs()
    lay, q, lists = inp["lay"], inp["queries"], inp["lists"]
    out = {}
    with G.GpuCorpus.from_array(inp["rows"]) as c:
        c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        with c.attach_column(lay["col"]) as col, c.make_partition(col) as part:
            res = c.maxsim_align(q, lists, FP_METRIC, part)   # the child's first search
            out["host.rows"], out["host.scores"], out["host.raw"] = res.rows, res.scores, res.raw
            hip = P._hip_runtime()
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            n = FP_NQ * FP_M * FP_T
            sizes = [q.nbytes, n * 4, n * 8, n * 4]
            ptrs = [C.c_void_p() for _ in sizes]
            for p, size in zip(ptrs, sizes):
                P._check(hip.hipMalloc(C.byref(p), size), "hipMalloc")
            P._check(hip.hipMemcpy(ptrs[0], q.ctypes.data_as(C.c_void_p), q.nbytes, 1), "hipMemcpy H2D")
            c.maxsim_align_device(part, ptrs[0].value, 0, FP_DIM, FP_NQ, FP_T, lists, FP_METRIC, ptrs[1].value, ptrs[2].value, ptrs[3].value)
            P._check(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
            got = [np.empty((FP_NQ, FP_M, FP_T), t) for t in (np.float32, np.uint64, np.int32)]
            for a, p in zip(got, ptrs[1:]):
                P._check(hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2), "hipMemcpy D2H")
            for p in ptrs:
                P._check(hip.hipFree(p), "hipFree")
            out["device.scores"], out["device.rows"], out["device.raw"] = got
    out["poison"] = np.array([G.selftest_poison()], np.int32)
    np.savez(argv[1], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
