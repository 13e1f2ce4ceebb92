"""The candidate multi-vector search tests' numpy references (DESIGN.md §3 "Candidate keys"), and -- run as a program,
`python tests/_maxsim_candidates.py <out.npz>` -- the scenario tests/test_gpu_maxsim_candidates.py starts as a child process
whose FIRST device work it is.

The reference of identity 1 is a filter: the full search's row at k = n_keys with every entry whose key is no candidate of the
set removed, cut at k and padded.  The plan's reference restates the slot rule: of the held entries the first occurrence of
every key, ranked by ascending key value.

Imports numpy and the standard library only; as a child it keeps the binding from loading torch.
"""
import ctypes as C
import os
import sys

import numpy as np

import _maxsim as MS
import _partitioned as P

PAD = P.PAD
SKIPPED = np.uint32(0xFFFFFFFF)
BLOCK = 128   # list positions of one block of M0: every set's rows are padded to a multiple


def held_distinct(cand, held_keys):
    """the distinct candidates of one list the partition holds, ascending (uint64)"""
    return np.intersect1d(np.asarray(cand, np.uint64).reshape(-1), np.asarray(held_keys, np.uint64))


def filter_full(full_scores, full_keys, n_keys, cand_lists, held_keys, k, metric):
    """identity 1.  full_*: [nq, >= n_keys], the full search at k >= n_keys (only the first n_keys entries are keys: a real key
    UINT64_MAX is told from padding by its place); cand_lists [nq, m].  -> (scores [nq, k], keys [nq, k], counts [nq])"""
    nq = full_scores.shape[0]
    sc, ky = MS.pad_rows(nq, k, metric)
    counts = np.zeros(nq, np.uint32)
    for q in range(nq):
        keep = np.isin(full_keys[q, :n_keys], held_distinct(cand_lists[q], held_keys))
        s, g = full_scores[q, :n_keys][keep][:k], full_keys[q, :n_keys][keep][:k]
        sc[q, :s.size], ky[q, :g.size], counts[q] = s, g, s.size
    return sc, ky, counts


def plan_reference(cand, held):
    """(slot [m] uint32, distinct, rows) of one list from every entry's held row count: the contract's words"""
    cand, held = np.asarray(cand, np.uint64).reshape(-1), np.asarray(held, np.uint64).reshape(-1)
    first = {}
    for i in range(cand.size):
        if held[i] and int(cand[i]) not in first:
            first[int(cand[i])] = i
    slot = np.full(cand.size, SKIPPED, np.uint32)
    for rank, key in enumerate(sorted(first)):
        slot[first[key]] = rank
    return slot, len(first), int(sum(int(held[i]) for i in first.values()))


def mixed_lists(held_keys, nq, m, skipped, seed):
    """[nq, m] lists, a different one with a different number of held candidates per set: set q draws about m / (q + 1) held
    keys (at most all), then repeats of them, then entries of `skipped` (unknown / dead keys, pads), shuffled"""
    rng = np.random.default_rng(P._seed("cand lists", seed, nq, m))
    held_keys = np.asarray(held_keys, np.uint64)
    out = np.empty((nq, m), np.uint64)
    for q in range(nq):
        want = max(1, min(held_keys.size, m // (q + 1) - q))
        mine = rng.choice(held_keys, want, replace=False)
        rest = m - want
        extra = np.concatenate([rng.choice(mine, rest // 2), rng.choice(np.asarray(skipped, np.uint64), rest - rest // 2)]) if rest else mine[:0]
        out[q] = rng.permutation(np.concatenate([mine, extra]))
    return out


def rows_ending_at(keys, counts, target, rng):
    """a subset of `keys` whose row counts add up to exactly `target`, or None: greedy from a shuffled order, then one key that
    closes the gap"""
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.int64)
    for _ in range(200):
        order = rng.permutation(keys.size)
        total, pick = 0, []
        for i in order:
            if total + counts[i] <= target:
                total += int(counts[i])
                pick.append(i)
            if total == target:
                return keys[np.array(pick)]
    return None


# ---- the fresh-process scenario: Float32 8192 x 100, the stock layout, 3 sets of 5 tokens, host call and device call
FP_DIM, FP_K, FP_METRIC, FP_NQ, FP_T, FP_M = 100, 10, 2, 3, 5, 40


def fresh_inputs():
    import _grouped as GR
    lay = GR.stock("u32")
    held = P.group_by(lay)[0]
    lists = mixed_lists(held, FP_NQ, FP_M, [lay["absent_key"], lay["dead_key"], int(PAD)], "fresh")
    return dict(lay=lay, rows=P.make_rows(P.N, FP_DIM, "f32"), queries=MS.make_sets(FP_NQ, FP_T, FP_DIM, "f32"), lists=lists)


def main(argv):
    if len(argv) != 2:
        print("usage: _maxsim_candidates.py <out.npz>", file=sys.stderr)
        return 2
    sys.modules.setdefault("torch", None)  # the binding would load torch's HIP runtime first where torch is installed
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from metrovector_amd import gpu as G
    inp = fresh_inputs()
    lay, q, lists = inp["lay"], inp["queries"], inp["lists"]
    out = {}
    with G.GpuCorpus.from_array(inp["rows"]) as c:
        c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        with c.attach_column(lay["col"]) as col, c.make_partition(col) as part:
            res = c.search_maxsim_candidates(q, lists, FP_K, FP_METRIC, part)   # the child's first search
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
            c.search_maxsim_candidates_device(part, ptrs[0].value, 0, FP_DIM, FP_NQ, FP_T, lists, FP_K, FP_METRIC, ptrs[1].value,
                                              ptrs[2].value, ptrs[3].value)
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
