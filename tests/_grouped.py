"""The grouped-search tests' numpy reference and layouts (DESIGN.md §3 "Grouped search"), and -- run as a program,
`python tests/_grouped.py <out.npz>` -- the scenario tests/test_gpu_grouped.py starts as a child process whose FIRST device work
it is.

The reference is the contract's walk: go through a query's ranked rows, take a row iff fewer than per_key rows of its key have
been taken, stop after k.  The layouts are tests/_partitioned.py's `layout` with other sizes: 8192 rows, every 10th dead, one
key wholly dead, the keys' rows scattered over all positions.

Imports numpy and the standard library only; as a child it keeps the binding from loading torch.
"""
import ctypes as C
import os
import sys

import numpy as np

import _partitioned as P

N = P.N
PAD = P.PAD
TILE, RANK_MAX, MAX_PER_KEY = 1024, 128, 64   # G1's tile, its counting tier's longest run, the largest cap
PER_KEYS = (1, 2, 3, 63, 64)

# (b) sizes around the caps and the wave, G1's counting tier's end and its tile, each +-1, and a few between the two so that
# some long run lies inside a tile whatever the keys' order
CAP_SIZES = (1, 2, 3, 4, 62, 63, 64, 65, 66, 127, 128, 129, 1023, 1024, 1025, 130, 200, 300, 500)
CAP_FURTHER = 40
# (c) one key holds most of the live rows, about 200 keys share the rest
DOMINANT_SIZES = (6500,)
DOMINANT_FURTHER = 200


def grouped_walk(ranked_local_rows, col, per_key, k):
    """-> the places in `ranked_local_rows` (a query's rows, best first) the grouped search takes: a row is taken iff fewer
    than per_key rows with its column value were taken in front of it; at most k."""
    r = np.asarray(ranked_local_rows, np.int64)
    if r.size == 0:
        return np.zeros(0, np.int64)
    keys = np.asarray(col)[r].astype(np.uint64)
    order = np.argsort(keys, kind="stable")          # key by key, ranked order inside a key
    ks = keys[order]
    head = np.ones(r.size, bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.maximum.accumulate(np.where(head, np.arange(r.size), 0))
    occ = np.empty(r.size, np.int64)
    occ[order] = np.arange(r.size) - start           # rows of the same key in front of each row
    return np.nonzero(occ < per_key)[0][:k]


def walk_by_dict(ranked_local_rows, col, per_key, k):
    """the same, as the contract words it"""
    taken, out = {}, []
    for place, r in enumerate(np.asarray(ranked_local_rows).tolist()):
        if len(out) == k:
            break
        key = int(col[r])
        if taken.get(key, 0) < per_key:
            taken[key] = taken.get(key, 0) + 1
            out.append(place)
    return np.array(out, np.int64)


def stock(flavour):
    return P.layout(flavour)


def caps(flavour):
    return P.layout(flavour, N, CAP_SIZES, CAP_FURTHER)


def dominant(flavour):
    return P.layout(flavour, N, DOMINANT_SIZES, DOMINANT_FURTHER)


def own_keys(flavour):
    """(d) every row its own key"""
    dead = np.zeros(N, bool)
    dead[::10] = True
    rng = np.random.default_rng(P._seed("own", flavour))
    col = rng.permutation(N).astype(P.NP_OF[flavour]) * P.NP_OF[flavour](3)
    if flavour == "u64":
        col = col | (np.uint64(1) << np.uint64(40))
    return dict(col=col, dead=dead)


def one_key(flavour):
    """(e) one key for all rows"""
    dead = np.zeros(N, bool)
    dead[::10] = True
    return dict(col=np.full(N, 77, P.NP_OF[flavour]), dead=dead)


def all_dead(flavour):
    """(f) all rows deleted"""
    return dict(col=(np.arange(N) % 50).astype(P.NP_OF[flavour]), dead=np.ones(N, bool))


def live_rows(lay):
    return np.nonzero(~lay["dead"])[0]


def runs(lay):
    """(length, crossing) of every run G1 sees: what each TILE-entry tile of the key-ordered list holds of each key"""
    _, counts = P.group_by(lay)
    ends = np.cumsum(counts.astype(np.int64))
    out = []
    for s, e in zip(ends - counts.astype(np.int64), ends):
        for t in range(s // TILE, (e - 1) // TILE + 1):
            lo, hi = max(s, t * TILE), min(e, (t + 1) * TILE)
            out.append((hi - lo, s // TILE != (e - 1) // TILE))
    return out


def run_tier(length, per_key, crossing):
    """the contract's tier of a run (include/mvf_gpu.h: mvfgpu_selftest_group_plan)"""
    if crossing:
        return 2
    if length <= per_key:
        return 0
    return 1 if length <= RANK_MAX else 2


def expected(ranked_scores, ranked_indices, ranked_raw, places, k, metric):
    """the result row from a query's full ranking and the walk's places, padded as a search pads"""
    s = np.full(k, np.inf if metric == 0 else -np.inf, np.float32)
    i = np.full(k, PAD, np.uint64)
    r = np.zeros(k, np.int32)
    s[:places.size], i[:places.size], r[:places.size] = ranked_scores[places], ranked_indices[places], ranked_raw[places]
    return s, i, r


# ---- the fresh-process scenario: Float32 8192 x 100, the stock layout, 5 queries, host call and device call
FP_DIM, FP_K, FP_PER_KEY, FP_METRIC, FP_NQ = 100, 100, 2, 2, 5


def fresh_inputs():
    return dict(lay=stock("u32"), rows=P.make_rows(N, FP_DIM, "f32"), queries=P.make_queries(FP_NQ, FP_DIM, "f32"))


def main(argv):
    if len(argv) != 2:
        print("usage: _grouped.py <out.npz>", file=sys.stderr)
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
            res = c.search_grouped(q, FP_K, FP_PER_KEY, FP_METRIC, part)   # the child's first search
            out["host.scores"], out["host.indices"], out["host.raw"] = res.scores, res.indices, res.raw
            out["host.keys"] = col.gather(res.indices)
            hip = P._hip_runtime()
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            nres = q.shape[0] * FP_K
            sizes = [q.nbytes, nres * 4, nres * 8, nres * 4]
            ptrs = [C.c_void_p() for _ in sizes]
            for p, size in zip(ptrs, sizes):
                P._check(hip.hipMalloc(C.byref(p), size), "hipMalloc")
            P._check(hip.hipMemcpy(ptrs[0], q.ctypes.data_as(C.c_void_p), q.nbytes, 1), "hipMemcpy H2D")
            c.search_grouped_device(part, ptrs[0].value, 0, q.shape[1], q.shape[0], FP_K, FP_PER_KEY, FP_METRIC, ptrs[1].value,
                                    ptrs[2].value, ptrs[3].value)
            P._check(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
            got = [np.empty((q.shape[0], FP_K), t) for t in (np.float32, np.uint64, np.int32)]
            for a, p in zip(got, ptrs[1:]):
                P._check(hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2), "hipMemcpy D2H")
            for p in ptrs:
                P._check(hip.hipFree(p), "hipFree")
            out["device.scores"], out["device.indices"], out["device.raw"] = got
    out["poison"] = np.array([G.selftest_poison()], np.int32)
    np.savez(argv[1], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
