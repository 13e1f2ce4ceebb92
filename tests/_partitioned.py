"""The layout of the partitioned-search tests (DESIGN.md §3 "Partitioned search") and its numpy reference, and -- run as a
program, `python tests/_partitioned.py <out.npz>` -- the scenario tests/test_gpu_partitioned.py starts as a child process whose
FIRST device work it is.

8192 rows.  Dead: every 10th position, among them ALL rows of one key.  Live partition sizes 3000, 1025, 1024, 1023, 300, 64,
2, 1, 1 and the remaining live rows spread over 60 further keys; positions are assigned to keys by a seeded permutation, so
every partition is scattered over the whole position range.  The reference of a query is the rows with col == key that are
live, in ascending position.

Imports numpy and the standard library only; as a child it keeps the binding from loading torch and reaches the device
through the HIP runtime the library itself is bound to.
"""
import ctypes as C
import hashlib
import os
import sys
import zlib

import numpy as np

N = 8192
LIVE_SIZES = (3000, 1025, 1024, 1023, 300, 64, 2, 1, 1)
FURTHER = 60
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)

# the values of the sized partitions, in LIVE_SIZES' order, then values further keys must include
SPECIAL = {
    "u32": [0xFFFFFFFF, 0, 0xFFFFFFFE, 7, 70000, 1 << 24, 65535, 65536, 3],
    "u64": [(1 << 64) - 1, 0, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63,
            (5 << 32) | 77, (6 << 32) | 77,     # equal in the low half only
            (9 << 32) | 1, (9 << 32) | 2],      # equal in the high half only
}
DEAD_KEY = {"u32": 123456, "u64": (5 << 32) | 123456}     # every row of it is deleted
ABSENT_KEY = {"u32": 424242, "u64": (5 << 32) | 78}       # no row carries it
NP_OF = {"u32": np.uint32, "u64": np.uint64}


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def layout(flavour, n=N, sizes=LIVE_SIZES, further=FURTHER):
    """-> dict(col [n] of the flavour's type, dead bool[n], keys: the sized partitions' values in `sizes` order,
    all_keys: every value with a live row, dead_key, absent_key)"""
    rng = np.random.default_rng(_seed("layout", flavour, n, sizes, further))
    dead = np.zeros(n, bool)
    dead[::10] = True
    live_pos = rng.permutation(np.nonzero(~dead)[0])
    assert sum(sizes) + further <= live_pos.size
    values = list(SPECIAL[flavour])
    taken = set(values) | {DEAD_KEY[flavour], ABSENT_KEY[flavour]}
    hi = 1 << (32 if flavour == "u32" else 64)
    while len(values) < len(sizes) + further:
        v = int(rng.integers(0, 1 << 20)) if len(values) % 2 else int(rng.integers(0, hi, dtype=np.uint64))
        if v not in taken:
            values.append(v), taken.add(v)
    col = np.zeros(n, NP_OF[flavour])
    at = 0
    for v, size in zip(values, sizes):
        col[live_pos[at:at + size]] = v
        at += size
    for v, chunk in zip(values[len(sizes):], np.array_split(live_pos[at:], further)):
        col[chunk] = v
    dead_pos = np.nonzero(dead)[0]
    col[dead_pos[::2]] = DEAD_KEY[flavour]                                   # all of its rows are dead
    col[dead_pos[1::2]] = rng.choice(np.array(values, NP_OF[flavour]), dead_pos[1::2].size)  # dead rows inside live partitions
    return dict(col=col, dead=dead, keys=values[:len(sizes)], all_keys=values, dead_key=DEAD_KEY[flavour],
                absent_key=ABSENT_KEY[flavour])


def reference_rows(lay, key):
    """the local rows a query with `key` is answered from: ascending"""
    return np.nonzero((lay["col"].astype(np.uint64) == np.uint64(key)) & ~lay["dead"])[0]


def group_by(lay):
    """(distinct keys of the live rows ascending, their counts) as uint64"""
    k, c = np.unique(lay["col"][~lay["dead"]].astype(np.uint64), return_counts=True)
    return k, c.astype(np.uint64)


# ---- layouts whose pair sort covers many tiles (scan_partition.h: kPartSortTile = 2048 pairs per block)
WIDE_N, WIDE_KEYS, SORT_TILE = 40_000, 300, 2048
WIDE_MID = 0x00A5C30F5A3C9600  # bits 8..55 of every key of "u64_two_digits"
WIDE_KINDS = ("u64_two_digits", "u32_random", "one_key", "distinct")


def wide_layout(kind, n=WIDE_N, live=None):
    """-> dict(col, dead, big: the key that holds most live rows or None).  `live` None: every 10th position is dead (36 000
    live rows of 40 000: 18 tiles); a number: exactly that many live rows, the dead ones drawn by a seeded permutation.
      u64_two_digits  300 keys that differ only in bits 0..7 and 56..63 (two of the eight digits), one of them on about 70 %
                      of the live rows, the others spread evenly: every key lies scattered over all positions
      u32_random      the same shares over 300 random u32 values: all four digits differ
      one_key         every live row carries one key (no digit differs); the dead rows carry others
      distinct        every live row carries a key of its own
    Dead rows carry values no live row has in bits 8..55 (u64) or at all (u32), and some carry live keys."""
    rng = np.random.default_rng(_seed("wide", kind, n, live))
    dead = np.zeros(n, bool)
    if live is None:
        dead[::10] = True
    else:
        dead[rng.permutation(n)[:n - live]] = True
    m = int((~dead).sum())
    u64 = kind != "u32_random"
    if kind == "u64_two_digits":
        cells = rng.choice(1 << 16, WIDE_KEYS, replace=False).astype(np.uint64)
        values = np.uint64(WIDE_MID) | ((cells >> np.uint64(8)) << np.uint64(56)) | (cells & np.uint64(255))
    elif kind == "u32_random":
        values = np.unique(rng.integers(0, 1 << 32, 2 * WIDE_KEYS, dtype=np.uint64))[:WIDE_KEYS]
        values = values[rng.permutation(values.size)]
    elif kind == "one_key":
        values = np.array([0x0123456789ABCDEF], np.uint64)
    else:
        values = np.unique(rng.integers(0, 1 << 63, 2 * m, dtype=np.uint64))[:m]
        values = values[rng.permutation(m)]
    if kind == "distinct":
        which = np.arange(m)
    elif values.size == 1:
        which = np.zeros(m, np.int64)
    else:
        which = np.where(rng.random(m) < 0.7, 0, rng.integers(1, values.size, m))
    col = np.zeros(n, np.uint64)
    col[~dead] = values[which]
    dead_pos = np.nonzero(dead)[0]
    col[dead_pos] = (rng.integers(0, 1 << 63, dead_pos.size, dtype=np.uint64) | np.uint64(1 << 40)) if u64 else np.uint64(0xFFFFFFFF)
    col[dead_pos[::3]] = values[rng.integers(0, values.size, dead_pos[::3].size)]  # dead rows inside live partitions
    if not u64:
        assert 0xFFFFFFFF not in values.tolist()
    return dict(col=col.astype(np.uint64 if u64 else np.uint32), dead=dead, big=None if kind == "distinct" else int(values[0]))


def sample_keys(lay, count=16):
    """keys to search a wide layout by: the largest, the smallest, six whose run of the sorted pairs crosses, begins at or
    ends at a tile edge (a multiple of SORT_TILE), then others evenly up to `count`"""
    keys, counts = group_by(lay)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    end = first + counts.astype(np.int64)
    pick = [int(np.argmax(counts)), int(np.argmin(counts))]
    pick += np.nonzero((first // SORT_TILE != (end - 1) // SORT_TILE) | (first % SORT_TILE == 0) | (end % SORT_TILE == 0))[0][1:7].tolist()
    pick += np.linspace(0, keys.size - 1, count).astype(np.int64).tolist()
    return [int(keys[i]) for i in list(dict.fromkeys(pick))[:count]]


def mixed_keys(lay, nq=64):
    """one key per query: every sized partition, an absent key, the fully deleted key, further keys and repeats"""
    base = list(lay["keys"]) + [lay["absent_key"], lay["dead_key"]] + list(lay["all_keys"][len(lay["keys"]):len(lay["keys"]) + 8])
    rng = np.random.default_rng(_seed("mixed", nq))
    out = base + [base[int(i)] for i in rng.integers(0, len(base), max(nq - len(base), 0))]
    return np.array(out[:nq], np.uint64)[rng.permutation(nq)]


def make_rows(n, dim, dt):
    rng = np.random.default_rng(_seed("rows", n, dim, dt))
    if dt == "i8":
        return rng.integers(-128, 128, (n, dim)).astype(np.int8)
    if dt == "u8":
        return rng.integers(0, 256, (n, dim)).astype(np.uint8)
    return rng.standard_normal((n, dim)).astype(np.float16 if dt == "f16" else np.float32)


def make_queries(nq, dim, dt):
    rng = np.random.default_rng(_seed("queries", nq, dim, dt))
    if dt == "i8":
        return rng.integers(-128, 128, (nq, dim)).astype(np.int8)
    if dt == "u8":
        return rng.integers(0, 256, (nq, dim)).astype(np.uint8)
    return rng.standard_normal((nq, dim)).astype(np.float32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---- the fresh-process scenario: Float32 8192 x 100, the 64-query mixed batch, host call and device call
FP_DIM, FP_K, FP_METRIC = 100, 10, 2


def fresh_inputs():
    lay = layout("u32")
    return dict(lay=lay, rows=make_rows(N, FP_DIM, "f32"), queries=make_queries(64, FP_DIM, "f32"), keys=mixed_keys(lay, 64))


def _hip_runtime():
    """the HIP runtime this process' libmvf_gpu.so is bound to"""
    with open("/proc/self/maps") as fh:
        for line in fh:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise SystemExit("no HIP runtime is loaded")


def _check(e, what):
    if e != 0:
        raise SystemExit(f"{what}: HIP error {e}")


def main(argv):
    if len(argv) != 2:
        print("usage: _partitioned.py <out.npz>", file=sys.stderr)
        return 2
    sys.modules.setdefault("torch", None)  # the binding would load torch's HIP runtime first where torch is installed
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from metrovector_amd import gpu as G
    inp = fresh_inputs()
    lay, q, keys = inp["lay"], inp["queries"], inp["keys"]
    out = {}
    with G.GpuCorpus.from_array(inp["rows"]) as c:
        c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        with c.attach_column(lay["col"]) as col, c.make_partition(col) as part:
            res = c.search_partitioned(q, keys, FP_K, FP_METRIC, part)
            out["host.scores"], out["host.indices"], out["host.raw"] = res.scores, res.indices, res.raw
            hip = _hip_runtime()
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            nres = q.shape[0] * FP_K
            sizes = [q.nbytes, nres * 4, nres * 8, nres * 4]
            ptrs = [C.c_void_p() for _ in sizes]
            for p, size in zip(ptrs, sizes):
                _check(hip.hipMalloc(C.byref(p), size), "hipMalloc")
            _check(hip.hipMemcpy(ptrs[0], q.ctypes.data_as(C.c_void_p), q.nbytes, 1), "hipMemcpy H2D")
            c.search_partitioned_device(part, ptrs[0].value, 0, q.shape[1], q.shape[0], keys, FP_K, FP_METRIC, ptrs[1].value,
                                        ptrs[2].value, ptrs[3].value)
            _check(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
            got = [np.empty((q.shape[0], FP_K), t) for t in (np.float32, np.uint64, np.int32)]
            for a, p in zip(got, ptrs[1:]):
                _check(hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2), "hipMemcpy D2H")
            for p in ptrs:
                _check(hip.hipFree(p), "hipFree")
            out["device.scores"], out["device.indices"], out["device.raw"] = got
    out["poison"] = np.array([G.selftest_poison()], np.int32)
    np.savez(argv[1], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
