"""What the tests of the Hamming search share (include/mvf_gpu_hamming.h; DESIGN.md §3 "Hamming search"): the stream classes
of the header's functions and the numpy reference every GPU answer is compared with, byte for byte.  Behind them, for the
forms tests (DESIGN.md §5 "H0 / H1", "Tested forms"): FORM_CELLS, the hand-written table of cases that reach each of the 23
scan kernels; the seeded data builders; the per-slice lists and merge_path, which predicts the path H1 takes; and the wrong
models -- variants of the reference that a subtly wrong kernel would compute, which the CPU tier tells apart on that data."""
import functools
from typing import NamedTuple, Optional

import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)

# The stream class of every function include/mvf_gpu_hamming.h declares, in tests/_streams.py's words (its ENTRY_CLASS lists
# include/mvf_gpu.h's functions), and the device form the measurement aid among them runs.
ENTRY_CLASS = {
    "mvfgpu_search_hamming": "runs under corpus_device_call",
    "mvfgpu_search_hamming_device": "runs under corpus_device_call",
    "mvfgpu_selftest_hamming_form": "takes no handle",
    "mvfgpu_selftest_hamming_stage_ms": "runs under corpus_device_call",
}
TIMED_FORM_OF = {"mvfgpu_selftest_hamming_stage_ms": "mvfgpu_search_hamming_device"}


def _bits(a):
    """the set bits of every uint8 of a"""
    return np.bitwise_count(a) if hasattr(np, "bitwise_count") else np.unpackbits(a[..., None], axis=-1).sum(-1, dtype=np.uint8)


def distances(queries, rows):
    """d[q, r] = the bits in which uint8 queries [nq, dim] and rows [n, dim] differ"""
    return _bits(queries[:, None, :] ^ rows[None, :, :]).sum(-1, dtype=np.int64)


def reference(queries, rows, k, dead=None, ids=None, index_base=0):
    """(scores f32, indices u64, raw i32) [nq, k] of the contract: the k live rows of smallest distance, ties by ascending
    position, an L2 search's padding behind them.  Queries are taken a few at a time to bound the unpacked bits."""
    nq, n = queries.shape[0], rows.shape[0]
    live = np.arange(n) if dead is None else np.nonzero(~dead)[0]
    name = (np.arange(n, dtype=np.uint64) + np.uint64(index_base)) if ids is None else ids
    sc = np.full((nq, k), np.inf, np.float32)
    idx = np.full((nq, k), PAD, np.uint64)
    raw = np.zeros((nq, k), np.int32)
    take = min(k, live.size)
    step = max(1, (1 << 27) // max(1, live.size * rows.shape[1] * 8))
    for q0 in range(0, nq, step):
        d = distances(queries[q0:q0 + step], rows[live])
        order = np.argsort(d, axis=1, kind="stable")[:, :take]  # stable: equal distances stay in position order
        best = np.take_along_axis(d, order, axis=1)
        raw[q0:q0 + step, :take] = best
        sc[q0:q0 + step, :take] = best.astype(np.float32)
        idx[q0:q0 + step, :take] = name[live[order]]
    return sc, idx, raw


def same(res, want):
    """a SearchResult equals the reference's (scores, indices, raw) in every byte"""
    return (res.indices.tobytes() == want[1].tobytes() and res.raw.tobytes() == want[2].tobytes()
            and res.scores.tobytes() == want[0].tobytes())


# ---- the forms (DESIGN.md §5 "H0 / H1"; tests/test_hamming_forms_cpu.py, tests/test_gpu_hamming_forms.py) ----

REGISTER, STREAMING = 0, 1
STEP_ROWS = 256     # rows of one H0 iteration at most
SLICE_ROWS = 1024   # rows of a slice at least
MERGE_LDS = 16384   # list entries H1 sorts in one round
MERGE_MAX = 65536   # list entries H1 merges per query at most
INDEX_BASE = 1000
ID_BASE = np.uint64(10**12)

# (dimension, nq, k) -> (form, G, QT, QB): the case and the scan kernel it runs, written down by hand from DESIGN.md §5
# "H0 / H1" -- pitch = dimension rounded up to 16, V = pitch / 16 steps; register form up to a pitch of 256 with
# G = next_pow2(V), streaming form beyond with G = 32 up to V = 32 and 64 above; QT = min(next_pow2(nq), what the buffers
# allow: 16 up to k = 256, 8 up to 512, 4 at 1024 in the register form; 8 and 150 KiB / (buffer + pitch) in the streaming
# form); QB = min(G, QT) in the register form, QT in the streaming form.  Dimensions with idle lanes (V < G) wherever a
# group has more than two lanes, the full groups of 64 / 128 / 256 / 512 bytes as second entries; nq leaves an idle query
# slot in every tile of more than one query (3 of 4, 5 of 8, 9 of 16).
FORM_CELLS = {
    (13, 1, 10): (REGISTER, 1, 1, 1),        # V = 1, 13 of 16 bytes
    (16, 9, 10): (REGISTER, 1, 16, 1),       # the same kernel walking a tile of 16
    (27, 1, 10): (REGISTER, 2, 1, 1),        # V = 2 (a group of two is never short of a step)
    (27, 2, 10): (REGISTER, 2, 2, 2),
    (32, 9, 10): (REGISTER, 2, 16, 2),
    (40, 1, 10): (REGISTER, 4, 1, 1),        # V = 3 of 4
    (40, 2, 10): (REGISTER, 4, 2, 2),
    (40, 3, 10): (REGISTER, 4, 4, 4),
    (64, 9, 10): (REGISTER, 4, 16, 4),       # V = 4: the full group
    (100, 1, 10): (REGISTER, 8, 1, 1),       # V = 7 of 8
    (100, 2, 10): (REGISTER, 8, 2, 2),
    (100, 3, 10): (REGISTER, 8, 4, 4),
    (100, 5, 10): (REGISTER, 8, 8, 8),
    (128, 9, 10): (REGISTER, 8, 16, 8),      # V = 8: the full group
    (200, 1, 10): (REGISTER, 16, 1, 1),      # V = 13 of 16
    (200, 2, 10): (REGISTER, 16, 2, 2),
    (200, 3, 10): (REGISTER, 16, 4, 4),
    (150, 9, 600): (REGISTER, 16, 4, 4),     # V = 10 of 16; the tile of 4 that k above 512 leaves
    (200, 5, 10): (REGISTER, 16, 8, 8),
    (200, 9, 10): (REGISTER, 16, 16, 16),
    (256, 9, 10): (REGISTER, 16, 16, 16),    # V = 16: the full group
    (300, 1, 10): (STREAMING, 32, 1, 1),     # V = 19 of 32
    (300, 2, 10): (STREAMING, 32, 2, 2),
    (300, 3, 10): (STREAMING, 32, 4, 4),
    (300, 5, 10): (STREAMING, 32, 8, 8),
    (512, 5, 10): (STREAMING, 32, 8, 8),     # V = 32: the full group
    (1100, 1, 10): (STREAMING, 64, 1, 1),    # V = 69: five lanes take two steps, the others one
    (1100, 2, 10): (STREAMING, 64, 2, 2),
    (1100, 3, 10): (STREAMING, 64, 4, 4),
    (2100, 5, 10): (STREAMING, 64, 8, 8),    # V = 132
    (2100, 3, 1024): (STREAMING, 64, 4, 4),  # buffers of 2048 entries
    (33025, 8, 10): (STREAMING, 64, 4, 4),   # the longest row: 150 KiB hold four of them beside the buffers
}


def cell_id(cell):
    form, g, qt, qb = FORM_CELLS[cell]
    return f"{'stream' if form else 'reg'}-g{g}-qt{qt}-qb{qb}-d{cell[0]}-nq{cell[1]}-k{cell[2]}"


def cell_rows(dim):
    """(rows, slices) of a cell's corpora: 1100 rows are two slices of 550, whose third iteration is partial; the longest
    rows come 64 to a corpus, one slice"""
    return (64, 1) if dim == 33025 else (1100, 2)


def next_pow2(v):
    return 1 << max(0, int(v) - 1).bit_length()


class World(NamedTuple):
    x: np.ndarray                 # rows [n, dim] uint8
    q: np.ndarray                 # queries [nq, dim] uint8
    dead: Optional[np.ndarray]    # deleted positions [n] bool, or None
    ids: Optional[np.ndarray]     # vector ids [n] uint64, or None


def _rng(*parts):
    return np.random.default_rng([0x48414D] + [int(p) for p in parts])


def spread(dim, rows, nq):
    """random bytes; every third query a near-copy of a row (the low bit of about half its bytes flipped)"""
    rng = _rng(1, dim, rows, nq)
    x = rng.integers(0, 256, (rows, dim), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, dim), dtype=np.uint8)
    near = np.arange(0, nq, 3)
    q[near] = x[(7 + 5 * near) % rows] ^ rng.integers(0, 2, (near.size, dim), dtype=np.uint8)
    return World(x, q, None, None)


def tied(dim, rows, nq):
    """rows drawn from 8 vectors: hundreds of ties at the k-th rank; a fifth of the rows deleted, ids permuted.  The first
    two queries are two of the vectors, so their ties start at distance 0."""
    rng = _rng(2, dim, rows, nq)
    base = rng.integers(0, 256, (8, dim), dtype=np.uint8)
    x = np.ascontiguousarray(base[rng.integers(0, 8, rows)])
    q = np.ascontiguousarray(np.concatenate([base[:2], rng.integers(0, 256, (nq, dim), dtype=np.uint8)])[:nq])
    dead = rng.random(rows) < 0.2
    ids = rng.permutation(rows).astype(np.uint64) + ID_BASE
    return World(x, q, dead, ids)


def descending(dim, rows, nq, slices):
    """For query 0 the rows of every slice come farthest first: place i of a slice of n rows differs from the query in
    dimension * 8 - i * (dimension * 8 + 1) // n bits (the first in all of them, the last in fewer than (bits + 1) / n), so equal distances run
    for n / (bits + 1) rows at most, and every row beats the k-th best of the rows in front of it as long as that run is
    no longer than k: each row enters the buffer, which fills as fast as it can.  The other queries are random."""
    rng = _rng(3, dim, rows, nq)
    bits = dim * 8
    q = rng.integers(0, 256, (nq, dim), dtype=np.uint8)
    per = -(-rows // slices)
    at = np.arange(rows)
    n_s = np.minimum(per, rows - at // per * per)  # the rows of the row's own slice
    far = bits - (at % per) * (bits + 1) // n_s
    rank = rng.permutation(bits)                   # the order in which the bits come back into line
    x = q[0][None, :] ^ np.packbits(rank[None, :] < far[:, None], axis=1)
    return World(np.ascontiguousarray(x), q, None, None)


BUILDERS = ("spread", "tied", "descending")


@functools.lru_cache(maxsize=None)
def cell_worlds(cell):
    """the three corpora of a cell, by builder name"""
    dim, nq, _ = cell
    rows, slices = cell_rows(dim)
    return {"spread": spread(dim, rows, nq), "tied": tied(dim, rows, nq), "descending": descending(dim, rows, nq, slices)}


# ---- the merge cases: 16-byte rows, k = 1024, shapes whose slice count the rows or H1's limit decide, not the CU count ----

MERGE_K = 1024
ONE_ROUND, BOUND_ONE_ROUND, ROUNDS = "one round", "bound, then one round", "rounds"


def _near(rng, q0, n, equal):
    """n rows within one bit of q0, a share `equal` of them equal to it"""
    flip = np.zeros((n, q0.size), np.uint8)
    bit = rng.integers(0, q0.size * 8, n)
    flip[np.arange(n), bit >> 3] = np.uint8(1) << (bit & 7).astype(np.uint8)
    flip[rng.random(n) < equal] = 0
    return q0[None, :] ^ flip


def merge_dense(nq):
    """64 slices of 1032 rows; each holds 1023 rows within one bit of query 0 (one in a hundred equal to it) at random
    places and 9 random rows: every slice's k-th best is a far row, the bound the nearest of them, and all 64 x 1023 near
    rows lie below it -- H1 takes the rounds with a real bound, and the answer takes rows of every slice"""
    rng = _rng(4, nq)
    slices, per = 64, 1032
    q = rng.integers(0, 256, (nq, 16), dtype=np.uint8)
    x = rng.integers(0, 256, (slices * per, 16), dtype=np.uint8)
    for s in range(slices):
        x[s * per + rng.permutation(per)[:1023]] = _near(rng, q[0], 1023, 0.01)
    return World(x, q, None, None), slices


def merge_one_slice():
    """the same shape with random rows, but for 1024 rows of slice 37 within one bit of query 0: the k best lie in that
    slice, its k-th best is the bound and the k-th result, and 1024 entries lie at or below it -- the bound, then one round"""
    rng = _rng(5)
    slices, per = 64, 1032
    q = rng.integers(0, 256, (1, 16), dtype=np.uint8)
    x = rng.integers(0, 256, (slices * per, 16), dtype=np.uint8)
    x[37 * per + rng.permutation(per)[:1024]] = _near(rng, q[0], 1024, 0.01)
    return World(x, q, None, None), slices


def merge_edge(slices):
    """slices x 1024 random rows, one query near a row: 16 slices are exactly 16384 list entries, one round on both sides of
    the launch; 17 are the rounds on full lists, and the last slice's rows arrive in the second"""
    return spread(16, slices * 1024, 1), slices


MERGE_CASES = {  # name -> (builder, intended path of query 0)
    "dense-nq1": (lambda: merge_dense(1), ROUNDS),
    "dense-nq2": (lambda: merge_dense(2), ROUNDS),
    "one-slice": (merge_one_slice, BOUND_ONE_ROUND),
    "edge-16-slices": (lambda: merge_edge(16), ONE_ROUND),
    "edge-17-slices": (lambda: merge_edge(17), ROUNDS),
}


@functools.lru_cache(maxsize=None)
def merge_world(name):
    return MERGE_CASES[name][0]()


def slice_lists(d_row, k, slices, dead=None):
    """what H0 leaves of one query: per slice the sorted composites (distance << 32 | position) of its k best live rows"""
    n = d_row.size
    per = -(-n // slices)
    comp = (d_row.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    if dead is not None:
        comp = np.where(dead, PAD, comp)
    lists = [np.sort(comp[s * per:(s + 1) * per]) for s in range(slices)]
    return [c[c != PAD][:k] for c in lists]


def merge_bound(lists, k):
    """(H1's bound: the smallest of the full slices' k-th composites, None where no slice is full; the entries at or below it)"""
    kth = [c[k - 1] for c in lists if c.size >= k]
    if not kth:
        return None, sum(c.size for c in lists)
    return min(kth), sum(int((c <= min(kth)).sum()) for c in lists)


def merge_path(lists, k):
    """the path H1 takes for one query, from its per-slice lists"""
    if len(lists) * next_pow2(k) <= MERGE_LDS:
        return ONE_ROUND
    return BOUND_ONE_ROUND if merge_bound(lists, k)[1] <= MERGE_LDS else ROUNDS


def answer_of(comp, k, ids=None, index_base=0):
    """a sorted list of composites as one query's (scores, indices, raw) [1, k]"""
    comp = comp[:k]
    sc, idx, raw = np.full((1, k), np.inf, np.float32), np.full((1, k), PAD, np.uint64), np.zeros((1, k), np.int32)
    d, r = (comp >> np.uint64(32)).astype(np.int64), (comp & np.uint64(0xFFFFFFFF)).astype(np.int64)
    sc[0, :comp.size], raw[0, :comp.size] = d.astype(np.float32), d
    idx[0, :comp.size] = (r.astype(np.uint64) + np.uint64(index_base)) if ids is None else ids[r]
    return sc, idx, raw


def merged(lists, k, wrong=None):
    """H1 on one query's lists: the k smallest composites.  Wrong models: "first round only" stops behind the first 16384
    entries of lists[slice][next_pow2(k)]; "bound dropped" takes `<` for `<=` at the bound (count and collection alike)."""
    kcap, everything = next_pow2(k), np.concatenate(lists)
    if wrong == "first round only":
        everything = np.concatenate([np.concatenate([c, np.full(kcap - c.size, PAD, np.uint64)]) for c in lists])[:MERGE_LDS]
        everything = everything[everything != PAD]
    elif wrong == "bound dropped":
        bound = merge_bound(lists, k)[0]
        if len(lists) * kcap > MERGE_LDS and bound is not None and int((everything < bound).sum()) <= MERGE_LDS:
            everything = everything[everything < bound]
    else:
        assert wrong is None
    return np.sort(everything)[:k]


MERGE_MODELS = ("first round only", "bound dropped")


# ---- the reference on a distance matrix, and the wrong models of H0 ----

def step_distances(queries, rows):
    """part[q, r, s] = the differing bits inside 16-byte step s; their sum over s is distances(queries, rows)"""
    dim = rows.shape[1]
    pad = -dim % 16
    x = np.pad(queries, ((0, 0), (0, pad)))[:, None, :] ^ np.pad(rows, ((0, 0), (0, pad)))[None, :, :]
    return _bits(x).reshape(x.shape[0], x.shape[1], -1, 16).sum(-1, dtype=np.int64)


def select(d, k, dead=None, ids=None, index_base=0, last_first=False):
    """reference() from the distances d [nq, n] on; last_first breaks ties by DESCENDING position"""
    nq, n = d.shape
    live = np.arange(n) if dead is None else np.nonzero(~dead)[0]
    name = (np.arange(n, dtype=np.uint64) + np.uint64(index_base)) if ids is None else ids
    sc, idx, raw = np.full((nq, k), np.inf, np.float32), np.full((nq, k), PAD, np.uint64), np.zeros((nq, k), np.int32)
    take = min(k, live.size)
    dl = d[:, live]
    if last_first:
        order = (live.size - 1 - np.argsort(dl[:, ::-1], axis=1, kind="stable"))[:, :take]
    else:
        order = np.argsort(dl, axis=1, kind="stable")[:, :take]
    best = np.take_along_axis(dl, order, axis=1)
    raw[:, :take], sc[:, :take], idx[:, :take] = best, best.astype(np.float32), name[live[order]]
    return sc, idx, raw


def tail_rows(n, slices):
    """[n] bool: the rows of every slice's last iteration of 256 where that one is partial"""
    per = -(-n // slices)
    at = np.arange(n)
    n_s = np.minimum(per, n - at // per * per)
    return at % per >= n_s // STEP_ROWS * STEP_ROWS


def wrong_ties_descending(d, k, w, slices):
    return select(d, k, w.dead, w.ids, INDEX_BASE, last_first=True)


def wrong_neighbours_exchanged(d, k, w, slices):
    """the answers of queries j and j ^ 1 of a batch exchanged (a last query without a partner keeps its own)"""
    j = np.arange(d.shape[0]) ^ 1
    j[j >= d.shape[0]] = d.shape[0] - 1
    return tuple(a[j] for a in select(d, k, w.dead, w.ids, INDEX_BASE))


def wrong_tail_lost(d, k, w, slices):
    lost = tail_rows(d.shape[1], slices)
    return select(d, k, lost if w.dead is None else lost | w.dead, w.ids, INDEX_BASE)


def wrong_tombstones_ignored(d, k, w, slices):
    return select(d, k, None, w.ids, INDEX_BASE)


def wrong_tombstones_by_id(d, k, w, slices):
    dead = w.dead if w.ids is None or w.dead is None else w.dead[(w.ids - ID_BASE).astype(np.int64)]
    return select(d, k, dead, w.ids, INDEX_BASE)


def wrong_step_left_out(part, s, k, w):
    """16-byte step s of the rows left out of the distance"""
    return select(part.sum(-1) - part[:, :, s], k, w.dead, w.ids, INDEX_BASE)


# name -> (model, the least nq it can show at).  Leaving out a step has its own test: one model per step of the cell.
WRONG_MODELS = {
    "ties by descending position": (wrong_ties_descending, 1),
    "queries j and j ^ 1 exchanged": (wrong_neighbours_exchanged, 2),
    "partial last iteration lost": (wrong_tail_lost, 1),
    "tombstones ignored": (wrong_tombstones_ignored, 1),
    "tombstones looked up by id": (wrong_tombstones_by_id, 1),
}


def same_answers(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
