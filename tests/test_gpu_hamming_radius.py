"""Hamming radius search on the GPU (include/mvf_gpu_hamming_radius.h; DESIGN.md §3 "Hamming radius search", §5 "HR2 / HRP"):
every answer against a plain numpy reference, byte for byte -- counts, indices, raw distances and score bits, no query left out."""
import functools

import numpy as np
import pytest

from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def distances(q, x):
    """i64 [nq, rows] from the unpacked bits"""
    qb, xb = np.unpackbits(q, axis=1).astype(np.int64), np.unpackbits(x, axis=1).astype(np.int64)
    return qb.sum(1)[:, None] + xb.sum(1)[None, :] - 2 * qb @ xb.T


def reference(q, x, radii, m, dead=None, ids=None, index_base=0):
    """(counts u64 [nq], scores f32, indices u64, raw i32 [nq, m]): a stable argsort of d over the live rows, cut at the radius"""
    d = distances(q, x)
    live = np.arange(len(x)) if dead is None else np.nonzero(~dead)[0]
    name = (np.arange(len(x), dtype=np.uint64) + np.uint64(index_base)) if ids is None else ids
    r = np.broadcast_to(np.asarray(radii, np.int64), (len(q),))
    counts = (d[:, live] <= r[:, None]).sum(1).astype(np.uint64)
    sc, idx, raw = np.full((len(q), m), np.inf, np.float32), np.full((len(q), m), PAD, np.uint64), np.zeros((len(q), m), np.int32)
    for i in range(len(q)):
        order = live[np.argsort(d[i, live], kind="stable")][:min(int(counts[i]), m)]
        raw[i, :len(order)], idx[i, :len(order)] = d[i, order], name[order]
        sc[i, :len(order)] = d[i, order].astype(np.float32)
    return counts, sc, idx, raw


def same(res, want):
    return (res.counts.tobytes() == want[0].tobytes() and res.indices.tobytes() == want[2].tobytes()
            and res.raw.tobytes() == want[3].tobytes() and res.scores.tobytes() == want[1].tobytes())


@functools.lru_cache(maxsize=None)
def world(kind, dim, rows, nq):
    """(x, q, dead, ids, index_base).  spread: random bits.  tied: rows drawn from 8 vectors (hundreds of ties at every cut go by
    position), a fifth deleted, ids permuted.  worst-first: for query 2 the rows of each of the two slices come farthest first."""
    rng = np.random.default_rng([0x4852, dim, rows, nq])
    q = rng.integers(0, 256, (nq, dim), dtype=np.uint8)
    x = rng.integers(0, 256, (rows, dim), dtype=np.uint8)
    if kind == "spread":
        return x, q, None, None, 1000
    if kind == "tied":
        x = np.ascontiguousarray(x[:8][rng.integers(0, min(8, rows), rows)])
        return x, q, rng.random(rows) < 0.2, rng.permutation(rows).astype(np.uint64) + np.uint64(10**12), 0
    per = -(-rows // 2)
    at = np.arange(rows)
    differ = (8 * dim) - (at % per) * (8 * dim) // per  # bits of the row that differ from query 2
    flip = rng.permutation(8 * dim)[None, :] < differ[:, None]
    return np.packbits(flip, axis=1) ^ q[2][None, :], q, None, None, 7


def mixed_radii(q, x, dead, m):
    """per query, in turn: 0 (query 0 is planted as an exact copy by the caller), a radius matching nothing, the distance of the
    m-th live row exactly (the inclusive edge, and a tie across the cut where rows repeat), 8 x dimension, 2^32 - 1"""
    d = distances(q, x)[:, ~dead] if dead is not None else distances(q, x)
    kth = np.sort(d, axis=1)[:, min(max(m, 1), d.shape[1]) - 1]
    nothing = np.maximum(d.min(1) - 1, 0)  # (matches nothing unless the nearest row is an exact copy)
    r = np.stack([np.zeros(len(q), np.int64), nothing, kth, np.full(len(q), 8 * q.shape[1]), np.full(len(q), 2**32 - 1)])
    return r[np.arange(len(q)) % 5, np.arange(len(q))].astype(np.uint32)


def check(kind, dim, rows, nq, m):
    x, q, dead, ids, base = world(kind, dim, rows, nq)
    q = q.copy()
    q[0] = x[rows // 2]  # a planted exact copy under radius 0 (deleted or not, as the corpus has it)
    radii = mixed_radii(q, x, dead, m)
    with G.GpuCorpus.from_array(x, device=0, index_base=base) as c:
        if dead is not None:
            c.set_tombstones(np.packbits(dead, bitorder="little"))
            c.set_vector_ids(ids)
        res = c.search_hamming_radius(q, radii, m)
    assert same(res, reference(q, x, radii, m, dead, ids, base))


def tile_of(dim, nq):
    """the query-tile rule: the smallest of 16 .. 128 that holds the window, capped by the prepared tile's LDS"""
    return min(128 if dim <= 256 else 64, max(16, 1 << (min(nq, 1024) - 1).bit_length()))


@pytest.mark.parametrize("kind", ["spread", "tied", "worst-first"])
@pytest.mark.parametrize("dim", [1, 16, 17, 64, 65, 128, 129, 256, 257, 512])
def test_dimensions(dim, kind):
    """tail masks in the first and in a later step, both LDS caps, a chunk tail of zeros; two slices of 550 rows, whose third
    iteration is partial"""
    f = G.hamming_radius_form(dim, 17, 1100)
    assert f.row_slices == 2 and 550 % 256 and f.query_tile == tile_of(dim, 17) and f.chunks == (dim + 63) // 64
    check(kind, dim, 1100, 17, 10)


@pytest.mark.parametrize("rows", [1, 15, 17, 63, 65])
def test_row_counts(rows):
    """below a fragment and below a wave tile; padding beyond the live rows"""
    check("spread", 48, rows, 7, 10)
    check("tied", 48, rows, 7, 10)


@pytest.mark.parametrize("dim,nq", [(128, n) for n in (1, 16, 17, 33, 65, 128, 1025)] + [(300, 65)])
def test_query_counts(dim, nq):
    """every NC, an idle column, a second tile, a second window"""
    assert G.hamming_radius_form(dim, nq, 300).query_tile == tile_of(dim, nq)
    check("spread", dim, 300, nq, 10)


@pytest.mark.parametrize("m", [0, 1, 100, 1024])
def test_max_per_query(m):
    """counts only with NULL buffers; counts below and above max_per_query in one call (the radii are mixed)"""
    check("tied", 17, 1100, 10, m)
    check("worst-first", 300, 1100, 10, m)


def test_overflow_is_completed_by_the_top_k_search_and_the_recipe_holds():
    """9000 rows: query 1 matches more than the device list's 8192 and is completed on the host, its neighbours are not; every
    query's entries are search_hamming's at k = max_per_query cut at the radius, on the same handle"""
    x, q, _, _, base = world("spread", 24, 9000, 5)
    radii, m = np.array([80, 192, 90, 0, 85], np.uint32), 100
    with G.GpuCorpus.from_array(x, device=0, index_base=base) as c:
        res, top = c.search_hamming_radius(q, radii, m), c.search_hamming(q, m)
    want = reference(q, x, radii, m, index_base=base)
    assert same(res, want) and res.counts[1] == 9000 and res.overflowed.tolist() == [False, True, False, False, False]
    assert 0 < res.counts[0] < 8192 and res.counts[3] == 0
    cut = top.raw <= radii[:, None].astype(np.int64)
    assert np.array_equal(res.indices[cut], top.indices[cut]) and np.array_equal(res.raw[cut], top.raw[cut]) and (res.indices[~cut] == PAD).all()
    assert np.array_equal(np.minimum(res.counts, m), cut.sum(1))


def test_extremes():
    """the accumulators' limits at 512 bytes: all-ones against all-zeros is d = 4096, the start value -4097 .. 4095"""
    x = np.random.default_rng(1).integers(0, 256, (40, 512), dtype=np.uint8)
    x[3], x[20] = 0, 0xFF
    q = np.stack([np.full(512, 0xFF, np.uint8), np.zeros(512, np.uint8), np.full(512, 0xFF, np.uint8)])
    radii = np.array([4096, 4095, 0], np.uint32)
    with G.GpuCorpus.from_array(x, device=0) as c:
        res = c.search_hamming_radius(q, radii, 40)
    assert same(res, reference(q, x, radii, 40))
    assert res.counts.tolist() == [40, 39, 1] and res.raw[0, -1] == 4096 and res.indices[0, -1] == 3 and res.scores[0, -1] == np.float32(4096)


def test_the_handle_answers_its_other_calls_as_before():
    x, q, _, _, _ = world("spread", 48, 1100, 17)
    s8 = np.random.default_rng(3).integers(-128, 128, (4, 8 * 48), dtype=np.int8)
    with G.GpuCorpus.from_array(x, device=0) as c:
        before = c.search_hamming(q, 10), c.search_signbits(s8, 10)
        res = c.search_hamming_radius(q, 150, 20)
        after = c.search_hamming(q, 10), c.search_signbits(s8, 10)
    assert same(res, reference(q, x, 150, 20))
    for a, b in zip(before, after):
        assert a.indices.tobytes() == b.indices.tobytes() and a.raw.tobytes() == b.raw.tobytes() and a.scores.tobytes() == b.scores.tobytes()


def test_refusals_that_need_a_handle():
    x = np.random.default_rng(2).integers(0, 256, (300, 513), dtype=np.uint8)
    with G.GpuCorpus.from_array(x, device=0) as c:
        with pytest.raises(E.InvalidArgument, match="rows above 512 packed bytes are not built for Hamming radius search"):
            c.search_hamming_radius(x[:2], 5, 5)
    with G.GpuCorpus.from_array(np.ascontiguousarray(x[:, :64]).view(np.int8), device=0) as c:
        with pytest.raises(E.BuildError):
            c.search_hamming_radius(x[:2, :64], 5, 5)
    with G.GpuCorpus.from_array(np.ascontiguousarray(x[:, :64]), device=0) as c:
        with pytest.raises(E.BuildError):
            c.search_hamming_radius(x[:2, :64].view(np.int8), 5, 5)
        with pytest.raises(E.DimensionMismatch):
            c.search_hamming_radius(np.ascontiguousarray(x[:2, :63]), 5, 5)
        assert same(c.search_hamming_radius(x[:2, :64], 5, 5), reference(np.ascontiguousarray(x[:2, :64]), np.ascontiguousarray(x[:, :64]), 5, 5))
