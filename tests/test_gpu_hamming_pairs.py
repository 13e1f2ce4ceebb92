"""Hamming pair join on the GPU (include/mvf_gpu_hamming_pairs.h; DESIGN.md §3 "Hamming pair join", §5 "HJ / HJP"): every
answer against a plain numpy reference, byte for byte -- total, degrees, listed, first, second and raw."""
import functools

import numpy as np
import pytest

from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu


def reference(x, radius, dead=None, ids=None, index_base=0):
    """(total, degrees u32 [rows], first u64, second u64, raw i32): the upper triangle over the live rows in np.nonzero's order,
    which is ascending (i, j); distances from the unpacked bits in float64 (exact below 2^53)"""
    b = np.unpackbits(x, axis=1).astype(np.float64)
    pc = b.sum(1)
    d = pc[:, None] + pc[None, :] - 2 * (b @ b.T)
    live = np.ones(len(x), bool) if dead is None else ~dead
    hit = np.triu(d <= radius, 1) & live[:, None] & live[None, :]
    i, j = np.nonzero(hit)
    name = (np.arange(len(x), dtype=np.uint64) + np.uint64(index_base)) if ids is None else ids
    return len(i), (hit.sum(0) + hit.sum(1)).astype(np.uint32), name[i], name[j], d[i, j].astype(np.int32)


def same(res, want, listed=True):
    n = want[0] if listed else 0
    return (res.total == want[0] and res.listed == listed and res.degrees.tobytes() == want[1].tobytes()
            and res.first.tobytes() == want[2][:n].tobytes() and res.second.tobytes() == want[3][:n].tobytes()
            and res.raw.tobytes() == want[4][:n].tobytes())


def radius_of(dim):
    return max(1, dim)  # an eighth of the bits: no two random rows of 17 bytes or more come near it


@functools.lru_cache(maxsize=None)
def world(kind, dim, rows):
    """(x, dead, ids, index_base, radius, reference).
    planted: random bits, and pairs at exactly r, r + 1 and 0 bits across every boundary the kernel has -- the corpus' two ends,
    two column tiles, two spans, two rows of one A fragment, and a row whose own copy is deleted.
    tied: rows drawn from 8 vectors, a fifth deleted, ids permuted: a dense answer at radius 0, degrees in the hundreds."""
    rng = np.random.default_rng([0x484A, dim, rows])
    x = rng.integers(0, 256, (rows, dim), dtype=np.uint8)
    if kind == "tied":
        x = np.ascontiguousarray(x[:8][rng.integers(0, min(8, rows), rows)])
        dead, ids, base, r = rng.random(rows) < 0.2, rng.permutation(rows).astype(np.uint64) + np.uint64(10**12), 77, 0
    else:
        f = G.hamming_pairs_form(dim, rows)
        r, dead, ids, base, used = radius_of(dim), np.zeros(rows, bool), None, 1000, set()
        qt, span = f.query_tile, f.span_rows
        for a, b, dist in ((0, rows - 1, r), (qt - 1, qt, r + 1), (span - 1, span, 0), (qt + 4, qt + 5, r), (2, 3, 0), (span - 2, span + 1, r),
                           (qt - 2, 2 * qt + 1, r + 1), (1, rows - 2, 0)):
            if 0 <= a < b < rows and not {a, b} & used:
                used |= {a, b}
                flip = np.zeros(8 * dim, bool)
                flip[rng.choice(8 * dim, dist, replace=False)] = True
                x[b] = x[a] ^ np.packbits(flip)
        if rows > 3:
            dead[3] = True  # row 2's copy
    return x, dead, ids, base, r, reference(x, r, dead, ids, base)


def join(kind, dim, rows, max_pairs=1 << 20):
    x, dead, ids, base, r, want = world(kind, dim, rows)
    with G.GpuCorpus.from_array(x, device=0, index_base=base) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        if ids is not None:
            c.set_vector_ids(ids)
        return c.hamming_pairs(r, max_pairs), want


@pytest.mark.parametrize("kind", ["planted", "tied"])
@pytest.mark.parametrize("dim", [1, 17, 64, 65, 256, 257, 512])
def test_dimensions(dim, kind):
    """tail masks in the first and in a later step, both tile caps, a chunk tail of zeros; 1100 rows are two spans and 9 or 18
    column tiles, the last of them partial"""
    f = G.hamming_pairs_form(dim, 1100)
    assert f.spans == 2 and f.query_tile == (128 if dim <= 256 else 64) and 1100 % f.query_tile
    res, want = join(kind, dim, 1100)
    assert same(res, want) and want[0] > 3 and int(want[1].sum()) == 2 * want[0]
    if kind == "tied":
        assert want[1].max() >= 100
    elif dim >= 17:
        assert {radius_of(dim), 0} <= set(want[4].tolist()) and want[2][0] == 1000 and want[3][0] == 1000 + 1099


@pytest.mark.parametrize("rows", [1, 2, 15, 17, 65, 300])
def test_row_counts(rows):
    """no pair at all, below a fragment, every tile width, idle columns behind the corpus' end"""
    for kind in ("planted", "tied"):
        res, want = join(kind, 48, rows)
        assert same(res, want), kind


def test_several_spans_and_tiles_that_skip_spans():
    f = G.hamming_pairs_form(16, 2300)
    assert f.spans >= 2 and f.tiles > 2 and f.blocks < f.tiles * f.spans  # a (tile, span) that is not launched
    for kind in ("planted", "tied"):
        res, want = join(kind, 16, 2300)
        assert same(res, want), kind


@pytest.mark.parametrize("room", ["none", "exact", "one short", "most"])
def test_max_pairs(room):
    """0 with NULL buffers; exactly the total; one entry short: nothing listed, total and degrees still exact; 2^24"""
    want = world("tied", 17, 1100)[-1]
    m = {"none": 0, "exact": want[0], "one short": want[0] - 1, "most": 1 << 24}[room]
    res, _ = join("tied", 17, 1100, m)
    assert want[0] > 10000 and same(res, want, listed=room in ("exact", "most"))


@pytest.mark.parametrize("radius,total", [(4096, 40 * 39 // 2), (4095, 40 * 39 // 2 - 2), (0, 1), (2**32 - 1, 40 * 39 // 2)])
def test_extremes(radius, total):
    """the accumulators' limits at 512 bytes: all-ones against all-zeros is d = 4096, the start value -4097 .. 4095"""
    x = np.random.default_rng(1).integers(0, 256, (40, 512), dtype=np.uint8)
    x[3], x[20], x[33] = 0, 0xFF, 0
    with G.GpuCorpus.from_array(x, device=0) as c:
        res = c.hamming_pairs(radius)
    want = reference(x, radius)
    assert same(res, want) and res.total == total


def test_the_handle_answers_its_other_calls_as_before_and_the_recipe_holds():
    """degrees[i] = the radius search's count for row i as a query, minus the row itself, on the same handle"""
    x, dead, _, base, r, want = world("planted", 48, 300)
    with G.GpuCorpus.from_array(x, device=0, index_base=base) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        before = c.search_hamming(x[:17], 10), c.search_hamming_radius(x, r, 0)
        res = c.hamming_pairs(r)
        after = c.search_hamming(x[:17], 10), c.search_hamming_radius(x, r, 0)
    assert same(res, want)
    assert before[0].indices.tobytes() == after[0].indices.tobytes() and before[0].raw.tobytes() == after[0].raw.tobytes()
    assert before[1].counts.tobytes() == after[1].counts.tobytes()
    assert np.array_equal(res.degrees[~dead], after[1].counts[~dead] - 1) and not res.degrees[dead].any()


def test_refusals_that_need_a_handle():
    x = np.random.default_rng(2).integers(0, 256, (300, 513), dtype=np.uint8)
    with G.GpuCorpus.from_array(x, device=0) as c:
        with pytest.raises(E.InvalidArgument, match="rows above 512 packed bytes are not built for the Hamming pair join"):
            c.hamming_pairs(5)
    with G.GpuCorpus.from_array(np.ascontiguousarray(x[:, :64]).view(np.int8), device=0) as c:
        with pytest.raises(E.BuildError):
            c.hamming_pairs(5)
