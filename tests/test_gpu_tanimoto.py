"""Tanimoto search on the GPU (include/mvf_gpu_tanimoto.h; DESIGN.md §3 "Tanimoto search", §5 "TQ / T2"): every answer against
a plain numpy reference, byte for byte -- indices and score bits, no query left out."""
import functools

import numpy as np
import pytest

from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def reference(q, x, k, dead=None, ids=None, index_base=0):
    """(scores f32, indices u64) [nq, k]: the k live rows of largest T = c / u (0 for u = 0), ties by ascending position, then
    the padding"""
    qb, xb = np.unpackbits(q, axis=1).astype(np.int64), np.unpackbits(x, axis=1).astype(np.int64)
    c = qb @ xb.T
    u = qb.sum(1)[:, None] + xb.sum(1)[None, :] - c
    t = np.where(u > 0, c.astype(np.float32) / np.maximum(u, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    live = np.arange(len(x)) if dead is None else np.nonzero(~dead)[0]
    name = (np.arange(len(x), dtype=np.uint64) + np.uint64(index_base)) if ids is None else ids
    order = np.argsort(-t[:, live], axis=1, kind="stable")[:, :k]  # stable: equal scores stay in position order
    take = order.shape[1]
    sc, idx = np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), PAD, np.uint64)
    sc[:, :take], idx[:, :take] = np.take_along_axis(t[:, live], order, axis=1), name[live[order]]
    return sc, idx


def same(res, want):
    return res.indices.tobytes() == want[1].tobytes() and res.scores.tobytes() == want[0].tobytes()


def random_bits(rng, n, dim):
    """n packed vectors of mixed density 0.05 .. 0.9, so that the popcounts vary"""
    return np.packbits(rng.random((n, 8 * dim)) < rng.uniform(0.05, 0.9, (n, 1)), axis=1)


@functools.lru_cache(maxsize=None)
def world(kind, dim, rows, nq):
    """(x, q, dead, ids, index_base).  spread: rows and queries of mixed density.  tied: rows drawn from 8 vectors (hundreds of
    ties at rank k go by position), a fifth deleted, ids permuted.  ascending: for query 0 the rows of each of the two slices
    come worst first, so every row enters its buffer and the buffers settle again and again."""
    rng = np.random.default_rng([0x7A41, dim, rows, nq])
    q, x = random_bits(rng, nq, dim), random_bits(rng, rows, dim)
    if kind == "spread":
        return x, q, None, None, 1000
    if kind == "tied":
        x = np.ascontiguousarray(x[:8][rng.integers(0, min(8, rows), rows)])
        return x, q, rng.random(rows) < 0.2, rng.permutation(rows).astype(np.uint64) + np.uint64(10**12), 0
    q[0] = 0xFF  # T(q0, row) = popcount(row) / (8 dim): a row's rank in its slice is its number of set bits
    per = -(-rows // 2)
    at = np.arange(rows)
    ones = (at % per) * (8 * dim) // np.minimum(per, rows - at // per * per)
    return np.packbits(rng.permutation(8 * dim)[None, :] < ones[:, None], axis=1), q, None, None, 7


def check(kind, dim, rows, nq, k):
    x, q, dead, ids, base = world(kind, dim, rows, nq)
    with G.GpuCorpus.from_array(x, device=0, index_base=base) as c:
        if dead is not None:
            c.set_tombstones(np.packbits(dead, bitorder="little"))
            c.set_vector_ids(ids)
        res = c.search_tanimoto(q, k)
    assert same(res, reference(q, x, k, dead, ids, base))


def tile_of(dim, nq):
    """the query-tile rule: the smallest of 16 .. 128 that holds the window, capped by the prepared tile's LDS"""
    return min(128 if dim <= 256 else 64, max(16, 1 << (min(nq, 1024) - 1).bit_length()))


@pytest.mark.parametrize("kind", ["spread", "tied", "ascending"])
@pytest.mark.parametrize("dim", [1, 16, 17, 48, 64, 65, 128, 129, 256, 257, 500, 512])
def test_dimensions(dim, kind):
    """tail masks in the first and in a later step, both LDS caps, a chunk tail of zeros; two slices of 550 rows, whose third
    iteration is partial"""
    f = G.tanimoto_form(dim, 17, 10, 1100)
    assert (f.row_slices, f.slice_rows, f.query_tile, f.chunks) == (2, 550, tile_of(dim, 17), (dim + 63) // 64)
    check(kind, dim, 1100, 17, 10)


@pytest.mark.parametrize("rows", [1, 15, 17, 63, 65, 257])
def test_row_counts(rows):
    """partial fragments, partial wave tiles, padding beyond the live rows"""
    check("spread", 48, rows, 3, 10)
    check("tied", 48, rows, 3, 10)


@pytest.mark.parametrize("dim,nq", [(128, n) for n in (1, 15, 16, 17, 33, 127, 128, 129, 1025)] + [(300, n) for n in (63, 64, 65)]
                         + [(512, n) for n in (31, 32, 33)])
def test_query_counts(dim, nq):
    """every tile size, a last tile with idle slots, more tiles than one; 1025 queries are a second window"""
    assert G.tanimoto_form(dim, nq, 10, 300).query_tile == tile_of(dim, nq)
    check("spread", dim, 300, nq, 10)


@pytest.mark.parametrize("dim", [17, 300])
@pytest.mark.parametrize("k", [1, 100, 1024])
def test_k(dim, k):
    check("tied", dim, 1100, 5, k)
    check("ascending", dim, 1100, 5, k)


def first_bits(n, skip=0):
    """a 512-byte vector whose bits skip .. skip + n - 1 are set"""
    at = np.arange(4096)
    return np.packbits((at >= skip) & (at < skip + n))


def test_edges():
    """0 / 0, 4096 / 4096, 1/2 twice, and three fractions next to each other at the format's resolution: with a = 3072,
    c / u = 2727/4090 > 2729/4093 > 2731/4096, each pair cross-adjacent (c1 u2 - c2 u1 = 1, a gap of about 2^-24)"""
    x = random_bits(np.random.default_rng(1), 40, 512)
    x[3], x[20], x[25] = 0, 0xFF, first_bits(1024)
    for row, (c, u) in ((30, (2731, 4096)), (31, (2729, 4093)), (32, (2727, 4090))):
        x[row] = first_bits(c) | first_bits(u - 3072, skip=3072)
    q = np.stack([first_bits(0), first_bits(4096), first_bits(2048), first_bits(3072)])
    with G.GpuCorpus.from_array(x, device=0) as c:
        res = c.search_tanimoto(q, 40)
    assert same(res, reference(q, x, 40))
    assert not res.scores[0].any() and res.indices[0].tolist() == list(range(40))               # 0 / u and 0 / 0: by position
    assert res.indices[1, 0] == 20 and res.scores[1, :1].view(np.uint32)[0] == 0x3F800000         # c = u = 4096
    half = res.indices[2][res.scores[2] == np.float32(0.5)].tolist()
    assert [r for r in half if r in (20, 25)] == [20, 25]                                         # 2048/4096, 1024/2048
    at = {int(r): j for j, r in enumerate(res.indices[3])}
    assert at[32] < at[31] < at[30] and len(set(res.scores[3][[at[30], at[31], at[32]]].tolist())) == 3


def hamming_reference(q, x, k):
    d = np.unpackbits(q[:, None, :] ^ x[None, :, :], axis=2).sum(-1, dtype=np.int64)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    raw = np.take_along_axis(d, order, axis=1).astype(np.int32)
    return raw.astype(np.float32), order.astype(np.uint64), raw


def test_one_handle_several_calls():
    """Tanimoto, Hamming and the device call alternated on one handle: each its own reference, and the Hamming answer the same
    bytes before and after (H1's float-key flag stays clear for it)"""
    import torch
    x, q, _, _, _ = world("spread", 48, 1100, 17)
    k = 10
    with G.GpuCorpus.from_array(x, device=0) as c:
        before = c.search_hamming(q, k)
        host = c.search_tanimoto(q, k)
        after = c.search_hamming(q, k)
        dq = torch.from_numpy(q).cuda()
        ds, di = torch.empty((17, k), dtype=torch.float32, device="cuda"), torch.empty((17, k), dtype=torch.int64, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        c.search_tanimoto_device(dq.data_ptr(), G.UINT8, 48, 17, k, ds.data_ptr(), di.data_ptr(), st.cuda_stream)
        st.synchronize()
        dev = (ds.cpu().numpy().tobytes(), di.cpu().numpy().tobytes())
        ms = c.tanimoto_stage_ms(dq.data_ptr(), G.UINT8, 48, 17, k, ds.data_ptr(), di.data_ptr(), st.cuda_stream)
        again = c.search_hamming(q, k)
    want, ham = reference(q, x, k), hamming_reference(q, x, k)
    assert same(host, want) and host.raw is None and dev == (want[0].tobytes(), want[1].tobytes())
    assert len(ms) == 3 and min(ms) >= 0 and ds.cpu().numpy().tobytes() == want[0].tobytes()
    for res in (before, after, again):
        assert res.indices.tobytes() == ham[1].tobytes() and res.raw.tobytes() == ham[2].tobytes() and res.scores.tobytes() == ham[0].tobytes()


def test_refusals_leave_the_handle_and_the_device_alone():
    x = random_bits(np.random.default_rng(2), 300, 513)
    with G.GpuCorpus.from_array(x, device=0) as c:
        with pytest.raises(E.InvalidArgument, match="rows above 512 packed bytes are not built for Tanimoto search"):
            c.search_tanimoto(x[:2], 5)
    with G.GpuCorpus.from_array(np.ascontiguousarray(x[:, :64]).view(np.int8), device=0) as c:
        with pytest.raises(E.BuildError):
            c.search_tanimoto(x[:2, :64], 5)
    x = np.ascontiguousarray(x[:, :64])
    with G.GpuCorpus.from_array(x, device=0) as c:
        with pytest.raises(E.BuildError):
            c.search_tanimoto(x[:2].view(np.int8), 5)
        with pytest.raises(E.DimensionMismatch):
            c.search_tanimoto(np.ascontiguousarray(x[:2, :63]), 5)
        with pytest.raises(E.InvalidArgument, match="k above 1024 is not built for Tanimoto search"):
            c.search_tanimoto(x[:2], 1025)
        assert same(c.search_tanimoto(x[:2], 5), reference(x[:2], x, 5))
