"""Sign-bit search on the GPU (include/mvf_gpu_signbits.h; DESIGN.md §3 "Sign-bit search", §5 "SQ / S2"): every answer against
a plain numpy reference, byte for byte -- indices, raw scores and score bits, no query left out."""
import functools

import numpy as np
import pytest

from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def reference(q, x, k, dead=None, ids=None, index_base=0):
    """(scores f32, indices u64, raw i32) [nq, k]: the k live rows of largest s, ties by ascending position, then the padding"""
    bits = np.unpackbits(x, axis=1, bitorder="little")
    s = q.astype(np.int64) @ (2 * bits.astype(np.int64) - 1).T
    live = np.arange(len(x)) if dead is None else np.nonzero(~dead)[0]
    name = (np.arange(len(x), dtype=np.uint64) + np.uint64(index_base)) if ids is None else ids
    order = np.argsort(-s[:, live], axis=1, kind="stable")[:, :k]  # stable: equal scores stay in position order
    take = order.shape[1]
    sc, idx, raw = np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), PAD, np.uint64), np.zeros((len(q), k), np.int32)
    raw[:, :take] = np.take_along_axis(s[:, live], order, axis=1)
    sc[:, :take], idx[:, :take] = raw[:, :take].astype(np.float32), name[live[order]]
    return sc, idx, raw


def same(res, want):
    return (res.indices.tobytes() == want[1].tobytes() and res.raw.tobytes() == want[2].tobytes()
            and res.scores.tobytes() == want[0].tobytes())


@functools.lru_cache(maxsize=None)
def world(kind, dim, rows, nq):
    """(x, q, dead, ids, index_base).  spread: random bits and random int8 queries, -128 among them.  tied: rows drawn from 8
    vectors (hundreds of ties at rank k go by position), a fifth deleted, ids permuted.  ascending: for query 0 the rows of each
    of the two slices come worst first, so every row enters its buffer and the buffers settle again and again."""
    rng = np.random.default_rng([0x5347, dim, rows, nq])
    q = rng.integers(-128, 128, (nq, 8 * dim), dtype=np.int8)
    q[:, ::5] = -128
    x = rng.integers(0, 256, (rows, dim), dtype=np.uint8)
    if kind == "spread":
        return x, q, None, None, 1000
    if kind == "tied":
        x = np.ascontiguousarray(x[:8][rng.integers(0, min(8, rows), rows)])
        return x, q, rng.random(rows) < 0.2, rng.permutation(rows).astype(np.uint64) + np.uint64(10**12), 0
    q[0][q[0] == 0] = 1
    per = -(-rows // 2)
    at = np.arange(rows)
    agree = (at % per) * (8 * dim) // np.minimum(per, rows - at // per * per)  # elements of the row on query 0's side
    bits = (rng.permutation(8 * dim)[None, :] < agree[:, None]) == (q[0] > 0)[None, :]
    return np.packbits(bits, axis=1, bitorder="little"), q, None, None, 7


def check(kind, dim, rows, nq, k):
    x, q, dead, ids, base = world(kind, dim, rows, nq)
    with G.GpuCorpus.from_array(x, device=0, index_base=base) as c:
        if dead is not None:
            c.set_tombstones(np.packbits(dead, bitorder="little"))
            c.set_vector_ids(ids)
        res = c.search_signbits(q, k)
    assert same(res, reference(q, x, k, dead, ids, base))


def tile_of(dim, nq):
    """the query-tile rule: the smallest of 16 .. 128 that holds the window, capped by the prepared tile's LDS"""
    cap = 128 if dim <= 128 else 64 if dim <= 256 else 32
    return min(cap, max(16, 1 << (min(nq, 1024) - 1).bit_length()))


@pytest.mark.parametrize("kind", ["spread", "tied", "ascending"])
@pytest.mark.parametrize("dim", [1, 16, 17, 48, 64, 65, 128, 129, 256, 257, 500, 512])
def test_dimensions(dim, kind):
    """tail masks in the first and in a later step, every LDS cap on both sides, a chunk tail of zeros; two slices of 550 rows,
    whose third iteration is partial"""
    f = G.signbits_form(dim, 17, 10, 1100)
    assert f.row_slices == 2 and 550 % 256 and f.query_tile == tile_of(dim, 17) and f.chunks == (dim + 63) // 64
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
    assert G.signbits_form(dim, nq, 10, 300).query_tile == tile_of(dim, nq)
    check("spread", dim, 300, nq, 10)


@pytest.mark.parametrize("dim", [17, 300])
@pytest.mark.parametrize("k", [1, 100, 1024])
def test_k(dim, k):
    check("tied", dim, 1100, 5, k)
    check("ascending", dim, 1100, 5, k)


def test_extremes():
    """the accumulators' and the bias' limits: +-128 x 4096 and +-127 x 4096"""
    x = np.random.default_rng(1).integers(0, 256, (40, 512), dtype=np.uint8)
    x[3], x[20] = 0, 0xFF
    q = np.stack([np.full(4096, -128, np.int8), np.full(4096, 127, np.int8)])
    with G.GpuCorpus.from_array(x, device=0) as c:
        res = c.search_signbits(q, 40)
    assert same(res, reference(q, x, 40))
    assert res.raw[0, [0, -1]].tolist() == [524288, -524288] and res.indices[0, [0, -1]].tolist() == [3, 20]
    assert res.raw[1, [0, -1]].tolist() == [520192, -520192] and res.scores[0, 0] == np.float32(524288)


def hamming_reference(q, x, k):
    d = np.unpackbits(q[:, None, :] ^ x[None, :, :], axis=2).sum(-1, dtype=np.int64)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    raw = np.take_along_axis(d, order, axis=1).astype(np.int32)
    return raw.astype(np.float32), order.astype(np.uint64), raw


@pytest.mark.parametrize("hamming_first", [True, False])
def test_one_handle_both_calls_and_the_device_call(hamming_first):
    import torch
    x, q, _, _, _ = world("spread", 48, 1100, 17)
    hq, k = x[5:9] ^ np.uint8(1), 10
    with G.GpuCorpus.from_array(x, device=0) as c:
        ham = c.search_hamming(hq, k) if hamming_first else None
        host = c.search_signbits(q, k)
        ham = ham or c.search_hamming(hq, k)
        dq = torch.from_numpy(q).cuda()
        ds, dr = torch.empty((17, k), dtype=torch.float32, device="cuda"), torch.empty((17, k), dtype=torch.int32, device="cuda")
        di = torch.empty((17, k), dtype=torch.int64, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        c.search_signbits_device(dq.data_ptr(), G.INT8, 8 * 48, 17, k, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), st.cuda_stream)
        st.synchronize()
        ms = c.signbits_stage_ms(dq.data_ptr(), G.INT8, 8 * 48, 17, k, ds.data_ptr(), di.data_ptr(), st.cuda_stream)
    assert same(host, reference(q, x, k)) and same(ham, hamming_reference(hq, x, k)) and len(ms) == 3 and min(ms) >= 0
    assert di.cpu().numpy().view(np.uint64).tobytes() == host.indices.tobytes()
    assert ds.cpu().numpy().tobytes() == host.scores.tobytes() and dr.cpu().numpy().tobytes() == host.raw.tobytes()


def test_the_unpacked_inner_product_recipe_gives_the_same_answer():
    x, q, _, _, _ = world("spread", 128, 1100, 17)
    pm = (2 * np.unpackbits(x, axis=1, bitorder="little").astype(np.int8) - 1).astype(np.int8)
    with G.GpuCorpus.from_array(x, device=0) as c, G.GpuCorpus.from_array(pm, device=0) as c8:
        res, ip = c.search_signbits(q, 10), c8.search(q, 10, G.INNER_PRODUCT)
    assert res.indices.tobytes() == ip.indices.tobytes() and res.raw.tobytes() == ip.raw.tobytes()


def test_refusals_leave_the_handle_and_the_device_alone():
    x = np.random.default_rng(2).integers(0, 256, (300, 513), dtype=np.uint8)
    q = np.ones((2, 8 * 513), np.int8)
    with G.GpuCorpus.from_array(x, device=0) as c:
        with pytest.raises(E.InvalidArgument, match="rows above 512 packed bytes are not built for sign-bit search"):
            c.search_signbits(q, 5)
        assert same(c.search_hamming(x[:2], 5), hamming_reference(x[:2], x, 5))
    with G.GpuCorpus.from_array(np.ascontiguousarray(x[:, :64]).view(np.int8), device=0) as c:
        with pytest.raises(E.BuildError):
            c.search_signbits(q[:, :512], 5)
    with G.GpuCorpus.from_array(np.ascontiguousarray(x[:, :64]), device=0) as c:
        with pytest.raises(E.BuildError):
            c.search_signbits(q[:, :512].astype(np.uint8), 5)
        with pytest.raises(E.DimensionMismatch):
            c.search_signbits(np.ascontiguousarray(q[:, :504]), 5)
        assert same(c.search_signbits(np.ascontiguousarray(q[:, :512]), 5), reference(q[:, :512], x[:, :64], 5))
