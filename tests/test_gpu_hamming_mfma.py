"""-m gpu tests of the Hamming search's MFMA route (include/mvf_gpu_hamming_route.h; DESIGN.md §5 "HQ / H2"): route 2 forced on the
handle, every answer compared with the numpy reference of tests/_hamming.py byte for byte -- indices, raw distances, score bits."""
import numpy as np
import pytest

from metrovector_amd import gpu as G

import _hamming as H

pytestmark = pytest.mark.gpu


def world(builder, dim, rows, nq, k):
    if builder == "descending":  # farthest first inside each of the launch's slices
        return H.descending(dim, rows, nq, G.hamming_mfma_form(dim, nq, k, rows).row_slices)
    return getattr(H, builder)(dim, rows, nq)


def corpus_of(w, route=2):
    c = G.GpuCorpus.from_array(w.x, device=0, index_base=H.INDEX_BASE)
    if w.dead is not None:
        c.set_tombstones(np.packbits(w.dead, bitorder="little"))
    if w.ids is not None:
        c.set_vector_ids(w.ids)
    c.set_hamming_route(route)
    return c


def check(w, k):
    dim = w.x.shape[1]
    assert G.hamming_route(dim, min(w.q.shape[0], 1024), k, w.x.shape[0], 2) == 2
    with corpus_of(w) as c:
        res = c.search_hamming(w.q, k)
    assert H.same(res, H.reference(w.q, w.x, k, w.dead, w.ids, H.INDEX_BASE))


@pytest.mark.parametrize("builder", H.BUILDERS)
@pytest.mark.parametrize("dim", [1, 16, 17, 48, 100, 128, 256, 257, 500, 512])
def test_dimensions(dim, builder):
    """a tail mask in the first step and in a later one, full steps, both tile forms, the largest eligible row; two slices of 550
    rows with a partial last iteration; `tied`: deletions, ids, ties at rank k; `descending`: every row enters, repeated settles"""
    assert G.hamming_mfma_form(dim, 17, 10, 1100).row_slices == 2
    check(world(builder, dim, 1100, 17, 10), 10)


@pytest.mark.parametrize("rows", [1, 15, 17, 63, 65, 257])
def test_row_counts(rows):
    """partial fragments, partial wave tiles, a partial block iteration; k beyond the live rows pads"""
    check(H.spread(48, rows, 5), 10)


@pytest.mark.parametrize("dim,rows,nq", [(128, 1100, nq) for nq in (1, 15, 16, 127, 128, 129)] + [(300, 1100, nq) for nq in (63, 64, 65)]
                         + [(128, 300, 1025)])
def test_query_counts(dim, rows, nq):
    """idle query columns and a second tile on both sides of the tile of 128 and of 64; 1025 queries: a second window"""
    assert G.hamming_mfma_form(dim, nq, 10, rows).query_tile == (128 if dim <= 256 else 64)
    check(H.spread(dim, rows, nq), 10)


@pytest.mark.parametrize("dim,k,rows", [(d, k, 1100) for d in (17, 300) for k in (1, 100, 1024)] + [(17, 1024, 166400)])
def test_list_lengths(dim, k, rows):
    """every row enters: buffers of 512 entries settle every second iteration; the last case's 64 slices of 2600 rows fill the
    2048 entries of k = 1024 and settle them before the slice ends"""
    if rows > 1100:
        f = G.hamming_mfma_form(dim, 3, k, rows)
        assert f.slice_rows > 2 * 1024 + H.STEP_ROWS and f.row_slices == 64
    check(world("descending", dim, rows, 3, k), k)


def test_accumulator_extremes():
    """4096 bits: all-ones rows against an all-zeros query (d = 4096 from a start of 0) and the reverse (a start of 4096); ones
    against ones take the partial sums to -4096"""
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, (300, 512), dtype=np.uint8)
    x[::3], x[1::3] = 0xFF, 0
    q = np.stack([np.zeros(512, np.uint8), np.full(512, 0xFF, np.uint8), x[2]])
    with corpus_of(H.World(x, q, None, None)) as c:
        res = c.search_hamming(q, 300)
    assert int(res.raw.max()) == 4096 and int(res.raw.min()) == 0
    assert H.same(res, H.reference(q, x, 300, index_base=H.INDEX_BASE))


def test_an_ineligible_handle_stays_on_route_1():
    w = H.spread(513, 300, 5)
    assert G.hamming_route(513, 5, 10, 300, 2) == 1
    with corpus_of(w) as c:
        assert H.same(c.search_hamming(w.q, 10), H.reference(w.q, w.x, 10, index_base=H.INDEX_BASE))


def test_routes_back_to_back_the_device_call_and_the_handle_afterwards():
    import torch
    w, k = H.tied(48, 3001, 20), 100
    with corpus_of(w, route=1) as c:
        before = c.search(w.q, k, G.L2)
        one = c.search_hamming(w.q, k)
        c.set_hamming_route(2)
        two = c.search_hamming(w.q, k)
        dq = torch.from_numpy(w.q).cuda()
        ds = torch.empty((20, k), dtype=torch.float32, device="cuda")
        di = torch.empty((20, k), dtype=torch.int64, device="cuda")
        dr = torch.empty((20, k), dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        c.search_hamming_device(dq.data_ptr(), G.UINT8, 48, 20, k, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), st.cuda_stream)
        st.synchronize()
        after = c.search(w.q, k, G.L2)
    want = H.reference(w.q, w.x, k, w.dead, w.ids, H.INDEX_BASE)
    assert H.same(one, want) and H.same(two, want)
    assert (ds.cpu().numpy().tobytes(), di.cpu().numpy().tobytes(), dr.cpu().numpy().tobytes()) == tuple(a.tobytes() for a in want)
    assert H.same(after, (before.scores, before.indices, before.raw))
