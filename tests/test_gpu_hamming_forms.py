"""-m gpu tests of the Hamming search on every form it can dispatch (DESIGN.md §5 "H0 / H1", "Tested forms"): the 23 scan
kernels -- 15 register forms hamming_reg_kernel<G, QB>, 8 streaming forms hamming_stream_kernel<G, QT> -- through the cases of
tests/_hamming.py's FORM_CELLS, each asserted with the library's form function before it searches, on three corpora: random
rows with near-copy queries, rows drawn from 8 vectors with deletions and permuted ids, and rows that come farthest first,
so that every one enters the selection buffer.  Behind them two device windows (1024 queries and the rest, through the host
call, the device call on a stream of its own and the device call without raw distances), the three paths of the merge H1 --
one round, the bound and one round with the bound entry as the k-th result, the rounds behind a real bound and on full lists
-- with the path predicted from the reference's per-slice lists, and the stage timer.  Every answer is compared with the
numpy reference byte for byte: indices, raw distances and score bits, no query left out.  tests/test_hamming_forms_cpu.py
shows without a device that this data tells the reference from its wrong variants.
Run time on an MI355X: the 42 tests take 2.5 s together, the slowest 1.3 s (the first: it also pays the first use of the
device; every other one at most 0.2 s).  Nothing was cut, and device code is unchanged: the tests pass on the kernels as
they were."""
import numpy as np
import pytest

from metrovector_amd import gpu as G

import _hamming as H

pytestmark = pytest.mark.gpu

CELLS = list(H.FORM_CELLS)


def assert_cell(cell, rows, slices, cus=0):
    """the kernel the case is listed for is the one the launch takes"""
    dim, nq, k = cell
    f = G.hamming_form(dim, nq, k, rows, cus)
    qb = min(f.lanes_per_row, f.query_tile) if f.form == H.REGISTER else f.query_tile
    got = (f.form, f.lanes_per_row, f.query_tile, qb)
    assert got == H.FORM_CELLS[cell], f"{cell}: listed as {H.FORM_CELLS[cell]}, the library says {f}"
    assert f.row_slices == slices, f"{cell}: {rows} rows listed as {slices} slices, the library says {f}"
    return f


def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def corpus_of(w):
    c = G.GpuCorpus.from_array(w.x, device=0, index_base=H.INDEX_BASE)
    if w.dead is not None:
        c.set_tombstones(np.packbits(w.dead, bitorder="little"))
    if w.ids is not None:
        c.set_vector_ids(w.ids)
    return c


@pytest.mark.parametrize("cell", CELLS, ids=[H.cell_id(c) for c in CELLS])
def test_every_scan_kernel_against_numpy(cell):
    dim, nq, k = cell
    rows, slices = H.cell_rows(dim)
    assert_cell(cell, rows, slices, num_cus())
    worlds = H.cell_worlds(cell)
    for builder in H.BUILDERS:
        w = worlds[builder]
        assert w.x.shape == (rows, dim) and w.q.shape == (nq, dim) and (w.dead is not None) == (builder == "tied")
        with corpus_of(w) as c:
            res = c.search_hamming(w.q, k)
        assert H.same(res, H.reference(w.q, w.x, k, w.dead, w.ids, H.INDEX_BASE)), f"{cell}: {builder}"


class DeviceBuffers:
    """queries and result buffers of a device call, the results filled with a pattern no answer holds"""

    def __init__(self, q, k):
        import torch
        self.q = torch.from_numpy(q).cuda()
        self.sc = torch.full((q.shape[0], k), -1.0, dtype=torch.float32, device="cuda")
        self.idx = torch.full((q.shape[0], k), -2, dtype=torch.int64, device="cuda")
        self.raw = torch.full((q.shape[0], k), -3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def bytes(self):
        return self.sc.cpu().numpy().tobytes(), self.idx.cpu().numpy().tobytes(), self.raw.cpu().numpy().tobytes()


@pytest.mark.parametrize("dim,nq", [(16, 1030), (300, 1030), (300, 1027)])
def test_two_device_windows(dim, nq):
    """1024 queries and the rest: the second window's offsets into queries, lists and results, with a query tile of its own
    -- 16 and 8 queries at 16 bytes; at 300 bytes 8 and 8 with six queries left, which is why three left (8 and 4) run too"""
    import torch
    k, rows = 3, 1100
    first, rest = G.hamming_form(dim, 1024, k, rows, num_cus()), G.hamming_form(dim, nq - 1024, k, rows, num_cus())
    assert (first.query_tile, rest.query_tile) == {(16, 1030): (16, 8), (300, 1030): (8, 8), (300, 1027): (8, 4)}[dim, nq]
    assert first.row_slices == rest.row_slices == 2 and first.form == rest.form == (dim > 256)
    w = H.spread(dim, rows, 1030)
    q = np.ascontiguousarray(w.q[:nq])
    want = H.reference(q, w.x, k, index_base=H.INDEX_BASE)
    with corpus_of(w) as c:
        host = c.search_hamming(q, k)
        assert H.same(host, want), "the host call"
        st = torch.cuda.Stream()
        full, bare = DeviceBuffers(q, k), DeviceBuffers(q, k)
        c.search_hamming_device(full.q.data_ptr(), G.UINT8, dim, nq, k, full.sc.data_ptr(), full.idx.data_ptr(), full.raw.data_ptr(), st.cuda_stream)
        c.search_hamming_device(bare.q.data_ptr(), G.UINT8, dim, nq, k, bare.sc.data_ptr(), bare.idx.data_ptr(), 0, st.cuda_stream)
        st.synchronize()
        assert full.bytes() == (host.scores.tobytes(), host.indices.tobytes(), host.raw.tobytes()), "the device call"
        assert bare.bytes()[:2] == full.bytes()[:2], "without d_raw: scores and indices unchanged"
        assert bare.bytes()[2] == np.full((nq, k), -3, np.int32).tobytes(), "without d_raw nothing is written in its place"


@pytest.mark.parametrize("name", list(H.MERGE_CASES))
def test_merge_paths(name):
    """H1 on the path the case is built for, predicted from the reference's per-slice lists before the search"""
    w, slices = H.merge_world(name)
    nq, k = w.q.shape[0], H.MERGE_K
    assert G.hamming_form(16, nq, k, w.x.shape[0], num_cus()).row_slices == slices
    d = H.distances(w.q, w.x)
    assert H.merge_path(H.slice_lists(d[0], k, slices), k) == H.MERGE_CASES[name][1]
    with corpus_of(w) as c:
        res = c.search_hamming(w.q, k)
    assert H.same(res, H.reference(w.q, w.x, k, index_base=H.INDEX_BASE)), name


@pytest.mark.parametrize("cell", [(200, 5, 10), (1100, 3, 10)], ids=H.cell_id)
def test_stage_timer(cell):
    """the timed form fills the buffers as the device call does and reports two times (their size is not asserted)"""
    import torch
    dim, nq, k = cell
    rows, slices = H.cell_rows(dim)
    assert_cell(cell, rows, slices, num_cus())
    w = H.cell_worlds(cell)["spread"]
    with corpus_of(w) as c:
        st = torch.cuda.Stream()
        plain, timed = DeviceBuffers(w.q, k), DeviceBuffers(w.q, k)
        c.search_hamming_device(plain.q.data_ptr(), G.UINT8, dim, nq, k, plain.sc.data_ptr(), plain.idx.data_ptr(), 0, st.cuda_stream)
        ms = c.hamming_stage_ms(timed.q.data_ptr(), G.UINT8, dim, nq, k, timed.sc.data_ptr(), timed.idx.data_ptr(), st.cuda_stream)
        st.synchronize()
        assert len(ms) == 2 and all(np.isfinite(t) and t >= 0.0 for t in ms), ms
        assert timed.bytes() == plain.bytes()
        want = H.reference(w.q, w.x, k, index_base=H.INDEX_BASE)
        assert plain.bytes()[:2] == (want[0].tobytes(), want[1].tobytes())
