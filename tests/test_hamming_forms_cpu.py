"""The Hamming search's forms, CPU tier (DESIGN.md §5 "H0 / H1", "Tested forms"): what makes tests/test_gpu_hamming_forms.py
worth its run is checked here, without a device.  tests/_hamming.py's hand-written FORM_CELLS against the library's form
function and against the 23 scan kernels the launch can pick; every wrong model -- a reference with one of the mistakes a
kernel form could make -- told apart from the reference on the corpora the GPU test runs for that cell, every left-out
16-byte step on the random corpus; merge_path's prediction for each merge case with the figures that make it so; and the
property that makes the farthest-first corpus the worst case of the selection."""
import bisect

import numpy as np
import pytest

from metrovector_amd import gpu as G

import _hamming as H

CELLS = list(H.FORM_CELLS)
CELL_IDS = [H.cell_id(c) for c in CELLS]

# DESIGN.md §5 "H0 / H1": the register form has G = next_pow2(pitch / 16) <= 16 lanes and reduces QB = min(G, QT) queries at a
# time, QT a power of two up to 16; the streaming form has 32 or 64 lanes and tiles of up to 8 queries.
REGISTER_KERNELS = {(H.REGISTER, g, qb) for g in (1, 2, 4, 8, 16) for qb in (1, 2, 4, 8, 16) if qb <= g}
STREAMING_KERNELS = {(H.STREAMING, g, qt) for g in (32, 64) for qt in (1, 2, 4, 8)}


def kernel_of(form, g, qt, qb):
    """the instantiation's own parameters: hamming_reg_kernel<G, QB> or hamming_stream_kernel<G, QT>"""
    return (form, g, qb if form == H.REGISTER else qt)


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_the_table_is_what_the_library_decides(cell):
    dim, nq, k = cell
    rows, slices = H.cell_rows(dim)
    for cus in (0, 64, 256, 304):
        f = G.hamming_form(dim, nq, k, rows, cus)
        qb = min(f.lanes_per_row, f.query_tile) if f.form == H.REGISTER else f.query_tile  # the kernel's own rule
        assert (f.form, f.lanes_per_row, f.query_tile, qb) == H.FORM_CELLS[cell], f"{cell} is listed as {H.FORM_CELLS[cell]}: {f}"
        assert f.row_slices == slices, f"{cell}: {rows} rows are listed as {slices} slices: {f}"
    steps = (dim + 15) // 16
    if f.form == H.REGISTER:
        assert f.lanes_per_row == H.next_pow2(steps)
    else:
        assert steps > 16 and f.lanes_per_row == (32 if steps <= 32 else 64)


def test_the_table_reaches_the_23_scan_kernels_and_no_other():
    assert len(REGISTER_KERNELS) == 15 and len(STREAMING_KERNELS) == 8
    reached = {kernel_of(*v) for v in H.FORM_CELLS.values()}
    want = REGISTER_KERNELS | STREAMING_KERNELS
    assert reached == want, f"no case for {sorted(want - reached)}, no kernel for {sorted(reached - want)}"
    steps = {(v[1], (c[0] + 15) // 16) for c, v in H.FORM_CELLS.items()}
    for g, idle in ((4, 3), (8, 7), (16, 10), (16, 13), (32, 19), (64, 69)):
        assert (g, idle) in steps, f"no case of {idle} steps on {g} lanes"
    for g, dim in ((4, 64), (8, 128), (16, 256), (32, 512)):
        assert any(c[0] == dim and v[1] == g for c, v in H.FORM_CELLS.items()), f"the full group of {dim} bytes is not listed"
    idle_slot = {kernel_of(*v) for c, v in H.FORM_CELLS.items() if c[1] % v[2]}
    for kernel in want:  # (a tile of two that is not full is a tile of one)
        tiles = {v[2] for v in H.FORM_CELLS.values() if kernel_of(*v) == kernel}
        assert max(tiles) <= 2 or kernel in idle_slot, f"{kernel}: no case leaves a query slot of its tile idle"
    assert H.FORM_CELLS[150, 9, 600][3] == 4 and H.FORM_CELLS[200, 3, 10][3] == 4, "QB = 4 on 16 lanes: by k and by nq"


def test_select_is_the_reference_on_a_distance_matrix():
    for w in H.cell_worlds((40, 3, 10)).values():
        for k in (1, 10, 1024):
            assert H.same_answers(H.select(H.distances(w.q, w.x), k, w.dead, w.ids, 7), H.reference(w.q, w.x, k, w.dead, w.ids, 7))
        part = H.step_distances(w.q, w.x)
        assert part.shape[2] == 3 and (part.sum(-1) == H.distances(w.q, w.x)).all()
        assert (part[:, :, 2] == H.distances(w.q[:, 32:], w.x[:, 32:])).all()
    rev = H.select(np.array([[5, 3, 5, 3, 9]]), 4, last_first=True)
    assert rev[1].tolist() == [[3, 1, 2, 0]] and rev[2].tolist() == [[3, 3, 5, 5]]
    assert H.tail_rows(1100, 2).nonzero()[0].tolist() == list(range(512, 550)) + list(range(1062, 1100))
    assert H.tail_rows(64, 1).all() and not H.tail_rows(1024, 2).any()


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_wrong_models_are_told_apart(cell):
    """each wrong model answers differently from the reference on one at least of the cell's corpora.  The exchange of
    neighbouring queries needs two queries; a one-query cell has no batch to mix up."""
    dim, nq, k = cell
    slices = H.cell_rows(dim)[1]
    worlds = H.cell_worlds(cell)
    told = {name: [] for name in H.WRONG_MODELS}
    for builder in H.BUILDERS:
        w = worlds[builder]
        d = H.distances(w.q, w.x)
        ref = H.select(d, k, w.dead, w.ids, H.INDEX_BASE)
        for name, (model, least_nq) in H.WRONG_MODELS.items():
            if nq >= least_nq and not H.same_answers(model(d, k, w, slices), ref):
                told[name].append(builder)
    for name, (model, least_nq) in H.WRONG_MODELS.items():
        assert least_nq in (1, 2)
        assert told[name] or nq < least_nq, f"{cell}: no corpus tells '{name}' from the reference"
    assert "tied" in told["ties by descending position"] and "tied" in told["tombstones ignored"] and "tied" in told["tombstones looked up by id"]
    assert "descending" in told["partial last iteration lost"]


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_every_left_out_step_differs_on_the_random_corpus(cell):
    dim, nq, k = cell
    w = H.cell_worlds(cell)["spread"]
    part = H.step_distances(w.q, w.x)
    assert part.shape[2] == (dim + 15) // 16
    ref = H.select(part.sum(-1), k, None, None, H.INDEX_BASE)
    same = [s for s in range(part.shape[2]) if H.same_answers(H.wrong_step_left_out(part, s, k, w), ref)]
    assert not same, f"{cell}: leaving out steps {same} changes nothing"


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_farthest_first_every_row_enters(cell):
    """for query 0 every row's composite is below the k-th best of the rows in front of it in its slice"""
    dim, nq, k = cell
    rows, slices = H.cell_rows(dim)
    w = H.cell_worlds(cell)["descending"]
    d = H.distances(w.q[:1], w.x)[0]
    per = -(-rows // slices)
    for lo in range(0, rows, per):
        n_s = min(lo + per, rows) - lo
        assert (np.diff(d[lo:lo + per]) <= 0).all() and d[lo] == dim * 8 and d[lo + n_s - 1] == -(-(dim * 8 + 1) // n_s) - 1
        best = []  # the k smallest composites so far, ascending
        for r in range(lo, min(lo + per, rows)):
            comp = (int(d[r]) << 32) | r
            assert len(best) < k or comp < best[k - 1], f"{cell}: row {r} does not enter"
            bisect.insort(best, comp)
            del best[k:]


def _lists(name):
    w, slices = H.merge_world(name)
    d = H.distances(w.q, w.x)
    return w, slices, d, [H.slice_lists(d[j], H.MERGE_K, slices) for j in range(w.q.shape[0])]


@pytest.mark.parametrize("name", list(H.MERGE_CASES))
def test_merge_cases_take_their_paths(name):
    w, slices, d, lists = _lists(name)
    rows, k = w.x.shape[0], H.MERGE_K
    assert rows % slices == 0 and all(c.size == min(k, rows // slices) for c in lists[0])
    capped = min(-(-rows // H.SLICE_ROWS), H.MERGE_MAX // H.next_pow2(k))  # by the rows or by what H1 merges, never by the CUs
    assert slices == capped
    for cus in (64, 256, 304):
        assert G.hamming_form(16, w.q.shape[0], k, rows, cus).row_slices == slices, cus
    assert H.merge_path(lists[0], k) == H.MERGE_CASES[name][1]
    bound, below = H.merge_bound(lists[0], k)
    ref = H.select(d, k, None, None, H.INDEX_BASE)
    for j, per_slice in enumerate(lists):
        answer = H.merged(per_slice, k)
        assert H.same_answers(H.answer_of(answer, k, None, H.INDEX_BASE), tuple(a[j:j + 1] for a in ref)), "the merge of the lists is the reference"
    answer = H.merged(lists[0], k)
    if name.startswith("dense"):
        assert below == 64 * 1023 + 1 > H.MERGE_LDS and bound >> np.uint64(32) > 32, "a far row bounds, and nearly everything lies below it"
        assert bound not in answer and set((answer >> np.uint64(32)).tolist()) == {0, 1}
        assert set(((answer & np.uint64(0xFFFFFFFF)) // np.uint64(1032)).tolist()) == set(range(64)), "rows of every slice"
    elif name == "one-slice":
        assert below == k and answer[k - 1] == bound, "the bound entry is the k-th result"
        assert set(((answer & np.uint64(0xFFFFFFFF)) // np.uint64(1032)).tolist()) == {37}
    elif name == "edge-16-slices":
        assert slices * H.next_pow2(k) == H.MERGE_LDS, "exactly one round's entries"
    else:
        assert slices * H.next_pow2(k) == H.MERGE_LDS + 1024 and below > H.MERGE_LDS
        assert (answer & np.uint64(0xFFFFFFFF) >= np.uint64(16 * 1024)).any(), "rows of the last slice are in the answer"


def test_merge_models_are_told_apart():
    told = {m: [] for m in H.MERGE_MODELS}
    for name in H.MERGE_CASES:
        w, slices, d, lists = _lists(name)
        for m in H.MERGE_MODELS:
            if H.merged(lists[0], H.MERGE_K, m).tobytes() != H.merged(lists[0], H.MERGE_K).tobytes():
                told[m].append(name)
    assert {"dense-nq1", "dense-nq2", "one-slice", "edge-17-slices"} <= set(told["first round only"]), told
    assert told["bound dropped"] == ["one-slice"], told
    # (with `<` the dense case still counts more than one round's entries below its bound and sorts everything, rightly)
