"""k-NN join, CPU tier: the C ABI entry points and the Python mirrors exist, refuse bad arguments before any device call,
and the numpy restatement of the semantics (tests/_knn.py; DESIGN.md §3 "Join") is pinned on small corpora whose answers
are worked out by hand -- including that per-shard answers merged by mvfgpu_merge_topk_host give the whole corpus' answer."""
import ctypes as C

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import gpu as G

import _knn as K

INV, BUILD, DIM, DEVICE = 12, 10, 6, 11
PAD = K.PAD
L2, IP, COS = 0, 1, 2


def _call(device=False, corpus=None, qcorpus=None, metric=0, first=0, count=1, k=2, flags=1, sc=True, idx=True):
    room = max(min(count, 16) * min(k, 16), 1)  # the refused calls write nothing, the served ones are small
    s = np.zeros(room, np.float32)
    i = np.zeros(room, np.uint64)
    p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    if device:
        rc = lib.mvfgpu_knn_join_device(corpus, qcorpus, metric, first, count, k, flags, p(s, sc), p(i, idx), None, None)
    else:
        rc = lib.mvfgpu_knn_join(corpus, qcorpus, metric, first, count, k, flags, p(s, sc), p(i, idx), None)
    return rc, lib.mvfgpu_last_error_message().decode()


def test_entry_points_are_exported_and_declared():
    lib = _lib.gpu()
    assert hasattr(lib, "mvfgpu_knn_join") and hasattr(lib, "mvfgpu_knn_join_device")
    assert len(lib.mvfgpu_knn_join.argtypes) == 10 and len(lib.mvfgpu_knn_join_device.argtypes) == 11
    assert hasattr(G.GpuCorpus, "knn_join") and hasattr(G.GpuCorpus, "knn_join_device")
    assert G.JOIN_WINDOW == K.WINDOW == 1024 and G.JOIN_EXCLUDE_SELF == K.EXCLUDE_SELF == 1
    assert callable(M.build_knn_graph) and "build_knn_graph" in M.__all__
    assert lib.mvfgpu_abi_version() == _lib.ABI_VERSION  # additive: the version stays


def test_the_header_and_the_rust_mirror_declare_the_join():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mvf_gpu.h")).read()
    assert "#define MVFGPU_JOIN_WINDOW 1024u" in hdr and "#define MVFGPU_JOIN_EXCLUDE_SELF 1u" in hdr
    assert "int mvfgpu_knn_join(" in hdr and "int mvfgpu_knn_join_device(" in hdr
    rs = open(os.path.join(root, "bindings", "rust", "src", "lib.rs")).read()
    assert "fn mvfgpu_knn_join(" in rs and "fn mvfgpu_knn_join_device(" in rs
    assert "knn_graph" in open(os.path.join(root, "include", "mvf.hpp")).read()


@pytest.mark.parametrize("device", [False, True])
def test_refusals_precede_any_device_call(device):
    """Each refusal arrives with its own code on a box without a GPU too: nothing is asked of a device first."""
    rc, msg = _call(device, corpus=None)
    assert rc == INV and "corpus is NULL" in msg
    rc, msg = _call(device, flags=2)
    assert rc == INV and "flag" in msg
    rc, msg = _call(device, flags=0x80000001)
    assert rc == INV and "flag" in msg
    rc, msg = _call(device, metric=7)
    assert rc == INV and "metric" in msg
    rc, msg = _call(device, k=0)
    assert rc == INV and "k must be" in msg
    rc, msg = _call(device, k=2**31, flags=1)       # with the flag k runs to MVFGPU_MAX_K - 1 ...
    assert rc == INV and "k must be" in msg
    rc, msg = _call(device, k=2**31, flags=0)       # ... without it to MVFGPU_MAX_K: the handle check refuses next
    assert rc == INV and "corpus is NULL" in msg
    rc, msg = _call(device, k=2**31 + 1, flags=0)
    assert rc == INV and "k must be" in msg
    with pytest.raises(M.InvalidArgument):
        _lib.gpu_check(rc)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_refusals_on_a_live_handle(device):
    rows = np.arange(40, dtype=np.float32).reshape(10, 4)
    with G.GpuCorpus.from_array(rows) as c, G.GpuCorpus.from_array(rows[:, :3].copy()) as c3, \
            G.GpuCorpus.from_array(rows.astype(np.float16)) as ch:
        rc, msg = _call(device, c._h, first=5, count=6)
        assert rc == INV and "range" in msg
        rc, msg = _call(device, c._h, first=11, count=0)
        assert rc == INV and "range" in msg
        rc, msg = _call(device, c._h, first=2**63, count=2**63)
        assert rc == INV and "range" in msg
        rc, msg = _call(device, c._h, sc=False)
        assert rc == INV and "NULL" in msg
        rc, msg = _call(device, c._h, idx=False)
        assert rc == INV and "NULL" in msg
        rc, msg = _call(device, c._h, c3._h)
        assert rc == DIM and "Dimension mismatch" in msg
        rc, msg = _call(device, c._h, ch._h)
        assert rc == BUILD and "data type" in msg
        rc, _ = _call(device, c._h, count=0, sc=False, idx=False)  # nothing asked for: nothing needed
        assert rc == 0
        rc, _ = _call(device, c._h, first=10, count=0)
        assert rc == 0
        # a refusal leaves no device error behind: the handle still searches
        assert c.search(rows[:1], 1).indices[0, 0] == 0


def test_valid_arguments_without_a_gpu_are_a_device_error():
    """A join needs a handle, and a handle needs a device: on a box without one the creation says MVF_ERR_DEVICE (as
    every compute entry point does); with one, the same valid arguments are served."""
    lib = _lib.gpu()
    h = C.c_void_p()
    rows = np.arange(16, dtype=np.float32).reshape(4, 4)
    rc = lib.mvfgpu_corpus_create(rows.ctypes.data_as(C.c_void_p), 4, 4, 0, 16, 0, 0, C.byref(h))
    if rc != 0:
        assert rc == DEVICE
        return
    try:
        rc, msg = _call(False, h, count=4, k=2)
        assert rc == 0, msg
    finally:
        lib.mvfgpu_corpus_destroy(h)


# ---- the restatement, on corpora worked out by hand ---------------------------------------------------------------

def _l2(q, x):
    return ((np.asarray(q, np.float64)[:, None, :] - np.asarray(x, np.float64)[None, :, :]) ** 2).sum(-1).astype(np.float32)


def _ip(q, x):
    return (np.asarray(q, np.float64) @ np.asarray(x, np.float64).T).astype(np.float32)


def test_more_than_k_duplicates_at_lower_positions_drop_the_last_entry_not_a_duplicate():
    """Rows 0..4 are one point, row 5 another.  Query row 4, k = 2, L2: the top 3 of all rows is 0, 1, 2 (ties by position) --
    self (4) is not among them, so the LAST entry goes and both answers are duplicates at distance 0."""
    x = np.array([[1.0, 1.0]] * 5 + [[3.0, 3.0]], np.float32)
    S, I, _ = K.join_from_scores(_l2(x, x), L2, 2, np.arange(6))
    assert I[4].tolist() == [0, 1] and S[4].tolist() == [0.0, 0.0]
    assert I[0].tolist() == [1, 2]          # self IS in the top 3 of row 0: removed, the next two stay
    assert I[2].tolist() == [0, 1]
    assert I[5].tolist() == [0, 1] and S[5].tolist() == [8.0, 8.0]
    for i in range(6):
        assert i not in I[i].tolist()


def test_inner_product_where_a_longer_row_outscores_self():
    """Under InnerProduct a row is not its own best match: (1, 0) scores 1 with itself and 5 with (5, 0)."""
    x = np.array([[1.0, 0.0], [5.0, 0.0], [0.0, 2.0], [-1.0, 0.0]], np.float32)
    S, I, _ = K.join_from_scores(_ip(x, x), IP, 2, np.arange(4))
    assert I[0].tolist() == [1, 2] and S[0].tolist() == [5.0, 0.0]      # top 3 of all: 1 (5), 0 (1, self), 2 (0)
    assert I[1].tolist() == [0, 2] and S[1].tolist() == [5.0, 0.0]      # top 3: 1 (25, self), 0 (5), 2 (0)
    assert I[2].tolist() == [0, 1] and S[2].tolist() == [0.0, 0.0]      # top 3: 2 (4, self), 0 (0), 1 (0)
    assert I[3].tolist() == [2, 0] and S[3].tolist() == [0.0, -1.0]     # top 3: 3 (1, self), 2 (0), 0 (-1)
    S0, I0, _ = K.join_from_scores(_ip(x, x), IP, 2, np.arange(4), exclude=False)
    assert I0[0].tolist() == [1, 0] and I0[3].tolist() == [3, 2]        # without the flag self is a result like any other


def test_a_nan_row_as_query_and_as_neighbour():
    x = np.array([[0.0], [np.nan], [1.0], [3.0]], np.float32)
    S, I, _ = K.join_from_scores(_l2(x, x), L2, 3, np.arange(4))
    # row 0: distances 0 (self), NaN, 1, 9 -> 2, 3, then the NaN row last
    assert I[0].tolist() == [2, 3, 1] and S[0][:2].tolist() == [1.0, 9.0] and np.isnan(S[0][2])
    # the NaN row as a query: every score is NaN, the order is by position, self (1) is removed by POSITION
    assert I[1].tolist() == [0, 2, 3] and np.isnan(S[1]).all()
    # k = 2: its top 3 by position is 0, 1, 2 -> self removed -> 0, 2
    _, I2, _ = K.join_from_scores(_l2(x, x), L2, 2, np.arange(4))
    assert I2[1].tolist() == [0, 2]


def test_duplicate_ids_on_duplicate_rows_exclusion_is_by_position():
    """Rows 0 and 1 are the same point and carry the same id 7: row 0's nearest other row is row 1, reported as id 7."""
    x = np.array([[2.0], [2.0], [5.0]], np.float32)
    ids = np.array([7, 7, 9], np.uint64)
    S, I, _ = K.join_from_scores(_l2(x, x), L2, 2, np.arange(3), c_ids=ids)
    assert I[0].tolist() == [7, 9] and S[0].tolist() == [0.0, 9.0]
    assert I[1].tolist() == [7, 9] and S[1].tolist() == [0.0, 9.0]
    assert I[2].tolist() == [7, 7]


def test_k_at_least_the_live_rows_pads_and_a_deleted_query_row_is_all_padding():
    x = np.array([[0.0], [1.0], [2.0], [4.0]], np.float32)
    dead = np.array([False, False, True, False])
    for metric, pad in ((L2, np.inf), (IP, -np.inf)):
        sc = _l2(x, x) if metric == L2 else _ip(x, x)
        S, I, R = K.join_from_scores(sc, metric, 4, np.arange(4), c_dead=dead, q_dead=dead)
        assert I[2].tolist() == [PAD] * 4 and (S[2] == pad).all() and (R[2] == 0).all()   # the deleted query row
        assert I[0][2:].tolist() == [PAD, PAD] and (S[0][2:] == pad).all()                  # two live others, then padding
        assert 2 not in I.tolist()[0] + I.tolist()[1] + I.tolist()[3]                        # the deleted row is nobody's neighbour
    S, I, _ = K.join_from_scores(_l2(x, x), L2, 4, np.arange(4), c_dead=dead, q_dead=dead)
    assert I[0][:2].tolist() == [1, 3] and I[3][:2].tolist() == [1, 0]


def test_two_handles_overlapping_and_disjoint_ranges():
    """C holds global positions 10..15, Q a window of the same rows: overlapping ranges exclude by GLOBAL position; disjoint
    ranges leave the flag without effect and k' = k."""
    xc = np.arange(6, dtype=np.float32)[:, None]
    # Q = rows at global positions 12..14 (index_base 12), values equal to C's local rows 2..4
    xq = xc[2:5]
    assert K.k_prime(2, True, 12, 3, 10, 6) == 3 and K.k_prime(2, False, 12, 3, 10, 6) == 2
    S, I, _ = K.join_from_scores(_l2(xq, xc), L2, 2, np.arange(12, 15), q_span=(12, 3), c_index_base=10)
    assert I.tolist() == [[11, 13], [12, 14], [13, 15]]
    # the same values under a disjoint range (Q at 100..102): k' = k, self-valued rows are reported at distance 0
    assert K.k_prime(2, True, 100, 3, 10, 6) == 2
    S, I, _ = K.join_from_scores(_l2(xq, xc), L2, 2, np.arange(100, 103), q_span=(100, 3), c_index_base=10)
    assert I.tolist() == [[12, 11], [13, 12], [14, 13]] and S[:, 0].tolist() == [0.0, 0.0, 0.0]
    # ranges that touch but do not meet: Q = [4, 10), C = [10, 16)
    assert not K.ranges_meet(4, 6, 10, 6) and K.ranges_meet(4, 7, 10, 6)


def test_the_removal_rule_on_lists():
    s = np.array([0.0, 0.5, 1.0, 2.0], np.float32)
    i = np.array([3, 9, 4, 1], np.uint64)
    r = np.array([5, 6, 7, 8], np.int32)
    S, I, R = K.remove_self(s, i, r, 9, 3, L2)
    assert I.tolist() == [3, 4, 1] and S.tolist() == [0.0, 1.0, 2.0] and R.tolist() == [5, 7, 8]
    S, I, R = K.remove_self(s, i, r, 77, 3, L2)          # self not among the k': the last entry goes
    assert I.tolist() == [3, 9, 4] and R.tolist() == [5, 6, 7]
    S, I, R = K.remove_self(s, i, r, 9, 4, L2)           # k' = k: nothing is removed
    assert I.tolist() == [3, 9, 4, 1]
    ip = np.array([3, 9, PAD, PAD], np.uint64)           # padding stays padding, ids apply to real entries only
    S, I, R = K.remove_self(s, ip, r, 3, 3, L2, c_index_base=2, c_ids=np.arange(100, 110, dtype=np.uint64))
    assert I.tolist() == [107, PAD, PAD]
    assert K.windows(5, 2050) == [(5, 1024), (1029, 1024), (2053, 2)] and K.windows(0, 0) == []


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_per_shard_answers_merged_on_the_host_give_the_whole_answer(metric):
    """For each shard as Q: join against every shard as C with the flag, merge the lists in ascending row-range order
    (mvfgpu_merge_topk_host needs no GPU) == the whole corpus' self-join.  Self is removed in exactly one of the lists."""
    rng = np.random.default_rng(3 + metric)
    n, dim, k = 90, 5, 7
    x = rng.integers(-3, 4, size=(n, dim)).astype(np.float32)   # small integers: many exact ties, exact f32 scores
    x[40] = x[3]
    x[41] = x[3]
    x[80] = x[3]
    if metric == L2:
        full = _l2(x, x)
    elif metric == IP:
        full = _ip(x, x)
    else:
        nrm = np.sqrt((x.astype(np.float64) ** 2).sum(1))
        den = nrm[:, None] * nrm[None, :]
        full = np.where(den > 0, (x.astype(np.float64) @ x.astype(np.float64).T) / np.where(den > 0, den, 1), 0).astype(np.float32)
    dead = np.zeros(n, bool)
    dead[[5, 41, 77]] = True
    want = K.join_from_scores(full, metric, k, np.arange(n), c_dead=dead, q_dead=dead)
    bounds = [0, 25, 60, 90]
    for qs in range(3):
        q0, q1 = bounds[qs], bounds[qs + 1]
        Ss, Is, Rs = [], [], []
        for cs in range(3):
            c0, c1 = bounds[cs], bounds[cs + 1]
            S, I, R = K.join_from_scores(full[q0:q1, c0:c1], metric, k, np.arange(q0, q1), q_span=(q0, q1 - q0), c_index_base=c0,
                                         c_dead=dead[c0:c1], q_dead=dead[q0:q1])
            Ss.append(S), Is.append(I), Rs.append(R)
        m = G.merge_topk_host(np.stack(Ss), np.stack(Is), np.stack(Rs), metric, G.FLOAT32)
        live = ~dead[q0:q1]
        assert (m.indices[live] == want[1][q0:q1][live]).all()
        assert (m.scores[live].view(np.uint32) == want[0][q0:q1][live].view(np.uint32)).all()
        assert (m.indices[~live] == PAD).all()
