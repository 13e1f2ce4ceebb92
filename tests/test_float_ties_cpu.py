"""The duplicate-row corpora of tests/_dups.py without a GPU: the exact expectation of corpus B against the oracle (strict-order
f32, an implementation that shares nothing with _dups.py), the share of clear queries in every case tests/test_gpu_float_ties.py
runs, the properties on the oracle's own answers, and planted faults that the checkers have to reject."""
import numpy as np
import pytest

import _dups as D
from _util import PAD, assert_float_topk

METRICS = (0, 1, 2)


def cp_small(name):
    return D.B_SHAPES[name][2] <= 32


def _oracle_live(oracle, cp, metric, q, k, live):
    """oracle.search over the live rows, mapped back to positions."""
    pos = np.nonzero(live)[0]
    sc, idx, _ = oracle.search(np.ascontiguousarray(cp.rows[pos]), cp.dtype, metric, q, k)
    real = idx != PAD
    out = np.full(idx.shape, PAD, np.uint64)
    out[real] = pos[idx[real].astype(np.int64)].astype(np.uint64)
    return sc, out


@pytest.mark.parametrize("name", ["n20k_d200", "n20k_d32"])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("tomb", [False, True])
def test_corpus_b_expectation_is_the_oracles_answer_on_every_clear_query(oracle, name, dtype, tomb):
    cp, q = D.get_b(name, dtype), D.get_queries(name)[:48 if cp_small(name) else 24]  # (the share over all 200 queries is asserted below)
    live = ~D.get_dead(name) if tomb else np.ones(cp.n, bool)
    for metric in METRICS:
        for k in (1, 7, 100, 1000):
            sc, got = _oracle_live(oracle, cp, metric, q, k, live)
            want = D.expected_topk(cp, metric, q, k, live)
            clear = D.clear_queries(cp, metric, q, k, live)
            assert clear.mean() >= 0.75
            for i in np.nonzero(clear)[0]:
                r = D.first_difference(got[i], want[i])
                assert r is None, f"{name} dtype {dtype} metric {metric} k {k} query {i}: rank {r}: oracle {got[i][r]}, expected {want[i][r]}"
            for i in range(0, len(q), 9):
                D.assert_dup_properties(metric, sc[i], got[i], cp.group_of, live, k, what=f"{name} metric {metric} k {k} query {i}")


@pytest.mark.parametrize("name,kind,ks", D.CLEAR_CASES)
@pytest.mark.parametrize("dtype", [0, 1])
def test_clear_share_of_every_case_the_gpu_file_runs(name, kind, ks, dtype):
    """A condition on the inputs, not a measurement of the library: at least 75 % of the shape's 200 queries are clear for
    every metric, k and set of live rows the GPU file uses, and so is one of the first ten (one- to five-query cases)."""
    cp, q = D.get_b(name, dtype), D.get_queries(name)
    live = D.get_live(name, kind, cp)
    for metric in METRICS:
        for k in ks:
            clear = D.clear_queries(cp, metric, q, k, live)
            assert clear.mean() >= 0.75, f"{name} dtype {dtype} {kind} metric {metric} k {k}: clear share {clear.mean():.2f}"
            assert clear[:10].any(), f"{name} dtype {dtype} {kind} metric {metric} k {k}: none of the first ten queries is clear"


@pytest.mark.parametrize("dtype", [0, 1])
def test_clear_share_of_the_join_window(dtype):
    """The join's queries are stored rows: L2 between the distinct vectors, the query's own vector at distance 0."""
    cp = D.get_b("n20k_d200", dtype)
    window = cp.rows[D.JOIN_FIRST:D.JOIN_FIRST + D.JOIN_COUNT].astype(np.float32)
    assert np.unique(cp.group_of[D.JOIN_FIRST:D.JOIN_FIRST + D.JOIN_COUNT]).size >= 8, "the window holds copies of several groups"
    for k in D.JOIN_KS:
        assert D.clear_queries(cp, 0, window, k + 1).mean() >= 0.75


@pytest.mark.parametrize("name", sorted(D.A_SHAPES))
@pytest.mark.parametrize("dtype", [0, 1])
def test_corpus_a_properties_hold_on_the_oracles_answers(oracle, name, dtype):
    cp, q = D.get_a(oracle, name, dtype), D.get_queries(name)[:12]
    sizes = cp.sizes()
    assert 0.27 * cp.n <= (sizes - 1).sum() <= 0.33 * cp.n and sizes.max() == 40 and sizes[cp.zero_group] == 40
    zero = cp.rows[cp.group_of == cp.zero_group]
    assert (zero == 0).all() and np.signbit(zero[:, 0]).sum() == 20
    for g in (1, 2, 3):  # scattered: no group sits in one corner of the position range
        m = np.nonzero(cp.group_of == g)[0]
        assert (cp.rows[m] == cp.rows[m[0]]).all() and (m.size < 8 or m.max() - m.min() > cp.n // 4)
    dead = D.get_dead(name)
    for live in (np.ones(cp.n, bool), ~dead):
        for metric in METRICS:
            for k in (7, 1000):
                sc, got = _oracle_live(oracle, cp, metric, q, k, live)
                for i in range(len(q)):
                    D.assert_dup_properties(metric, sc[i], got[i], cp.group_of, live, k, what=f"A {name} metric {metric} k {k} query {i}")


def test_helpers():
    cp = D.get_b("n20k_d200", 0)
    sizes = sorted(cp.sizes().tolist())
    assert sizes[:9] == list(D.SKEWED[:9]) and 400 in sizes and sizes[-1] == 20_000 // 6 and len(sizes) == D.D_VECTORS
    cuts = D.shard_cuts(cp)
    assert len(cuts) == 4
    big = np.argsort(cp.sizes())[::-1][:2]
    for i, c in enumerate(cuts[1:-1], 1):  # a copy of a large group ends the shard, others follow
        g = big[i % 2]
        assert cp.group_of[c - 1] == g and (cp.group_of[c:] == g).any()
    ids = D.permuted_ids(5, cp.n)
    assert np.unique(ids).size == cp.n
    some = np.array([5, 0, cp.n - 1], np.uint64)
    assert (D.positions_of_ids(ids, np.concatenate([ids[some.astype(np.int64)], [PAD]])) == np.concatenate([some, [PAD]])).all()
    allow = D.get_allow("n20k_d200", cp)
    admitted = np.bincount(cp.group_of[allow], minlength=D.D_VECTORS)
    assert (admitted == (cp.sizes() + 1) // 2).all()
    assert abs(D.get_dead("n20k_d200").mean() - 0.2) < 1e-3


# ---- planted faults ----------------------------------------------------------------------------------------------------

N_F, DIM_F = 2000, 16


@pytest.fixture(scope="module")
def planted(oracle):
    """Corpus B with two groups made special: the group of 5 copies holds a NaN, the group of 8 copies lies beyond the f32
    range of L2 (+inf).  The correct answer is the oracle's."""
    cp = D.corpus_b(77, N_F, DIM_F, 0)
    sizes = cp.sizes()
    g_nan, g_inf = int(np.nonzero(sizes == 5)[0][0]), int(np.nonzero(sizes == 8)[0][0])
    rows = cp.rows.copy()
    rows[cp.group_of == g_nan, 0] = np.nan
    rows[cp.group_of == g_inf] = 3.0e38
    q = D.gaussian_queries(78, 1, DIM_F)
    all_scores = oracle.scores(rows, 0, 0, q[0])[0]
    assert np.isnan(all_scores[cp.group_of == g_nan]).all() and np.isposinf(all_scores[cp.group_of == g_inf]).all()
    return cp, rows, q, all_scores, g_nan, g_inf


def _answer(oracle, planted, k):
    cp, rows, q, all_scores, _, _ = planted
    sc, idx, _ = oracle.search(rows, 0, 0, q, k)
    return sc[0].copy(), idx[0].copy()


def _both(planted, sc, idx, k):
    cp, rows, q, all_scores, _, _ = planted
    live = np.ones(cp.n, bool)
    return (lambda: D.assert_dup_properties(0, sc, idx, cp.group_of, live, k),
            lambda: assert_float_topk(0, sc, idx, all_scores, rows, q[0], k))


def _cut_k(planted):
    """A k that cuts the list inside a group: at least two of its copies returned, at least one not."""
    cp, rows, q, all_scores, _, _ = planted
    order = np.lexsort((np.arange(cp.n), all_scores))
    g = cp.group_of[order]
    for k in range(60, 900):
        inside = g[:k] == g[k - 1]
        if g[k] == g[k - 1] and inside.sum() >= 2 and g[0] != g[k - 1]:
            return k
    raise AssertionError("no such k")


def test_the_correct_answers_pass(oracle, planted):
    for k in (N_F, _cut_k(planted), 7):
        sc, idx = _answer(oracle, planted, k)
        for check in _both(planted, sc, idx, k):
            check()


def test_fault_two_entries_of_equal_score_swapped(oracle, planted):
    k = _cut_k(planted)
    sc, idx = _answer(oracle, planted, k)
    assert sc[k - 1] == sc[k - 2]
    idx[[k - 2, k - 1]] = idx[[k - 1, k - 2]]
    dup, topk = _both(planted, sc, idx, k)
    with pytest.raises(AssertionError, match="order breaks at rank"):
        dup()
    with pytest.raises(AssertionError, match="not sorted best-first, ties by position"):
        topk()


def test_fault_a_groups_first_copy_replaced_by_a_later_unreturned_one(oracle, planted):
    cp = planted[0]
    k = _cut_k(planted)
    sc, idx = _answer(oracle, planted, k)
    g = cp.group_of[idx[k - 1]]
    ranks = np.nonzero(cp.group_of[idx.astype(np.int64)] == g)[0]
    members = np.nonzero(cp.group_of == g)[0]
    later = members[members > idx[k - 1]][0]
    idx[ranks] = np.concatenate([idx[ranks][1:], [np.uint64(later)]])  # still ascending in position, still one score
    dup, topk = _both(planted, sc, idx, k)
    with pytest.raises(AssertionError, match="not prefix-closed"):
        dup()
    topk()  # both rows have the oracle's k-th score: a legal boundary tie for the tolerance-aware helper -- the hole check 3 closes


def test_fault_a_nan_entry_in_the_middle(oracle, planted):
    sc, idx = _answer(oracle, planted, N_F)
    assert np.isnan(sc[-5:]).all() and not np.isnan(sc[:-5]).any()
    at = N_F // 2
    order = np.concatenate([np.arange(at), [N_F - 5], np.arange(at, N_F - 5), np.arange(N_F - 4, N_F)])
    sc, idx = sc[order], idx[order]
    dup, topk = _both(planted, sc, idx, N_F)
    with pytest.raises(AssertionError, match="order breaks at rank"):
        dup()
    with pytest.raises(AssertionError, match="NaN last"):
        topk()


def test_fault_one_copy_one_ulp_off(oracle, planted):
    cp = planted[0]
    k = _cut_k(planted)
    sc, idx = _answer(oracle, planted, k)
    g = cp.group_of[idx.astype(np.int64)]
    r = int(np.nonzero(g[1:] != g[:-1])[0][0])  # the last copy of the best group: one ulp worse keeps the order
    assert r >= 1 and sc[r] == sc[r - 1]
    sc[r] = np.nextafter(sc[r], np.float32(np.inf))
    assert sc[r] < sc[r + 1]
    dup, topk = _both(planted, sc, idx, k)
    with pytest.raises(AssertionError, match="different score bits"):
        dup()
    topk()  # one ulp is far inside the tolerance


def test_fault_an_infinite_l2_score_made_finite(oracle, planted):
    sc, idx = _answer(oracle, planted, N_F)
    inf = np.nonzero(np.isposinf(sc))[0]
    assert inf.size == 8
    sc[inf] = np.float32(3.0e38)  # the whole group alike: identical bits, order kept
    dup, topk = _both(planted, sc, idx, N_F)
    dup()
    with pytest.raises(AssertionError, match="beyond the f32 range is not \\+inf"):
        topk()
    sc[inf[0]] = np.nan
    with pytest.raises(AssertionError):
        topk()


def test_fault_a_nan_l2_score_made_a_number(oracle, planted):
    sc, idx = _answer(oracle, planted, N_F)
    sc[-5:] = np.inf
    with pytest.raises(AssertionError, match="NaN row is not NaN"):
        _both(planted, sc, idx, N_F)[1]()


def test_fault_a_clear_winner_dropped(oracle, planted):
    k = _cut_k(planted)
    sc, idx = _answer(oracle, planted, k + 1)
    sc, idx = sc[1:].copy(), idx[1:].copy()
    dup, topk = _both(planted, sc, idx, k)
    with pytest.raises(AssertionError, match="missing clear winners"):
        topk()
    with pytest.raises(AssertionError, match="not prefix-closed"):
        dup()
