"""A numpy restatement of the k-NN join (mvfgpu_knn_join, DESIGN.md §3 "Join"), for the tests: from a full score matrix, or
from the top-k' lists of a search, to the join's answer -- the removal rule, tombstones, ids and padding.  Nothing here is
fast and nothing here touches the library."""
import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
WINDOW = 1024         # MVFGPU_JOIN_WINDOW
EXCLUDE_SELF = 1      # MVFGPU_JOIN_EXCLUDE_SELF
L2, INNER_PRODUCT, COSINE = 0, 1, 2


def pad_score(metric):
    return np.float32(np.inf if metric == L2 else -np.inf)


def ranges_meet(q_base, q_n, c_base, c_n):
    """Can a query row's global position be a row of the searched handle at all?"""
    return q_base < c_base + c_n and c_base < q_base + q_n


def k_prime(k, exclude, q_base, q_n, c_base, c_n):
    """What the join asks the search for: k + 1 where a query row can be among its own results, else k."""
    return k + 1 if exclude and ranges_meet(q_base, q_n, c_base, c_n) else k


def best_first(scores, metric):
    """Positions of one query's rows in the library's order: best first, ties by ascending position, NaN last,
    -0.0 == +0.0."""
    s = np.asarray(scores, np.float64)
    key = s if metric == L2 else -s
    nan = np.isnan(key)
    return np.lexsort((np.arange(s.size), np.where(nan, 0.0, key), nan))


def remove_self(scores, positions, raw, self_pos, k, metric, c_index_base=0, c_ids=None, deleted_query=False):
    """The removal rule on ONE query's list of k' >= k ordered entries (positions, UINT64_MAX = padding) -> its k entries:
    k' > k: the entry at the query row's own position goes if it is there, else the last one; then the ids are applied.
    A deleted query row is all padding."""
    positions = np.asarray(positions, np.uint64)
    scores = np.asarray(scores, np.float32)
    raw = np.zeros(positions.size, np.int32) if raw is None else np.asarray(raw, np.int32)
    if deleted_query:
        return np.full(k, pad_score(metric), np.float32), np.full(k, PAD, np.uint64), np.zeros(k, np.int32)
    keep = np.arange(positions.size)
    if positions.size > k:
        hit = np.nonzero(positions == np.uint64(self_pos))[0]
        assert hit.size <= 1, "a search reports a row once"
        keep = np.delete(keep, hit[0] if hit.size else positions.size - 1)
    keep = keep[:k]
    pos = positions[keep]
    out = pos.copy()
    if c_ids is not None:
        real = pos != PAD
        out[real] = np.asarray(c_ids, np.uint64)[(pos[real] - np.uint64(c_index_base)).astype(np.int64)]
    return scores[keep].copy(), out, raw[keep].copy()


def search_lists(scores, metric, kk, c_index_base=0, c_dead=None, raw=None):
    """A search restated: the kk best live rows of every query (scores [nq, n]) as positions, padded."""
    scores = np.atleast_2d(np.asarray(scores))
    nq, n = scores.shape
    S = np.full((nq, kk), pad_score(metric), np.float32)
    I = np.full((nq, kk), PAD, np.uint64)
    R = np.zeros((nq, kk), np.int32)
    for i in range(nq):
        order = best_first(scores[i], metric)
        if c_dead is not None:
            order = order[~np.asarray(c_dead, bool)[order]]
        order = order[:kk]
        S[i, :order.size] = scores[i][order]
        I[i, :order.size] = order.astype(np.uint64) + np.uint64(c_index_base)
        if raw is not None:
            R[i, :order.size] = np.asarray(raw)[i][order]
    return S, I, R


def join_from_lists(S, I, R, q_positions, k, metric, c_index_base=0, c_ids=None, q_dead=None):
    """Top-k' lists (positions) of the queries at global positions q_positions -> the join's [nq, k] answer."""
    nq = len(q_positions)
    oS = np.empty((nq, k), np.float32)
    oI = np.empty((nq, k), np.uint64)
    oR = np.empty((nq, k), np.int32)
    for i in range(nq):
        oS[i], oI[i], oR[i] = remove_self(S[i], I[i], None if R is None else R[i], q_positions[i], k, metric, c_index_base, c_ids,
                                          deleted_query=bool(q_dead is not None and q_dead[i]))
    return oS, oI, oR


def join_from_scores(scores, metric, k, q_positions, exclude=True, q_span=None, c_index_base=0, c_dead=None, c_ids=None,
                     q_dead=None, raw=None):
    """The join from the full score matrix scores[i, r] = query row i against local row r of the searched handle.
    q_positions: the query rows' global positions; q_span = (index_base, rows) of the query handle (default: the span of
    q_positions), which with the searched handle's decides k'."""
    scores = np.atleast_2d(np.asarray(scores))
    n = scores.shape[1]
    q_positions = np.asarray(q_positions, np.uint64)
    if q_span is None:
        q_span = (int(q_positions.min()), int(q_positions.max()) - int(q_positions.min()) + 1) if q_positions.size else (0, 0)
    kk = k_prime(k, exclude, q_span[0], q_span[1], c_index_base, n)
    S, I, R = search_lists(scores, metric, kk, c_index_base, c_dead, raw)
    return join_from_lists(S, I, R, q_positions, k, metric, c_index_base, c_ids, q_dead)


def windows(first, count):
    """(first row, rows) of the join's consecutive windows."""
    return [(first + off, min(WINDOW, count - off)) for off in range(0, count, WINDOW)]


def widen(rows):
    """Stored rows -> the queries the join stages: Float32 as stored, Float16 widened exactly, Int8 / UInt8 as stored."""
    rows = np.asarray(rows)
    return rows.astype(np.float32) if rows.dtype in (np.float16, np.float32) else rows
