"""Helpers of the filtered-search tests (DESIGN.md §3 "Filtered search") and the oracle restatement of its semantics:
a filtered search is the oracle's search over rows[admitted], mapped back to positions -- a row is admitted iff its allow
bit (first_bit + local row, LSB first) is set and it is not deleted."""
import numpy as np

from _util import assert_float_topk

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def admitted_mask(bits, first_bit, n, dead=None):
    """bool[n]: local row r is admitted by the packed bitmap `bits` read from bit `first_bit`, and not deleted."""
    allow = np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[first_bit:first_bit + n].astype(bool)
    assert allow.size == n, "the bitmap covers fewer rows than the shard holds"
    return allow & ~dead if dead is not None else allow


def shard_bitmap(allow, first_bit, total_bits=None, outside=1):
    """The packed bitmap that holds `allow` (bool over a shard's rows) from bit first_bit on; every other bit is `outside`."""
    n = allow.size
    total = max(total_bits or 0, first_bit + n)
    total = (total + 7) // 8 * 8
    full = np.full(total, bool(outside))
    full[first_bit:first_bit + n] = allow
    return np.packbits(full, bitorder="little")


def device_words(allow, outside=1):
    """u32 words over local rows for the device form; bits at and beyond the rows are `outside`."""
    n = allow.size
    nw = (n + 31) // 32
    full = np.full(nw * 32, bool(outside))
    full[:n] = allow
    return np.packbits(full, bitorder="little").view(np.uint32).copy()


def oracle_filtered(oracle, rows, dtype, metric, q, k, admit, ids=None, index_base=0):
    """The oracle's top-k of every query over rows[admit], reported at the rows' positions (or ids):
    -> (scores f32[nq, k], indices u64[nq, k], raw i32[nq, k]); padding where fewer than k rows are admitted."""
    q = np.atleast_2d(q)
    live = np.nonzero(admit)[0]
    if live.size == 0:
        pad = np.inf if metric == 0 else -np.inf
        return (np.full((q.shape[0], k), pad, np.float32), np.full((q.shape[0], k), PAD, np.uint64), np.zeros((q.shape[0], k), np.int32))
    sc, idx, raw = oracle.search(rows[live], dtype, metric, q, k)
    out = np.full(idx.shape, PAD, np.uint64)
    ok = idx != PAD
    pos = live[idx[ok].astype(np.int64)]
    out[ok] = ids[pos] if ids is not None else pos.astype(np.uint64) + np.uint64(index_base)
    return sc, out, raw


def assert_float_filtered(oracle, rows, dtype, metric, q, k, admit, got_scores, got_idx, index_base=0, all_scores=None):
    """Float spaces, ONE query: only admitted rows are returned, and they are the top-k of the admitted rows by the oracle's
    score of every admitted row, within the project tolerance (assert_float_topk).  all_scores: another reference's score of EVERY row (float64 sums for wide rows: tests/_wide.py)."""
    live = np.nonzero(admit)[0]
    kk = min(k, live.size)
    li = (np.asarray(got_idx[:kk]) - np.uint64(index_base)).astype(np.int64)
    pos = np.searchsorted(live, li)
    assert live.size == 0 or ((pos < live.size).all() and (live[np.minimum(pos, live.size - 1)] == li).all()), \
        "a row that is not admitted (or deleted) was returned"
    sub_i = np.concatenate([pos.astype(np.uint64), np.asarray(got_idx[kk:], np.uint64)])
    sub = rows[live]
    if all_scores is not None:
        all_s = np.asarray(all_scores)[live]
    else:
        all_s = oracle.scores(sub, dtype, metric, q)[0] if live.size else np.zeros(0, np.float32)
    assert_float_topk(metric, got_scores, sub_i, all_s, sub.astype(np.float32), np.asarray(q, np.float32), k)


def mask_patterns(n, block):
    """The bit-geometry patterns: all, none, first row, last row, every 97th row, a run straddling every block boundary."""
    pats = {"all": np.ones(n, bool), "none": np.zeros(n, bool)}
    first = np.zeros(n, bool)
    first[0] = True
    last = np.zeros(n, bool)
    last[n - 1] = True
    every = np.zeros(n, bool)
    every[::97] = True
    pats.update(first=first, last=last, every97=every)
    if n > block:
        runs = np.zeros(n, bool)
        for b in range(block, n, block):
            runs[max(b - 40, 0):min(b + 40, n)] = True
        pats["runs"] = runs
    return pats
