"""Candidate-search expectations from the oracle's scores ("Candidate search"): the k best of a query's
distinct, live, in-shard candidates, as mvfgpu_search orders and pads them."""
import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def candidate_rows(entries, n, index_base=0, dead=None, ids=None):
    """The local rows a list names: positions (index_base + row) or, with `ids`, vector ids (the first row holding an id);
    UINT64_MAX, entries outside the shard and deleted rows skipped, duplicates once.  Ascending."""
    e = np.asarray(entries, np.uint64).reshape(-1)
    e = e[e != PAD]
    if ids is not None:
        first = {}
        for r, v in enumerate(np.asarray(ids, np.uint64).tolist()):
            first.setdefault(v, r)
        loc = np.array([first.get(v, -1) for v in e.tolist()], np.int64)
    else:
        loc = np.where((e >= np.uint64(index_base)) & (e - np.uint64(index_base) < np.uint64(n)),
                       (e - np.uint64(index_base)).astype(np.int64) if e.size else e.astype(np.int64), -1)
    loc = np.unique(loc[loc >= 0])
    if dead is not None and loc.size:
        loc = loc[~dead[loc]]
    return loc


def oracle_candidates(oracle, rows, dtype, metric, query, entries, k, dead=None, index_base=0, ids=None, all_scores=None):
    """(count, scores[k], indices[k], raw[k]) with the library's padding; best first by the oracle's order key (NaN last),
    ties by position."""
    n = rows.shape[0]
    sel = candidate_rows(entries, n, index_base=index_base, dead=dead, ids=ids)
    if all_scores is None:
        sc, keys, raw = oracle.scores(rows, dtype, metric, query)
    else:
        sc, keys, raw = all_scores
    order = sel[np.lexsort((sel, keys[sel]))]
    out_s = np.full(k, np.inf if metric == 0 else -np.inf, np.float32)
    out_i = np.full(k, PAD, np.uint64)
    out_r = np.zeros(k, np.int32)
    take = order[:k]
    out_s[:take.size] = sc[take]
    out_i[:take.size] = (np.asarray(ids, np.uint64)[take] if ids is not None else take.astype(np.uint64) + np.uint64(index_base))
    out_r[:take.size] = raw[take]
    return int(sel.size), out_s, out_i, out_r
