"""Corpora of exactly duplicated float rows and their exact answers (DESIGN.md §2 "Duplicate rows", §3 "Order").

A row's score is a function of (query, row bytes) alone, so all copies of a vector carry identical score bits, and where the
DISTINCT vectors' scores lie far apart compared with §3's tolerance the whole top-k index list of a float route is determined
without any tolerance: the distinct vectors in float64 score order, each expanded into its live copies in ascending position,
cut at k.  Everything here is numpy on the CPU; the library is never called."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from _util import PAD, TOL, first_out_of_order

NP_OF = {0: np.float32, 1: np.float16}
CLEAR_FACTOR = 8.0  # a score gap of 8 tolerances: 4x over the two tolerances that could make two rows swap
SKEWED = (1, 1, 2, 3, 5, 8, 13, 40, 100, 400)
D_VECTORS = 24      # (32 distinct vectors leave only ~70 % of gaussian queries clear: do not raise)


@dataclass
class DupCorpus:
    rows: np.ndarray       # [n, dim] in the storage type
    group_of: np.ndarray   # i64 [n]: the group (distinct vector) of every position
    dtype: int
    vectors: np.ndarray | None = None  # corpus B: [D, dim], group g holds copies of vectors[g]
    zero_group: int | None = None      # corpus A: the group of the all-zero vector (half of its copies are -0.0)
    _members: dict = field(default_factory=dict, repr=False)

    @property
    def n(self):
        return len(self.group_of)

    def sizes(self):
        return np.bincount(self.group_of)


def corpus_a(oracle, seed, n, dim, dtype):
    """Many small groups: synthetic rows, ~30 % of the positions overwritten with copies of other rows in groups of 2 ... 40
    whose members a seeded permutation scatters over the whole position range; group 0 is the zero vector, 40 copies, every
    second one -0.0 in every element.  Rows that are nobody's copy are groups of one."""
    rng = np.random.default_rng(seed)
    rows = np.array(oracle.synth_rows(seed, 0, n, dim, dtype))
    perm = rng.permutation(n)
    group_of = np.full(n, -1, np.int64)
    at, copies, g = 0, 0, 0
    while copies < 0.3 * n and at + 40 <= n:
        size = 40 if g == 0 else int(rng.integers(2, 41))
        members = perm[at:at + size]
        if g == 0:
            rows[members] = 0.0
            rows[np.sort(members)[1::2]] = -0.0
        else:
            rows[members] = rows[members[0]]
        group_of[members] = g
        at, copies, g = at + size, copies + size - 1, g + 1
    single = group_of < 0
    group_of[single] = g + np.arange(int(single.sum()))
    return DupCorpus(rows, group_of, dtype, zero_group=0)


def skewed_sizes(n, d=D_VECTORS):
    """1, 1, 2, 3, 5, 8, 13, 40, 100, 400, one group of ~n / 6 and the rest filling n in growing steps."""
    big = n // 6
    rest_n = n - sum(SKEWED) - big
    nrest = d - len(SKEWED) - 1
    assert rest_n >= nrest > 0, "n is too small for the skewed list"
    w = np.arange(1, nrest + 1, dtype=np.float64)
    rest = np.maximum(1, np.floor(rest_n * w / w.sum())).astype(np.int64)
    rest[-1] += rest_n - rest.sum()
    sizes = np.array(list(SKEWED) + [big] + rest.tolist(), np.int64)
    assert sizes.sum() == n and (sizes > 0).all()
    return sizes


def corpus_b(seed, n, dim, dtype, d=D_VECTORS):
    """Few vectors, skewed groups: d standard-normal vectors, each scaled by a factor from U(0.5, 2) and rounded to the storage
    type, copied into groups of `skewed_sizes`; sizes and members are shuffled over vectors and positions with the seed."""
    rng = np.random.default_rng(seed)
    vectors = (rng.standard_normal((d, dim)) * rng.uniform(0.5, 2.0, (d, 1))).astype(NP_OF[dtype])
    sizes = skewed_sizes(n, d)[rng.permutation(d)]
    group_of = np.repeat(np.arange(d, dtype=np.int64), sizes)[rng.permutation(n)]
    return DupCorpus(np.ascontiguousarray(vectors[group_of]), group_of, dtype, vectors=vectors)


def gaussian_queries(seed, nq, dim):
    return np.random.default_rng(seed).standard_normal((nq, dim)).astype(np.float32)


def tombstones(seed, n, share=0.2):
    """dead[position]: a seeded `share` of the copies deleted."""
    dead = np.zeros(n, bool)
    dead[np.random.default_rng(seed).choice(n, int(share * n), replace=False)] = True
    return dead


def permuted_ids(seed, n, base=10**12):
    """ids[position]: a permutation, so that the id order says nothing about the position order."""
    return np.random.default_rng(seed).permutation(n).astype(np.uint64) + np.uint64(base)


def positions_of_ids(ids, got):
    """The positions behind reported ids (padding stays padding)."""
    got = np.asarray(got, np.uint64)
    order = np.argsort(ids)
    out = np.full(got.shape, PAD, np.uint64)
    real = got != PAD
    at = np.searchsorted(ids[order], got[real])
    assert (at < ids.size).all() and (ids[order][np.minimum(at, ids.size - 1)] == got[real]).all(), "an id nobody holds was reported"
    out[real] = order[at].astype(np.uint64)
    return out


def shard_cuts(cp, nshards=3):
    """Row-range cut points placed INSIDE the largest groups: cut i falls directly behind the member of one of the two
    largest groups that lies nearest to i * n / nshards, so copies of that group end one shard and others start the next."""
    big = np.argsort(cp.sizes())[::-1][:2]
    cuts = [0]
    for i in range(1, nshards):
        m = np.nonzero(cp.group_of == big[i % 2])[0]
        cuts.append(int(m[np.argmin(np.abs(m - i * cp.n // nshards))]) + 1)
    cuts.append(cp.n)
    assert cuts == sorted(set(cuts)), cuts
    return cuts


# ---- the exact answer of corpus B --------------------------------------------------------------------------------------

def vector_scores(metric, vectors, queries):
    """(score f64 [nq, d], §3 tolerance f64 [nq, d]) of every query against every distinct vector, from the exactly widened
    values: L2 1e-5 * score, InnerProduct 1e-5 * |q||x|, Cosine 1e-5."""
    memo = (id(vectors), id(queries), metric)
    hit = _SCORES.get(memo)
    if hit is not None and hit[0] is vectors and hit[1] is queries:
        return hit[2]
    if len(_SCORES) > 16:
        _SCORES.clear()
    out = _SCORES[memo] = (vectors, queries, _vector_scores(metric, vectors, queries))
    return out[2]


_SCORES = {}


def _vector_scores(metric, vectors, queries):
    x = np.asarray(vectors).astype(np.float64)
    q = np.atleast_2d(np.asarray(queries)).astype(np.float64)
    xn, qn = np.sqrt((x * x).sum(1)), np.sqrt((q * q).sum(1))
    if metric == 0:
        s = np.sqrt(((q[:, None, :] - x[None, :, :]) ** 2).sum(2))
        return s, TOL * np.abs(s)
    dot = q @ x.T
    den = qn[:, None] * xn[None, :]
    if metric == 1:
        return dot, TOL * den
    return np.where(den > 0, dot / np.where(den > 0, den, 1.0), 0.0), np.full(dot.shape, TOL)


def members_of(cp, live):
    """Per group the live positions, ascending (cached per `live` array)."""
    hit = cp._members.get(id(live))
    if hit is None or hit[0] is not live:
        pos = np.nonzero(live)[0]
        order = np.argsort(cp.group_of[pos], kind="stable")
        g = cp.group_of[pos][order]
        ngroups = int(cp.group_of.max()) + 1
        bounds = np.searchsorted(g, np.arange(ngroups + 1))
        hit = (live, [pos[order][bounds[i]:bounds[i + 1]] for i in range(ngroups)])
        if len(cp._members) > 8:
            cp._members.clear()
        cp._members[id(live)] = hit
    return hit[1]


def _vector_order(metric, s):
    key = s if metric == 0 else -s
    return np.argsort(key, kind="stable"), key


def expected_topk(cp, metric, queries, k, live=None):
    """u64 [nq, k]: per query the distinct vectors in float64 score order, each expanded into its live copies in ascending
    position, cut at k and padded with UINT64_MAX (§3: k > rows pads)."""
    live = np.ones(cp.n, bool) if live is None else live
    mem = members_of(cp, live)
    s, _ = vector_scores(metric, cp.vectors, queries)
    out = np.full((s.shape[0], k), PAD, np.uint64)
    for i in range(s.shape[0]):
        order, _ = _vector_order(metric, s[i])
        got, parts = 0, []
        for g in order:
            if got >= k:
                break
            parts.append(mem[g])
            got += mem[g].size
        lst = np.concatenate(parts)[:k] if parts else np.zeros(0, np.int64)
        out[i, :lst.size] = lst.astype(np.uint64)
    return out


def clear_pairs(metric, s, tol, present):
    """ONE query: (order, clear): the vectors with a live copy in score order and, per adjacent pair of that order, whether the
    float64 score gap exceeds CLEAR_FACTOR x the larger of the two scores' tolerances."""
    order, key = _vector_order(metric, s)
    order = order[present[order]]
    gap = np.diff(key[order])
    return order, gap > CLEAR_FACTOR * np.maximum(tol[order][:-1], tol[order][1:])


def clear_queries(cp, metric, queries, k, live=None):
    """bool [nq]: the gap condition holds for every adjacent pair of vectors in score order up to and including the pair
    behind the group that holds rank k.  Only these queries are compared with `expected_topk`."""
    live = np.ones(cp.n, bool) if live is None else live
    nlive = np.array([m.size for m in members_of(cp, live)])
    s, tol = vector_scores(metric, cp.vectors, queries)
    present = np.nonzero(nlive > 0)[0]
    s, tol, nlive = s[:, present], tol[:, present], nlive[present]
    key = s if metric == 0 else -s
    order = np.argsort(key, axis=1, kind="stable")
    key, tol = np.take_along_axis(key, order, 1), np.take_along_axis(tol, order, 1)
    clear = np.diff(key, axis=1) > CLEAR_FACTOR * np.maximum(tol[:, :-1], tol[:, 1:])
    holds_k = (np.cumsum(nlive[order], axis=1) < k).sum(1)  # index in the order of the group holding rank k
    needed = np.arange(clear.shape[1])[None, :] <= holds_k[:, None]
    return (clear | ~needed).all(1)


# ---- properties that need no separation --------------------------------------------------------------------------------

_RANK_CACHE = {}


def _live_rank(group_of, live):
    """rank[p]: the number of live copies of p's group at positions below p (cached per pair of arrays)."""
    key = (id(group_of), id(live))
    hit = _RANK_CACHE.get(key)
    if hit is None or hit[0] is not group_of or hit[1] is not live:
        pos = np.nonzero(live)[0]
        order = np.argsort(group_of[pos], kind="stable")
        g = group_of[pos][order]
        start = np.nonzero(np.concatenate([[True], g[1:] != g[:-1]]))[0] if g.size else np.zeros(0, np.int64)
        run = np.repeat(start, np.diff(np.concatenate([start, [g.size]])))
        rank = np.full(len(group_of), -1, np.int64)
        rank[pos[order]] = np.arange(g.size) - run
        if len(_RANK_CACHE) > 8:
            _RANK_CACHE.clear()
        hit = _RANK_CACHE[key] = (group_of, live, rank)
    return hit[2]


def score_bits(sc):
    """u32 bits of f32 scores with -0.0 folded into +0.0 and every NaN into one."""
    sc = np.asarray(sc, np.float32)
    return np.where(np.isnan(sc), np.uint32(0x7FC00000), np.where(sc == 0, np.float32(0), sc).view(np.uint32))


def first_bit_difference(sc, pos, group_of):
    """(rank a, rank b) of two returned copies of one group whose score bits differ, or None."""
    bits = score_bits(sc)
    g = group_of[pos]
    order = np.argsort(g, kind="stable")
    diff = np.nonzero((g[order][1:] == g[order][:-1]) & (bits[order][1:] != bits[order][:-1]))[0]
    return (int(order[diff[0]]), int(order[diff[0] + 1])) if diff.size else None


def assert_dup_properties(metric, scores, indices, group_of, live, k, index_base=0, what=""):
    """ONE query's result list over a corpus of duplicated rows; `indices` are positions (+ index_base).
    1. all returned copies of one group carry identical score bits (scores equal to 0.0 compare as == 0.0, either sign: the
       zero vector's copies hold +0.0 or -0.0; NaN compares as NaN);
    2. the list is strictly ascending in (§3 order key of the score, position) over ALL real entries, NaN last;
    3. prefix-closed: if the copy at position p is returned, every live copy of its group at a position below p is too.
    Also: min(k, live rows) real entries of live rows, none twice, padding behind them."""
    n = len(group_of)
    kk = min(k, int(np.count_nonzero(live)))
    indices = np.asarray(indices, np.uint64)
    sc = np.asarray(scores, np.float32)
    assert (indices[kk:] == PAD).all() and (indices[:kk] != PAD).all(), f"{what}: {kk} real entries expected, then padding"
    assert (sc[kk:] == (np.inf if metric == 0 else -np.inf)).all(), f"{what}: padding scores"
    pos = (indices[:kk] - np.uint64(index_base)).astype(np.int64)
    sc = sc[:kk]
    assert ((pos >= 0) & (pos < n)).all(), f"{what}: a position outside the corpus"
    assert live[pos].all(), f"{what}: a deleted row was returned: {pos[~live[pos]][:5]}"
    assert np.unique(pos).size == kk, f"{what}: a row was returned twice"
    # 2
    r = first_out_of_order(metric, sc, pos)
    assert r is None, (f"{what}: order breaks at rank {r}: (score {sc[r - 1]!r}, row {pos[r - 1]}) is followed by "
                       f"(score {sc[r]!r}, row {pos[r]})")
    # 1
    d = first_bit_difference(sc, pos, group_of)
    if d is not None:
        a, b = d
        bits = score_bits(sc)
        raise AssertionError(f"{what}: copies of one vector (group {group_of[pos[a]]}) carry different score bits: rank {a} row {pos[a]} "
                             f"{sc[a]!r} (0x{bits[a]:08x}), rank {b} row {pos[b]} {sc[b]!r} (0x{bits[b]:08x})")
    g = group_of[pos]
    # 3
    rank = _live_rank(group_of, live)[pos]
    returned = np.bincount(g, minlength=int(g.max()) + 1 if kk else 0)
    hole = np.nonzero(rank >= returned[g])[0]
    if hole.size:
        h = hole[0]
        raise AssertionError(f"{what}: not prefix-closed: rank {h} is row {pos[h]}, live copy number {rank[h]} of group {g[h]}, "
                             f"but only {returned[g[h]]} of its copies were returned -- an earlier copy is missing")


def first_difference(got, want):
    """Rank of the first entry in which two index lists differ, or None."""
    d = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return int(d[0]) if d.size else None


# ---- the cases of tests/test_gpu_float_ties.py (tests/test_float_ties_cpu.py asserts their clear share) ----------------------

# name -> (seed, rows, dimension).  Float32 / Float16 row bytes and K1's lane groups (one query): d48 192 / 96 B, 16 / 8 lanes;
# d96 384 / 192 B, 16 lanes; d200 800 / 400 B, 64 / 32 lanes; d776 3104 / 1552 B, 64 lanes; d4 one lane, d16 4 lanes, d32 8 / 4
# lanes.  90 000 rows span three phases of the batched schedule (4K / 16K / 64K rows) and several blocks of K1.
B_SHAPES = {"n90k_d48": (148, 90_000, 48), "n40k_d96": (196, 40_000, 96), "n20k_d200": (300, 20_000, 200),
            "n6k_d776": (876, 6_000, 776), "n20k_d4": (104, 20_000, 4), "n20k_d16": (116, 20_000, 16), "n20k_d32": (132, 20_000, 32)}
A_SHAPES = {"n40k_d96": (96, 40_000, 96), "n20k_d200": (200, 20_000, 200)}
NQ_SET = 200                                  # every case takes the first nq of its shape's 200 gaussian queries
KS = (1, 7, 100, 409, 1000, 1025, 3000)
_CORPORA = {}


def get_b(name, dtype):
    """Corpus B of a named shape: built once, shared, never changed."""
    hit = _CORPORA.get(("b", name, dtype))
    if hit is None:
        seed, n, dim = B_SHAPES[name]
        hit = _CORPORA[("b", name, dtype)] = corpus_b(seed, n, dim, dtype)
    return hit


def get_a(oracle, name, dtype):
    hit = _CORPORA.get(("a", name, dtype))
    if hit is None:
        seed, n, dim = A_SHAPES[name]
        hit = _CORPORA[("a", name, dtype)] = corpus_a(oracle, seed, n, dim, dtype)
    return hit


def get_queries(name):
    hit = _CORPORA.get(("q", name))
    if hit is None:
        seed, _, dim = (B_SHAPES.get(name) or A_SHAPES[name])
        hit = _CORPORA[("q", name)] = gaussian_queries(seed + 1000, NQ_SET, dim)
    return hit


def get_dead(name):
    """The shape's tombstones: 20 % of the copies."""
    hit = _CORPORA.get(("dead", name))
    if hit is None:
        seed, n, _ = (B_SHAPES.get(name) or A_SHAPES[name])
        hit = _CORPORA[("dead", name)] = tombstones(seed + 2000, n)
    return hit


def half_of_every_group(seed, group_of):
    """allow[position]: a seeded half (rounded up) of the members of every group."""
    r = np.random.default_rng(seed).random(len(group_of))
    order = np.lexsort((r, group_of))
    g = group_of[order]
    start = np.nonzero(np.concatenate([[True], g[1:] != g[:-1]]))[0]
    size = np.diff(np.concatenate([start, [g.size]]))
    rank = np.arange(g.size) - np.repeat(start, size)
    allow = np.zeros(len(group_of), bool)
    allow[order] = rank < np.repeat((size + 1) // 2, size)
    return allow


def get_allow(name, cp):
    key = ("allow", name, cp.vectors is None)  # (A and B shapes share names, not groups)
    hit = _CORPORA.get(key)
    if hit is None:
        seed = (B_SHAPES.get(name) or A_SHAPES[name])[0]
        hit = _CORPORA[key] = half_of_every_group(seed + 3000, cp.group_of)
    return hit


# the join case: a self-join of "n20k_d200" over this window of query rows (one short window of the batched route)
JOIN_FIRST, JOIN_COUNT, JOIN_KS = 777, 100, (3, 50, 600)

K_PASS = (1, 7, 100, 409, 1000)
# (shape, live rows, ks) of every case the GPU file compares with the exact list: tests/test_float_ties_cpu.py asserts the
# clear share of each, the GPU file refuses to run a case that is not listed
CLEAR_CASES = [(name, "all", K_PASS) for name in B_SHAPES] + [
    ("n40k_d96", "all", (1025, 3000)), ("n40k_d96", "tombstones", KS), ("n40k_d96", "allow", K_PASS), ("n40k_d96", "allow & ~dead", K_PASS),
    ("n90k_d48", "tombstones", K_PASS)]
_LIVE = {}


def get_live(name, kind, cp):
    """The live rows of a case: one array per (shape, kind), so that what is cached per array is computed once."""
    key = (name, kind, cp.vectors is None)
    hit = _LIVE.get(key)
    if hit is None:
        hit = {"all": lambda: np.ones(cp.n, bool), "tombstones": lambda: ~get_dead(name), "allow": lambda: get_allow(name, cp),
               "allow & ~dead": lambda: get_allow(name, cp) & ~get_dead(name)}[kind]()
        _LIVE[key] = hit
    return hit


def listed(name, kind, k):
    return any(n == name and kd == kind and k in ks for n, kd, ks in CLEAR_CASES)
