"""What the diversified re-ranking's tests share (tests/test_mmr_cpu.py, tests/test_gpu_mmr.py; DESIGN.md §3 "Diversified
re-ranking"): the stream classes of include/mvf_gpu_mmr.h's functions, the greedy walk restated in numpy float32, the recipe
that builds a call's expected bytes from the library's own candidate searches, and -- run as a program,
`python tests/_mmr.py <out.npz>` -- the parity case the GPU tests start as a fresh (poisoned) child process.
Behind them, for the tests of the walk kernel's forms (DESIGN.md §5 "D0"; tests/test_gpu_mmr_forms.py): the table of (type,
dimension) cases with the cell each holds, two references independent of every kernel -- exact integers for Int8 / UInt8, the
walk in float64 held along the kernel's own path for the float types --, walks wrong in one way as models, and the duplicate-row
list whose tied copies straddle every ownership edge of the block.
Imports numpy and the standard library only; as a child it keeps the binding from loading torch."""
import os
import sys

import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
L2 = 0

# The stream class of every function include/mvf_gpu_mmr.h declares, in tests/_streams.py's words (its ENTRY_CLASS lists
# include/mvf_gpu.h's functions), and the device form the measurement aid among them runs.
ENTRY_CLASS = {
    "mvfgpu_search_mmr": "runs under corpus_device_call",
    "mvfgpu_search_mmr_device": "runs under corpus_device_call",
    "mvfgpu_selftest_mmr_walk": "takes no handle",
    "mvfgpu_selftest_mmr_form": "takes no handle",
    "mvfgpu_selftest_mmr_stage_ms": "runs under corpus_device_call",
}
TIMED_FORM_OF = {"mvfgpu_selftest_mmr_stage_ms": "mvfgpu_search_mmr_device"}


def value(metric, scores):
    """v(x): larger is better for every metric -- exact negation under L2"""
    s = np.asarray(scores, np.float32)
    return np.negative(s) if metric == L2 else s


def first_in_search_order(metric, scores):
    """the position mvfgpu_search ranks first among `scores` (position order): best first, -0.0 == +0.0, NaN last, ties by
    ascending position"""
    s = np.asarray(scores, np.float32)
    ok = np.nonzero(~np.isnan(s))[0]
    if ok.size == 0:
        return 0
    v = value(metric, s[ok])
    return int(ok[np.argmax(v)])  # argmax: the first of equal values; -0.0 == +0.0 in a comparison


def numpy_walk(metric, rel_scores, sim_scores, lam, k, first=None):
    """The walk of the contract in numpy float32.  rel_scores f32 [c] and sim_scores f32 [c, c] (sim_scores[s, d]: row s as the
    query) in SCORE form, both in ascending position; `first`: pick 0 where the caller knows the search's order better than the
    f32 scores tell (exact integers that round to one f32).  -> (order: list of min(k, c) positions, objective f32 [same]).
    Every operation is one numpy float32 operation: numpy never fuses a multiplication into a subtraction."""
    rel = value(metric, rel_scores)
    c = rel.size
    a = np.float32(lam)
    b = np.float32(1.0) - a
    red = np.full(c, -np.inf, np.float32)
    taken = np.zeros(c, bool)
    order, objective = [], []
    with np.errstate(all="ignore"):
        for j in range(min(k, c)):
            if j == 0:
                s = first_in_search_order(metric, rel_scores) if first is None else int(first)
                objective.append(a * rel[s])
            else:
                obj = (a * rel) - (b * red)          # two roundings, then a third
                free = np.nonzero(~taken)[0]
                ok = free[~np.isnan(obj[free])]
                s = int(ok[np.argmax(obj[ok])]) if ok.size else int(free[0])
                objective.append(obj[s])
            order.append(s)
            taken[s] = True
            if j + 1 == min(k, c):
                break
            sim = value(metric, sim_scores[s])
            # fmaxf that ignores a NaN; of two equal values (-0.0 and +0.0) the one already held stays
            new = np.where(np.isnan(sim), red, np.where(np.isnan(red), sim, np.where(red < sim, sim, red)))
            red = np.where(taken, red, new).astype(np.float32)
    objective = np.array(objective, np.float32)
    # the contract reports every NaN objective as the quiet NaN 0x7FC00000: which NaN an operation hands on is the processor's
    objective[np.isnan(objective)] = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    return order, objective


def pad_score(metric):
    return np.float32(np.inf if metric == L2 else -np.inf)


def format_picks(metric, k, order, objective, scores, indices, raw, count):
    """the call's output row from the picks (positions into the candidates' arrays): (scores, indices, raw, objective, count)"""
    S = np.full(k, pad_score(metric), np.float32)
    I = np.full(k, PAD, np.uint64)
    R = np.zeros(k, np.int32)
    O = np.full(k, pad_score(metric), np.float32)
    n = len(order)
    if n:
        o = np.asarray(order, np.int64)
        S[:n], I[:n], R[:n], O[:n] = scores[o], indices[o], raw[o], objective
    return S, I, R, O, np.uint64(count)


def recipe(corpus, metric, query, entries, k, lam):
    """Identity 1: the expected output row of one query from library calls and the numpy walk.  R = search_candidates of the
    query with k = m; G = search_candidates of the candidates' own rows as queries (gather_rows; Float16 rows widened with
    astype(float32)) over the same list.  `entries` are positions (no vector ids attached)."""
    entries = np.ascontiguousarray(entries, np.uint64).reshape(1, -1)
    m = entries.shape[1]
    if m == 0:
        return format_picks(metric, k, [], np.zeros(0, np.float32), None, None, None, 0)
    q = np.asarray(query)[None, :]
    R = corpus.search_candidates(q, entries, m, metric)
    c = int(R.counts[0])
    if c == 0:
        return format_picks(metric, k, [], np.zeros(0, np.float32), None, None, None, 0)
    by_pos = np.argsort(R.indices[0][:c], kind="stable")
    pos, rel, raw = R.indices[0][:c][by_pos], R.scores[0][:c][by_pos], R.raw[0][:c][by_pos]
    first = int(np.nonzero(by_pos == 0)[0][0])       # the search's first entry, as a position rank
    sim = np.zeros((c, c), np.float32)
    if c > 1 and k > 1:
        rows = corpus.gather_rows(pos)
        if rows.dtype == np.float16:
            rows = rows.astype(np.float32)
        Gs = corpus.search_candidates(rows, np.repeat(entries, c, axis=0), m, metric)
        assert (Gs.counts == np.uint64(c)).all()
        o = np.argsort(Gs.indices[:, :c], axis=1, kind="stable")
        assert (np.take_along_axis(Gs.indices[:, :c], o, 1) == pos[None, :]).all()
        sim = np.take_along_axis(Gs.scores[:, :c], o, 1)
    order, objective = numpy_walk(metric, rel, sim, lam, k, first=first)
    return format_picks(metric, k, order, objective, rel, pos, raw, c)


def assert_rows_equal(got, want, j, what=""):
    """got: an MmrResult; want: format_picks' row for query j -- byte for byte"""
    S, I, R, O, cnt = want
    assert int(got.counts[j]) == int(cnt), f"{what} query {j}: count {int(got.counts[j])} != {int(cnt)}"
    assert got.indices[j].tobytes() == I.tobytes(), f"{what} query {j}: picks {got.indices[j][:8]} != {I[:8]}"
    assert got.scores[j].tobytes() == S.tobytes(), f"{what} query {j}: score bits"
    assert got.raw[j].tobytes() == R.tobytes(), f"{what} query {j}: raw"
    assert got.objective[j].tobytes() == O.tobytes(), f"{what} query {j}: objective bits {got.objective[j][:6]} != {O[:6]}"


def planted_world(seed=77, n=3000, dim=128, m=64, copies=8):
    """(rows f32 [n, dim] of unit norm, query, list u64 [m] ascending, the positions of the copies): the listed rows lie at
    cosine 0.55 .. 0.8 of the query in otherwise random directions, and `copies` of them are one and the same row at cosine 0.9,
    the best.  Under lambda = 0.5 a further copy's objective is 0.45 - 0.5 = -0.05, every other row's stays above +0.03 over 16
    picks (a float64 run of the walk): margins far beyond f32 rounding."""
    rng = np.random.default_rng(seed)

    def beside(q, alpha):
        noise = rng.standard_normal(dim)
        noise -= (noise @ q) * q
        return alpha * q + np.sqrt(1.0 - alpha * alpha) * noise / np.linalg.norm(noise)

    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    lst = np.sort(rng.choice(n, m, replace=False))
    for r in lst:
        rows[r] = beside(q, 0.55 + 0.25 * rng.random())
    where = np.sort(lst[rng.choice(m, copies, replace=False)])
    rows[where] = beside(q, 0.9)
    rows = rows.astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True).astype(np.float32)
    rows[where] = rows[where[0]]
    return rows, q.astype(np.float32), lst.astype(np.uint64), where.astype(np.uint64)


# ---- the walk kernel's forms (DESIGN.md §5 "D0"; tests/test_gpu_mmr_forms.py, tests/test_mmr_cpu.py) --------------------------
DTYPE = {"f32": 0, "f16": 1, "i8": 2, "u8": 3}
NP_OF = {"f32": np.float32, "f16": np.float16, "i8": np.int8, "u8": np.uint8}
ELEM = {"f32": 4, "f16": 2, "i8": 1, "u8": 1}
INT_RANGE = {"i8": (-128, 127), "u8": (0, 255)}
LDS_QUERY_BYTES = 40 * 1024     # kCandQueryLdsMax (scan_gather.h)
LAMBDAS = (0.0, 0.3, 0.5, 1.0)

# (type, dimension) -> the cell it holds: (lanes per row G, steps per lane J, the picked row staged in LDS), worked out by hand
# from choose_group (api.hip) and mmr_form (scan_mmr.h); mvfgpu_selftest_mmr_form is the authority the tests hold it to.
# V = 16-byte vectors per row.  G: V <= 1 one lane, V <= 4 four, V <= 8 eight, V < 192 sixteen, else 64; a V in 17..191 that is
# no multiple of 8 takes 32 lanes (V < 32) or 64 (V > 32).  The padded f32 copy of a float row takes G J 16 bytes (Float16:
# G J 32) and stays in LDS up to 40 KiB: 64 x 40 x 16 = 64 x 20 x 32 = 40960 at dimension 10240, one step more at 10241.
FORM_CELLS = {
    ("f32", 4): (1, 1, True), ("f32", 16): (4, 1, True), ("f32", 20): (8, 1, True), ("f32", 128): (16, 2, True),
    ("f32", 100): (32, 1, True), ("f32", 136): (64, 1, True), ("f32", 768): (64, 3, True), ("f32", 770): (64, 4, True),
    ("f32", 10240): (64, 40, True), ("f32", 10241): (64, 41, False),
    ("f16", 8): (1, 1, True), ("f16", 24): (4, 1, True), ("f16", 40): (8, 1, True), ("f16", 128): (16, 1, True),
    ("f16", 200): (32, 1, True), ("f16", 264): (64, 1, True), ("f16", 10240): (64, 20, True), ("f16", 10241): (64, 21, False),
    ("i8", 16): (1, 1, True), ("i8", 20): (4, 1, True), ("i8", 100): (8, 1, True), ("i8", 256): (16, 1, True),
    ("i8", 400): (32, 1, True), ("i8", 530): (64, 1, True), ("i8", 33025): (64, 33, True),
    ("u8", 16): (1, 1, True), ("u8", 20): (4, 1, True), ("u8", 100): (8, 1, True), ("u8", 256): (16, 1, True),
    ("u8", 400): (32, 1, True), ("u8", 530): (64, 1, True), ("u8", 33025): (64, 33, True),
}
FORM_CASES = list(FORM_CELLS)
# widths only MVF_K1_G reaches, (type, dimension, forced width) -> cell: 64 lanes on a row of 5 vectors (59 lanes of a group
# lie past the row) and 16 lanes at dimension 10241 (through the cache with 161 / 81 steps per lane)
FORCED_CELLS = {
    ("f32", 20, 64): (64, 1, True), ("f16", 40, 64): (64, 1, True), ("i8", 80, 64): (64, 1, True), ("u8", 80, 64): (64, 1, True),
    ("f32", 10241, 16): (16, 161, False), ("f16", 10241, 16): (16, 81, False),
}
FORCED_CASES = list(FORCED_CELLS)
FORM_SWITCH = [("f32", 10240, 10241), ("f16", 10240, 10241)]   # the last dimension staged in LDS, the first through the cache
F64_K = 32                      # picks of the float64 check
F64_OWN_UNCLEAR_MAX, F64_DEVICE_UNCLEAR_MAX = 4, 8


def form_rule(dt, dim, forced=0):
    """choose_group's rule for one query per pass and mmr_form's, restated: (G, J, qlds)"""
    V = (dim * ELEM[dt] + 15) // 16
    g = 1 if V <= 1 else 4 if V <= 4 else 8 if V <= 8 else 16 if V < 192 else 64
    if V % 8 != 0 and 16 < V < 192:
        g = 64 if V > 32 else 32
    g = forced or g
    J = (V + g - 1) // g
    qbytes = g * J * (32 if dt == "f16" else 16)
    return g, J, dt in ("i8", "u8") or qbytes <= LDS_QUERY_BYTES


def is_int(dt):
    return dt in ("i8", "u8")


def form_rows(dim):
    """rows of a form case's corpus: 3001; 300 from dimension 10240 on (about 12 MB of Float32)"""
    return 300 if dim >= 10240 else 3001


def form_ms(dim):
    """the list lengths a case rotates over: a wave and a tail, two strides of the block, ragged and full"""
    return (65, 257) if dim >= 10240 else (65, 257, 1000, 1024)


def _seed(*parts):
    import zlib
    return zlib.crc32(repr(parts).encode())


def form_world(dt, dim):
    """(rows [n, dim] in the storage type, queries [3, dim]: f32, or the integer type).  Integer rows are uniform over the
    type's range.  Float rows are six gaussian directions mixed with gaussian weights plus a tenth of full-dimension noise, each
    row scaled by a factor from U(0.5, 2): every element takes part in every sum, and the scores of a list spread as those of
    6-dimensional vectors do whatever the dimension -- gaussian rows of 10 000 dimensions have all their cosines within 0.03
    of each other, a few §3 tolerances per candidate, and no step of a walk over them would be decided."""
    n = form_rows(dim)
    rng = np.random.default_rng(_seed("mmr form world", dt, dim))
    if is_int(dt):
        lo, hi = INT_RANGE[dt]
        return (rng.integers(lo, hi + 1, (n, dim)).astype(NP_OF[dt]), rng.integers(lo, hi + 1, (3, dim)).astype(NP_OF[dt]))
    r = min(dim, 6)
    basis = rng.standard_normal((r, dim)) * np.sqrt(r / dim)
    mix = rng.standard_normal((n + 3, r)) @ basis + 0.1 * np.sqrt(r / dim) * rng.standard_normal((n + 3, dim))
    mix[:n] *= rng.uniform(0.5, 2.0, (n, 1))
    return np.ascontiguousarray(mix[:n].astype(NP_OF[dt])), np.ascontiguousarray(mix[n:].astype(np.float32))


def form_lists(dt, dim, tag, n, nq, m):
    """[nq, m] u64: query 0 lists m distinct rows (count = m); the others hold foreign entries, repeats and pads"""
    rng = np.random.default_rng(_seed("mmr form lists", dt, dim, tag, nq, m))
    lists = rng.integers(0, n + n // 10, size=(nq, m)).astype(np.uint64)
    lists[:, ::7] = PAD
    lists[0] = rng.permutation(n)[:m]
    return lists


def form_calls(ci, mi, dim, qlds):
    """the (m, k, lambda, nq) of case ci's calls under the mi-th metric: k = m (every position is picked: the last scoring
    passes run with almost every row taken) with one query, k = 3 (8 through the cache: the scratch row is rewritten while other
    waves have read it) with three, and the F64_K picks the float64 check follows"""
    ms = form_ms(dim)
    m1, m2 = ms[(ci + mi) % len(ms)], ms[(ci + mi + len(ms) // 2) % len(ms)]
    return [(m1, m1, LAMBDAS[(ci + mi) % 4], 1), (m2, 3 if qlds else 8, LAMBDAS[(ci + mi + 1) % 4], 3),
            (f64_m(ci, dim), F64_K, f64_lambda(ci, mi), 1)]


def f64_m(ci, dim):
    ms = form_ms(dim)
    return ms[(ci + 1) % len(ms)]


def f64_lambda(ci, mi):
    return (0.3, 0.5)[(ci + mi) % 2]


def f64_list(dt, dim, n, m):
    """the list of the float64 check (one per case, every metric): m distinct rows.  tests/test_mmr_cpu.py holds every case's
    seed to the clear-step condition"""
    rng = np.random.default_rng(_seed("mmr f64 list", dt, dim))
    return rng.permutation(n)[:m].astype(np.uint64)


# -- Int8 / UInt8: exact
def int_reference(rows, entries, query, metric, lam, k):
    """the expected output row of one query over Int8 / UInt8 rows from exact integers (W.int_raw -> W.int_scores) and the numpy
    walk, independent of every kernel: pick 0 by the exact integers, the later picks by the f32 objective"""
    import _wide as W
    from _candidates import candidate_rows
    sel = candidate_rows(entries, rows.shape[0])
    if sel.size == 0:
        return format_picks(metric, k, [], np.zeros(0, np.float32), None, None, None, 0)
    x = rows[sel]
    sc, key, raw = W.int_scores(metric, *W.int_raw(x, np.asarray(query)[None, :]))
    first = int(np.lexsort((np.arange(sel.size), key[0]))[0])
    sim = W.int_scores(metric, *W.int_raw(x, x))[0]            # sim[s, d]: row s as the query
    order, obj = numpy_walk(metric, sc[0], sim, lam, k, first=first)
    return format_picks(metric, k, order, obj, sc[0], sel.astype(np.uint64), raw[0], sel.size)


# -- floats: float64 along the kernel's own path
def f64_terms(rows_sel, query, tol_unit):
    """{metric: (rel f64 [c], sim f64 [c, c], tol_rel [c], tol_sim [c, c])} in SCORE form, from the exactly widened rows, the
    stored rows themselves as the queries of sim (sim[s, d]: row s as the query); tol: §3's tolerance of each score --
    tol_unit relative under L2, absolute under Cosine, x |q||x| under InnerProduct"""
    import _wide as W
    x64 = rows_sel.astype(np.float64)
    xn = np.sqrt(np.einsum("ij,ij->i", x64, x64))
    qn = float(np.linalg.norm(np.asarray(query, np.float64)))
    rel = W.f64_scores_all(rows_sel, np.asarray(query)[None, :])
    sim = W.f64_scores_all(rows_sel, rows_sel)
    out = {}
    for metric in (0, 1, 2):
        r, s = rel[metric][0], sim[metric]
        if metric == 0:
            tr, ts = tol_unit * np.abs(r), tol_unit * np.abs(s)
        elif metric == 2:
            tr, ts = np.full(r.shape, tol_unit), np.full(s.shape, tol_unit)
        else:
            tr, ts = tol_unit * qn * xn, tol_unit * xn[:, None] * xn[None, :]
        out[metric] = (r, s, tr, ts)
    return out


F32_ROUNDING = 2.0 ** -24


def f64_walk(metric, lam, terms, k, picks=None, objective=None, scores=None):
    """DESIGN.md §3's walk in float64, held along a given path: at step j, with `picks`[:j] as the history, the float64
    objective of every candidate not yet picked (step 0: the relevance alone) and its tolerance -- a tol(rel) + b (the largest
    tol of the sims that went into red) + three f32 roundings of the terms.  Asserted per step: the pick lies within the band
    (its tolerance plus the float64 maximum's) of the float64 maximum; where no second candidate lies within the band of the
    maximum (a CLEAR step) the pick is the maximum; of exact copies (equal rel and red in float64) the lowest position not yet
    picked is taken; the reported objective and score lie within their tolerances.  picks None: the float64 walk's own path
    (nothing to assert).  -> (unclear steps, the largest measured error as a fraction of its tolerance)."""
    rel_s, sim_s, tol_rel, tol_sim = terms
    sign = -1.0 if metric == L2 else 1.0
    relv = sign * rel_s
    a = float(np.float32(lam))
    b = float(np.float32(1.0) - np.float32(lam))
    c = relv.size
    taken = np.zeros(c, bool)
    red, redtol = np.full(c, -np.inf), np.zeros(c)
    unclear, worst = 0, 0.0
    for j in range(min(k, c)):
        free = np.nonzero(~taken)[0]
        if j == 0:
            obj, tol = relv, tol_rel
        else:
            with np.errstate(invalid="ignore"):
                obj = a * relv - b * red
                tol = a * tol_rel + b * redtol + F32_ROUNDING * (np.abs(a * relv) + np.abs(b * red) + np.abs(obj))
        top = int(free[np.argmax(obj[free])])
        others = free[free != top]
        clear = not ((obj[top] - obj[others]) <= (tol[top] + tol[others])).any()
        unclear += not clear
        p = top if picks is None else int(picks[j])
        if picks is not None:
            what = f"step {j}, pick {p}, the float64 maximum {top}"
            assert not taken[p], f"{what}: picked twice"
            gap, band = obj[top] - obj[p], tol[top] + tol[p]
            assert gap <= band, f"{what}: the pick's objective {obj[p]!r} lies {gap!r} under the maximum, beyond the band {band!r}"
            assert not clear or p == top, f"{what}: a clear step"
            copies = free[(relv[free] == relv[p]) & (red[free] == red[p]) & (free < p)]
            assert copies.size == 0, f"{what}: the copy at position {copies[:1]} holds the same objective and comes first"
            rep = a * relv[p] if j == 0 else obj[p]
            reptol = a * tol_rel[p] + F32_ROUNDING * abs(rep) if j == 0 else tol[p]
            eo, es = abs(float(objective[j]) - rep), abs(float(scores[j]) - rel_s[p])
            assert eo <= reptol, f"{what}: the reported objective {objective[j]!r} is {eo!r} off {rep!r}, tolerance {reptol!r}"
            assert es <= tol_rel[p], f"{what}: the reported score {scores[j]!r} is {es!r} off {rel_s[p]!r}, tolerance {tol_rel[p]!r}"
            worst = max([worst, eo / reptol if reptol > 0 else 0.0, es / tol_rel[p] if tol_rel[p] > 0 else 0.0,
                         gap / band if band > 0 else 0.0])
        taken[p] = True
        red = np.maximum(red, sign * sim_s[p])
        redtol = np.maximum(redtol, tol_sim[p])
    return unclear, worst


def wrong_walk(metric, rel_scores, sim_scores, lam, k, model):
    """numpy float32 models of walks that are wrong in one way -> (order, objective) as numpy_walk's: "top_k" ignores red,
    "sum" adds the sims up where the contract takes their maximum, "l2_sign" takes the sim's SCORE for its value (wrong under
    L2 only), "descending" breaks ties by descending position"""
    rel = value(metric, rel_scores)
    c = rel.size
    a = np.float32(lam)
    b = np.float32(1.0) - a
    red = np.zeros(c, np.float32) if model == "sum" else np.full(c, -np.inf, np.float32)
    taken = np.zeros(c, bool)
    order, objective = [], []
    for j in range(min(k, c)):
        obj = rel if j == 0 else ((a * rel) if model == "top_k" else (a * rel) - (b * red))
        free = np.nonzero(~taken)[0]
        best = obj[free].max()
        tied = free[obj[free] == best]
        s = int(tied[-1] if model == "descending" else tied[0])
        order.append(s)
        objective.append(a * rel[s] if j == 0 else obj[s])
        taken[s] = True
        sim = np.asarray(sim_scores[s], np.float32) if model == "l2_sign" else value(metric, sim_scores[s])
        red = (red + sim).astype(np.float32) if model == "sum" else np.maximum(red, sim)
    return order, np.array(objective, np.float32)


# -- duplicate rows: ties at the ownership edges (tests/_dups.py corpus_b)
DUP_N, DUP_DIM, DUP_M, DUP_SEED = 3000, 96, 1024, 4096


def dup_list(n=DUP_N, m=DUP_M, seed=DUP_SEED):
    return np.sort(np.random.default_rng(seed).permutation(n)[:m]).astype(np.uint64)


def tie_edges(groups):
    """groups [c]: the vector of every list position (ascending row = D0's position i) -> the ownership edges tied copies
    straddle: (two waves, two 256-strides of the block, one thread's two strides)"""
    i = np.arange(groups.size)
    waves = strides = thread = False
    for g in np.unique(groups):
        at = i[groups == g]
        waves |= np.unique((at % 256) // 64).size > 1
        strides |= np.unique(at // 256).size > 1
        lanes = at % 256
        thread |= np.unique(lanes).size < lanes.size
    return bool(waves), bool(strides), bool(thread)


def first_descending_copy(picks, groups):
    """picks: positions in pick order -> (rank a, rank b), a < b, of two copies of one vector picked in descending position, or
    None: untaken copies always hold bit-equal objectives, so the lower position goes first"""
    picks = np.asarray(picks, np.int64)
    last = {}
    for r, p in enumerate(picks.tolist()):
        g = int(groups[p])
        if g in last and picks[last[g]] > p:
            return last[g], r
        last[g] = r
    return None


# -- Float16 format edges (tests/_edges.py): one K1 shape of 32 lanes, two queries of its pool
EDGE_SHAPE, EDGE_M, EDGE_K, EDGE_LAMBDA = "d200", 257, 257, 0.3   # k = m: rows of every scale are picked


def edge_lists(case):
    return form_lists("f16", case.dim, "edges", case.n, 2, EDGE_M)


# ---- the fresh-process scenario (tests/test_gpu_mmr.py: test_a_fresh_poisoned_process) ------------------------------------------
FP_N, FP_DIM, FP_M, FP_K, FP_NQ, FP_LAMBDA, FP_METRIC = 3001, 100, 257, 40, 3, 0.3, 2


def fresh_inputs():
    rng = np.random.default_rng(20250)
    rows = rng.standard_normal((FP_N, FP_DIM)).astype(np.float16)
    queries = rng.standard_normal((FP_NQ, FP_DIM)).astype(np.float32)
    lists = rng.integers(0, FP_N + 100, size=(FP_NQ, FP_M)).astype(np.uint64)
    lists[:, ::9] = PAD
    return rows, queries, lists


def main(argv):
    if len(argv) != 2:
        print("usage: _mmr.py <out.npz>", file=sys.stderr)
        return 2
    sys.modules.setdefault("torch", None)  # the binding would load torch's HIP runtime first where torch is installed
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from metrovector_amd import gpu as G
    rows, queries, lists = fresh_inputs()
    out = {}
    with G.GpuCorpus.from_array(rows) as c:
        res = c.search_mmr(queries, lists, FP_K, FP_LAMBDA, FP_METRIC)  # the child's first search
        out["scores"], out["indices"], out["raw"], out["objective"], out["counts"] = res.scores, res.indices, res.raw, res.objective, res.counts
    out["poison"] = np.array([G.selftest_poison()], np.int32)
    np.savez(argv[1], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
