"""What the diversified re-ranking's tests share (tests/test_mmr_cpu.py, tests/test_gpu_mmr.py; DESIGN.md §3 "Diversified
re-ranking"): the stream classes of include/mvf_gpu_mmr.h's functions, the greedy walk restated in numpy float32, the recipe
that builds a call's expected bytes from the library's own candidate searches, and -- run as a program,
`python tests/_mmr.py <out.npz>` -- the parity case the GPU tests start as a fresh (poisoned) child process.
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
