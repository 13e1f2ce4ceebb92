"""Diversified re-ranking (mvfgpu_search_mmr[_device], include/mvf_gpu_mmr.h) on one MI355X: per shape
  * the two stage times of the device call (mvfgpu_selftest_mmr_stage_ms: C0 + relevance, D0), median of the timed calls;
  * D0's algorithmic bytes -- sum over the queries of (min(k, count) - 1) x count x row pitch, a count, read from the cache --
    over D0's time;
  * the whole device call between HIP events on one torch stream, and mvfgpu_search_candidates_device alone on the same lists
    at the same k: the floor;
  * the blocking host call's wall time against THE HOST RECIPE IT REPLACES, timed in the same process and alternating with it:
    per query a candidate search with k = m, gather_rows of its rows, a candidate search of those rows as queries over the
    same list, and the greedy walk in numpy float32 (tests/_mmr.py: recipe) -- whose bytes the call must reproduce, checked
    for the first query of every shape.
Every shape is warmed up; each figure is the median of the timed repetitions with their minimum and maximum.  Candidate lists
are the fetch_k = m best rows of each query (mvfgpu_search).

    python scripts/probe_mmr.py [--out profiles/r19_mmr.txt] [--small]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _mmr as MM  # noqa: E402
from metrovector_amd import gpu as G  # noqa: E402
from oracle import mvf_oracle as O  # noqa: E402

SEED = 0x4D564631
ES = {G.FLOAT32: 4, G.FLOAT16: 2}
NAME = {G.FLOAT32: "f32", G.FLOAT16: "f16"}
METRIC = {G.L2: "L2", G.INNER_PRODUCT: "IP", G.COSINE: "cosine"}
LAMBDA = 0.5


def spread(ts):
    return f"{np.median(ts):9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def event_ms(fn, stream, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 100k-row corpora, 1 and 8 queries")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"diversified re-ranking (MMR), MI355X, synthetic corpora, lambda = {LAMBDA}; lists = each query's fetch_k = m best rows; "
        "median [min .. max] of the timed repetitions after a warm-up of every shape")
    say("stages / device call / floor: HIP events, device pointers;  host call / recipe: wall clock around blocking host-buffer "
        "calls, alternating;  D0 rate: algorithmic bytes (a count; the rows are re-read from the cache) over D0's time")
    st = torch.cuda.Stream()
    cases = [(10_000_000, 768, G.FLOAT32, G.COSINE), (50_000_000, 128, G.FLOAT16, G.INNER_PRODUCT)]
    nqs = [1, 64, 1024]
    if a.small:
        cases = [(100_000, 768, G.FLOAT32, G.COSINE), (100_000, 128, G.FLOAT16, G.INNER_PRODUCT)]
        nqs = [1, 8]
    for n, dim, dt, metric in cases:
        pitch = (dim * ES[dt] + 15) // 16 * 16
        with G.GpuCorpus.synthetic(n, dim, dt, SEED) as c:
            for m, k in [(20, 4), (100, 10), (1000, 100)]:
                for nq in nqs:
                    qs = O.synth_queries(SEED + nq + m, nq, dim, dt)
                    lists = np.ascontiguousarray(c.search(qs, m, metric).indices)
                    dq = torch.from_numpy(qs).cuda()
                    dl = torch.from_numpy(lists.view(np.int64)).cuda()
                    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                    di = torch.empty((nq, k), dtype=torch.int64, device="cuda")
                    dc = torch.empty(nq, dtype=torch.int64, device="cuda")
                    torch.cuda.synchronize()
                    reps = 5 if nq * m * k <= 64 * 1000 * 100 else 3

                    def dev_call():
                        c.search_mmr_device(dq.data_ptr(), G.FLOAT32, dim, nq, dl.data_ptr(), m, k, LAMBDA, metric, ds.data_ptr(),
                                            di.data_ptr(), 0, 0, dc.data_ptr(), st.cuda_stream)

                    def floor_call():
                        c.search_candidates_device(dq.data_ptr(), G.FLOAT32, dim, nq, dl.data_ptr(), m, k, metric, ds.data_ptr(),
                                                   di.data_ptr(), 0, dc.data_ptr(), st.cuda_stream)

                    def stages():
                        return c.mmr_stage_ms(dq.data_ptr(), G.FLOAT32, dim, nq, dl.data_ptr(), m, k, LAMBDA, metric, ds.data_ptr(),
                                              di.data_ptr(), st.cuda_stream)

                    def recipe_all():
                        return [MM.recipe(c, metric, qs[j], lists[j], k, LAMBDA) for j in range(nq)]

                    # warm-up of every timed form at this shape
                    dev_call(), floor_call(), stages()
                    st.synchronize()
                    got = c.search_mmr(qs, lists, k, LAMBDA, metric)
                    want0 = MM.recipe(c, metric, qs[0], lists[0], k, LAMBDA)
                    same = all(x.tobytes() == y.tobytes() for x, y in zip(
                        (got.scores[0], got.indices[0], got.raw[0], got.objective[0], got.counts[0]), want0))
                    t_dev = event_ms(dev_call, st, reps)
                    t_floor = event_ms(floor_call, st, reps)
                    sm = np.array([stages() for _ in range(reps)])
                    cnt = got.counts.astype(np.int64)
                    d0_bytes = int(((np.minimum(cnt, k) - 1).clip(min=0) * cnt).sum()) * pitch
                    t_host, t_recipe = [], []
                    for _ in range(reps):  # alternating
                        t0 = time.perf_counter()
                        c.search_mmr(qs, lists, k, LAMBDA, metric)
                        t1 = time.perf_counter()
                        recipe_all()
                        t2 = time.perf_counter()
                        t_host.append((t1 - t0) * 1e3)
                        t_recipe.append((t2 - t1) * 1e3)
                    d0 = float(np.median(sm[:, 1]))
                    say(f"{n / 1e6:g}M x {dim} {NAME[dt]} {METRIC[metric]:6s} m {m:4d} k {k:3d} nq {nq:4d}: "
                        f"C0+relevance {spread(sm[:, 0])}  D0 {spread(sm[:, 1])}  D0 {d0_bytes / 1e6:9.1f} MB -> {d0_bytes / (d0 * 1e-3) / 1e9:8.1f} GB/s")
                    say(f"{'':45s} device call {spread(t_dev)}  floor (search_candidates_device) {spread(t_floor)}")
                    say(f"{'':45s} host call   {spread(t_host)}  host recipe {spread(t_recipe)}  "
                        f"recipe / call {np.median(t_recipe) / np.median(t_host):7.1f}x  first query's bytes equal the recipe's: {'yes' if same else 'NO'}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
