"""Candidate search (mvfgpu_search_candidates_device): device ms per call, timed with HIP events around the call on one
torch stream inside this process (median of 5 after 2 warm calls), and the gathered rate nq * m * row bytes / time.  The
full top-k search of the same queries (mvfgpu_search_device) is timed the same way for contrast; the one-query case is
the blocking host call's wall time.  Lists are uniform random rows of the synthetic corpus.

    python scripts/probe_candidates.py [--out profiles/r07_candidates.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metrovector_amd import gpu as G  # noqa: E402
from oracle import mvf_oracle as O  # noqa: E402

SEED = 0x4D564631
ES = {G.FLOAT32: 4, G.FLOAT16: 2, G.INT8: 1, G.UINT8: 1}
NAME = {G.FLOAT32: "f32", G.FLOAT16: "f16", G.INT8: "int8", G.UINT8: "uint8"}
METRIC = {G.L2: "L2", G.INNER_PRODUCT: "IP", G.COSINE: "cosine"}


def device_ms(fn, stream, reps=5):
    for _ in range(2):
        fn()
    stream.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("candidate search, MI355X, synthetic corpora, k = 100, device ms = HIP events around one call on a torch stream "
        "(median of 5), gathered TB/s = nq * m * row bytes / device time")
    st = torch.cuda.Stream()
    rng = np.random.default_rng(7)
    cases = [(10_000_000, 768, G.FLOAT32, G.COSINE, [(1024, 1000, "uniform random"), (1024, 1000, "same rows sorted"),
                                                    (1024, 10000, "uniform random")]),
             (50_000_000, 768, G.INT8, G.INNER_PRODUCT, [(256, 1000, "uniform random")]),
             (12_500_000, 1024, G.FLOAT16, G.L2, [(1024, 1000, "uniform random")])]
    k = 100
    for n, dim, dt, metric, shapes in cases:
        rb = dim * ES[dt]
        with G.GpuCorpus.synthetic(n, dim, dt, SEED) as c:
            for nq, m, kind in shapes:
                qs = O.synth_queries(SEED + nq, nq, dim, dt)
                dq = torch.from_numpy(qs).cuda()
                lists = rng.integers(0, n, size=(nq, m)).astype(np.uint64)
                if kind.startswith("same rows sorted"):
                    lists = np.sort(lists, axis=1)
                dl = torch.from_numpy(lists.view(np.int64)).cuda()
                ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                di = torch.empty((nq, k), dtype=torch.int64, device="cuda")
                dc = torch.empty(nq, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                t = device_ms(lambda: c.search_candidates_device(dq.data_ptr(), dt if dt in (G.INT8, G.UINT8) else G.FLOAT32, dim,
                                                                 nq, dl.data_ptr(), m, k, metric, ds.data_ptr(), di.data_ptr(),
                                                                 0, dc.data_ptr(), st.cuda_stream), st)
                tb = nq * m * rb / (t * 1e-3) / 1e12
                cnt = int(dc.cpu().numpy().sum())
                line = (f"{n / 1e6:g}M x {dim} {NAME[dt]:4s} {METRIC[metric]:6s}: "
                        f"{nq:5d} x {m:5d} {kind:16s}: {t:8.3f} ms  gathered {tb:5.2f} TB/s  (distinct rows {cnt})")
                if kind == "uniform random" and m == 1000:
                    t_full = device_ms(lambda: c.search_device(dq.data_ptr(), dt if dt in (G.INT8, G.UINT8) else G.FLOAT32, dim,
                                                               nq, k, metric, ds.data_ptr(), di.data_ptr(), 0, st.cuda_stream), st)
                    line += f"  | full top-{k} search of the same queries {t_full:8.3f} ms"
                say(line)
            if dt == G.FLOAT32:  # one query, the blocking host call
                q = O.synth_queries(SEED + 1, 1, dim, dt)
                lst = rng.integers(0, n, size=(1, 10000)).astype(np.uint64)
                for _ in range(2):
                    c.search_candidates(q, lst, k, metric)
                ts = []
                for _ in range(9):
                    t0 = time.perf_counter()
                    c.search_candidates(q, lst, k, metric)
                    ts.append(time.perf_counter() - t0)
                t = float(np.median(ts)) * 1e3
                say(f"{n / 1e6:g}M x {dim} {NAME[dt]:4s}: {1:5d} x {10000:5d} uniform random  : host call wall {t:8.3f} ms "
                    f"(median of 9)  gathered {10000 * rb / (t * 1e-3) / 1e12:5.2f} TB/s")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
