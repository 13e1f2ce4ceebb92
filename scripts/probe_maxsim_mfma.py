"""The multi-vector search's MFMA selection route against the one-pass route (mvfgpu_set_maxsim_route; DESIGN.md §5 "A0 / P0").

  workloads 1. 10M x 768 Float32, Cosine      2. 50M x 128 Float16, InnerProduct (the ColBERT shape)
  column    keys of 100 rows (rows / 100 keys), every key scattered over all positions
  tokens    T = 32 and 128;   nq = 1 and 16 query sets;   k = 100
  routes    1 and 2 through mvfgpu_search_maxsim_device on the same handle and partition, alternating inside one process
  stages    mvfgpu_selftest_maxsim_mfma_stage_ms: preparation / A0 / sums + kth best + P0 / M0 over the candidates' blocks /
            M1 + mask / tail, the candidate keys and the blocks scored again per set
  A0        its row bytes per second (the held rows once per chunk of tokens) against 8 TB/s, its flop rate (2 x rows x padded
            dimension x query rows) against 157.3 TF

Device events around each route on one stream, `rounds` each after one warm round: the median and the spread (max - min).
The yardstick is route 1 in the same process.

    python scripts/probe_maxsim_mfma.py [--only 1 2] [--rows1 10000000] [--rows2 50000000] [--out profiles/r18_maxsim_mfma.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metrovector_amd import gpu as G  # noqa: E402

HBM_TBS, MFMA_F32_TF = 8.0, 157.3


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def spread(xs):
    return float(max(xs) - min(xs))


def column(n):
    """keys of 100 rows, shuffled so that every key is scattered over all positions"""
    perm = np.random.default_rng(n).permutation(n)
    c = np.empty(n, np.uint32)
    c[perm] = (np.arange(n) // 100).astype(np.uint32)
    return c


def main() -> None:
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows1", type=int, default=10_000_000)
    ap.add_argument("--rows2", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--only", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    k = args.k
    lines = ["Multi-vector search: the MFMA selection route (2) against the one-pass route (1).  One MI355X, synthetic rows, keys of 100",
             f"rows, k = {k}, UInt32 key column; scripts/probe_maxsim_mfma.py.  ms: device events around the call on one stream, the routes",
             f"alternating in one process, median of {args.rounds} after a warm round, (spread = max - min of the {args.rounds}).", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:  # as it goes: a run that is cut short leaves what it measured
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    stream = torch.cuda.current_stream().cuda_stream
    works = {1: (args.rows1, 768, G.FLOAT32, G.COSINE, "Float32, Cosine", 64 * 3 * 16),
             2: (args.rows2, 128, G.FLOAT16, G.INNER_PRODUCT, "Float16, InnerProduct", 16 * 1 * 32)}
    tmax, qmax = max(args.tokens), max(args.sets)
    for work in args.only:
        n, dim, dtype, metric, what, token_bytes = works[work]
        say(f"{work}. {n} x {dim} {what}")
        col = column(n)
        with G.GpuCorpus.synthetic(n, dim, dtype, 1) as c:
            pitch = int(c.info().pitch_bytes)
            q = torch.randn((qmax, tmax, dim), dtype=torch.float32, device="cuda")
            ds = torch.empty((qmax, k), dtype=torch.float32, device="cuda")
            dk = torch.empty((qmax, k), dtype=torch.int64, device="cuda")
            with c.attach_column(col) as dc, c.make_partition(dc) as part:
                inf = part.info()
                nk, live = int(inf.n_keys), int(inf.live_rows)
                say(f"   {nk} keys, largest {inf.largest}, {-(-live // 128)} blocks of 128 list positions")
                for T in args.tokens:
                    for nq in args.sets:
                        sets = q[:nq, :T].contiguous()

                        def search(route):
                            c.set_maxsim_route(route)
                            c.search_maxsim_device(part, sets.data_ptr(), 0, dim, nq, T, k, metric, ds.data_ptr(), dk.data_ptr(), 0, stream)

                        search(1), search(2)  # the warm round (route 2's builds the row norms)
                        t1, t2 = [], []
                        for _ in range(args.rounds):
                            t1.append(timed(lambda: search(1)))
                            t2.append(timed(lambda: search(2)))
                        c.set_maxsim_route(0)
                        st = [c.maxsim_mfma_stage_ms(part, sets.data_ptr(), 0, dim, nq, T, k, metric, ds.data_ptr(), dk.data_ptr(), stream)
                              for _ in range(args.rounds + 1)][1:]
                        ms = [med([s[0][i] for s in st]) for i in range(6)]
                        cand, blocks = st[-1][1], st[-1][2]
                        chunk = G.maxsim_plan(nk, T, nq, 0, 512 << 20)[0]  # A0's own chunk: no tokens in LDS
                        passes = -(-T // chunk)
                        kpad = -(-pitch // 32) * 32 // (4 if dtype == G.FLOAT32 else 2)
                        tbs = live * pitch * passes / (ms[1] * 1e-3) / 1e12
                        tf = 2.0 * live * kpad * nq * T / (ms[1] * 1e-3) / 1e12
                        say(f"   T {T:3d} nq {nq:2d}: route 1 {med(t1):9.3f} ms (spread {spread(t1):.3f})   route 2 {med(t2):9.3f} ms (spread {spread(t2):.3f})"
                            f"   route 2 / route 1 {med(t2) / med(t1):.3f}")
                        say(f"             rounds: route 1 {[round(x, 3) for x in t1]}  route 2 {[round(x, 3) for x in t2]}")
                        say(f"             stages: preparation {ms[0]:.3f}  A0 {ms[1]:.3f}  sums + kth + P0 {ms[2]:.3f}  M0 over candidates {ms[3]:.3f}"
                            f"  M1 + mask {ms[4]:.3f}  tail {ms[5]:.3f} ms")
                        say(f"             candidates per set: min {int(cand.min())} max {int(cand.max())} of {nk} keys;  blocks scored again per set: "
                            f"min {int(blocks.min())} max {int(blocks.max())}")
                        say(f"             A0: {passes} chunks of up to {chunk} tokens: {tbs:.3f} TB/s of row bytes ({100 * tbs / HBM_TBS:.0f} % of {HBM_TBS} TB/s), "
                            f"{tf:.1f} TF ({100 * tf / MFMA_F32_TF:.0f} % of {MFMA_F32_TF} TF)")
            say("")


if __name__ == "__main__":
    main()
