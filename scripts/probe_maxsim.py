"""Multi-vector search (mvfgpu_search_maxsim_device; DESIGN.md §5 "M0 / M1 — multi-vector search"): its stages, M0 against one
G0 pass of the grouped search, and the recipe it replaces.

  workloads 1. 10M x 768 Float32, Cosine      2. 50M x 128 Float16, InnerProduct (the ColBERT shape)
  columns   a. keys of 100 rows (rows / 100 keys)      b. Zipf-sized keys;   every key scattered over all positions
  tokens    T = 32 and 128;   one query set;   k = 100
  stages    mvfgpu_selftest_maxsim_stage_ms: key ordinals / M0 / M1 / tail, summed over the call's chunks
  G0        mvfgpu_selftest_grouped_stage_ms with four queries on the same handle: one gathered pass over all held rows
  recipe    the T tokens through mvfgpu_search_grouped_device, per_key = 1, k = n_keys, 32 tokens per call; its host-side
            summing and sorting are left out, which favours the recipe

Device events around each variant on one stream, the variants alternating inside one process, `rounds` each after one warm
round, median.

    python scripts/probe_maxsim.py [--only 1 2] [--rows1 10000000] [--rows2 50000000] [--out profiles/r16_maxsim.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metrovector_amd import gpu as G  # noqa: E402

RECIPE_SLICE = 32  # tokens per grouped call of the recipe: its result rows are n_keys long


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def columns(n):
    """the two key columns over n rows, shuffled so that every key is scattered over all positions"""
    rng = np.random.default_rng(n)
    perm = rng.permutation(n)
    out = {}
    c = np.empty(n, np.uint32)
    c[perm] = (np.arange(n) // 100).astype(np.uint32)
    out["a"] = c
    sizes = np.minimum(rng.zipf(1.3, n // 4), max(n // 10, 1)).astype(np.int64)  # Zipf(1.3) sizes, at most a tenth of the rows each
    nkeys = int(np.searchsorted(np.cumsum(sizes), n)) + 1
    sizes = sizes[:nkeys]
    sizes[-1] -= int(sizes.sum()) - n
    c = np.empty(n, np.uint32)
    c[perm] = np.repeat(np.arange(nkeys, dtype=np.uint32), sizes)
    out["b"] = c
    return out


def main() -> None:
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows1", type=int, default=10_000_000)
    ap.add_argument("--rows2", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--only", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    k = args.k
    lines = [f"Multi-vector search: stages, M0 against one G0 pass, and the recipe of grouped searches.  One MI355X, synthetic rows, one",
             f"query set, k = {k}, UInt32 key column; scripts/probe_maxsim.py.  ms: device events around the variant on one stream, the",
             f"variants alternating in one process, median of {args.rounds} after a warm round.", ""]

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
    # (rows, dimension, type, metric, words, bytes of a padded token in LDS: the one-query lane group's G x J vectors of 16 (f32
    # rows) or 32 bytes (f16 rows) -- 64 x 3 and 16 x 1 here)
    works = {1: (args.rows1, 768, G.FLOAT32, G.COSINE, "Float32, Cosine", 64 * 3 * 16),
             2: (args.rows2, 128, G.FLOAT16, G.INNER_PRODUCT, "Float16, InnerProduct", 16 * 1 * 32)}
    names = {"a": "keys of 100 rows", "b": "Zipf-sized keys"}
    tmax = max(args.tokens)
    for work in args.only:
        n, dim, dtype, metric, what, token_bytes = works[work]
        say(f"{work}. {n} x {dim} {what}")
        cols = columns(n)
        with G.GpuCorpus.synthetic(n, dim, dtype, 1) as c:
            pitch = int(c.info().pitch_bytes)
            q = torch.randn((tmax, dim), dtype=torch.float32, device="cuda")
            ds = torch.empty((k,), dtype=torch.float32, device="cuda")
            dk = torch.empty((k,), dtype=torch.int64, device="cuda")
            g4s = torch.empty((4, k), dtype=torch.float32, device="cuda")
            g4i = torch.empty((4, k), dtype=torch.int64, device="cuda")
            for which in ("a", "b"):
                with c.attach_column(cols[which]) as dc, c.make_partition(dc) as part:
                    inf = part.info()
                    nk = int(inf.n_keys)
                    say(f"   {which}. {names[which]}: {nk} keys, largest {inf.largest}")
                    rs = torch.empty((RECIPE_SLICE, nk), dtype=torch.float32, device="cuda")
                    ri = torch.empty((RECIPE_SLICE, nk), dtype=torch.int64, device="cuda")
                    g0 = [c.grouped_stage_ms(part, q.data_ptr(), 0, dim, 4, k, 1, metric, g4s.data_ptr(), g4i.data_ptr(), stream)[1]
                          for _ in range(args.rounds + 1)][1:]
                    say(f"      one G0 pass (four queries): {med(g0):.3f} ms {[round(x, 3) for x in g0]}")
                    for T in args.tokens:
                        def maxsim():
                            c.search_maxsim_device(part, q.data_ptr(), 0, dim, 1, T, k, metric, ds.data_ptr(), dk.data_ptr(), 0, stream)

                        def recipe():
                            for t0 in range(0, T, RECIPE_SLICE):
                                tn = min(RECIPE_SLICE, T - t0)
                                c.search_grouped_device(part, q.data_ptr() + t0 * dim * 4, 0, dim, tn, nk, 1, metric, rs.data_ptr(), ri.data_ptr(), 0, stream)

                        maxsim(), recipe()
                        tm, tr = [], []
                        for _ in range(args.rounds):
                            tm.append(timed(maxsim))
                            tr.append(timed(recipe))
                        st = [c.maxsim_stage_ms(part, q.data_ptr(), 0, dim, 1, T, k, metric, ds.data_ptr(), dk.data_ptr(), stream)
                              for _ in range(args.rounds + 1)][1:]
                        o, m0, m1, tail = (med([s[i] for s in st]) for i in range(4))
                        chunk = G.maxsim_plan(nk, T, 1, token_bytes, 512 << 20)[0]
                        passes = -(-T // chunk)
                        say(f"      T {T:3d}: maxsim {med(tm):9.3f} ms   recipe {med(tr):10.3f} ms   maxsim / recipe {med(tm) / med(tr):.3f}")
                        say(f"             rounds: maxsim {[round(x, 3) for x in tm]}  recipe {[round(x, 3) for x in tr]}")
                        say(f"             stages: ordinals {o:.3f}  M0 {m0:.3f}  M1 {m1:.3f}  tail {tail:.3f} ms;  M0 / one G0 pass = {m0 / med(g0):.2f};"
                            f"  M0 per token {m0 / T:.3f} ms")
                        say(f"             M0: {passes} chunks of up to {chunk} tokens, the held rows read once per chunk: "
                            f"{int(inf.live_rows) * pitch * passes / (m0 * 1e-3) / 1e12:.3f} TB/s of row bytes")
            say("")


if __name__ == "__main__":
    main()
