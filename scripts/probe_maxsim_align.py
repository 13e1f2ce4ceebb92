"""MaxSim alignments (mvfgpu_maxsim_align_device; DESIGN.md §5 "M0-arg and the alignment writer"): its stages against the
candidate multi-vector search's M0 on the same lists in the same process, and against the recipe it replaces.

  workloads 1. 10M x 768 Float32, Cosine, 100 000 keys of 100 rows      2. 50M x 128 Float16, InnerProduct, 500 000 keys
  lists     m = 100, 1000, 10 000, drawn at random without repeats, a different list per query set
  batches   nq = 1 and nq = 64;   T = 32 tokens
  stages    mvfgpu_selftest_maxsim_align_stage_ms: plan upload + E0 / M0-arg / writer, summed over chunks and windows
  baseline  the M0 stage of mvfgpu_selftest_maxsim_candidates_stage_ms (k = m) on the same lists, alternating with the above
  recipe    the wall time of ONE mvfgpu_search_partitioned call over the nq T m (token, key) pairs at k = 1, host buffers; left
            out ("not measured") where the pairs exceed --recipe-pairs

`rounds` of each after one warm round, median; the ratio M0-arg / M0 stands next to the baseline's own spread (max - min over its
rounds, relative to its median).

    python scripts/probe_maxsim_align.py [--only 1 2] [--rows1 10000000] [--rows2 50000000] [--out profiles/r23_maxsim_align.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metrovector_amd import gpu as G  # noqa: E402

ROWS_PER_KEY = 100


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def main() -> None:
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows1", type=int, default=10_000_000)
    ap.add_argument("--rows2", type=int, default=50_000_000)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--m", type=int, nargs="+", default=[100, 1000, 10_000])
    ap.add_argument("--only", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--recipe-pairs", type=int, default=400_000, help="the recipe is timed up to this many (token, key) pairs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    T, R = args.tokens, args.rounds
    lines = [f"MaxSim alignments against the candidate search's M0 on the same lists.  One MI355X, synthetic rows, keys of {ROWS_PER_KEY} rows",
             f"scattered over all positions, UInt32 key column, T = {T}, random lists without repeats, a different one per query set;",
             f"scripts/probe_maxsim_align.py.  Stage times in ms from device events (the stage timers), the two calls alternating in one",
             f"process, median of {R} after a warm round; spread = (max - min) / median over the baseline's rounds.  recipe: the wall time",
             "of one mvfgpu_search_partitioned call over the nq T m (token, key) pairs at k = 1, host buffers.", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:  # as it goes: a run that is cut short leaves what it measured
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    stream = torch.cuda.current_stream().cuda_stream
    works = {1: (args.rows1, 768, G.FLOAT32, G.COSINE, "Float32, Cosine"), 2: (args.rows2, 128, G.FLOAT16, G.INNER_PRODUCT, "Float16, InnerProduct")}
    for work in args.only:
        n, dim, dtype, metric, what = works[work]
        rng = np.random.default_rng(n)
        col = np.empty(n, np.uint32)
        col[rng.permutation(n)] = (np.arange(n) // ROWS_PER_KEY).astype(np.uint32)
        with G.GpuCorpus.synthetic(n, dim, dtype, 1) as c, c.attach_column(col) as dc, c.make_partition(dc) as part:
            inf = part.info()
            nk, pitch = int(inf.n_keys), int(c.info().pitch_bytes)
            keys = part.keys()[0]
            token_bytes = G.maxsim_form(dtype, dim).token_bytes
            say(f"{work}. {n} x {dim} {what}: {nk} keys, {int(inf.live_rows)} held rows of {pitch} bytes, a padded token of {token_bytes} bytes")
            for nq in args.nq:
                q = torch.randn((nq, T, dim), dtype=torch.float32, device="cuda")
                for m in args.m:
                    mm = min(m, nk)
                    lists = np.stack([rng.choice(keys, mm, replace=False) for _ in range(nq)])
                    n_out = nq * mm * T
                    a_sc = torch.empty(n_out, dtype=torch.float32, device="cuda")
                    a_rows = torch.empty(n_out, dtype=torch.int64, device="cuda")
                    a_raw = torch.empty(n_out, dtype=torch.int32, device="cuda")
                    c_sc = torch.empty((nq, mm), dtype=torch.float32, device="cuda")
                    c_keys = torch.empty((nq, mm), dtype=torch.int64, device="cuda")

                    def align():
                        return c.maxsim_align_stage_ms(part, q.data_ptr(), 0, dim, nq, T, lists, metric, a_sc.data_ptr(), a_rows.data_ptr(),
                                                       a_raw.data_ptr(), stream)

                    def cand():
                        return c.maxsim_candidates_stage_ms(part, q.data_ptr(), 0, dim, nq, T, lists, mm, metric, c_sc.data_ptr(), c_keys.data_ptr(), stream)

                    align(), cand()
                    sa, sc = [], []
                    for r in range(R):   # alternating order
                        for fn, to in ((align, sa), (cand, sc)) if r % 2 == 0 else ((cand, sc), (align, sa)):
                            to.append(fn())
                    e0, m0a, wr = (med([s[i] for s in sa]) for i in range(3))
                    m0s = [s[1] for s in sc]
                    m0 = med(m0s)
                    spread = (max(m0s) - min(m0s)) / m0
                    ratio = m0a / m0
                    chunk = G.maxsim_align_plan(mm, T, 1, token_bytes, 512 << 20)[0]
                    crow = nq * mm * ROWS_PER_KEY
                    say(f"   nq {nq:3d}  m {mm:6d}: plan + E0 {e0:8.3f}  M0-arg {m0a:9.3f}  writer {wr:7.3f} ms;  candidate search's M0 {m0:9.3f} ms "
                        f"[{min(m0s):.3f}, {max(m0s):.3f}], spread {100 * spread:.2f} %;  M0-arg / M0 = {ratio:.3f} "
                        f"({'inside' if abs(ratio - 1.0) <= spread else 'OUTSIDE'} the spread);  "
                        f"{crow * pitch * -(-T // chunk) / (m0a * 1e-3) / 1e12:.3f} TB/s of gathered row bytes in {-(-T // chunk)} chunks of up to {chunk} tokens")
                    # identity 2 on the probe's own data: a key's scores summed in token order are the candidate search's score
                    s = a_sc.view(nq, mm, T)
                    total = s[:, :, 0].clone()
                    for t in range(1, T):
                        total = total + s[:, :, t]
                    order = torch.argsort(torch.from_numpy(lists.astype(np.int64)).cuda(), dim=1)
                    by_key = torch.gather(total, 1, order)
                    csort = torch.argsort(c_keys, dim=1)
                    same = bool((torch.gather(c_sc, 1, csort).view(torch.int32) == by_key.view(torch.int32)).all())
                    say(f"      the scores' f32 sums in token order equal the candidate search's score bits: {same}")
                    pairs = nq * T * mm
                    if pairs > args.recipe_pairs:
                        say(f"      recipe: not measured ({pairs} pairs exceed --recipe-pairs {args.recipe_pairs})")
                        continue
                    hq = np.ascontiguousarray(np.broadcast_to(q.cpu().numpy()[:, None, :, :], (nq, mm, T, dim))).reshape(pairs, dim)
                    hk = np.repeat(lists.reshape(-1), T)
                    c.search_partitioned(hq[:T], hk[:T], 1, metric, part)
                    walls = []
                    for _ in range(R):
                        t0 = time.perf_counter()
                        res = c.search_partitioned(hq, hk, 1, metric, part)
                        walls.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    got = c.maxsim_align(q.cpu().numpy(), lists, metric, part)
                    wall_align = (time.perf_counter() - t0) * 1e3
                    same = bool((got.rows.reshape(-1) == res.indices.reshape(-1)).all()) and \
                        bool((got.scores.reshape(-1).view(np.uint32) == res.scores.reshape(-1).view(np.uint32)).all())
                    say(f"      recipe: {med(walls):10.3f} ms wall for {pairs} partitioned searches at k = 1 {[round(x, 1) for x in walls]};  the host "
                        f"call mvfgpu_maxsim_align: {wall_align:.3f} ms wall = {wall_align / med(walls):.4f} x;  the same rows and score bits: {same}")
            say("")


if __name__ == "__main__":
    main()
