"""Candidate multi-vector search (mvfgpu_search_maxsim_candidates_device; DESIGN.md §5 "E0 -- candidate keys"): its stages
against the full search on the same partition in the same process.

  workloads 1. 10M x 768 Float32, Cosine, 100 000 keys of 100 rows      2. 50M x 128 Float16, InnerProduct, 500 000 keys
  lists     m = 100, 1000, 10 000 and every key, drawn at random without repeats, a different list per query set
  batches   nq = 1 and nq = 64;   T = 32 tokens;   k = 100
  baseline  mvfgpu_search_maxsim_device (total) and mvfgpu_selftest_maxsim_stage_ms (ordinals / M0 / M1 / tail)
  stages    mvfgpu_selftest_maxsim_candidates_stage_ms: plan upload + E0 / M0 / M1 / tail, summed over chunks and windows

Device events around each variant on one stream, the variants alternating inside one process, `rounds` each after one warm
round, median.  The candidate call's events enclose its host plan (the device idles while the host looks the keys up); `host`
is the wall time the call takes to return.

    python scripts/probe_maxsim_candidates.py [--only 1 2] [--rows1 10000000] [--rows2 50000000] [--out profiles/r17_maxsim_candidates.txt]
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
GATHER_TBS = "5.98-6.03"  # profiles/r04_gather_random_rows.txt: random whole rows


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def main() -> None:
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows1", type=int, default=10_000_000)
    ap.add_argument("--rows2", type=int, default=50_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--m", type=int, nargs="+", default=[100, 1000, 10_000, 0], help="0: every key")
    ap.add_argument("--only", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    k, T, R = args.k, args.tokens, args.rounds
    lines = [f"Candidate multi-vector search against the full search on the same partition.  One MI355X, synthetic rows, keys of {ROWS_PER_KEY}",
             f"rows scattered over all positions, UInt32 key column, T = {T}, k = {k}, random lists without repeats, a different one per",
             f"query set; scripts/probe_maxsim_candidates.py.  ms: device events around the variant on one stream, the variants alternating",
             f"in one process, median of {R} after a warm round.  The random-gather rate of whole rows is {GATHER_TBS} TB/s",
             "(profiles/r04_gather_random_rows.txt).", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:  # as it goes: a run that is cut short leaves what it measured
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), host

    stream = torch.cuda.current_stream().cuda_stream
    # (rows, dimension, type, metric, words, bytes of a padded token in LDS)
    works = {1: (args.rows1, 768, G.FLOAT32, G.COSINE, "Float32, Cosine", 64 * 3 * 16),
             2: (args.rows2, 128, G.FLOAT16, G.INNER_PRODUCT, "Float16, InnerProduct", 16 * 1 * 32)}
    for work in args.only:
        n, dim, dtype, metric, what, token_bytes = works[work]
        rng = np.random.default_rng(n)
        col = np.empty(n, np.uint32)
        col[rng.permutation(n)] = (np.arange(n) // ROWS_PER_KEY).astype(np.uint32)
        with G.GpuCorpus.synthetic(n, dim, dtype, 1) as c, c.attach_column(col) as dc, c.make_partition(dc) as part:
            inf = part.info()
            nk, held, pitch = int(inf.n_keys), int(inf.live_rows), int(c.info().pitch_bytes)
            keys = part.keys()[0]
            say(f"{work}. {n} x {dim} {what}: {nk} keys, {held} held rows of {pitch} bytes")
            chunk = G.maxsim_plan(nk, T, 1, token_bytes, 512 << 20)[0]
            passes = -(-T // chunk)
            for nq in args.nq:
                q = torch.randn((nq, T, dim), dtype=torch.float32, device="cuda")
                ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                dk = torch.empty((nq, k), dtype=torch.int64, device="cuda")
                fs = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                fk = torch.empty((nq, k), dtype=torch.int64, device="cuda")

                def full():
                    c.search_maxsim_device(part, q.data_ptr(), 0, dim, nq, T, k, metric, fs.data_ptr(), fk.data_ptr(), 0, stream)

                def full_stages():
                    return c.maxsim_stage_ms(part, q.data_ptr(), 0, dim, nq, T, k, metric, fs.data_ptr(), fk.data_ptr(), stream)

                full(), full_stages()
                tf, sf = [], []   # the baseline's rounds are spread over the lists' below: the variants alternate
                say(f"   nq {nq}: {passes} chunks of up to {chunk} tokens")
                rows_out = []
                for m in args.m:
                    mm = nk if m == 0 else min(m, nk)
                    lists = np.stack([rng.choice(keys, mm, replace=False) for _ in range(nq)])

                    def cand():
                        c.search_maxsim_candidates_device(part, q.data_ptr(), 0, dim, nq, T, lists, k, metric, ds.data_ptr(), dk.data_ptr(), 0, stream)

                    def cand_stages():
                        return c.maxsim_candidates_stage_ms(part, q.data_ptr(), 0, dim, nq, T, lists, k, metric, ds.data_ptr(), dk.data_ptr(), stream)

                    cand(), cand_stages()
                    tc, hc, sc = [], [], []
                    for _ in range(R):
                        t, h = timed(cand)
                        tc.append(t), hc.append(h)
                        tf.append(timed(full)[0])
                        sc.append(cand_stages())
                        sf.append(full_stages())
                    if mm == nk:   # identity 2 on the probe's own data
                        same = bool((dk == fk).all()) and bool((ds.view(torch.int32) == fs.view(torch.int32)).all())
                        say(f"      every key listed: the candidate call's keys and score bits equal the full search's: {same}")
                    rows_out.append((mm, lists.shape[1] * ROWS_PER_KEY * nq, tc, hc, sc))
                o, m0, m1, tail = (med([s[i] for s in sf]) for i in range(4))
                m0s = [s[1] for s in sf]
                full_rt = held * nq * T / (m0 * 1e-3)
                say(f"      full search: {med(tf):10.3f} ms  (min {min(tf):.3f}, max {max(tf):.3f} over {len(tf)} rounds)")
                say(f"         stages: ordinals {o:.3f}  M0 {m0:.3f}  M1 {m1:.3f}  tail {tail:.3f} ms;  M0 min {min(m0s):.3f} max {max(m0s):.3f}: "
                    f"spread {100 * (max(m0s) - min(m0s)) / m0:.2f} %")
                say(f"         M0: {full_rt / 1e9:.2f} G row-tokens/s, {held * nq * pitch * passes / (m0 * 1e-3) / 1e12:.3f} TB/s of row bytes")
                for mm, crow, tc, hc, sc in rows_out:
                    e0, c0, c1, ct = (med([s[i] for s in sc]) for i in range(4))
                    model = m0 * (crow / (held * nq))
                    say(f"      m {mm:7d}: candidates {med(tc):10.3f} ms  {[round(x, 3) for x in tc]}  host {med(hc):.3f} ms;  / full search = {med(tc) / med(tf):.4f}")
                    say(f"         stages: plan + E0 {e0:.3f}  M0 {c0:.3f}  M1 {c1:.3f}  tail {ct:.3f} ms;  {crow} candidate rows "
                        f"({100 * crow / (held * nq):.2f} % of the held rows x sets)")
                    say(f"         M0: {crow * T / (c0 * 1e-3) / 1e9:.2f} G row-tokens/s = {crow * T / (c0 * 1e-3) / full_rt:.3f} x the full search's;  "
                        f"{crow * pitch * passes / (c0 * 1e-3) / 1e12:.3f} TB/s of gathered row bytes;  "
                        f"(candidate rows / held rows) x full M0 = {model:.3f} ms: measured / that = {c0 / model:.2f}")
                    if mm == nk:
                        inside = min(m0s) <= c0 <= max(m0s)
                        say(f"         every key: M0 {c0:.3f} ms against the full search's {m0:.3f} ms [{min(m0s):.3f}, {max(m0s):.3f}]: "
                            f"{'inside' if inside else 'OUTSIDE'} the baseline's own spread ({100 * (c0 - m0) / m0:+.2f} %)")
                    elif mm * 10 <= nk:
                        say(f"         m <= 10 % of the keys: the whole call {'takes less than' if med(tc) < med(tf) else 'DOES NOT take less than'} the full search")
            say("")


if __name__ == "__main__":
    main()
