"""Grouped search (mvfgpu_search_grouped_device; DESIGN.md §5 "G0 / G1 — grouped search"): its stages, the floor and the host
recipe it replaces.

  columns   1. 1M keys of 10 rows (rows / 10 keys)      2. Zipf-sized keys      3. one key holding 30 % of the rows, 10-row keys
  per_key   1 and 3;   queries 1 and 16;   k = 100, Cosine
  stages    mvfgpu_selftest_grouped_stage_ms: segment bounds / G0 / G1 / tail (batches of one window: 1 and 4 queries)
  floor     a one-query mvfgpu_search_device on scan path 1, k = 100, on the same handle: every stored live row read once
  recipe    the host loop: mvfgpu_search at k' = 4 k, cap on the host with the column, double k' until every list is full

Device events around each variant on one stream, the variants alternating inside one process, `rounds` each after one warm
round, median; the recipe waits on the host, so its wall time is what counts.

    python scripts/probe_grouped.py [--rows 10000000] [--dim 768] [--out profiles/r15_grouped.txt] [--only 1 2 3]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metrovector_amd import gpu as G  # noqa: E402

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def columns(n):
    """the three key columns over n rows, shuffled so that every key is scattered over all positions"""
    rng = np.random.default_rng(n)
    perm = rng.permutation(n)
    out = {}
    c = np.empty(n, np.uint32)
    c[perm] = (np.arange(n) // 10).astype(np.uint32)
    out[1] = c
    sizes = np.minimum(rng.zipf(1.3, n), max(n // 10, 1)).astype(np.int64)  # Zipf(1.3) sizes, at most a tenth of the rows each
    nkeys = int(np.searchsorted(np.cumsum(sizes), n)) + 1
    sizes = sizes[:nkeys]
    sizes[-1] -= int(sizes.sum()) - n
    c = np.empty(n, np.uint32)
    c[perm] = np.repeat(np.arange(nkeys, dtype=np.uint32), sizes)
    out[2] = c
    big = int(0.3 * n)
    c = np.empty(n, np.uint32)
    c[perm] = np.concatenate([np.zeros(big, np.uint32), 1 + (np.arange(n - big) // 10).astype(np.uint32)])
    out[3] = c
    return out


def cap(indices, col, per_key, k):
    """the first k entries of a ranked list with at most per_key per key"""
    keys = col[indices]
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    head = np.ones(ks.size, bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.maximum.accumulate(np.where(head, np.arange(ks.size), 0))
    occ = np.empty(ks.size, np.int64)
    occ[order] = np.arange(ks.size) - start
    return indices[occ < per_key][:k]


def main() -> None:
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dim, k = args.rows, args.dim, args.k
    lines = [f"Grouped search: stages, floor and the host recipe.  One MI355X, {n} x {dim} Float32 (synthetic), Cosine, k = {k}, UInt32 key",
             f"column; scripts/probe_grouped.py.  ms: device events around the variant on one stream, the variants alternating in one",
             f"process, median of {args.rounds} after a warm round; wall: time.perf_counter to the stream's end.", ""]

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
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

    cols = columns(n)
    stream = torch.cuda.current_stream().cuda_stream
    names = {1: f"{n // 10} keys of 10 rows", 2: "Zipf-sized keys", 3: "one key of 30 % of the rows, 10-row keys"}
    with G.GpuCorpus.synthetic(n, dim, G.FLOAT32, 1) as c:
        q16 = torch.randn((16, dim), dtype=torch.float32, device="cuda")
        q16_host = q16.cpu().numpy()
        ds = torch.empty((16, k), dtype=torch.float32, device="cuda")
        di = torch.empty((16, k), dtype=torch.int64, device="cuda")

        def floor():
            c.search_device(q16.data_ptr(), 0, dim, 1, k, G.COSINE, ds.data_ptr(), di.data_ptr(), 0, stream)

        c.set_scan_path(1)
        floor()
        floors = [timed(floor)[0] for _ in range(args.rounds)]
        c.set_scan_path(0)
        say(f"floor: one-query mvfgpu_search_device, scan path 1, k = {k}: {med(floors):.3f} ms {[round(x, 3) for x in floors]}")
        say("")
        for work in args.only:
            col = cols[work]
            with c.attach_column(col) as dc, c.make_partition(dc) as part:
                inf = part.info()
                say(f"{work}. {names[work]}: {inf.n_keys} keys, largest {inf.largest}")
                for per_key in (1, 3):
                    for nq in (1, 16):
                        def grouped():
                            c.search_grouped_device(part, q16.data_ptr(), 0, dim, nq, k, per_key, G.COSINE, ds.data_ptr(), di.data_ptr(), 0, stream)

                        def recipe():
                            kp, rounds = 4 * k, 0
                            while True:
                                res = c.search(q16_host[:nq], min(kp, n), G.COSINE)
                                rounds += 1
                                full = True
                                for j in range(nq):
                                    real = res.indices[j][res.indices[j] != PAD].astype(np.int64)
                                    if cap(real, col, per_key, k).size < k and kp < n:
                                        full = False
                                        break
                                if full:
                                    return rounds, kp
                                kp *= 2

                        grouped(), recipe()
                        tg, tr = [], []
                        for _ in range(args.rounds):
                            tg.append(timed(grouped))
                            t0 = time.perf_counter()
                            rr = recipe()
                            tr.append((time.perf_counter() - t0) * 1e3)
                        g_ms, g_wall = med([t[0] for t in tg]), med([t[1] for t in tg])
                        # the same rows as the recipe's
                        got = di.cpu().numpy().view(np.uint64)[:nq]
                        res = c.search(q16_host[:nq], min(rr[1], n), G.COSINE)
                        differ = sum(int(not np.array_equal(cap(res.indices[j][res.indices[j] != PAD].astype(np.int64), col, per_key, k),
                                                            got[j][got[j] != PAD].astype(np.int64))) for j in range(nq))
                        say(f"   per_key {per_key}, {nq:2d} queries: grouped {g_ms:9.3f} ms (wall {g_wall:9.3f}) = {g_ms / med(floors) / nq:.2f} floors per query;"
                            f"  host recipe wall {med(tr):9.3f} ms ({rr[0]} searches, last k' {rr[1]});  grouped / recipe {g_wall / med(tr):.3f};"
                            f"  queries that differ from the recipe's: {differ}")
                        say(f"      rounds: grouped {[round(t[0], 3) for t in tg]}  recipe {[round(t, 3) for t in tr]}")
                    for nq in (1, 4):
                        st = [c.grouped_stage_ms(part, q16.data_ptr(), 0, dim, nq, k, per_key, G.COSINE, ds.data_ptr(), di.data_ptr(), stream)
                              for _ in range(args.rounds + 1)][1:]
                        b, g0, g1, tail = (med([s[i] for s in st]) for i in range(4))
                        say(f"   per_key {per_key}, {nq:2d} queries, stages: bounds {b:.3f}  G0 {g0:.3f}  G1 {g1:.3f}  tail {tail:.3f} ms;"
                            f"  (G1 + tail) / G0 = {(g1 + tail) / g0:.3f};  G0 / floor = {g0 / med(floors):.2f}")
                say("")


if __name__ == "__main__":
    main()
