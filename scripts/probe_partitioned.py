"""Partitioned search (mvfgpu_partition_*, mvfgpu_search_partitioned_device; DESIGN.md §5 "B0 / B1 / B2 / S1") against the loop it
replaces: per distinct key of the batch one mvfgpu_filter_create_where(col == key) and one mvfgpu_search_filtered_device with
that key's queries (already gathered per key on the device, outside the timed span).

  1. 10 000 tenants of 1000 rows; 1024 queries, each with a random tenant            (all small tier)
  2. tenant sizes spread from 100 to 1M rows; 1024 queries, keys drawn in proportion to size
  3. 16 tenants of 625 000 rows; 64 queries                                          (all large tier, dense keys)
  4. mvfgpu_partition_create for each of the three columns: wall time and device_bytes

Device events around each variant on one stream (the loop waits on the host inside; its wall time is reported too), the two
variants alternating inside one process, three rounds each after one warm round, median.

    python scripts/probe_partitioned.py [--rows 10000000] [--dim 768] [--out profiles/r14_partitioned.txt] [--only 1 2 3 4]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metrovector_amd import gpu as G  # noqa: E402

GATHER_TBS = (5.98, 6.03)  # random 3-KiB rows, profiles/r04_gather_random_rows.txt


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def columns(n):
    """the three tenant columns over n rows, shuffled so that every tenant is scattered over all positions"""
    rng = np.random.default_rng(n)
    perm = rng.permutation(n)
    out = {}
    c1 = np.empty(n, np.uint32)
    c1[perm] = (np.arange(n) // 1000).astype(np.uint32)
    out[1] = c1
    sizes = []
    grid = np.unique(np.round(np.logspace(2, 6, 41)).astype(np.int64))
    while sum(sizes) < n:
        for s in grid[::-1]:
            if sum(sizes) + s <= n:
                sizes.append(int(s))
        if sum(sizes) + grid[0] > n:
            break
    if sum(sizes) < n:  # the remainder joins the last tenant
        sizes[-1] += n - sum(sizes)
    c2 = np.empty(n, np.uint32)
    c2[perm] = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    out[2] = c2
    c3 = np.empty(n, np.uint32)
    c3[perm] = (np.arange(n) // max(n // 16, 1)).astype(np.uint32).clip(0, 15)
    out[3] = c3
    return out


def draw_keys(work, col, nq, rng):
    if work == 1:
        return rng.integers(0, int(col.max()) + 1, nq).astype(np.uint64)
    if work == 2:
        return col[rng.integers(0, col.size, nq)].astype(np.uint64)  # a random row's tenant: in proportion to size
    return rng.integers(0, 16, nq).astype(np.uint64)


def main() -> None:
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", type=int, nargs="+", default=[1, 2, 3, 4])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dim, k = args.rows, args.dim, args.k
    lines = [f"Partitioned search against one where-filter + filtered search per distinct key.  One MI355X, {n} x {dim} Float32 (synthetic),",
             f"Cosine, k = {k}, UInt32 tenant column; scripts/probe_partitioned.py.  ms: device events around the variant on one stream, the",
             f"variants alternating in one process, median of {args.rounds} after a warm round; wall: time.perf_counter to the stream's end.", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cols = columns(n)
    stream = torch.cuda.current_stream().cuda_stream
    with G.GpuCorpus.synthetic(n, dim, G.FLOAT32, 1) as c:
        pitch = c.info().pitch_bytes
        for work in (1, 2, 3):
            col = cols[work]
            with c.attach_column(col) as dc:
                t0 = time.perf_counter()
                part = c.make_partition(dc)
                create_ms = (time.perf_counter() - t0) * 1e3
                creates = [create_ms]
                if 4 in args.only:
                    for _ in range(args.rounds):
                        part.close()
                        t0 = time.perf_counter()
                        part = c.make_partition(dc)
                        creates.append((time.perf_counter() - t0) * 1e3)
                    inf = part.info()
                    say(f"4. column {work}: mvfgpu_partition_create wall {med(creates[1:]):8.2f} ms (first {creates[0]:.2f}); {inf.n_keys} keys, "
                        f"largest {inf.largest}, device_bytes {inf.device_bytes} ({inf.device_bytes / n:.2f} B/row), host_bytes {inf.host_bytes}")
                if work not in args.only:
                    part.close()
                    continue
                nq = 64 if work == 3 else 1024
                rng = np.random.default_rng(100 + work)
                keys = draw_keys(work, col, nq, rng)
                counts = part.lookup(keys)
                tier, groups = G.partition_plan(counts, keys, k)
                q = torch.randn((nq, dim), dtype=torch.float32, device="cuda")
                ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
                di = torch.empty((nq, k), dtype=torch.int64, device="cuda")
                # the loop's inputs: per distinct key its queries, contiguous
                distinct = np.unique(keys)
                per_key = []
                for key in distinct.tolist():
                    sel = np.nonzero(keys == key)[0]
                    per_key.append((key, sel, q[torch.from_numpy(sel).cuda()].contiguous(),
                                    torch.empty((sel.size, k), dtype=torch.float32, device="cuda"),
                                    torch.empty((sel.size, k), dtype=torch.int64, device="cuda")))

                def run_part():
                    c.search_partitioned_device(part, q.data_ptr(), 0, dim, nq, keys, k, G.COSINE, ds.data_ptr(), di.data_ptr(), 0, stream)

                def run_loop():
                    for key, sel, qq, ss, ii in per_key:
                        with c.make_filter_where([(dc, "==", int(key))]) as f:
                            c.search_filtered_device(f, qq.data_ptr(), 0, dim, sel.size, k, G.COSINE, ss.data_ptr(), ii.data_ptr(), 0, stream)

                def timed(fn):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    a.record()
                    fn()
                    b.record()
                    torch.cuda.synchronize()
                    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

                run_part(), run_loop()
                torch.cuda.synchronize()
                # the same answers: indices of every query
                differ = sum(int((di[torch.from_numpy(sel).cuda()] != ii).any(dim=1).sum()) for key, sel, qq, ss, ii in per_key)
                tp, tl = [], []
                for _ in range(args.rounds):
                    tp.append(timed(run_part))
                    tl.append(timed(run_loop))
                p_ms, p_wall = med([t[0] for t in tp]), med([t[1] for t in tp])
                l_ms, l_wall = med([t[0] for t in tl]), med([t[1] for t in tl])
                gathered = int(counts.sum())
                # rows the partitioned call loads: a small-tier query its own, a large key's once per group of 4 of its queries
                # (four padded queries of this shape fit the 40-KiB budget)
                reads = 0
                for key, first in zip(*np.unique(keys, return_index=True)):
                    cnt, nk = int(counts[first]), int((keys == key).sum())
                    reads += cnt * (nk if cnt <= 1024 and k <= 1024 else (nk + 3) // 4)
                say(f"{work}. {nq} queries, {distinct.size} distinct keys; tiers: {int((tier == 1).sum())} small, {int((tier == 2).sum())} large in "
                    f"{groups} gathered searches; rows scored {gathered}; queries whose indices differ from the loop's: {differ}")
                say(f"   partitioned {p_ms:9.3f} ms (wall {p_wall:9.3f})   loop {l_ms:9.3f} ms (wall {l_wall:9.3f})   ratio partitioned / loop "
                    f"{p_ms / l_ms:.3f} (wall {p_wall / l_wall:.3f})")
                say(f"   rows scored per second {gathered / (p_ms * 1e-3):.3e}; rows loaded {reads}, {reads / (p_ms * 1e-3):.3e} per second: {reads * pitch / (p_ms * 1e-3) / 1e12:.2f} TB/s "
                    f"of row bytes over the whole call (random-gather rate {GATHER_TBS[0]}-{GATHER_TBS[1]} TB/s, profiles/r04_gather_random_rows.txt)")
                say(f"   rounds: partitioned {[round(t[0], 3) for t in tp]}  loop {[round(t[0], 3) for t in tl]}")
                part.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
