"""Radius search (mvfgpu_search_radius) against the top-k search of the same shape: wall ms per blocking call (host
queries, host results), the fraction of the 8 TB/s HBM peak the radius scan's bytes make of that time (the rows are read
once per pass of 1 or 4 queries), match counts and how many queries overflowed their device list (completed by the
top-k search).  Radii come from the top-k scores of the same queries, so the match counts are what the rows give.

    python scripts/probe_radius.py [--out FILE] [--skip-10m-batch]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from metrovector_amd import gpu as G  # noqa: E402
from oracle import mvf_oracle as O  # noqa: E402

HBM = 8.0e12
SEED = 0x4D564631


def timed(fn, reps):
    fn()  # warm: kernels loaded, scratch allocated
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-10m-batch", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("radius search vs top-k, MI355X, f32 L2, synthetic corpus (DESIGN.md section 6), host buffers, median wall ms")
    n, dim = 10_000_000, 768
    with G.GpuCorpus.synthetic(n, dim, G.FLOAT32, SEED) as c:
        pitch = c.info().pitch_bytes
        q = O.synth_queries(SEED + 1, 1, dim, O.F32)
        for want in (10, 1000, 100_000):
            top = c.search(q, want, G.L2)
            radius = float(top.scores[0, want - 1])
            t_top, _ = timed(lambda: c.search(q, min(want, 100), G.L2), 5)
            for m in (min(want, 100), 0):
                t, res = timed(lambda: c.search_radius(q, radius, m, G.L2), 5)
                say(f"1 query  {n}x{dim}: ~{want:>6} matches  max_per_query={m:4d}: radius {t*1e3:8.3f} ms "
                    f"({n * pitch / t / HBM:5.3f} of 8 TB/s)  count={int(res.counts[0]):7d} overflowed={int(res.overflowed.sum())}  "
                    f"| top-{min(want, 100)} {t_top*1e3:8.3f} ms")
    # the route crossover (mvfgpu_selftest_radius_route: batched from 16 queries on Float32 rows): both routes at a few sizes
    n = 1_000_000
    with G.GpuCorpus.synthetic(n, dim, G.FLOAT32, SEED) as c:
        for nq in (4, 8, 16, 32, 128):
            qs = O.synth_queries(SEED + 3, nq, dim, O.F32)
            radii = c.search(qs, 100, G.L2).scores[:, 99].copy()
            t = {}
            for path in (1, 2):
                c.set_scan_path(path)
                t[path], _ = timed(lambda: c.search_radius(qs, radii, 128, G.L2), 3)
            c.set_scan_path(0)
            say(f"{nq:4d} queries {n}x{dim}: streaming route {t[1]*1e3:7.2f} ms  batched route {t[2]*1e3:7.2f} ms  "
                f"(default: {'batched' if G.radius_route(G.FLOAT32, nq) else 'streaming'})")
    for n, reps in ((1_000_000, 3), (10_000_000, 1)):
        if n == 10_000_000 and a.skip_10m_batch:
            continue
        nq = 1024
        with G.GpuCorpus.synthetic(n, dim, G.FLOAT32, SEED) as c:
            pitch = c.info().pitch_bytes
            qs = O.synth_queries(SEED + 2, nq, dim, O.F32)
            top = c.search(qs, 100, G.L2)
            radii = top.scores[:, 99].copy()
            t_top, _ = timed(lambda: c.search(qs, 100, G.L2), reps)
            t, res = timed(lambda: c.search_radius(qs, radii, 128, G.L2), reps)
            route = G.radius_route(G.FLOAT32, nq)
            roof = (f"{2 * nq * n * dim / t / 157.3e12:5.3f} of the 157.3 TF f32 MFMA peak, batched route" if route else
                    f"{(nq + 3) // 4 * n * pitch / t / HBM:5.3f} of 8 TB/s over {(nq + 3) // 4} passes, streaming route")
            say(f"{nq} queries {n}x{dim}: ~100 matches  max_per_query=128: radius {t*1e3:9.2f} ms ({roof})  "
                f"counts median {int(np.median(res.counts))} max {int(res.counts.max())} overflowed={int(res.overflowed.sum())}  "
                f"| top-100 {t_top*1e3:8.2f} ms  ratio {t / t_top:6.1f}x")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
