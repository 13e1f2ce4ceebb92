"""One Float32 query, top-100 cosine: the int8-shadow stream (scan path 0's default above the threshold; path 6 below it)
against K1 on the stored rows (path 1), by corpus size -- the crossover behind api.hip kStreamI8MinBytes.  Device time of
the whole search (mvfgpu_timing.search_ms: first to last kernel) and the host call's wall time, medians.  Development aid."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import _synth as O  # the library's own generator (scripts/_synth.py)
from metrovector_amd import gpu as G

DIM, K, REPS = 768, 100, 40
q = O.synth_queries(0x4D564632, 8, DIM, 0)
for mib in (256, 512, 1024, 2048, 4096):
    n = (mib << 20) // (DIM * 4)
    c = G.GpuCorpus.synthetic(n, DIM, 0, 0x4D564631)
    res = {}
    for name, path in (("shadow", 6), ("stored", 1)):
        c.set_scan_path(path)
        c.search(q[:1], K, G.COSINE)  # (builds the norms / the shadow once)
        c.set_profiling(True)
        dev, wall = [], []
        for i in range(REPS):
            t0 = time.perf_counter()
            c.search(q[i % 8:i % 8 + 1], K, G.COSINE)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(c.last_timing().search_ms)
        c.set_profiling(False)
        res[name] = (float(np.median(dev)), float(np.median(wall)))
    print(f"{mib:5d} MiB ({n:9d} rows): shadow {res['shadow'][0]:7.3f} ms device {res['shadow'][1]:7.3f} ms wall | "
          f"stored {res['stored'][0]:7.3f} ms device {res['stored'][1]:7.3f} ms wall | "
          f"ratio {res['stored'][0] / res['shadow'][0]:5.2f}x", flush=True)
    c.close()
