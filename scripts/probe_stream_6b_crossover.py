"""One Float32 query, top-100 cosine: the 6-bit shadow stream (scan path 7) against the int8 shadow stream (scan path 6), by
corpus size -- the crossover behind api.hip kStream6MinBytes.  Device time of the whole search (mvfgpu_timing.search_ms: first
to last kernel) and of the scan alone, median and spread (min .. max) over REPS searches, and the cost of the first search
on each route (it builds the shadow).  Development aid.
    python scripts/probe_stream_6b_crossover.py [GiB ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import _synth as O  # the library's own generator (scripts/_synth.py)
from metrovector_amd import gpu as G

DIM, K, REPS = 768, 100, 30
sizes = [float(a) for a in sys.argv[1:]] or [1, 2, 4, 8, 16]
q = O.synth_queries(0x4D564632, 8, DIM, 0)
for gib in sizes:
    n = int(gib * (1 << 30)) // (DIM * 4)
    c = G.GpuCorpus.synthetic(n, DIM, 0, 0x4D564631)
    c.set_scan_path(1)
    c.search(q[:1], K, G.COSINE)  # (the norms)
    res = {}
    for name, path in (("int8", 6), ("6bit", 7)):
        c.set_scan_path(path)
        t0 = time.perf_counter()
        c.search(q[:1], K, G.COSINE)  # builds the shadow
        first = (time.perf_counter() - t0) * 1e3
        c.set_profiling(True)
        dev, scan = [], []
        for i in range(REPS):
            c.search(q[i % 8:i % 8 + 1], K, G.COSINE)
            t = c.last_timing()
            dev.append(t.search_ms)
            scan.append(t.scan_ms)
        t = c.last_timing()
        c.set_profiling(False)
        res[name] = (float(np.median(dev)), min(dev), max(dev), float(np.median(scan)), t.scan_bytes, first, t.repaired_queries)
    a, b = res["int8"], res["6bit"]
    print(f"{gib:5.1f} GiB ({n:9d} rows): int8 {a[0]:7.4f} ms ({a[1]:.4f} .. {a[2]:.4f}; scan {a[3]:.4f} = {a[4] / a[3] / 1e9:.2f} TB/s; first {a[5]:.1f} ms) | "
          f"6-bit {b[0]:7.4f} ms ({b[1]:.4f} .. {b[2]:.4f}; scan {b[3]:.4f} = {b[4] / b[3] / 1e9:.2f} TB/s; first {b[5]:.1f} ms; repaired {b[6]}) | "
          f"int8 / 6-bit {a[0] / b[0]:5.3f}", flush=True)
    c.close()
