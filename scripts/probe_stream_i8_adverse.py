"""Adverse data for the default int8-shadow stream of one Float32 query: 10M x 768 rows, correlated in runs of 32 rows
(each run = one anchor + noise) with a near-duplicate of the row before every 37th row, queries near stored rows.  Per
search: the route it took, its device time, whether it was repaired, and that its answer is K1's bits (scan path 1);
then how many searches the repair feedback takes to send the corpus back to the stored rows.  Development aid."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from metrovector_amd import gpu as G

N, DIM, K, SEARCHES = 10_000_000, 768, 100, 24
g = torch.Generator(device="cuda").manual_seed(7)
rows = torch.empty((N, DIM), dtype=torch.float32)
step = 500_000
for r0 in range(0, N, step):
    m = min(step, N - r0)
    anchors = torch.randn((m + 31) // 32, DIM, device="cuda", generator=g)
    blk = anchors.repeat_interleave(32, 0)[:m] * 0.8 + torch.randn(m, DIM, device="cuda", generator=g) * 0.25
    dup = torch.arange(37, m, 37, device="cuda")
    blk[dup] = blk[dup - 1] + torch.randn(len(dup), DIM, device="cuda", generator=g) * 1e-4
    rows[r0:r0 + m] = blk.cpu()
rows_np = rows.numpy()
rng = np.random.default_rng(3)
picks = rng.integers(0, N, SEARCHES)
q = (rows_np[picks] + rng.standard_normal((SEARCHES, DIM)).astype(np.float32) * 1e-3).astype(np.float32)
with G.GpuCorpus.from_array(rows_np) as c:
    del rows, rows_np
    c.set_profiling(True)
    worst = 0.0
    c.set_scan_path(1)
    c.search(q[:1], K, G.COSINE)
    k1_ms = c.last_timing().search_ms
    switched = None
    for i in range(SEARCHES):
        c.set_scan_path(0)
        got = c.search(q[i:i + 1], K, G.COSINE)
        t = c.last_timing()
        route, ms, rep = t.scan_kernel, t.search_ms, t.repaired_queries
        c.set_scan_path(1)
        want = c.search(q[i:i + 1], K, G.COSINE)
        k1_ms = c.last_timing().search_ms
        same = (got.indices == want.indices).all() and (got.scores.view(np.uint32) == want.scores.view(np.uint32)).all()
        if route == 1 and switched is None:
            switched = i
        if route == 7:
            worst = max(worst, ms / k1_ms)
        print(f"search {i:2d}: route {'shadow' if route == 7 else 'stored'} {ms:7.3f} ms (K1 {k1_ms:7.3f} ms) "
              f"repaired {rep}  bit-identical {same}", flush=True)
        assert same
    print(f"fell back to the stored rows at search {switched}; worst shadow search = {worst:.2f} x a K1 search", flush=True)
