"""One Float32 query, top-100 cosine on scan path 0: the 6-bit shadow held in the 5+1 layout (csrc/shadow_5p1.h: five bits of
every row, the sixth on demand) against the same shadow in the 6-bit layout (MVF_STREAM_5P1=0), one handle each on the same
rows.  Device time of the whole search and of the scan alone (median, min .. max over REPS searches, eight queries in turn),
the low-plane lines the scan requested out of those the rows hold (mvfgpu_debug_stream_lo_lines), and whether the two handles
return the same bits.  Development aid.
    python scripts/probe_stream_5p1.py [rows [dim [k]]]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import _synth as O  # the library's own generator (scripts/_synth.py)
from metrovector_amd import gpu as G

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
k = int(sys.argv[3]) if len(sys.argv) > 3 else 100
REPS = 40
q = O.synth_queries(0x4D564632, 8, dim, 0)
answers = {}
for name, env in (("6-bit layout", "0"), ("5+1 layout", "1")):
    os.environ["MVF_STREAM_5P1"] = env  # read when the handle is created
    c = G.GpuCorpus.synthetic(n, dim, 0, 0x4D564631)
    c.set_scan_path(0 if n * dim * 4 >= (4 << 30) else 7)
    c.search(q[:1], k, G.COSINE)  # norms, shadow
    c.set_profiling(True)
    dev, scan, frac, res = [], [], [], []
    for i in range(REPS):
        res.append(c.search(q[i % 8:i % 8 + 1], k, G.COSINE))
        t = c.last_timing()
        dev.append(t.search_ms)
        scan.append(t.scan_ms)
        frac.append(c.stream_lo_lines())
    answers[name] = res
    f, tot = frac[-1]
    fr = [a / b for a, b in frac if b]
    print(f"{name}: {n} x {dim}, k {k}: search {np.median(dev):.4f} ms ({min(dev):.4f} .. {max(dev):.4f}), scan {np.median(scan):.4f} ms "
          f"({min(scan):.4f} .. {max(scan):.4f}); kernel {t.scan_kernel}, repaired {t.repaired_queries}; low-plane lines {f} of {tot}"
          + (f" = {f / tot:.4f} (over the searches {min(fr):.4f} .. {max(fr):.4f})" if tot else ""), flush=True)
    c.close()
a, b = answers["6-bit layout"], answers["5+1 layout"]
same = all((x.indices == y.indices).all() and (x.scores.view(np.uint32) == y.scores.view(np.uint32)).all() and (x.raw == y.raw).all() for x, y in zip(a, b))
print("the two layouts return the same bits:", same)
