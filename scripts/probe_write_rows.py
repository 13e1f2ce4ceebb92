"""Row writes (mvfgpu_corpus_write_rows[_device], include/mvf_gpu_update.h) on one MI355X: a Float32 corpus (10M x 768 by
default) with the norms, the int8 shadow and the 6-bit shadow resident.  Records
  * the device time (HIP events around mvfgpu_corpus_write_rows_device, rows already in device memory) and the blocking host
    call's wall time for 1, 1 000 and 100 000 random distinct rows of benign data, median of the repetitions with their spread;
  * bytes_written per millisecond of device time at 100 000 rows (README.md quotes the HBM rate to compare it with);
  * the recipe a write replaces: destroy the handle, create it again from the host rows with the eager shadow build, and the
    first one-query search;
  * the one-query default-route search on the same handle before and after the 100 000-row write (five repetitions each, the
    route's kernel and bytes beside them): a difference beyond the spread of the five "before" figures is a finding.

    python scripts/probe_write_rows.py [--rows 10000000] [--dim 768] [--out profiles/r22_write_rows.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metrovector_amd import gpu as G  # noqa: E402
from oracle import mvf_oracle as O  # noqa: E402

SEED = 0x4D564631
K = 100


def spread(ts):
    return f"{np.median(ts):10.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, dim = a.rows, a.dim
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# row writes: {n} x {dim} f32, one device ({torch.cuda.get_device_name(0)})")
    q1 = np.ascontiguousarray(O.synth_queries(SEED + 1, 1, dim, O.F32))
    q64 = np.ascontiguousarray(O.synth_queries(SEED + 2, 64, dim, O.F32))
    c = G.GpuCorpus.synthetic(n, dim, G.FLOAT32, SEED)
    c.set_profiling(True)
    c.search(q64, K, G.COSINE)   # the norms and the int8 shadow
    c.search(q1, K, G.COSINE)    # the one-query route's shadow
    c.search(q1, K, G.COSINE)
    inf = c.info()
    say(f"resident: shadows {inf.shadows:#x} (1 int8, 2 f16, 8 6-bit), device bytes {inf.device_bytes / 1e9:.2f} GB")

    def one_query(reps=5):
        dev, wall = [], []
        for _ in range(reps):
            t = time.perf_counter()
            c.search(q1, K, G.COSINE)
            wall.append((time.perf_counter() - t) * 1e3)
            tm = c.last_timing()
            dev.append(tm.total_ms)
        return dev, wall, (tm.scan_kernel, tm.scan_bytes)

    before = one_query()
    say(f"one-query search before the writes: device {spread(before[0])}, host call {spread(before[1])}, scan_kernel {before[2][0]}, "
        f"scan_bytes {before[2][1]}")

    rng = np.random.default_rng(7)
    stream = torch.cuda.current_stream()
    for m in (1, 1000, 100_000):
        reps = 5
        dev, wall = [], []
        for r in range(reps + 1):  # the first repetition warms up (pinned buffers, the pool)
            pos = rng.choice(n, m, replace=False).astype(np.uint64)
            src = int(rng.integers(0, n - m + 1))
            new = c.read_rows(int(src), m)  # benign data: other rows of the same corpus
            dnew = torch.from_numpy(new).cuda()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rep = c.write_rows_device(pos, dnew.data_ptr(), dim * 4, stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            pos2 = rng.choice(n, m, replace=False).astype(np.uint64)
            t = time.perf_counter()
            c.write_rows(pos2, new)
            w = (time.perf_counter() - t) * 1e3
            if r:
                dev.append(e0.elapsed_time(e1))
                wall.append(w)
        say(f"write of {m:7d} rows: device {spread(dev)}, blocking host call {spread(wall)}; launches {rep['launches']}, refreshed "
            f"{rep['refreshed']:#x}, bytes_written {rep['bytes_written']}")
        if m == 100_000:
            ms = float(np.median(dev))
            say(f"    bytes_written / device time at {m} rows: {rep['bytes_written'] / ms / 1e6:.1f} MB per ms = "
                f"{rep['bytes_written'] / ms / 1e9:.3f} TB/s algorithmic (traffic is about twice that: each refresh reads the row again)")

    after = one_query()
    say(f"one-query search after the writes:  device {spread(after[0])}, host call {spread(after[1])}, scan_kernel {after[2][0]}, "
        f"scan_bytes {after[2][1]}")
    d = float(np.median(after[0]) - np.median(before[0]))
    sp = max(before[0]) - min(before[0])
    say(f"    difference of the medians {d:+.4f} ms; spread of the five before {sp:.4f} ms -> "
        f"{'within the spread' if abs(d) <= sp else 'BEYOND the spread: a finding'}")

    # the recipe a write replaces
    rows = c.read_rows(0, n)
    c.close()
    t = time.perf_counter()
    c = G.GpuCorpus.from_array(rows, prepare_batched=True)
    t_up = time.perf_counter() - t
    t = time.perf_counter()
    c.search(q1, K, G.COSINE)
    t_first = time.perf_counter() - t
    say(f"the recipe: create_ex with the eager shadow build {t_up * 1e3:.1f} ms ({rows.nbytes / t_up / 1e9:.1f} GB/s), first one-query "
        f"search {t_first * 1e3:.1f} ms, together {(t_up + t_first) * 1e3:.1f} ms (the destroy before it not counted)")
    c.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
