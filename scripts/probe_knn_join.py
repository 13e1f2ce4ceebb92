"""k-NN join (mvfgpu_knn_join[_device]) against the path it is built from, all legs of a comparison in ONE process:

  * yardstick: mvfgpu_search_device in a loop over the same windows, queries already contiguous in device memory, k' = k + 1
    results -- the join minus staging (J0) and finishing (J1).  HIP events around the calls on one torch stream, one warm
    round, then ROUNDS timed rounds of yardstick and join alternating; median and min..max are reported;
  * host call against device call (wall clock, results in host memory either way), and the un-overlapped version: one
    blocking host call per window;
  * the caller-side recipe the join replaces: read the rows back, widen, mvfgpu_search per window with k + 1, strip self;
  * repaired_queries summed over the windows and the selection the handle's feedback ended on, for the uniform synthetic
    corpus and for one with planted near-duplicates (as scripts/probe_stream_i8_adverse.py builds them).

    python scripts/probe_knn_join.py [--out profiles/r08_knn_join.txt] [--legs small|big|all]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metrovector_amd import _lib  # noqa: E402
from metrovector_amd import gpu as G  # noqa: E402

SEED = 0x4D564631
NAME = {G.FLOAT32: "f32", G.FLOAT16: "f16", G.INT8: "int8", G.UINT8: "uint8"}
METRIC = {G.L2: "L2", G.INNER_PRODUCT: "IP", G.COSINE: "cosine"}
W, K, ROUNDS = G.JOIN_WINDOW, 100, 5


def widen(rows):
    return rows.astype(np.float32) if rows.dtype in (np.float16, np.float32) else rows


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts):
    return f"{np.median(ts):9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def device_legs(c, dt, metric, first, nwin, st, say, tag):
    """join_device against the search_device loop; returns (median join ms, median yardstick ms)."""
    n, dim = c.rows, c.dimension
    count = nwin * W
    qd = dt if dt in (G.INT8, G.UINT8) else G.FLOAT32
    dq = torch.from_numpy(widen(c.read_rows(first, count))).cuda()
    ys = torch.empty((W, K + 1), dtype=torch.float32, device="cuda")
    yi = torch.empty((W, K + 1), dtype=torch.int64, device="cuda")
    js = torch.empty((count, K), dtype=torch.float32, device="cuda")
    ji = torch.empty((count, K), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    esz = dq.element_size()

    def yard():
        for w in range(nwin):
            c.search_device(dq.data_ptr() + w * W * dim * esz, qd, dim, W, K + 1, metric, ys.data_ptr(), yi.data_ptr(), 0, st.cuda_stream)

    def join():
        c.knn_join_device(K, metric, first, count, js.data_ptr(), ji.data_ptr(), 0, stream=st.cuda_stream)

    yard(), join()
    st.synchronize()
    ty, tj = [], []
    for _ in range(ROUNDS):
        ty.append(timed(yard, st))
        tj.append(timed(join, st))
    my, mj = float(np.median(ty)), float(np.median(tj))
    say(f"{tag}: {nwin} windows x {W} rows, k = {K}: search_device loop {spread(ty)}  join_device {spread(tj)}  "
        f"join / yardstick = {mj / my:.3f}  ({mj / nwin:.3f} ms per window)")
    return mj, my


def host_legs(c, metric, first, nwin, st, say, tag, recipe):
    count = nwin * W
    lib = _lib.gpu()
    sc = np.empty((count, K), np.float32)
    ix = np.empty((count, K), np.uint64)
    p = lambda a, off=0: C.c_void_p(a.ctypes.data + off)  # noqa: E731
    js = torch.empty((count, K), dtype=torch.float32, device="cuda")
    ji = torch.empty((count, K), dtype=torch.int64, device="cuda")
    hs = torch.empty((count, K), dtype=torch.float32).pin_memory()
    hi = torch.empty((count, K), dtype=torch.int64).pin_memory()

    def host():
        _lib.gpu_check(lib.mvfgpu_knn_join(c._h, None, metric, first, count, K, 1, p(sc), p(ix), None))

    def per_window():
        for w in range(nwin):
            _lib.gpu_check(lib.mvfgpu_knn_join(c._h, None, metric, first + w * W, W, K, 1, p(sc, w * W * K * 4), p(ix, w * W * K * 8), None))

    def device_then_copy():
        c.knn_join_device(K, metric, first, count, js.data_ptr(), ji.data_ptr(), 0, stream=st.cuda_stream)
        with torch.cuda.stream(st):
            hs.copy_(js, non_blocking=True)
            hi.copy_(ji, non_blocking=True)
        st.synchronize()

    def wall(fn):
        fn()
        ts = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    th, tw, td = wall(host), wall(per_window), wall(device_then_copy)
    say(f"{tag}: wall, results in host memory: host call (double-buffered) {spread(th)}  one blocking call per window {spread(tw)}  "
        f"device call + one copy at the end {spread(td)}  host / device = {np.median(th) / np.median(td):.3f}  "
        f"un-overlapped / host = {np.median(tw) / np.median(th):.3f}")
    if recipe:
        def old_way():
            rows = widen(c.read_rows(first, count))
            self_pos = np.arange(first, first + count, dtype=np.uint64)[:, None]
            for w in range(nwin):
                r = c.search(rows[w * W:(w + 1) * W], K + 1, metric)
                hit = r.indices == self_pos[w * W:(w + 1) * W]
                hit[~hit.any(axis=1), -1] = True     # self not among the k + 1: the last entry goes
                keep = ~hit
                ix[w * W:(w + 1) * W] = r.indices[keep].reshape(W, K)
                sc[w * W:(w + 1) * W] = r.scores[keep].reshape(W, K)
        tr = wall(old_way)
        want_i = ix.copy()
        host()
        say(f"{tag}: the caller-side recipe (read back, widen, mvfgpu_search k + 1 per window, strip on the host) {spread(tr)}  "
            f"recipe / host call = {np.median(tr) / np.median(th):.2f}  same indices: {bool((want_i == ix).all())}")


def repair_leg(c, metric, first, nwin, say, tag):
    lib = _lib.gpu()
    sc = np.empty((W, K), np.float32)
    ix = np.empty((W, K), np.uint64)
    total, per = 0, []
    for w in range(nwin):
        _lib.gpu_check(lib.mvfgpu_knn_join(c._h, None, metric, first + w * W, W, K, 1, C.c_void_p(sc.ctypes.data), C.c_void_p(ix.ctypes.data), None))
        t = c.last_timing()  # repaired_queries is kept whether or not the handle profiles; scan_kernel only with profiling on (0 here)
        total += t.repaired_queries
        per.append(t.scan_kernel)
    say(f"{tag}: repaired_queries over {nwin} windows of {W}: {total}  scan_kernel first / last window {per[0]} / {per[-1]}  "
        f"selection_state at the end {c.info().selection_state}")


def near_duplicate_rows(n, dim):
    g = torch.Generator(device="cuda").manual_seed(7)
    rows = torch.empty((n, dim), dtype=torch.float32)
    step = 250_000
    for r0 in range(0, n, step):
        m = min(step, n - r0)
        anchors = torch.randn((m + 31) // 32, dim, device="cuda", generator=g)
        blk = anchors.repeat_interleave(32, 0)[:m] * 0.8 + torch.randn(m, dim, device="cuda", generator=g) * 0.25
        dup = torch.arange(37, m, 37, device="cuda")
        blk[dup] = blk[dup - 1] + torch.randn(len(dup), dim, device="cuda", generator=g) * 1e-4
        rows[r0:r0 + m] = blk.cpu()
    return rows.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="all", choices=["small", "big", "all"])
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"k-NN join, MI355X, synthetic corpora (DESIGN.md section 6), self-join with MVFGPU_JOIN_EXCLUDE_SELF, k = {K}; device ms = HIP "
        f"events around the calls on one torch stream, median (min .. max) of {ROUNDS} rounds after one warm round, yardstick and join alternating")
    st = torch.cuda.Stream()
    first = 100_000
    if a.legs in ("small", "all"):
        for n, dim, dt, metric, nwin, recipe in [(1_000_000, 768, G.FLOAT32, G.COSINE, 64, False), (1_000_000, 768, G.FLOAT16, G.L2, 64, True),
                                                 (4_000_000, 768, G.INT8, G.INNER_PRODUCT, 64, False)]:
            tag = f"{n / 1e6:g}M x {dim} {NAME[dt]} {METRIC[metric]}"
            with G.GpuCorpus.synthetic(n, dim, dt, SEED) as c:
                device_legs(c, dt, metric, first, nwin, st, say, tag)
                if n == 1_000_000:
                    host_legs(c, metric, first, nwin, st, say, tag, recipe)
                if dt == G.FLOAT32:
                    repair_leg(c, metric, first, 16, say, tag + " uniform")
        rows = near_duplicate_rows(1_000_000, 768)
        with G.GpuCorpus.from_array(rows) as c:
            del rows
            tag = "1M x 768 f32 cosine, planted near-duplicates"
            repair_leg(c, G.COSINE, first, 16, say, tag)
            device_legs(c, G.FLOAT32, G.COSINE, first, 16, st, say, tag)
    if a.legs in ("big", "all"):
        with G.GpuCorpus.synthetic(10_000_000, 768, G.FLOAT32, SEED) as c:
            device_legs(c, G.FLOAT32, G.COSINE, first, 8, st, say, "10M x 768 f32 cosine")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
