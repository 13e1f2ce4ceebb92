"""Filtered search (mvfgpu_search_filtered_device): device ms per call, timed with HIP events around the call on one torch
stream inside this process; the variants of a comparison ALTERNATE inside the timing loop (variant A, variant B, A, B, ..),
one warm round first, the median of the rounds reported.

  1. mask route against the plain search of the same handle and nq (densities 0.9 and 0.5; nq 1 and 1024);
  2. list route against mask route (densities 1e-4 .. 0.3; nq 1, 16, 1024) and F2's achieved bytes/s
     (admitted rows x row pitch x query groups / time);
  3. mvfgpu_filter_create wall time, host form, with and without the row list (alternating, median of 5);
  --cliff: instead, the mask route of batched searches (nq 64, 256, 1024) under masks of density 0.015 .. 0.07, where the
     plain search's kernels -- as under tombstones of that weight -- flag their queries for the exact repair pass, against
     the list route (2 rounds: a flagged batch takes seconds).

    python scripts/probe_filtered.py [--out profiles/r09_filtered.txt] [--shapes f32,int8] [--rounds 5]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metrovector_amd import gpu as G  # noqa: E402
from oracle import mvf_oracle as O  # noqa: E402

SEED = 0x4D564631
NAME = {G.FLOAT32: "f32", G.INT8: "int8"}
METRIC = {G.INNER_PRODUCT: "dot", G.COSINE: "cosine"}
SHAPES = {"f32": (10_000_000, 768, G.FLOAT32, G.COSINE), "int8": (50_000_000, 768, G.INT8, G.INNER_PRODUCT)}
K = 100


def alternate_ms(fns, stream, rounds):
    """{name: median device ms}: every round runs every variant once, in order; the first round is warm-up."""
    ts = {name: [] for name in fns}
    for r in range(rounds + 1):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if r:
                ts[name].append(a.elapsed_time(b))
    return {name: float(np.median(v)) for name, v in ts.items()}


def forced_filter(c, allow_bits, route):
    if route:
        os.environ["MVF_FILTER_ROUTE"] = str(route)
    else:
        os.environ.pop("MVF_FILTER_ROUTE", None)
    c.reload_tuning()
    t0 = time.perf_counter()
    f = c.make_filter(allow_bits)
    return f, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="f32,int8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cliff", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say(f"filtered search, MI355X, synthetic corpora, k = {K}; device ms = HIP events around one call on a torch stream, the "
        f"variants of a line alternating in one loop, median of {a.rounds} rounds after one warm round")
    st = torch.cuda.Stream()
    rng = np.random.default_rng(7)
    for shape in a.shapes.split(","):
        n, dim, dt, metric = SHAPES[shape]
        qcode = dt if dt == G.INT8 else G.FLOAT32
        pitch = (dim * (4 if dt == G.FLOAT32 else 1) + 15) // 16 * 16
        tag = f"{n / 1e6:g}M x {dim} {NAME[dt]} {METRIC[metric]}"
        with G.GpuCorpus.synthetic(n, dim, dt, SEED) as c:
            bufs = {}
            for nq in (1, 16, 1024):
                dq = torch.from_numpy(O.synth_queries(SEED + nq, nq, dim, dt)).cuda()
                bufs[nq] = (dq, torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda"))
            torch.cuda.synchronize()

            def plain(nq):
                dq, ds, di = bufs[nq]
                return lambda: c.search_device(dq.data_ptr(), qcode, dim, nq, K, metric, ds.data_ptr(), di.data_ptr(), 0, st.cuda_stream)

            def filtered(f, nq):
                dq, ds, di = bufs[nq]
                return lambda: c.search_filtered_device(f, dq.data_ptr(), qcode, dim, nq, K, metric, ds.data_ptr(), di.data_ptr(), 0,
                                                        st.cuda_stream)

            for nq in (1, 1024):  # the first searches build norms and shadows: not timed
                plain(nq)()
            st.synchronize()
            if a.cliff:
                say(f"-- 2b. {tag}: batched searches under selective masks, mask route against list route")
                for density in (0.015, 0.02, 0.03, 0.05, 0.07):
                    bits = np.packbits(rng.random(n) < density, bitorder="little")
                    fm, _ = forced_filter(c, bits, 1)
                    fl, _ = forced_filter(c, bits, 2)
                    for nq in (64, 256, 1024):
                        if nq not in bufs:
                            dq = torch.from_numpy(O.synth_queries(SEED + nq, nq, dim, dt)).cuda()
                            bufs[nq] = (dq, torch.empty((nq, K), dtype=torch.float32, device="cuda"),
                                        torch.empty((nq, K), dtype=torch.int64, device="cuda"))
                        t = alternate_ms({"mask": filtered(fm, nq), "list": filtered(fl, nq)}, st, 2)
                        rule = G.filter_route(n, dim, dt, nq, K, fl.admitted)
                        say(f"{tag} density {density:g} admitted {fl.admitted:9d} nq {nq:5d}: mask {t['mask']:9.3f} ms  list {t['list']:9.3f} ms  "
                            f"list/mask {t['list'] / t['mask']:7.3f}  rule -> {'list' if rule == 2 else 'mask'}")
                    fm.close()
                    fl.close()
                os.environ.pop("MVF_FILTER_ROUTE", None)
                continue
            say(f"-- 1. {tag}: mask route against the plain search")
            for density in (0.9, 0.5):
                bits = np.packbits(rng.random(n) < density, bitorder="little")
                f, _ = forced_filter(c, bits, 1)
                for nq in (1, 1024):
                    t = alternate_ms({"plain": plain(nq), "mask": filtered(f, nq)}, st, a.rounds)
                    say(f"{tag} density {density:g} nq {nq:5d}: plain {t['plain']:9.3f} ms  mask {t['mask']:9.3f} ms  ratio {t['mask'] / t['plain']:.3f}")
                f.close()
            say(f"-- 2. {tag}: list route against mask route")
            for density in (1e-4, 1e-3, 1e-2, 1e-1, 0.3):
                bits = np.packbits(rng.random(n) < density, bitorder="little")
                fm, ms_nolist = forced_filter(c, bits, 1)
                fl, ms_list = forced_filter(c, bits, 2)
                m = fl.admitted
                for nq in (1, 16, 1024):
                    groups = (nq + 3) // 4
                    if m * pitch * groups > 1e12:  # seconds per call: the mask route wins by an order of magnitude, not timed
                        say(f"{tag} density {density:g} admitted {m:9d} nq {nq:5d}: list not timed ({m * pitch * groups / 1e12:.1f} TB of rows)")
                        continue
                    t = alternate_ms({"mask": filtered(fm, nq), "list": filtered(fl, nq)}, st, a.rounds)
                    rule = G.filter_route(n, dim, dt, nq, K, m)
                    say(f"{tag} density {density:g} admitted {m:9d} nq {nq:5d}: mask {t['mask']:9.3f} ms  list {t['list']:9.3f} ms  "
                        f"list/mask {t['list'] / t['mask']:7.3f}  F2 rows {m * pitch * groups / (t['list'] * 1e-3) / 1e12:5.2f} TB/s  rule -> "
                        f"{'list' if rule == 2 else 'mask'}")
                if shape == "f32":
                    walls = {1: [], 2: []}
                    for _ in range(5):
                        for route in (1, 2):
                            f, ms = forced_filter(c, bits, route)
                            f.close()
                            walls[route].append(ms)
                    say(f"-- 3. {tag} density {density:g}: mvfgpu_filter_create wall, host form, median of 5 alternating: without the list "
                        f"{np.median(walls[1]):.2f} ms, with the list ({m} rows) {np.median(walls[2]):.2f} ms")
                fm.close()
                fl.close()
            os.environ.pop("MVF_FILTER_ROUTE", None)


if __name__ == "__main__":
    main()
