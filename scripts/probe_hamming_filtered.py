"""Filtered Hamming search (mvfgpu_search_hamming_filtered[_device], include/mvf_gpu_hamming_filtered.h) on one MI355X: 10M random
rows of 128 packed bytes, k = 100, with 1, 16, 128 and 1024 queries under filters that admit 1e-4, 1e-3, 1e-2, 0.1 and 0.5 of the
rows; a second leg at 64 and 512 bytes with 1 and 1024 queries.  Per point, alternating in one process on one box, medians of 5
with their minimum and maximum after a warm-up of each, all from device events (the stage timers, which wait for the stream):
  mask   route 1: the Hamming search's scan with the filter's deny mask (MVF_FILTER_ROUTE=1 when the filter was made);
  list   route 2: HQ, HG, H1 (MVF_FILTER_ROUTE=2), its three stages, and HG's gathered bytes, admitted x query tiles x pitch,
         over HG's time;
  plain  the unfiltered mvfgpu_search_hamming_device on the same handle (mvfgpu_selftest_hamming_stage_ms): the baseline.
The two routes' results are compared byte for byte at every point.

    python scripts/probe_hamming_filtered.py [--out profiles/r30_hamming_filtered.txt] [--small]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metrovector_amd import gpu as G  # noqa: E402

K, REPS = 100, 5
DENSITIES = (1e-4, 1e-3, 1e-2, 0.1, 0.5)


def spread(ts):
    return f"{np.median(ts):8.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 200k rows")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:  # as it goes: a run that is cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    n = 200_000 if a.small else 10_000_000
    rng = np.random.default_rng(0x4847)
    st = torch.cuda.Stream()
    say(f"Filtered Hamming search, MI355X, {n / 1e6:g}M random rows, k = {K}; median [min .. max] of {REPS} repetitions from device "
        f"events, the three searches alternating after a warm-up of each; auto = the route the library's rule takes")
    wins = []
    for dim, nqs in ((128, (1, 16, 128, 1024)), (64, (1, 1024)), (512, (1, 1024))):
        x = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        qall = rng.integers(0, 256, (1024, dim), dtype=np.uint8)
        with G.GpuCorpus.from_array(x, device=0) as c:
            for density in DENSITIES:
                allow = rng.random(n) < density
                flt = {}
                for route in (1, 2):
                    os.environ["MVF_FILTER_ROUTE"] = str(route)
                    c.reload_tuning()
                    flt[route] = c.make_filter(allow)
                adm = flt[2].admitted
                assert flt[2].info().has_row_list == 1
                for nq in nqs:
                    dq = torch.from_numpy(np.ascontiguousarray(qall[:nq])).cuda()
                    out = {r: (torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda"))
                           for r in (0, 1, 2)}
                    torch.cuda.synchronize()

                    def run(r):
                        ds, di = out[r]
                        if r == 0:
                            return (0.0,) + c.hamming_stage_ms(dq.data_ptr(), G.UINT8, dim, nq, K, ds.data_ptr(), di.data_ptr(), st.cuda_stream)
                        return c.hamming_filtered_stage_ms(flt[r], dq.data_ptr(), G.UINT8, dim, nq, K, ds.data_ptr(), di.data_ptr(), st.cuda_stream)

                    t = {0: [], 1: [], 2: []}
                    for r in t:
                        run(r)
                    same = bool((out[1][0] == out[2][0]).all()) and bool((out[1][1] == out[2][1]).all())
                    for _ in range(REPS):
                        for r in t:
                            t[r].append(run(r))
                    tot = {r: np.array(t[r]).sum(1) for r in t}
                    f = G.hamming_filtered_form(dim, nq, K, n, adm, True, 2)
                    auto = G.hamming_filtered_form(dim, nq, K, n, adm, True, 0).route
                    hg = np.array(t[2])
                    tiles = -(-nq // f.query_tile)
                    rate = adm * tiles * ((dim + 15) // 16 * 16) / (float(np.median(hg[:, 1])) * 1e-3) / 1e9
                    ratio = float(np.median(tot[1]) / np.median(tot[2]))
                    wins.append((dim, nq, density, ratio, float(np.median(tot[1]) / np.median(tot[0]))))
                    say(f"{dim:4d} bytes nq {nq:4d} density {density:6g} ({adm} admitted; {f.list_slices} slices x {tiles} tiles of {f.query_tile}; auto {auto}): "
                        f"plain {spread(tot[0])} | mask {spread(tot[1])}, mask / plain {wins[-1][4]:5.2f}x | list {spread(tot[2])} = HQ {spread(hg[:, 0])} "
                        f"HG {spread(hg[:, 1])} H1 {spread(hg[:, 2])}, HG gathers {rate:8.2f} GB/s | mask / list {ratio:7.2f}x | same bytes: {'yes' if same else 'NO'}")
                for fl in flt.values():
                    fl.close()
        del x
    say("mask / list above 1.07 (the spread between boxes): " + ", ".join(f"({d}, {q}, {p:g}) {r:.2f}x" for d, q, p, r, _ in wins if r > 1.07))
    say("mask / list at or below 1.07: " + ", ".join(f"({d}, {q}, {p:g}) {r:.2f}x" for d, q, p, r, _ in wins if r <= 1.07))
    say(f"mask / plain: {min(w[4] for w in wins):.2f}x .. {max(w[4] for w in wins):.2f}x")


if __name__ == "__main__":
    main()
