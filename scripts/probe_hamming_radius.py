"""Hamming radius search (mvfgpu_search_hamming_radius, include/mvf_gpu_hamming_radius.h) on one MI355X: 10M random rows of 16,
128 and 512 packed bytes with 1, 16, 128 and 1024 queries, max_per_query = 100.  Per shape, alternating in one process on one box,
medians of 5 with their minimum and maximum after a warm-up of each:
  (a) this search with a SPARSE radius -- an eighth of the row's bits, which no random row comes near; five near-copies of every
      query are planted, so every query has a handful of matches -- : HQ, HR2 and HRP from the stage timer
      (mvfgpu_selftest_hamming_radius_stage_ms) and the blocking host call by the host clock; HR2's bytes, rows x bytes, over its
      time for one query, and its multiply-accumulates, nq x rows x bits, over its time for 1024 queries;
  (b) the same with a DENSE radius, 8 x dimension: every row matches every query, every list runs over, and the host call ends
      in the completing Hamming search (expected to be poor: reported, not tuned);
  (c) the recipe a caller had before: the Hamming search at k = 100, routes 1 and 2 (stage timer, scan + merge).
The counts of (a) are checked against the planted rows, those of (b) against the row count.

    python scripts/probe_hamming_radius.py [--out profiles/r27_hamming_radius.txt] [--small]
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

K, REPS, PLANTED = 100, 5, 5


def spread(ts):
    return f"{np.median(ts):8.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def host_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


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
    rng = np.random.default_rng(0x4852)
    st = torch.cuda.Stream()
    say(f"Hamming radius search against the Hamming top-k it stands beside, MI355X, {n / 1e6:g}M random rows, max_per_query = k = {K}; "
        f"median [min .. max] of {REPS} repetitions, the searches alternating after a warm-up of each")
    for dim in (16, 128, 512):
        x = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        qall = rng.integers(0, 256, (1024, dim), dtype=np.uint8)
        at = rng.choice(n, 1024 * PLANTED, replace=False)
        flips = np.zeros((1024 * PLANTED, 8 * dim), bool)
        for i in range(len(flips)):  # up to dim / 2 differing bits: well inside the sparse radius of dim bits
            flips[i, rng.choice(8 * dim, rng.integers(0, dim // 2 + 1), replace=False)] = True
        x[at] = np.repeat(qall, PLANTED, axis=0) ^ np.packbits(flips, axis=1)
        del flips
        with G.GpuCorpus.from_array(x, device=0) as c:
            for nq in (1, 16, 128, 1024):
                q = np.ascontiguousarray(qall[:nq])
                dq = torch.from_numpy(q).cuda()
                radii = {"sparse": np.full(nq, dim, np.uint32), "dense": np.full(nq, 8 * dim, np.uint32)}
                dr = {k_: torch.from_numpy(v.view(np.int32)).cuda() for k_, v in radii.items()}
                dc = torch.empty(nq, dtype=torch.int64, device="cuda")
                ds, di = torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()

                def stages(kind):
                    return c.hamming_radius_stage_ms(dq.data_ptr(), G.UINT8, dim, nq, dr[kind].data_ptr(), K, dc.data_ptr(), ds.data_ptr(),
                                                     di.data_ptr(), st.cuda_stream)

                def hamming(route):
                    c.set_hamming_route(route)
                    return c.hamming_stage_ms(dq.data_ptr(), G.UINT8, dim, nq, K, ds.data_ptr(), di.data_ptr(), st.cuda_stream)

                res = {kind: c.search_hamming_radius(q, radii[kind], K) for kind in radii}
                ok = "counts ok" if (res["sparse"].counts == PLANTED).all() and (res["dense"].counts == n).all() else \
                    f"COUNTS WRONG (sparse {res['sparse'].counts.min()} .. {res['sparse'].counts.max()})"
                stages("sparse"), stages("dense"), hamming(1), hamming(2)
                t = {"sparse": [], "dense": [], "sparse host": [], "dense host": [], 1: [], 2: []}
                for _ in range(REPS):
                    for kind in radii:
                        t[kind].append(stages(kind))
                        t[kind + " host"].append(host_ms(lambda: c.search_hamming_radius(q, radii[kind], K)))
                    for r in (1, 2):
                        t[r].append(sum(hamming(r)))
                c.set_hamming_route(0)
                f = G.hamming_radius_form(dim, nq, n)
                sp, de = np.array(t["sparse"]), np.array(t["dense"])
                scan = float(np.median(sp[:, 1])) * 1e-3
                rate = f"HR2 {n * dim / scan / 1e12:5.2f} TB/s" if nq == 1 else f"HR2 {nq * n * dim * 8 / scan / 1e12:6.1f} T MAC/s"
                total = float(np.median(sp.sum(1)))
                say(f"{dim:4d} bytes nq {nq:4d} ({f.row_slices} slices, tile {f.query_tile}, {f.blocks_per_cu} blocks/CU; {ok}):")
                say(f"    (a) sparse  HQ {spread(sp[:, 0])} HR2 {spread(sp[:, 1])} HRP {spread(sp[:, 2])} host call {spread(t['sparse host'])} | {rate}")
                say(f"    (b) dense   HQ {spread(de[:, 0])} HR2 {spread(de[:, 1])} HRP {spread(de[:, 2])} host call {spread(t['dense host'])}")
                say(f"    (c) Hamming top-{K}: route 1 {spread(t[1])}, (c1) / (a) {np.median(t[1]) / total:5.2f}x; route 2 {spread(t[2])}, "
                    f"(c2) / (a) {np.median(t[2]) / total:5.2f}x   [(a) = its three stages, {total:.3f} ms]")
        del x


if __name__ == "__main__":
    main()
