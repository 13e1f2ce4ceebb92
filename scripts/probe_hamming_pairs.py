"""Hamming pair join (mvfgpu_hamming_pairs, include/mvf_gpu_hamming_pairs.h) on one MI355X: 1M random rows of 16, 128 and 512
packed bytes.  Per width two radii:
  sparse -- an eighth of the row's bits, which no two random rows come near; one row in a thousand is replaced by a near-copy of
            another row, so the answer is about rows / 1000 pairs, all listed;
  dense  -- the radius at which a random row pairs with about a hundred others (from the binomial distribution of the distance
            of two random rows): about 50 x rows pairs, more than 2^24, so the call reports total and degrees and lists nothing.
Per shape, alternating in one process on one box, medians of 5 with their minimum and maximum after a warm-up of each:
  (a) HJ and HJP from the stage timer (mvfgpu_selftest_hamming_pairs_stage_ms; HJP's figure includes the call's one wait for
      the total) and the blocking call by the host clock; HJ's multiply-accumulates, rows x (rows - 1) / 2 x bits, over its time;
  (b) the recipe the call replaces: the packed rows (here: the host's copy, no read-back is charged) fed to
      mvfgpu_search_hamming_radius as queries in windows of 1024 with max_per_query = 1024, by the host clock;
  (c) HR2 alone on one window of 1024 queries (mvfgpu_selftest_hamming_radius_stage_ms), for its multiply-accumulates per second
      at the same row width.
The join's total and degrees are checked against the recipe's counts (degree = count - 1).

    python scripts/probe_hamming_pairs.py [--out profiles/r31_hamming_pairs.txt] [--small]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metrovector_amd import gpu as G  # noqa: E402

REPS, WINDOW, ROOM = 5, 1024, 1 << 24


def spread(ts):
    return f"{np.median(ts):10.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def host_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def dense_radius(bits, wanted, rows):
    """the largest r at which a random row still expects at most `wanted` partners among `rows`: the distance of two random rows
    is binomial(bits, 1/2) (exact integers: 2^4096 is no float)"""
    limit, acc, r = (wanted << bits) // rows, 0, -1
    while acc + math.comb(bits, r + 1) <= limit:
        r += 1
        acc += math.comb(bits, r)
    return max(r, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 100k rows")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:  # as it goes: a run that is cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    n = 100_000 if a.small else 1_000_000
    rng = np.random.default_rng(0x484A)
    st = torch.cuda.Stream()
    say(f"Hamming pair join against the windowed radius search it replaces, MI355X, {n / 1e6:g}M random rows, room for 2^24 pairs; "
        f"median [min .. max] of {REPS} repetitions, the two alternating after a warm-up of each")
    for dim in (16, 128, 512):
        x = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        copies = rng.choice(n, 2 * (n // 1000), replace=False)
        src, dst = copies[: n // 1000], copies[n // 1000:]
        flips = np.zeros((len(dst), 8 * dim), bool)
        for i in range(len(dst)):  # up to dim / 2 differing bits: well inside the sparse radius of dim bits
            flips[i, rng.choice(8 * dim, rng.integers(0, dim // 2 + 1), replace=False)] = True
        x[dst] = x[src] ^ np.packbits(flips, axis=1)
        del flips
        radii = {"sparse": dim, "dense": dense_radius(8 * dim, 100, n)}
        d_deg = torch.empty(n, dtype=torch.int32, device="cuda")
        d_first, d_second = torch.empty(ROOM, dtype=torch.int64, device="cuda"), torch.empty(ROOM, dtype=torch.int64, device="cuda")
        d_raw = torch.empty(ROOM, dtype=torch.int32, device="cuda")
        q1 = np.ascontiguousarray(x[:WINDOW])
        dq, dc = torch.from_numpy(q1).cuda(), torch.empty(WINDOW, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with G.GpuCorpus.from_array(x, device=0) as c:
            f = G.hamming_pairs_form(dim, n, max_pairs=ROOM)
            say(f"{dim:4d} bytes: tile {f.query_tile}, spans of {f.span_rows} rows, {f.tiles} tiles x {f.spans} spans, {f.blocks} blocks, "
                f"{f.lds_bytes} B LDS, scratch up to {f.scratch_bytes / 2**20:.0f} MiB")
            for kind, r in radii.items():
                def stages():
                    return c.hamming_pairs_stage_ms(r, ROOM, d_deg.data_ptr(), d_first.data_ptr(), d_second.data_ptr(), d_raw.data_ptr(), st.cuda_stream)

                def recipe():
                    counts = np.empty(n, np.uint64)
                    for w0 in range(0, n, WINDOW):
                        counts[w0:w0 + WINDOW] = c.search_hamming_radius(x[w0:w0 + WINDOW], r, WINDOW).counts
                    return counts

                def hr2():
                    dr = torch.full((WINDOW,), r, dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    return c.hamming_radius_stage_ms(dq.data_ptr(), G.UINT8, dim, WINDOW, dr.data_ptr(), 0, dc.data_ptr(), 0, 0, st.cuda_stream)[1]

                res, counts = c.hamming_pairs(r, ROOM), recipe()  # (the warm-up of both, and the check)
                ok = "total and degrees = the recipe's counts - 1" if np.array_equal(res.degrees, counts - 1) and 2 * res.total == int(res.degrees.sum()) \
                    else "THE JOIN AND THE RECIPE DISAGREE"
                stages(), hr2()
                t = {"stages": [], "call": [], "recipe": [], "hr2": []}
                for _ in range(REPS):
                    t["stages"].append(stages()[2:])
                    t["call"].append(host_ms(lambda: c.hamming_pairs(r, ROOM))[0])
                    t["recipe"].append(host_ms(recipe)[0])
                    t["hr2"].append(hr2())
                sg = np.array(t["stages"])
                macs = n * (n - 1) / 2 * 8 * dim
                say(f"  {kind:6s} radius {r:4d}: {res.total} pairs, {'listed' if res.listed else 'not listed'}, largest degree {int(res.degrees.max())}; {ok}")
                say(f"    (a) HJ {spread(sg[:, 0])}  HJP {spread(sg[:, 1])}  blocking call {spread(t['call'])} | "
                    f"HJ {macs / (np.median(sg[:, 0]) * 1e-3) / 1e12:7.1f} T MAC/s over the upper triangle")
                say(f"    (b) recipe, {-(-n // WINDOW)} windows {spread(t['recipe'])} | (b) / (a) blocking call {np.median(t['recipe']) / np.median(t['call']):6.2f}x")
                say(f"    (c) HR2, one window of {WINDOW} queries {spread(t['hr2'])} | "
                    f"HR2 {WINDOW * n * 8 * dim / (np.median(t['hr2']) * 1e-3) / 1e12:7.1f} T MAC/s")
        del x


if __name__ == "__main__":
    main()
