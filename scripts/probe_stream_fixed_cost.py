"""What one search of the headline costs OUTSIDE its kernels: the bench.py headline corpus (10M x 768 Float32 synthetic rows,
cosine, one query, top-100), built once, and `--steps` back-to-back `mvfgpu_search_device` calls timed with the wall clock
around a final synchronise (as bench.py: timed_steps) in the four combinations

    library profiling {on, off}  x  {three torch events per step, as ShardedSearcher.search records them, none}

rotated over `--rounds` rounds in ONE process.  Prints ms per step for every combination and round, the means, and the
differences: us per step the library's own markers cost, us per step the three torch events cost.  Also prints
`search_launches` of the newest search where the library reports it.  Development aid."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from metrovector_amd import gpu as G
from metrovector_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--scan-path", type=int, default=0)
ap.add_argument("--only", choices=["on3", "on0", "off3", "off0"], default=None,
                help="one combination only (a kernel trace of it: rocprofv3 --kernel-trace -- python ... --only off0 --rounds 1)")
args = ap.parse_args()

SEED = 0x4D564631  # bench.py's
corpus = G.GpuCorpus.synthetic(args.rows, args.dim, 0, SEED, device=0)
corpus.set_scan_path(args.scan_path)
dq = torch.empty((1, args.dim), dtype=torch.float32, device="cuda:0")
_lib.gpu_check(_lib.gpu().mvfgpu_synth_queries_device(dq.data_ptr(), 1, args.dim, 0, SEED + 1, 0, None))
ds = torch.empty((1, args.k), dtype=torch.float32, device="cuda:0")
di = torch.empty((1, args.k), dtype=torch.int64, device="cuda:0")
dr = torch.empty((1, args.k), dtype=torch.int32, device="cuda:0")
stream = torch.cuda.current_stream(0).cuda_stream
torch.cuda.synchronize()


def step(events):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if events else None
    if ev:
        ev[0].record()
    corpus.search_device(dq.data_ptr(), 0, args.dim, 1, args.k, G.COSINE, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), stream)
    if ev:
        ev[1].record()
        ev[2].record()
    return ev


route = None


def timed(profiling, events):
    global route
    corpus.set_profiling(profiling)
    keep = []
    for _ in range(args.warmup):
        keep.append(step(events))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        keep.append(step(events))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    if profiling:
        route = corpus.last_timing()
    corpus.set_profiling(False)
    return ms


combos = [(True, True), (True, False), (False, True), (False, False)]
name = {c: f"profiling {'on ' if c[0] else 'off'} / torch events {'3' if c[1] else '0'}" for c in combos}
timed(True, True)  # shadow build, first-use allocations
print(f"route: scan_kernel {route.scan_kernel}, search_launches {getattr(route, 'search_launches', 'n/a')}, scan_ms_avg "
      f"{route.scan_ms_avg:.4f}, search_ms_avg {route.search_ms_avg:.4f}", flush=True)
if args.only:
    combos = [(args.only[:2] == "on", args.only[-1] == "3")]
got = {c: [] for c in combos}
for r in range(args.rounds):
    order = combos[r % len(combos):] + combos[:r % len(combos)]
    for c in order:
        got[c].append(timed(*c))
    print(f"round {r}: " + "  ".join(f"[{name[c]}] {got[c][-1]:.4f}" for c in combos), flush=True)
mean = {c: sum(v) / len(v) for c, v in got.items()}
for c in combos:
    print(f"{name[c]}: mean {mean[c]:.4f} ms per step  (min {min(got[c]):.4f}, max {max(got[c]):.4f})")
if args.only:
    corpus.close()
    sys.exit(0)
lib = ((mean[(True, True)] - mean[(False, True)]) + (mean[(True, False)] - mean[(False, False)])) / 2 * 1e3
tev = ((mean[(True, True)] - mean[(True, False)]) + (mean[(False, True)] - mean[(False, False)])) / 2 * 1e3
print(f"library profiling markers: {lib:+.1f} us per step;  three torch events: {tev:+.1f} us per step")
corpus.close()
