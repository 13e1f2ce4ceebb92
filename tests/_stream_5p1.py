"""Shared by tests/test_gpu_stream_5p1.py and its child process: the grid of one-query searches on the forced 6-bit route (scan
path 7).  Run as a program (under MVF_STREAM_5P1=0, in a fresh process) it answers the grid from the 6-bit LAYOUT and stores the
answers for the parent to compare with its own, which come from the 5+1 layout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 0x4D564651
L2, IP, COS = 0, 1, 2
F32 = 0
N = 40_001  # not a multiple of the 64-row tile; about 40 scan blocks of 1024 rows
DIMS = (128, 192, 200, 768, 1024)
KS = (1, 10, 100, 204)
OLD_LAYOUT_DIM = 129  # dim mod 128 in 1..64: the 5+1 layout would be larger, the handle keeps the 6-bit one


def eligible(dim):
    return dim % 128 == 0 or dim % 128 > 64


def rows_of(oracle, dim, n=N):
    return np.ascontiguousarray(oracle.synth_rows(SEED, 0, n, dim, F32))


def query_of(oracle, dim):
    return oracle.synth_queries(SEED + 1, 1, dim, F32).copy()


def grid(c, q):
    """(metric, k) -> (result on scan path 7, its timing, its low-plane lines)"""
    out = {}
    c.set_scan_path(7)
    for metric in (L2, IP, COS):
        for k in KS:
            res = c.search(q, k, metric)
            out[(metric, k)] = (res, c.last_timing(), c.stream_lo_lines())
    return out


def main(path):
    from metrovector_amd import gpu as G
    from oracle import mvf_oracle
    mvf_oracle.build()
    assert os.environ.get("MVF_STREAM_5P1") == "0"
    out = {}
    for dim in [d for d in DIMS if eligible(d)] + [OLD_LAYOUT_DIM]:
        with G.GpuCorpus.from_array(rows_of(mvf_oracle, dim)) as c:
            c.set_profiling(True)
            for (metric, k), (res, t, lines) in grid(c, query_of(mvf_oracle, dim)).items():
                assert t.scan_kernel == 7 and lines == (0, 0), (dim, metric, k, t.scan_kernel, lines)
                out[f"{dim}/{metric}/{k}/i"] = res.indices
                out[f"{dim}/{metric}/{k}/r"] = res.raw
                out[f"{dim}/{metric}/{k}/s"] = res.scores.view(np.uint32)
            out[f"{dim}/bytes"] = np.array([c.info().device_bytes], np.uint64)
    np.savez(path, **out)
    print("ok")


if __name__ == "__main__":
    main(sys.argv[1])
