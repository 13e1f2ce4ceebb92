"""Digests of the output buffers of the routes that score rows with K1's arithmetic outside K1 -- radius (the streaming
route R1 and the batched route that ends in R3), candidates (short and long lists, k <= 1024 and k > 1024), the filtered
list route (queries in groups of four -- a lone query is a short group of four too -- and, at 3001 and 12296 Float32
dimensions, one by one) and a one-query Float32 search streamed over the int8 shadow -- from seeded calls on small synthetic
shapes: four row types x three metrics.  Two builds of libmvf_gpu.so that compute the
same bytes print the same lines:

    MVF_GPU_LIB_PATH=<one build>   python scripts/digest_routes.py > a.txt
    MVF_GPU_LIB_PATH=<another one> python scripts/digest_routes.py > b.txt && cmp a.txt b.txt
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["MVF_FILTER_ROUTE"] = "2"  # every filtered search below by the list route
import numpy as np  # noqa: E402

from metrovector_amd import gpu as G  # noqa: E402
from oracle import mvf_oracle as O  # noqa: E402

NAME = {G.FLOAT32: "f32", G.FLOAT16: "f16", G.INT8: "int8", G.UINT8: "uint8"}
METRIC = {G.L2: "L2", G.INNER_PRODUCT: "IP", G.COSINE: "cosine"}


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def say(what, res, counts=None):
    bufs = [res.scores, res.indices, res.raw] + ([counts] if counts is not None else [])
    print(f"{what:70s} {digest(*bufs)}", flush=True)


def radii_for(c, qs, metric, rank):
    top = c.search(qs, rank, metric)
    return top.scores[:, rank - 1].copy()


def main():
    rng = np.random.default_rng(17)
    # dims 7 / 100: lane groups of 1 .. 8 and 4 .. 32 across the types; Float32 3001: four queries no longer fit the LDS, the
    # filtered list route scores them one by one (as the candidate search always does); 12296: the one query read through the cache
    shapes = [(7, 4001), (100, 5003)]
    for dt in (G.FLOAT32, G.FLOAT16, G.INT8, G.UINT8):
        for dim, n in shapes + ([(3001, 600), (12296, 600)] if dt == G.FLOAT32 else []):
            rows = O.synth_rows(1000 + dim, 0, n, dim, dt)
            qs = O.synth_queries(2000 + dim, 9, dim, dt)
            dead = rng.random(n) < 0.1
            allow = rng.random(n) < 0.6
            short = rng.integers(0, n + n // 10, size=(9, 2 * 1024 + 5)).astype(np.uint64)
            long_ = rng.integers(0, n, size=(2, 9000)).astype(np.uint64)
            with G.GpuCorpus.from_array(rows, index_base=5) as c:
                c.set_tombstones(np.packbits(dead, bitorder="little"))
                for metric in (G.L2, G.INNER_PRODUCT, G.COSINE):
                    tag = f"{NAME[dt]:5s} dim {dim:5d} {METRIC[metric]:6s}"
                    c.set_scan_path(1)
                    r = radii_for(c, qs, metric, 40)
                    for nq in (1, 9):  # R1 with one and with four queries per pass
                        res = c.search_radius(qs[:nq], r[:nq], 64, metric)
                        say(f"{tag} radius streaming, {nq} queries", res, res.counts)
                    if dt == G.FLOAT32 and dim <= 100:
                        c.set_scan_path(2)  # the batched route: R3 re-scores
                        res = c.search_radius(qs, r, 64, metric)
                        say(f"{tag} radius batched, 9 queries", res, res.counts)
                    c.set_scan_path(0)
                    for k in (10, 1500):
                        res = c.search_candidates(qs, short + np.uint64(5), k, metric)
                        say(f"{tag} candidates m 2053 k {k}", res, res.counts)
                        if dim <= 100:
                            res = c.search_candidates(qs[:2], long_ + np.uint64(5), k, metric)
                            say(f"{tag} candidates m 9000 k {k}", res, res.counts)
                    with c.make_filter(allow) as f:
                        for nq, k in ((9, 10), (1, 10), (9, 1500)):  # two groups of four and a short one; a lone query; the sort ending
                            say(f"{tag} filtered list route, {nq} queries k {k}", c.search_filtered(qs[:nq], k, metric, f))
    # one Float32 query streamed over the int8 shadow (re-scored by rescore_k1_kernel)
    os.environ["MVF_STREAM_I8"] = "1"
    n, dim = 60_000, 128
    rows = O.synth_rows(51, 0, n, dim, G.FLOAT32)
    q = O.synth_queries(52, 300, dim, G.FLOAT32)
    with G.GpuCorpus.from_array(rows) as c:
        c.set_scan_path(5)
        c.search(q, 20, G.COSINE)  # builds the shadow
        c.set_scan_path(0)
        c.set_profiling(True)
        for metric in (G.L2, G.INNER_PRODUCT, G.COSINE):
            res = c.search(q[:1], 20, metric)
            say(f"f32   dim   128 {METRIC[metric]:6s} one query, int8 shadow stream (scan kernel {c.last_timing().scan_kernel})", res)


if __name__ == "__main__":
    main()
