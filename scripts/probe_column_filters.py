"""Column filters (mvfgpu_column_*, mvfgpu_filter_create_where; DESIGN.md §5 "P0"): what the predicate kernel achieves and
what a where-filter costs against the path it replaces.

  1. P0 alone (mvfgpu_selftest_where_kernel_ms: device events around each launch on the handle's stream): kernel time and
     achieved bytes/s.  Algorithmic bytes = each clause's column read once + n / 8 of allow words written (+ n / 8 of the base
     filter's mask where one is given).
  2. Wall time of mvfgpu_filter_create_where against numpy predicate + packbits + mvfgpu_filter_create on the same predicate,
     alternating in one loop, median.

    python scripts/probe_column_filters.py [--rows 10000000 100000000] [--out profiles/r11_column_filters.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metrovector_amd import gpu as G  # noqa: E402

READ_TBS = 6.9  # bare coalesced read, profiles/r02_access_shape_read_bandwidth.txt: 6.8-7.0 TB/s


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["Column filters: P0 (scan_columns.hip) alone, and mvfgpu_filter_create_where against the host path it replaces",
             "(numpy predicate + packbits + mvfgpu_filter_create).  One MI355X, rows of 8 int8 values, scripts/probe_column_filters.py.",
             f"Kernel ms: device events around each of 16 launches after one warm launch, median; fraction of the {READ_TBS} TB/s bare read",
             f"(profiles/r02_access_shape_read_bandwidth.txt).  Wall ms: time.perf_counter around each call, the two paths alternating, median of {args.rounds}.", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for n in args.rows:
        rng = np.random.default_rng(n)
        tenant = rng.integers(0, 1000, n, dtype=np.uint32)
        cat = rng.integers(0, 20000, n, dtype=np.uint32)
        ts = rng.integers(0, 2 ** 40, n, dtype=np.uint64)
        members = rng.permutation(20000)[:4096].astype(np.uint64)
        with G.GpuCorpus.synthetic(n, 8, G.INT8, 1) as c, c.attach_column(tenant) as ct, c.attach_column(cat) as cc, \
                c.attach_column(ts) as cs:
            cases = [
                ("one UInt32 clause   tenant == 7", [(ct, "==", 7)], lambda: tenant == 7, 4 * n),
                ("one UInt64 clause   ts >= 2^39", [(cs, ">=", 2 ** 39)], lambda: ts >= 2 ** 39, 8 * n),
                ("four clauses, two columns (tenant between, tenant !=, ts >=, ts <)",
                 [(ct, "between", (100, 499)), (ct, "!=", 250), (cs, ">=", 2 ** 38), (cs, "<", 2 ** 40 - 2 ** 37)],
                 lambda: (tenant >= 100) & (tenant <= 499) & (tenant != 250) & (ts >= 2 ** 38) & (ts < 2 ** 40 - 2 ** 37), 2 * 4 * n + 2 * 8 * n),
                ("IN with 4096 values (UInt32 category)", [(cc, "in", members)], lambda: np.isin(cat, members), 4 * n),
            ]
            for name, clauses, host_pred, col_bytes in cases:
                ms = med(c.where_kernel_ms(clauses, repeats=17)[1:])
                nbytes = col_bytes + n // 8
                tbs = nbytes / (ms * 1e-3) / 1e12
                say(f"{n / 1e6:5.0f}M rows  {name}")
                say(f"    P0 kernel {ms:8.3f} ms   {nbytes / 1e6:8.1f} MB   {tbs:5.2f} TB/s   {tbs / READ_TBS:4.2f} of the bare read")
                tw, th, thp = [], [], []
                admitted = None
                for r in range(args.rounds + 1):
                    t0 = time.perf_counter()
                    with_where = c.make_filter_where(clauses)
                    t1 = time.perf_counter()
                    mask = host_pred()
                    bits = np.packbits(mask, bitorder="little")
                    t2 = time.perf_counter()
                    with_bits = c.make_filter(bits)
                    t3 = time.perf_counter()
                    assert with_where.admitted == with_bits.admitted
                    admitted = with_where.admitted
                    with_where.close()
                    with_bits.close()
                    if r:  # the first round warms both
                        tw.append((t1 - t0) * 1e3)
                        thp.append((t2 - t1) * 1e3)
                        th.append((t3 - t1) * 1e3)
                say(f"    create_where wall {med(tw):8.3f} ms   host path {med(th):9.3f} ms (predicate + packbits {med(thp):9.3f} ms)   "
                    f"ratio {med(th) / med(tw):7.1f}x   admitted {admitted}")
            # the base filter's mask is one more read of n / 8
            with c.make_filter(tenant < 500) as base:
                ms = med(c.where_kernel_ms([(ct, "==", 7)], base=base, repeats=17)[1:])
                nbytes = 4 * n + n // 4
                say(f"{n / 1e6:5.0f}M rows  one UInt32 clause with a base filter")
                say(f"    P0 kernel {ms:8.3f} ms   {nbytes / 1e6:8.1f} MB   {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s")
        del tenant, cat, ts
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
