#!/usr/bin/env python3
"""CPU model of the 6-bit shadow stream's proven bound (shadow_6b.hip, query_16s.h): no GPU.
The quantisers and statistics of the shadow kernels restated in numpy on the oracle's rows; per metric the bound delta in
units of the score distribution's sigma, the constant c = delta / (sigma sqrt(dim)) that api.hip's stream_6b_shape uses, and
the predicted number of rows within 2 delta of the k-th best of `--rows` rows (Gaussian tail).
    python scripts/model_stream_6b_bound.py [--n 200000] [--dim 768] [--rows 10000000] [--k 100]"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import mvf_oracle as O  # noqa: E402

SEED = 0x4D564631


def quantise_rows(x, levels):
    """x6 (or x8), s_r, |x6|, |ex| per row: shadow_6b_kernel / shadow_i8_kernel."""
    sr = np.abs(x).max(axis=1) / np.float32(levels)
    t = np.where(sr[:, None] > 0, x / np.where(sr > 0, sr, 1)[:, None], 0).astype(np.float32)
    q = np.clip(np.rint(t), -levels, levels)
    e = t - q
    ex = np.sqrt((e.astype(np.float64) ** 2).sum(1)) * 1.0005 + 1e-3
    xa = np.sqrt((q.astype(np.float64) ** 2).sum(1)) * 1.0005 + ex
    return q.astype(np.int32), sr.astype(np.float64), xa, ex


def quantise_query(q, qmax):
    """Q, s_q, |Q|, |eq|: prep_query_i8s (qmax 127) / prep_query_16s (qmax 16256)."""
    sq = np.abs(q).max() / np.float32(qmax)
    t = (q / sq).astype(np.float32) if sq > 0 else np.zeros_like(q)
    Q = np.clip(np.rint(t), -qmax, qmax)
    e = t - Q
    return Q.astype(np.int64), float(sq), math.sqrt(float((Q.astype(np.float64) ** 2).sum())) * 1.0005, \
        math.sqrt(float((e.astype(np.float64) ** 2).sum())) * 1.0005 + 1e-3


def tail(z):
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def z_of(p):
    lo, hi = -10.0, 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if tail(mid) > p else (lo, mid)
    return 0.5 * (lo + hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, default=8)
    a = ap.parse_args()
    x = O.synth_rows(SEED, 0, a.n, a.dim, O.F32).astype(np.float32)
    qs = O.synth_queries(SEED + 1, a.queries, a.dim, O.F32).astype(np.float32)
    xn = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    print(f"# {a.n} x {a.dim} oracle rows, {a.queries} queries; tail extrapolated to {a.rows} rows at k = {a.k}")
    print("rows_bits,query_bits,metric,delta_sigma,c=delta/(sigma*sqrt(dim)),rows_within_2delta")
    for rbits, levels in ((8, 127), (6, 31), (5, 15)):
        _, sr, xa, ex = quantise_rows(x, levels)
        A, B = (sr * xa).max(), (sr * ex).max()
        Ac, Bc = (sr * xa / xn).max(), (sr * ex / xn).max()
        for qbits, qmax in ((8, 127), (16, 16256)):
            for metric, name in ((O.IP, "ip"), (O.COS, "cos"), (O.L2, "l2")):
                ds = []
                for q in qs:
                    _, sq, Qn, eq = quantise_query(q, qmax)
                    qn = math.sqrt(float((q.astype(np.float64) ** 2).sum()))
                    dot = x.astype(np.float64) @ q.astype(np.float64)
                    if metric == O.COS:
                        d, sigma = sq * (eq * Ac + Qn * Bc) / qn, (dot / (qn * xn)).std()
                    elif metric == O.IP:
                        d, sigma = sq * (eq * A + Qn * B), dot.std()
                    else:  # the selection works on the GEMM-form squared distance
                        d, sigma = 2 * sq * (eq * A + Qn * B), (qn * qn + xn * xn - 2 * dot).std()
                    ds.append(d / sigma)
                dsig = float(np.mean(ds))
                inside = a.rows * tail(z_of(a.k / a.rows) - 2 * dsig)
                print(f"{rbits},{qbits},{name},{dsig:.3f},{dsig / math.sqrt(a.dim):.5f},{inside:.0f}")


if __name__ == "__main__":
    main()
