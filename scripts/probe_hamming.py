"""Hamming search (mvfgpu_search_hamming[_device], include/mvf_gpu_hamming.h) on one MI355X, rows of 128 packed bytes
(1024 bits), k = 100, one query and 1024 queries:
  * H0's and H1's kernel times (mvfgpu_selftest_hamming_stage_ms) and the whole device call between HIP events;
  * one query: H0's algorithmic bytes (rows x pitch) over its time, against the 8 TB/s HBM peak;
  * 1024 queries: H0's word-operations, 2 x nq x rows x pitch / 4 (one xor and one popcount-add per word), over its time;
  * the ratio to THE RECIPE IT REPLACES, in the same process and alternating with it: mvfgpu_search_device(L2) on a second
    corpus holding the same rows unpacked to 0/1 UInt8 elements (8 x the bytes), warmed so that whatever it builds on first use
    exists.  Both paths must return the same indices and raw distances on the timed inputs; that is checked first.
The comparison runs on the same 10M rows: the unpacked copy is 10 GB of host memory (np.unpackbits) and 10 GB of HBM beside
the packed rows.  Only where the host cannot hold it (MemoryError) or the upload is refused does it fall back to 2M rows for
both paths, and says so.  Every figure is the median of the timed repetitions with their minimum and maximum, after a warm-up
of every form.

    python scripts/probe_hamming.py [--out profiles/r24_hamming.txt] [--small]
    rocprofv3 --pmc <counters> --output-format csv -d <dir> -- python scripts/probe_hamming.py --kernels-only
        (hardware counters of H0 / H1 in a run of their own: 10M rows, one and 1024 queries, two calls each, nothing timed)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metrovector_amd import gpu as G  # noqa: E402

DIM, K, REPS = 128, 100, 5
HBM_PEAK = 8e12


def spread(ts):
    return f"{np.median(ts):9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def event_ms(fn, stream, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 200k and 100k rows, 1 and 64 queries")
    ap.add_argument("--kernels-only", action="store_true", help="two device calls per shape and nothing else: for a counter run")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n_big, n_cmp, nqs = (200_000, 100_000, [1, 64]) if a.small else (10_000_000, 2_000_000, [1, 1024])
    rng = np.random.default_rng(0x48414D)
    st = torch.cuda.Stream()
    say(f"Hamming search, MI355X, random rows of {DIM} packed bytes ({DIM * 8} bits), k = {K}; median [min .. max] of {REPS} timed "
        "repetitions after a warm-up; H0 / H1: events around the kernels; call: events around the device call")

    def outputs(nq):
        return (torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda"),
                torch.empty((nq, K), dtype=torch.int32, device="cuda"))

    def time_hamming(c, n, q):
        nq = q.shape[0]
        dq = torch.from_numpy(q).cuda()
        ds, di, dr = outputs(nq)
        torch.cuda.synchronize()

        def call():
            c.search_hamming_device(dq.data_ptr(), G.UINT8, DIM, nq, K, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), st.cuda_stream)

        def stages():
            return c.hamming_stage_ms(dq.data_ptr(), G.UINT8, DIM, nq, K, ds.data_ptr(), di.data_ptr(), st.cuda_stream)

        call(), stages()
        st.synchronize()
        return call, np.array([stages() for _ in range(REPS)]), (di, dr)

    # the large scan, packed corpus alone
    x = rng.integers(0, 256, (n_big, DIM), dtype=np.uint8)
    with G.GpuCorpus.from_array(x, device=0) as c:
        for nq in nqs:
            q = rng.integers(0, 256, (nq, DIM), dtype=np.uint8)
            if a.kernels_only:
                dq = torch.from_numpy(q).cuda()
                ds, di, dr = outputs(nq)
                for _ in range(2):
                    c.search_hamming_device(dq.data_ptr(), G.UINT8, DIM, nq, K, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), st.cuda_stream)
                st.synchronize()
                continue
            call, sm, _ = time_hamming(c, n_big, q)
            t = event_ms(call, st, REPS)
            h0 = float(np.median(sm[:, 0])) * 1e-3
            f = G.hamming_form(DIM, min(nq, 1024), K, n_big)
            say(f"{n_big / 1e6:g}M rows nq {nq:4d} (form {f.form}, {f.lanes_per_row} lanes/row, tile {f.query_tile}, {f.row_slices} slices): "
                f"H0 {spread(sm[:, 0])}  H1 {spread(sm[:, 1])}  call {spread(t)}")
            if nq == 1:
                say(f"{'':20s} H0 reads {n_big * DIM / 1e9:.2f} GB -> {n_big * DIM / h0 / 1e12:.2f} TB/s = {100 * n_big * DIM / h0 / HBM_PEAK:.0f} % of the 8 TB/s peak")
            else:
                ops = 2.0 * nq * n_big * DIM / 4
                say(f"{'':20s} H0 {ops / 1e12:.2f} T word-operations -> {ops / h0 / 1e12:.1f} T/s; the rows' bytes once per query tile: "
                    f"{n_big * DIM * ((nq + f.query_tile - 1) // f.query_tile) / h0 / 1e12:.2f} TB/s")

    if a.kernels_only:
        return
    # the comparison with the unpacked L2 recipe, alternating: on all rows, on n_cmp where the unpacked copy cannot be held
    c8 = None
    try:
        x8 = np.unpackbits(x, axis=1)
        c8 = G.GpuCorpus.from_array(x8, device=0)
        n_cmp = n_big
    except Exception as e:  # noqa: BLE001 - any refusal of the large copy is reported and the small one taken
        say(f"the unpacked copy of {n_big / 1e6:g}M rows could not be held ({type(e).__name__}: {e}); comparing on {n_cmp / 1e6:g}M rows")
        x = np.ascontiguousarray(x[:n_cmp])
        x8 = np.unpackbits(x, axis=1)
        c8 = G.GpuCorpus.from_array(x8, device=0)
    del x8
    with G.GpuCorpus.from_array(x, device=0) as c, c8:
        for nq in nqs:
            q = rng.integers(0, 256, (nq, DIM), dtype=np.uint8)
            q8 = np.unpackbits(q, axis=1)
            call, sm, (di, dr) = time_hamming(c, n_cmp, q)
            dq8 = torch.from_numpy(q8).cuda()
            ds8, di8, dr8 = outputs(nq)
            torch.cuda.synchronize()

            def base():
                c8.search_device(dq8.data_ptr(), G.UINT8, DIM * 8, nq, K, G.L2, ds8.data_ptr(), di8.data_ptr(), dr8.data_ptr(), st.cuda_stream)

            for _ in range(3):  # the baseline's first calls build what it keeps
                base()
            call()
            st.synchronize()
            same = torch.equal(di, di8) and torch.equal(dr, dr8)
            t_new, t_base = [], []
            for _ in range(REPS):  # alternating
                t_new += event_ms(call, st, 1)
                t_base += event_ms(base, st, 1)
            say(f"{n_cmp / 1e6:g}M rows nq {nq:4d}: Hamming call {spread(t_new)} (H0 {spread(sm[:, 0])})  unpacked L2 search {spread(t_base)}  "
                f"baseline / Hamming {np.median(t_base) / np.median(t_new):6.2f}x  same indices and raw: {'yes' if same else 'NO'}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
