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
    python scripts/probe_hamming.py --routes [--out profiles/r25_hamming_mfma.txt] [--small]
        (route 1, H0 + H1, against route 2, HQ + H2 + H1 -- mvfgpu_set_hamming_route -- on one handle in one process, alternating,
        with the stage timer: 10M rows of 128 bytes at k = 100 over the window sizes 16 .. 1024, 10M rows of 32 .. 512 bytes at 1024
        queries, k = 1024 once; H2's multiply-accumulates, nq x rows x bits, over the time in front of H1 against the datasheet's
        dense FP4 and int8 matrix peaks; the answers of both routes compared on every timed shape; the unpacked L2 search once)
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


FP4_PEAK, I8_PEAK = 10.1e15 / 2, 5.0e15 / 2  # multiply-accumulates per second: the datasheet's dense MXFP4 and INT8 rates


def routes_table(say, small):
    """route 1 against route 2 per shape: the stage timer's (before H1, H1) of both, alternating, on one handle"""
    n = 200_000 if small else 10_000_000
    rng = np.random.default_rng(0x48414D)
    st = torch.cuda.Stream()
    say(f"Hamming search, routes 1 (H0 + H1) and 2 (HQ + H2 + H1) on one handle, MI355X, {n / 1e6:g}M random rows; stage timer, median "
        f"[min .. max] of {REPS} repetitions alternating between the routes after a warm-up of both; scan = everything in front of H1")
    shapes = [(DIM, nq, K) for nq in (16, 64, 128, 256, 1024)] + [(DIM, 1024, 1024)] + [(d, 1024, K) for d in (32, 64, 256, 512)]
    wins = []
    for dim in dict.fromkeys(d for d, _, _ in shapes):
        x = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        with G.GpuCorpus.from_array(x, device=0) as c:
            for _, nq, k in [sh for sh in shapes if sh[0] == dim]:
                dq = torch.from_numpy(rng.integers(0, 256, (nq, dim), dtype=np.uint8)).cuda()
                out = {r: (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))
                       for r in (1, 2)}
                torch.cuda.synchronize()

                def stages(r):
                    c.set_hamming_route(r)
                    return c.hamming_stage_ms(dq.data_ptr(), G.UINT8, dim, nq, k, out[r][0].data_ptr(), out[r][1].data_ptr(), st.cuda_stream)

                stages(1), stages(2)
                same = torch.equal(out[1][0], out[2][0]) and torch.equal(out[1][1], out[2][1])
                ms = {1: [], 2: []}
                for _ in range(REPS):
                    for r in (1, 2):
                        ms[r].append(stages(r))
                t = {r: np.array(ms[r]) for r in ms}
                tot = {r: float(np.median(t[r].sum(1))) for r in t}
                macs = float(nq) * n * dim * 8
                rate = macs / (float(np.median(t[2][:, 0])) * 1e-3)
                f = G.hamming_mfma_form(dim, nq, k, n)
                say(f"{dim:4d} bytes nq {nq:4d} k {k:4d}: route 1 scan {spread(t[1][:, 0])} H1 {spread(t[1][:, 1])} | route 2 ({f.row_slices} slices, "
                    f"tile {f.query_tile}) scan {spread(t[2][:, 0])} H1 {spread(t[2][:, 1])} | route 1 / route 2 {tot[1] / tot[2]:5.2f}x | H2 "
                    f"{rate / 1e12:7.1f} T MAC/s = {100 * rate / FP4_PEAK:4.1f} % of the FP4 peak, {100 * rate / I8_PEAK:4.1f} % of the int8 peak | "
                    f"same bytes: {'yes' if same else 'NO'}")
                wins.append(((dim, nq, k), tot[1] / tot[2]))
            c.set_hamming_route(0)
            if dim == DIM:  # the recipe the packed search replaces, on the same box: the rows unpacked to 0/1 bytes under L2
                try:
                    with G.GpuCorpus.from_array(np.unpackbits(x, axis=1), device=0) as c8:
                        dq8 = torch.from_numpy(rng.integers(0, 2, (1024, DIM * 8), dtype=np.uint8)).cuda()
                        o8 = (torch.empty((1024, K), dtype=torch.float32, device="cuda"), torch.empty((1024, K), dtype=torch.int64, device="cuda"))
                        torch.cuda.synchronize()

                        def base():
                            c8.search_device(dq8.data_ptr(), G.UINT8, DIM * 8, 1024, K, G.L2, o8[0].data_ptr(), o8[1].data_ptr(), 0, st.cuda_stream)

                        for _ in range(3):
                            base()
                        st.synchronize()
                        say(f"{DIM:4d} bytes nq 1024 k {K:4d}: the unpacked L2 search ({DIM * 8} UInt8 elements a row), device call {spread(event_ms(base, st, REPS))}")
                except Exception as e:  # noqa: BLE001 - a refusal of the 8 x larger copy is reported
                    say(f"the unpacked copy could not be held ({type(e).__name__}: {e}): the L2 search is not measured")
        del x
    say("route 1 / route 2 above 1.07 (the spread between boxes): " + ", ".join(f"{s} {w:.2f}x" for s, w in wins if w > 1.07))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 200k and 100k rows, 1 and 64 queries")
    ap.add_argument("--kernels-only", action="store_true", help="two device calls per shape and nothing else: for a counter run")
    ap.add_argument("--routes", action="store_true", help="route 1 against route 2 (the MFMA route) over window sizes, row lengths and k")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.routes:
        routes_table(say, a.small)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return

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
