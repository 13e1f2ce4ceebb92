"""Sign-bit search (mvfgpu_search_signbits[_device], include/mvf_gpu_signbits.h) on one MI355X: 10M random rows, k = 100, rows of
128 packed bytes with 1, 16, 128 and 1024 queries, rows of 64 and 512 bytes with 1024 queries.  Per shape, alternating in one
process on one box, medians of 5 with their minimum and maximum after a warm-up of each:
  (a) this call: SQ, S2 and H1 from the stage timer (mvfgpu_selftest_signbits_stage_ms) and the device call between events;
      S2's multiply-accumulates, nq x rows x bits, over its time against the datasheet's dense int8 peak;
  (b) THE RECIPE IT REPLACES: mvfgpu_search_device(InnerProduct) with the same Int8 queries over an Int8 corpus holding the same
      rows unpacked to +1 / -1 (8 x the bytes), between events; its answer must equal (a)'s in indices and raw values.  At 512
      bytes the unpacked copy is 41 GB: measured only with --unpack-512;
  (c) the Hamming search on the packed rows with the queries' sign bits, routes 1 and 2 (stage timer, scan + merge).
Then recall@100 of this first stage and of the Hamming first stage against the exact Float32 cosine top-100, on one synthetic
clustered corpus (200k rows of 1024 dimensions around 256 centres, 256 queries near rows): the share of the true top-100 among
each first stage's 100 and 1000 best.

    python scripts/probe_signbits.py [--out profiles/r26_signbits.txt] [--small] [--unpack-512]
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
I8_PEAK = 5.0e15 / 2  # multiply-accumulates per second: the datasheet's dense INT8 rate


def spread(ts):
    return f"{np.median(ts):8.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def event_ms(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def unpack_pm1(x):
    """the rows unpacked to +1 / -1 int8, element 8 i + b = bit b of byte i"""
    b = np.unpackbits(x, axis=1, bitorder="little").view(np.int8)
    np.multiply(b, 2, out=b)
    np.subtract(b, 1, out=b)
    return b


def timed_shapes(say, n, unpack_512):
    rng = np.random.default_rng(0x5347)
    st = torch.cuda.Stream()
    say(f"sign-bit search against the recipes it stands beside, MI355X, {n / 1e6:g}M random rows, k = {K}; median [min .. max] of {REPS} "
        "repetitions, the searches alternating after a warm-up of each")
    for dim, nqs in ((128, (1, 16, 128, 1024)), (64, (1024,)), (512, (1024,))):
        x = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        c8 = None
        if dim < 512 or unpack_512:
            try:
                c8 = G.GpuCorpus.from_array(unpack_pm1(x), device=0)
            except Exception as e:  # noqa: BLE001 - a refusal of the 8 x larger copy is reported
                say(f"{dim:4d} bytes: the unpacked copy could not be held ({type(e).__name__}: {e}): (b) is not measured")
        with G.GpuCorpus.from_array(x, device=0) as c:
            for nq in nqs:
                q = rng.integers(-127, 128, (nq, 8 * dim), dtype=np.int8)
                dq = torch.from_numpy(q).cuda()
                dh = torch.from_numpy(np.packbits(q > 0, axis=1, bitorder="little")).cuda()
                out = [(torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda"),
                        torch.empty((nq, K), dtype=torch.int32, device="cuda")) for _ in range(3)]
                torch.cuda.synchronize()

                def stages():
                    return c.signbits_stage_ms(dq.data_ptr(), G.INT8, 8 * dim, nq, K, out[0][0].data_ptr(), out[0][1].data_ptr(), st.cuda_stream)

                def call():
                    c.search_signbits_device(dq.data_ptr(), G.INT8, 8 * dim, nq, K, out[0][0].data_ptr(), out[0][1].data_ptr(),
                                             out[0][2].data_ptr(), st.cuda_stream)

                def recipe():
                    c8.search_device(dq.data_ptr(), G.INT8, 8 * dim, nq, K, G.INNER_PRODUCT, out[1][0].data_ptr(), out[1][1].data_ptr(),
                                     out[1][2].data_ptr(), st.cuda_stream)

                def hamming(route):
                    c.set_hamming_route(route)
                    return c.hamming_stage_ms(dh.data_ptr(), G.UINT8, dim, nq, K, out[2][0].data_ptr(), out[2][1].data_ptr(), st.cuda_stream)

                stages(), call(), hamming(1), hamming(2)
                same = "not compared"
                if c8 is not None:
                    for _ in range(3):  # the recipe's first calls build what it keeps
                        recipe()
                    st.synchronize()
                    same = "yes" if torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2]) else "NO"
                t = {"stages": [], "call": [], "recipe": [], 1: [], 2: []}
                for _ in range(REPS):
                    t["stages"].append(stages())
                    t["call"].append(event_ms(call, st))
                    if c8 is not None:
                        t["recipe"].append(event_ms(recipe, st))
                    for r in (1, 2):
                        t[r].append(sum(hamming(r)))
                c.set_hamming_route(0)
                sm = np.array(t["stages"])
                a_ms = float(np.median(t["call"]))
                rate = float(nq) * n * dim * 8 / (float(np.median(sm[:, 1])) * 1e-3)
                f = G.signbits_form(dim, nq, K, n)
                say(f"{dim:4d} bytes nq {nq:4d} ({f.row_slices} slices, tile {f.query_tile}): (a) SQ {spread(sm[:, 0])} S2 {spread(sm[:, 1])} H1 "
                    f"{spread(sm[:, 2])} call {spread(t['call'])} | S2 {rate / 1e12:7.1f} T MAC/s = {100 * rate / I8_PEAK:4.1f} % of the int8 peak")
                b_txt = f"(b) unpacked InnerProduct {spread(t['recipe'])}, (b) / (a) {np.median(t['recipe']) / a_ms:5.2f}x, same indices and raw: {same}" \
                    if c8 is not None else "(b) not measured"
                say(f"{'':19s}{b_txt} | (c) Hamming route 1 {spread(t[1])}, (c1) / (a) {np.median(t[1]) / a_ms:5.2f}x; route 2 {spread(t[2])}, "
                    f"(c2) / (a) {np.median(t[2]) / a_ms:5.2f}x")
        if c8 is not None:
            c8.close()
        del x


def recall(say, n):
    rng = np.random.default_rng(0x5348)
    d, nq = 1024, 256
    centres = rng.standard_normal((256, d), dtype=np.float32)
    x = centres[rng.integers(0, 256, n)] + 1.5 * rng.standard_normal((n, d), dtype=np.float32)
    q = x[rng.integers(0, n, nq)] + 0.5 * rng.standard_normal((nq, d), dtype=np.float32)
    with G.GpuCorpus.from_array(x, device=0) as cf:
        truth = cf.search(q, 100, G.COSINE).indices
    with G.GpuCorpus.from_array(G.pack_sign_bits(x), device=0) as c:
        got = {"sign-bit search (int8 query)": c.search_signbits(G.quantize_queries_int8(q), 1000).indices,
               "Hamming search (sign-bit query)": c.search_hamming(G.pack_sign_bits(q), 1000).indices}
    say(f"recall of the exact Float32 cosine top-100, {n / 1e3:g}k rows of {d} dimensions around 256 centres (noise 1.5), {nq} queries near rows:")
    for name, idx in got.items():
        at = [np.mean([len(set(t.tolist()) & set(g[:m].tolist())) / 100.0 for t, g in zip(truth, idx)]) for m in (100, 1000)]
        say(f"  {name:32s} among its 100 best {at[0]:.3f}, among its 1000 best {at[1]:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 200k rows, 20k rows for the recall")
    ap.add_argument("--unpack-512", action="store_true", help="(b) at 512 bytes too: 41 GB of host memory and of HBM")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:  # as it goes: a run that is cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    timed_shapes(say, 200_000 if a.small else 10_000_000, a.unpack_512)
    recall(say, 20_000 if a.small else 200_000)


if __name__ == "__main__":
    main()
