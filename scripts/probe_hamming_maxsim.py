"""Binary MaxSim (mvfgpu_search_hamming_maxsim[_device], include/mvf_gpu_hamming_maxsim.h) on one MI355X, k = 100, tokens of 16
packed bytes (128 bits), random rows, the key column shuffled so that the index's list is a real gather:
  shape 0: 10M rows under keys of 1000 rows (ColPali-like pages);   shape 1: 50M rows under keys of 100 rows;
each with one query set and with 16 sets, of 32 tokens.  Per shape and batch, alternating in one process on one box, medians of
5 with their minimum and maximum after a warm-up of each:
  (a) this call: prepare, scan (B0), sum and tail from the stage timer (mvfgpu_selftest_hamming_maxsim_stage_ms) and the device
      call between events, with the row bytes/s and the MAC/s (rows x query rows x bits) the scan achieves;
  (b) the recipe the call replaces: mvfgpu_search_maxsim under InnerProduct over the same rows unpacked to +-1 Int8, one byte per
      bit -- the same ranking (dot = bits - 2 d) at eight times the bytes --, its device call between events and its stages.
The first keys of (a) and (b) are compared at one set -- a smoke check, the tests hold the proof.

    python scripts/probe_hamming_maxsim.py [--out profiles/r29_hamming_maxsim.txt] [--shapes 0,1] [--small]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from metrovector_amd import gpu as G  # noqa: E402

K, REPS, DIM, T = 100, 5, 16, 32
SHAPES = ((10_000_000, 1000), (50_000_000, 100))  # (rows, rows per key)


def spread(ts):
    return f"{np.median(ts):8.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]"


def event_ms(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def random_bytes(rng, shape):
    n = int(np.prod(shape))
    return rng.integers(0, 2**64, (n + 7) // 8, dtype=np.uint64).view(np.uint8)[:n].reshape(shape)


def unpacked(x):
    """packed rows as +-1 Int8, one byte per bit: bit set -> +1"""
    out = np.empty((x.shape[0], x.shape[1] * 8), np.int8)
    for lo in range(0, x.shape[0], 1 << 20):
        out[lo:lo + (1 << 20)] = np.unpackbits(x[lo:lo + (1 << 20)], axis=1).astype(np.int8) * 2 - 1
    return out


def timed_shape(say, n, per_key):
    rng = np.random.default_rng([0x424D53, n])
    st = torch.cuda.Stream()
    x = random_bytes(rng, (n, DIM))
    col = (rng.permutation(n) // per_key).astype(np.uint32)
    say(f"{n / 1e6:g}M rows x {DIM} bytes, keys of {per_key} rows ({-(-n // per_key)} keys), k = {K}, sets of {T} tokens; median "
        f"[min .. max] of {REPS}, the two searches alternating after a warm-up of each")
    with G.GpuCorpus.from_array(x, device=0) as cb, G.GpuCorpus.from_array(unpacked(x), device=0) as ci:
        with cb.attach_column(col) as colb, ci.attach_column(col) as coli, cb.make_partition(colb) as pb, ci.make_partition(coli) as pi:
            for nq in (1, 16):
                q = random_bytes(rng, (nq, T, DIM))
                dq, dqi = torch.from_numpy(q).cuda(), torch.from_numpy(unpacked(q.reshape(-1, DIM)).reshape(nq, T, DIM * 8)).cuda()
                out = [(torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda"))
                       for _ in range(2)]
                torch.cuda.synchronize()

                def stages():
                    return cb.hamming_maxsim_stage_ms(pb, dq.data_ptr(), G.UINT8, DIM, nq, T, K, out[0][0].data_ptr(), out[0][1].data_ptr(), st.cuda_stream)

                def call():
                    cb.search_hamming_maxsim_device(pb, dq.data_ptr(), G.UINT8, DIM, nq, T, K, out[0][0].data_ptr(), out[0][1].data_ptr(), 0, st.cuda_stream)

                def recipe_stages():
                    return ci.maxsim_stage_ms(pi, dqi.data_ptr(), G.INT8, DIM * 8, nq, T, K, G.INNER_PRODUCT, out[1][0].data_ptr(), out[1][1].data_ptr(), st.cuda_stream)

                def recipe():
                    ci.search_maxsim_device(pi, dqi.data_ptr(), G.INT8, DIM * 8, nq, T, K, G.INNER_PRODUCT, out[1][0].data_ptr(), out[1][1].data_ptr(), 0, st.cuda_stream)

                stages(), call(), recipe_stages(), recipe()
                t = {"stages": [], "call": [], "rstages": [], "recipe": []}
                for _ in range(REPS):
                    t["stages"].append(stages())
                    t["call"].append(event_ms(call, st))
                    t["rstages"].append(recipe_stages())
                    t["recipe"].append(event_ms(recipe, st))
                sm, rm = np.array(t["stages"]), np.array(t["rstages"])
                a_ms, b_ms, scan = float(np.median(t["call"])), float(np.median(t["recipe"])), float(np.median(sm[:, 1]))
                f = G.hamming_maxsim_form(DIM, nq, T, -(-n // per_key), n)
                say(f"  {nq:2d} sets (chunk {f.chunk_tokens}, window {f.window_sets}): (a) prepare {spread(sm[:, 0])} B0 {spread(sm[:, 1])} sum "
                    f"{spread(sm[:, 2])} tail {spread(sm[:, 3])} call {spread(t['call'])}")
                say(f"{'':11s}B0: {n * DIM / scan / 1e6:.1f} GB/s of row bytes, {n * nq * T * DIM * 8 / scan / 1e9:.1f} TMAC/s")
                say(f"{'':11s}(b) Int8 +-1 recipe: ordinals {spread(rm[:, 0])} M0 {spread(rm[:, 1])} M1 {spread(rm[:, 2])} tail {spread(rm[:, 3])} call "
                    f"{spread(t['recipe'])}; (a) / (b) {a_ms / b_ms:5.3f}x")
                if nq == 1:
                    torch.cuda.synchronize()
                    same = bool((out[0][1] == out[1][1]).all()) and bool((out[1][0] == DIM * 8 * T - 2 * out[0][0]).all())
                    say(f"{'':11s}the keys of (a) and (b) are equal and score(b) = bits x tokens - 2 score(a): {'yes' if same else 'NO'}")
    del x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--small", action="store_true", help="a rehearsal: a fiftieth of the rows")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:  # as it goes: a run that is cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say("Binary MaxSim against the Int8 +-1 multi-vector search, MI355X")
    for i in (int(s) for s in a.shapes.split(",")):
        n, per_key = SHAPES[i]
        timed_shape(say, n // 50 if a.small else n, per_key)


if __name__ == "__main__":
    main()
