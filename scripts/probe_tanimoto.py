"""Tanimoto search (mvfgpu_search_tanimoto[_device], include/mvf_gpu_tanimoto.h) on one MI355X: 10M random rows of 128, 256 and
512 packed bytes, k = 100, with 1, 16, 128 and 1024 queries.  Per shape, alternating in one process on one box, medians of 5 with
their minimum and maximum after a warm-up of each:
  (a) this call: TQ, T2 and H1 from the stage timer (mvfgpu_selftest_tanimoto_stage_ms) and the device call between events;
  (b) mvfgpu_search_hamming on the same handle with the same queries, routes 1 and 2 (stage timer, scan + merge): the better of
      the two is what (a) is compared with.  T2 issues H2's MFMAs and one more per (step, fragment) for the row popcount, so
      close to route 2 at 1024 queries is the expectation; where (a) is slower, the stage that holds the difference is named.
Rows and queries are random with an eighth to three quarters of their bits set, so that the popcounts vary as fingerprints' do; at
128 bytes and 16 queries the returned scores are recomputed with numpy -- a smoke check, the tests hold the proof.

    python scripts/probe_tanimoto.py [--out profiles/r28_tanimoto.txt] [--small]
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


def mixed_rows(rng, n, dim):
    """n packed rows with an eighth, a quarter, a half or three quarters of their bits set, a quarter of the rows each: random
    bytes ANDed or ORed with other random bytes"""
    x = random_bytes(rng, (n, dim))
    for lo in range(0, n, 1 << 20):
        part = x[lo:lo + (1 << 20)]
        kind = rng.integers(0, 4, (len(part), 1))
        other = random_bytes(rng, part.shape)
        np.bitwise_and(part, other, out=part, where=kind <= 1)          # a quarter of the bits
        np.bitwise_and(part, other[:, ::-1], out=part, where=kind == 0)  # an eighth
        np.bitwise_or(part, other, out=part, where=kind == 2)           # three quarters
    return x


def score_check(x, q, res):
    """the returned scores against numpy for the returned rows: c / u as f32, descending"""
    rows = x[res.indices.astype(np.int64)]
    c = np.unpackbits(rows & q[:, None, :], axis=2).sum(-1, dtype=np.int64)
    u = np.unpackbits(rows | q[:, None, :], axis=2).sum(-1, dtype=np.int64)
    t = c.astype(np.float32) / np.maximum(u, 1).astype(np.float32)
    return bool((t == res.scores).all() and (np.diff(res.scores, axis=1) <= 0).all())


def timed_shapes(say, n):
    rng = np.random.default_rng(0x7A41)
    st = torch.cuda.Stream()
    say(f"Tanimoto search against the Hamming search on the same handle, MI355X, {n / 1e6:g}M rows of mixed density, k = {K}; median "
        f"[min .. max] of {REPS} repetitions, the searches alternating after a warm-up of each")
    for dim in (128, 256, 512):
        x = mixed_rows(rng, n, dim)
        with G.GpuCorpus.from_array(x, device=0) as c:
            for nq in (1, 16, 128, 1024):
                q = mixed_rows(rng, nq, dim)
                dq = torch.from_numpy(q).cuda()
                out = [(torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda"))
                       for _ in range(2)]
                torch.cuda.synchronize()

                def stages():
                    return c.tanimoto_stage_ms(dq.data_ptr(), G.UINT8, dim, nq, K, out[0][0].data_ptr(), out[0][1].data_ptr(), st.cuda_stream)

                def call():
                    c.search_tanimoto_device(dq.data_ptr(), G.UINT8, dim, nq, K, out[0][0].data_ptr(), out[0][1].data_ptr(), st.cuda_stream)

                def hamming(route):
                    c.set_hamming_route(route)
                    return c.hamming_stage_ms(dq.data_ptr(), G.UINT8, dim, nq, K, out[1][0].data_ptr(), out[1][1].data_ptr(), st.cuda_stream)

                stages(), call(), hamming(1), hamming(2)
                t = {"stages": [], "call": [], 1: [], 2: []}
                for _ in range(REPS):
                    t["stages"].append(stages())
                    t["call"].append(event_ms(call, st))
                    for r in (1, 2):
                        t[r].append(hamming(r))
                c.set_hamming_route(0)
                sm, h = np.array(t["stages"]), {r: np.array(t[r]) for r in (1, 2)}
                a_ms = float(np.median(t["call"]))
                best = min((1, 2), key=lambda r: np.median(h[r].sum(1)))
                b_ms = float(np.median(h[best].sum(1)))
                f = G.tanimoto_form(dim, nq, K, n)
                say(f"{dim:4d} bytes nq {nq:4d} ({f.row_slices} slices, tile {f.query_tile}): (a) TQ {spread(sm[:, 0])} T2 {spread(sm[:, 1])} H1 "
                    f"{spread(sm[:, 2])} call {spread(t['call'])}")
                where = ""
                if a_ms > b_ms:
                    d = [float(np.median(sm[:, 0])), float(np.median(sm[:, 1]) - np.median(h[best][:, 0])), float(np.median(sm[:, 2]) - np.median(h[best][:, 1]))]
                    where = f"; of the difference: prepare {d[0]:+.3f} ms, scan {d[1]:+.3f} ms, merge {d[2]:+.3f} ms"
                say(f"{'':19s}(b) Hamming route 1 {spread(h[1].sum(1))}, route 2 {spread(h[2].sum(1))}: the better is route {best}, "
                    f"(a) / (b) {a_ms / b_ms:5.2f}x{where}")
                if dim == 128 and nq == 16:
                    ok = score_check(x, q, c.search_tanimoto(q, K))
                    say(f"{'':19s}the returned scores equal numpy's c / u for the returned rows and descend: {'yes' if ok else 'NO'}")
        del x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal: 200k rows")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:  # as it goes: a run that is cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    timed_shapes(say, 200_000 if a.small else 10_000_000)


if __name__ == "__main__":
    main()
