"""What the tests of the Hamming search share (include/mvf_gpu_hamming.h; DESIGN.md §3 "Hamming search"): the stream classes
of the header's functions and the numpy reference every GPU answer is compared with, byte for byte."""
import numpy as np

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)

# The stream class of every function include/mvf_gpu_hamming.h declares, in tests/_streams.py's words (its ENTRY_CLASS lists
# include/mvf_gpu.h's functions), and the device form the measurement aid among them runs.
ENTRY_CLASS = {
    "mvfgpu_search_hamming": "runs under corpus_device_call",
    "mvfgpu_search_hamming_device": "runs under corpus_device_call",
    "mvfgpu_selftest_hamming_form": "takes no handle",
    "mvfgpu_selftest_hamming_stage_ms": "runs under corpus_device_call",
}
TIMED_FORM_OF = {"mvfgpu_selftest_hamming_stage_ms": "mvfgpu_search_hamming_device"}


def distances(queries, rows):
    """d[q, r] = the bits in which uint8 queries [nq, dim] and rows [n, dim] differ"""
    return np.unpackbits(queries[:, None, :] ^ rows[None, :, :], axis=-1).sum(-1, dtype=np.int64)


def reference(queries, rows, k, dead=None, ids=None, index_base=0):
    """(scores f32, indices u64, raw i32) [nq, k] of the contract: the k live rows of smallest distance, ties by ascending
    position, an L2 search's padding behind them.  Queries are taken a few at a time to bound the unpacked bits."""
    nq, n = queries.shape[0], rows.shape[0]
    live = np.arange(n) if dead is None else np.nonzero(~dead)[0]
    name = (np.arange(n, dtype=np.uint64) + np.uint64(index_base)) if ids is None else ids
    sc = np.full((nq, k), np.inf, np.float32)
    idx = np.full((nq, k), PAD, np.uint64)
    raw = np.zeros((nq, k), np.int32)
    take = min(k, live.size)
    step = max(1, (1 << 27) // max(1, live.size * rows.shape[1] * 8))
    for q0 in range(0, nq, step):
        d = distances(queries[q0:q0 + step], rows[live])
        order = np.argsort(d, axis=1, kind="stable")[:, :take]  # stable: equal distances stay in position order
        best = np.take_along_axis(d, order, axis=1)
        raw[q0:q0 + step, :take] = best
        sc[q0:q0 + step, :take] = best.astype(np.float32)
        idx[q0:q0 + step, :take] = name[live[order]]
    return sc, idx, raw


def same(res, want):
    """a SearchResult equals the reference's (scores, indices, raw) in every byte"""
    return (res.indices.tobytes() == want[1].tobytes() and res.raw.tobytes() == want[2].tobytes()
            and res.scores.tobytes() == want[0].tobytes())
