"""What the MFMA selection route's tests share (tests/test_maxsim_mfma_cpu.py, tests/test_gpu_maxsim_mfma.py), and -- run as a
program, `python tests/_maxsim_mfma.py <out.npz>` -- the scenario the GPU tests start as a child process: tests/_maxsim.py's
fresh-process inputs, host call and device call, on a handle that took its route from the environment (MVF_MAXSIM_ROUTE).
Imports numpy and the standard library only; as a child it keeps the binding from loading torch."""
import ctypes as C
import os
import sys

import numpy as np

import _maxsim as MS
import _partitioned as P

# The stream class of every function include/mvf_gpu_maxsim_route.h declares, in tests/_streams.py's words (its ENTRY_CLASS lists
# include/mvf_gpu.h's functions), and the device form the measurement aid among them times.
ENTRY_CLASS = {
    "mvfgpu_set_maxsim_route": "no device work",
    "mvfgpu_selftest_maxsim_route": "takes no handle",
    "mvfgpu_selftest_maxsim_margin": "takes no handle",
    "mvfgpu_selftest_maxsim_mfma_stage_ms": "runs under corpus_device_call",
}
TIMED_FORM_OF = {"mvfgpu_selftest_maxsim_mfma_stage_ms": "mvfgpu_search_maxsim_device"}

WORLD_B_SIZES, WORLD_B_FURTHER = (300, 129, 128, 127, 64, 2, 1), 1000


def world_b():
    """8192 rows, 1007 keys: the form layout's sized keys and 1000 further keys of six or seven rows each"""
    return P.layout("u32", P.N, WORLD_B_SIZES, WORLD_B_FURTHER)


def main(argv):
    if len(argv) != 2:
        print("usage: _maxsim_mfma.py <out.npz>", file=sys.stderr)
        return 2
    sys.modules.setdefault("torch", None)  # the binding would load torch's HIP runtime first where torch is installed
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from metrovector_amd import gpu as G
    inp = MS.fresh_inputs()
    lay, q = inp["lay"], inp["queries"]
    nq, T, k, metric, dim = MS.FP_NQ, MS.FP_T, MS.FP_K, MS.FP_METRIC, MS.FP_DIM
    out = {}
    with G.GpuCorpus.from_array(inp["rows"]) as c:
        c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        with c.attach_column(lay["col"]) as col, c.make_partition(col) as part:
            res = c.search_maxsim(q, k, metric, part)   # the child's first search
            out["host.scores"], out["host.keys"], out["host.counts"] = res.scores, res.keys, res.counts
            hip = P._hip_runtime()
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipFree.argtypes = [C.c_void_p]
            sizes = [q.nbytes, nq * k * 4, nq * k * 8, nq * 4]
            ptrs = [C.c_void_p() for _ in sizes]
            for p, size in zip(ptrs, sizes):
                P._check(hip.hipMalloc(C.byref(p), size), "hipMalloc")
            P._check(hip.hipMemcpy(ptrs[0], q.ctypes.data_as(C.c_void_p), q.nbytes, 1), "hipMemcpy H2D")
            c.search_maxsim_device(part, ptrs[0].value, 0, dim, nq, T, k, metric, ptrs[1].value, ptrs[2].value, ptrs[3].value)
            P._check(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
            got = [np.empty((nq, k), np.float32), np.empty((nq, k), np.uint64), np.empty(nq, np.uint32)]
            for a, p in zip(got, ptrs[1:]):
                P._check(hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2), "hipMemcpy D2H")
            # the route the handle read from the environment really selects: the stage timer of the same search counts candidates
            _, cand, blocks = c.maxsim_mfma_stage_ms(part, ptrs[0].value, 0, dim, nq, T, k, metric, ptrs[1].value, ptrs[2].value)
            out["candidates"], out["blocks"] = cand, blocks
            for p in ptrs:
                P._check(hip.hipFree(p), "hipFree")
            out["device.scores"], out["device.keys"], out["device.counts"] = got
    out["poison"] = np.array([G.selftest_poison()], np.int32)
    out["route"] = np.array([int(os.environ.get("MVF_MAXSIM_ROUTE", "0"))], np.int32)
    np.savez(argv[1], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
