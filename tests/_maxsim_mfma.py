"""What the MFMA selection route's tests share (tests/test_maxsim_mfma_cpu.py, tests/test_gpu_maxsim_mfma.py,
tests/test_gpu_maxsim_mfma_bound.py) -- the stream classes of the route's header, world B, the yardsticks the selection's
read-out is held to (P0's rule and a float64 recomputation of the sums, in numpy) and the planted world --, and -- run as a
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
# include/mvf_gpu.h's functions), and the device form each measurement aid among them runs.
ENTRY_CLASS = {
    "mvfgpu_set_maxsim_route": "no device work",
    "mvfgpu_selftest_maxsim_route": "takes no handle",
    "mvfgpu_selftest_maxsim_margin": "takes no handle",
    "mvfgpu_selftest_maxsim_mfma_stage_ms": "runs under corpus_device_call",
    "mvfgpu_selftest_maxsim_mfma_selection": "runs under corpus_device_call",
}
TIMED_FORM_OF = {"mvfgpu_selftest_maxsim_mfma_stage_ms": "mvfgpu_search_maxsim_device",
                 "mvfgpu_selftest_maxsim_mfma_selection": "mvfgpu_search_maxsim_device"}

WORLD_B_SIZES, WORLD_B_FURTHER = (300, 129, 128, 127, 64, 2, 1), 1000


def world_b():
    """8192 rows, 1007 keys: the form layout's sized keys and 1000 further keys of six or seven rows each"""
    return P.layout("u32", P.N, WORLD_B_SIZES, WORLD_B_FURTHER)


# ---- the yardsticks of the selection's read-out (tests/test_gpu_maxsim_mfma_bound.py; tests/test_maxsim_mfma_cpu.py tests them)
TOO_LARGE, TOO_SMALL = 1e37, 1e-30   # the premises of the bound: scan_maxsim_mfma.hip's kMfmaTooLarge / kMfmaTooSmall


def p0_rule(sums, forced, delta, theta, theta_nan):
    """P0's rule restated from the read-out alone -> bool [nq, n_keys].  sums f32 [nq, n_keys], forced bool [nq, n_keys], delta
    f64 [nq], theta f32 [nq], theta_nan bool [nq].  All double arithmetic on exactly representable inputs: 2 Delta is exact, the
    two subtractions round once each here as on the device (|thr| 2^-52 is exact, so a fused form rounds alike)."""
    with np.errstate(all="ignore"):
        thr = np.asarray(theta, np.float32).astype(np.float64) - 2.0 * np.asarray(delta, np.float64)
        thr = thr - np.abs(thr) * 2.0 ** -52
        every = np.asarray(theta_nan, bool) | ~np.isfinite(theta) | ~(np.asarray(delta, np.float64) < 1e300)
        return np.asarray(forced, bool) | ~np.isfinite(sums) | every[:, None] | (np.asarray(sums, np.float32).astype(np.float64) >= thr[:, None])


def theta_of(sums, forced, kk):
    """(theta f32 [nq], is the live NaN entry bool [nq]): the kk-th largest sum among the keys that are not forced and whose sum
    is finite -- equal sums rank by ordinal, which does not change the value --; fewer than kk such keys: the NaN entry"""
    theta, nan = np.full(len(sums), np.nan, np.float32), np.ones(len(sums), bool)
    for q, (S, f) in enumerate(zip(sums, forced)):
        v = np.sort(S[~f & np.isfinite(S)])[::-1]
        if v.size >= kk:
            theta[q], nan[q] = v[kk - 1], False
    return theta, nan


def f64_sums(x, starts, sets, metric):
    """The float64 recomputation of every key's sum, independent of every kernel.  x [live, dim]: the stored live rows in the
    index's order (f16 rows widen exactly), starts: the first position of every key, sets f32 [nq, T, dim].
    -> dict: best f64 [nq, T, n_keys]: per token the maximum over the key's rows (key_sums adds them up); bad bool [nq, T, n_keys]:
    a premise of the bound fails for the token and some row of the key -- a dot product that is not finite or reaches 1e37, under
    Cosine a denominator of the f32 norms (both non-zero) outside [1e-30, 1e37) --; dot_max, den_min, den_max: the extremes the
    finite worlds are held away from the premises' edges by.
    Cosine: float64 norms and K1's rule -- a zero norm gives score 0 --, a norm being zero where it is zero in f32 (a sum of
    squares below 2^-150 has no f32 value but 0)."""
    nq, T, dim = sets.shape
    x64, q64 = x.astype(np.float64), sets.reshape(nq * T, dim).astype(np.float64)
    with np.errstate(all="ignore"):
        dot = q64 @ x64.T
        bad = ~(np.abs(dot) < TOO_LARGE)
        out = {"dot_max": float(np.nanmax(np.abs(dot))), "den_min": np.inf, "den_max": 0.0}
        sc = dot
        if metric == 2:
            qq, xx = (q64 * q64).sum(1), (x64 * x64).sum(1)
            qn32, xn32 = np.sqrt(qq.astype(np.float32)).astype(np.float64), np.sqrt(xx.astype(np.float32)).astype(np.float64)
            both = (qn32[:, None] != 0) & (xn32[None, :] != 0)
            den32 = qn32[:, None] * xn32[None, :]
            bad |= both & ~((den32 >= TOO_SMALL) & (den32 < TOO_LARGE))
            sc = np.where(both, dot / (np.sqrt(qq)[:, None] * np.sqrt(xx)[None, :]), 0.0)
            if both.any():
                out["den_min"], out["den_max"] = float(np.nanmin(den32[both])), float(np.nanmax(den32[both]))
        out["best"] = np.maximum.reduceat(sc, starts, axis=1).reshape(nq, T, -1)
        out["bad"] = np.logical_or.reduceat(bad, starts, axis=1).reshape(nq, T, -1)
    return out


def key_sums(ref, nq, T):
    """(S f64 [nq, n_keys], fails bool [nq, n_keys]) of the leading nq sets and T tokens of f64_sums' result"""
    with np.errstate(all="ignore"):
        return ref["best"][:nq, :T].sum(1), ref["bad"][:nq, :T].any(1)


def planted_world(dt, dim):
    """(rows, layout, ordinal of the key whose only special row is tombstoned, ordinal of the all-zero key): the world of
    test_non_finite_huge_and_zero_values -- NaN, +-Inf, 1e30 (Float16 rows: 60000) and zero rows planted in keys of every size,
    a key of zero rows only, a key of NaN rows only --, and a NaN row planted on a tombstone of a key the rest leaves alone"""
    lay = MS.form_layout(2048)
    live, keys, starts, values = MS.key_order(lay)
    rows = P.make_rows(2048, dim, dt)
    big = 60000.0 if dt == "f16" else 1e30
    rng = np.random.default_rng(P._seed("mfma edges", dt, dim))
    at = rng.choice(live, 40, replace=False)
    for i, r in enumerate(at):
        kind = i % 8
        if kind == 0:
            rows[r, i % dim] = np.nan
        elif kind == 1:
            rows[r, i % dim] = np.inf
        elif kind == 2:
            rows[r, i % dim] = -np.inf
        elif kind == 3:
            rows[r, 0], rows[r, dim - 1] = np.inf, -np.inf
        elif kind == 4:
            rows[r] = big
        elif kind == 5:
            rows[r, i % dim] = -big
        else:
            rows[r] = 0
    small = np.nonzero((np.concatenate([starts[1:], [keys.size]]) - starts) <= 3)[0]
    rows[live[starts[small[0]]:starts[small[0] + 1]]] = 0
    rows[live[starts[small[1]]:starts[small[1] + 1]]] = np.nan
    touched = set(lay["col"][at].tolist()) | {int(values[small[0]]), int(values[small[1]])}
    dead = np.nonzero(lay["dead"])[0]
    mine = [r for r in dead if int(lay["col"][r]) not in touched and int(lay["col"][r]) in set(values.tolist())]
    assert mine, "a tombstoned row of a key that holds live rows and no planted one"
    rows[mine[0]] = np.nan
    return rows, lay, int(np.searchsorted(values, lay["col"][mine[0]])), int(small[0])


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
