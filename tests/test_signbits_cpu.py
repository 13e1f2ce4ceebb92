"""Sign-bit search, CPU tier (include/mvf_gpu_signbits.h; DESIGN.md §3 "Sign-bit search"): the header's functions against the
library, the refusals that need no device in their order, the form function's properties, and quantize_queries_int8."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT


def test_gpu_library_exports_the_header_s_symbols():
    text = open(os.path.join(ROOT, "include", "mvf_gpu_signbits.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mvfgpu_\w+)\s*\(", text, re.M))
    assert declared == {"mvfgpu_search_signbits", "mvfgpu_search_signbits_device", "mvfgpu_selftest_signbits_form",
                        "mvfgpu_selftest_signbits_stage_ms"}
    for name in declared:
        assert hasattr(_lib.gpu(), name), f"libmvf_gpu.so does not export {name}"
    assert '#include "mvf_gpu.h"' in text and "mvfgpu_search_signbits" not in open(os.path.join(ROOT, "include", "mvf_gpu.h")).read()
    for name in ("find_top_k_signbits", "signbits_form", "quantize_queries_int8"):
        assert callable(getattr(M, name)) and name in M.__all__


def _call(fn, q=True, nq=1, k=2, sc=True, idx=True, ms=True):
    buf = np.zeros(64, np.uint8)
    p = lambda on: buf.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    args = [None, p(q), G.INT8, 32, nq, k, p(sc), p(idx), None]
    if fn == "host":
        rc = lib.mvfgpu_search_signbits(*args)
    elif fn == "device":
        rc = lib.mvfgpu_search_signbits_device(*args, None)
    else:
        rc = lib.mvfgpu_selftest_signbits_stage_ms(*args, None, p(ms))
    return rc, lib.mvfgpu_last_error_message().decode()


@pytest.mark.parametrize("fn", ["host", "device", "timer"])
def test_refusals_precede_any_device_call(fn):
    """mvfgpu_search's handle-free checks with its messages, then k above one pass, then the handle (what a handle is refused
    for needs one: tests/test_gpu_signbits.py)"""
    assert _call(fn, nq=0) == (INV, "nq must be > 0")
    for k in (0, 2**31 + 1):
        assert _call(fn, k=k) == (INV, "k must be in 1..2^31")
    for kw in (dict(q=False), dict(sc=False), dict(idx=False)):
        assert _call(fn, **kw) == (INV, "NULL buffer"), kw
    rc, msg = _call(fn, k=1025)
    assert rc == INV and "k above 1024 is not built for sign-bit search" in msg
    assert _call(fn, k=1024) == (INV, "corpus is NULL")
    if fn == "timer":
        assert _call(fn, ms=False) == (INV, "NULL buffer")


def test_form_properties():
    for dim, nq, k, rows in ((0, 1, 1, 1), (513, 1, 1, 1), (16, 0, 1, 1), (16, 1, 0, 1), (16, 1, 1025, 1), (16, 1, 1, 2**32)):
        assert _lib.gpu().mvfgpu_selftest_signbits_form(dim, nq, k, rows, 0, None, None, None, None, None) == INV, (dim, nq, k, rows)
    for dim in (1, 16, 17, 64, 65, 128, 129, 256, 257, 500, 512):
        cap = 128 if dim <= 128 else 64 if dim <= 256 else 32
        for nq in (1, 16, 17, 33, 64, 65, 128, 129, 1024, 5000):
            for k in (1, 10, 100, 257, 1024):
                for rows in (0, 1, 1100, 3001, 10**5, 10**7, 2**32 - 65536):
                    for cus in (0, 64, 256):
                        f = G.signbits_form(dim, nq, k, rows, cus)
                        where = (dim, nq, k, rows, cus, f)
                        kcap = 1 << (k - 1).bit_length()
                        tiles = -(-min(nq, 1024) // f.query_tile)
                        # the smallest of 16 .. 128 that holds the window's queries, capped by the prepared tile's LDS
                        assert f.query_tile == min(cap, max(16, 1 << (min(nq, 1024) - 1).bit_length())), where
                        assert f.chunks == -(-dim // 64) and f.lds_bytes <= 160 * 1024, where
                        assert f.lds_bytes >= f.query_tile * 8 * 64 * f.chunks + 8 * max(2 * kcap, 512), where
                        assert f.row_slices * kcap <= 65536, where
                        # a slice holds 1024 rows at least: no more slices than whole or started runs of 1024 rows
                        assert (f.row_slices == 0) == (rows == 0) and f.row_slices <= -(-rows // 1024), where
                        assert f.scratch_bytes == f.row_slices * tiles * f.query_tile * max(2 * kcap, 512) * 8 <= 512 << 20, where
    assert G.signbits_form(128, 1, 100, 10**7, 256).row_slices == 512   # two blocks per CU where their LDS fits
    assert G.signbits_form(128, 1024, 100, 10**7, 256).row_slices == 32  # one where it does not: 8 tiles x 32 slices


def test_quantize_queries_int8():
    q = G.quantize_queries_int8(np.array([[0.5, -1.0, 0.0, 0.25, 0.996, -0.004, 0.0117, 1.0, -1.0, 0.5]], np.float32))
    assert q.dtype == np.int8 and q.tolist() == [[64, -127, 0, 32, 126, -1, 1, 127, -127, 64, 0, 0, 0, 0, 0, 0]]  # rint(63.5) = 64
    assert G.quantize_queries_int8(np.array([3.0, -6.0])).tolist() == [64, -127, 0, 0, 0, 0, 0, 0]                # its own scale
    assert G.quantize_queries_int8(np.zeros((2, 8))).tolist() == [[0] * 8] * 2                                     # stays zero
    two = G.quantize_queries_int8(np.array([[1e-3] * 8, [-5e4] * 8]))
    assert two.tolist() == [[127] * 8, [-127] * 8] and M.quantize_queries_int8 is G.quantize_queries_int8
