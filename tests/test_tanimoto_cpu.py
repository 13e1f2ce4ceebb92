"""Tanimoto search, CPU tier (include/mvf_gpu_tanimoto.h; DESIGN.md §3 "Tanimoto search"): the header's functions against the
library, the refusals that need no device in their order, the form function's properties, and the order key's argument."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT


def test_gpu_library_exports_the_header_s_symbols():
    text = open(os.path.join(ROOT, "include", "mvf_gpu_tanimoto.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mvfgpu_\w+)\s*\(", text, re.M))
    assert declared == {"mvfgpu_search_tanimoto", "mvfgpu_search_tanimoto_device", "mvfgpu_selftest_tanimoto_form",
                        "mvfgpu_selftest_tanimoto_stage_ms"}
    for name in declared:
        assert hasattr(_lib.gpu(), name), f"libmvf_gpu.so does not export {name}"
    assert '#include "mvf_gpu.h"' in text and "mvfgpu_search_tanimoto" not in open(os.path.join(ROOT, "include", "mvf_gpu.h")).read()
    for name in ("find_top_k_tanimoto", "tanimoto_form"):
        assert callable(getattr(M, name)) and name in M.__all__


def _call(fn, q=True, nq=1, k=2, sc=True, idx=True, ms=True):
    buf = np.zeros(64, np.uint8)
    p = lambda on: buf.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    args = [None, p(q), G.UINT8, 32, nq, k, p(sc), p(idx)]
    if fn == "host":
        rc = lib.mvfgpu_search_tanimoto(*args)
    elif fn == "device":
        rc = lib.mvfgpu_search_tanimoto_device(*args, None)
    else:
        rc = lib.mvfgpu_selftest_tanimoto_stage_ms(*args, None, p(ms))
    return rc, lib.mvfgpu_last_error_message().decode()


@pytest.mark.parametrize("fn", ["host", "device", "timer"])
def test_refusals_precede_any_device_call(fn):
    """mvfgpu_search's handle-free checks with its messages, then k above one pass, then the handle (what a handle is refused
    for needs one: tests/test_gpu_tanimoto.py)"""
    assert _call(fn, nq=0) == (INV, "nq must be > 0")
    for k in (0, 2**31 + 1):
        assert _call(fn, k=k) == (INV, "k must be in 1..2^31")
    for kw in (dict(q=False), dict(sc=False), dict(idx=False)):
        assert _call(fn, **kw) == (INV, "NULL buffer"), kw
    rc, msg = _call(fn, k=1025)
    assert rc == INV and "k above 1024 is not built for Tanimoto search" in msg
    assert _call(fn, k=1024) == (INV, "corpus is NULL")
    if fn == "timer":
        assert _call(fn, ms=False) == (INV, "NULL buffer")


def test_form_properties():
    for dim, nq, k, rows in ((0, 1, 1, 1), (513, 1, 1, 1), (16, 0, 1, 1), (16, 1, 0, 1), (16, 1, 1025, 1), (16, 1, 1, 2**32)):
        assert _lib.gpu().mvfgpu_selftest_tanimoto_form(dim, nq, k, rows, 0, None, None, None, None, None, None) == INV, (dim, nq, k, rows)
    for dim in (1, 16, 64, 128, 256, 257, 512):
        for nq in (1, 16, 17, 128, 1024):
            for k in (1, 100, 1024):
                for rows in (0, 1, 1100, 3001, 10**7, 2**32 - 65536):
                    for cus in (0, 64, 256):
                        f = G.tanimoto_form(dim, nq, k, rows, cus)
                        where = (dim, nq, k, rows, cus, f)
                        kcap = 1 << (k - 1).bit_length()
                        tiles = -(-nq // f.query_tile)
                        # the smallest of 16 .. 128 that holds the window's queries, capped by the prepared tile's LDS
                        assert f.query_tile == min(128 if dim <= 256 else 64, max(16, 1 << (nq - 1).bit_length())), where
                        assert f.chunks == -(-dim // 64) and f.lds_bytes <= 160 * 1024, where
                        assert f.lds_bytes >= f.query_tile * 4 * 64 * f.chunks + 8 * max(2 * kcap, 512), where
                        assert f.row_slices * kcap <= 65536, where
                        # a slice holds 1024 rows at least: no more slices than whole or started runs of 1024 rows
                        assert (f.row_slices == 0) == (rows == 0) and f.row_slices <= -(-rows // 1024), where
                        assert f.row_slices * f.slice_rows >= rows > (f.row_slices - 1) * f.slice_rows or rows == 0, where
                        assert f.scratch_bytes == f.row_slices * tiles * f.query_tile * max(2 * kcap, 512) * 8 <= 512 << 20, where
    assert G.tanimoto_form(128, 5000, 100, 10**7).query_tile == 128       # a window holds 1024 queries
    assert G.tanimoto_form(128, 1, 100, 10**7, 256).row_slices == 512     # two blocks per CU where their LDS fits
    assert G.tanimoto_form(512, 1024, 100, 10**7, 256).row_slices == 16   # one where it does not: 16 tiles x 16 slices


def test_the_f32_quotient_orders_as_the_rationals():
    """include/mvf_gpu_tanimoto.h, "The score and the order key": over the (c, u) a 512-byte row can give, dense near 1/3, 1/2
    and 1 where the floats are coarsest against the fractions' gaps, np.float32(c) / np.float32(u) sorts as Fraction(c, u) does
    and equal fractions have equal bits; 0x3F800000 - bits is then an ascending u32 key"""
    pairs = [(c, u) for u in list(range(1, 65)) + list(range(3900, 4097))
             for near in (u // 3, u // 2, u) for c in range(max(0, near - 8), min(u, near + 8) + 1)]
    pairs = sorted(set(pairs), key=lambda p: Fraction(*p))
    c, u = np.array(pairs, np.float32).T
    t = c / u
    assert t.dtype == np.float32 and len(pairs) > 10000
    exact = [Fraction(*p) for p in pairs]
    rises = np.array([a < b for a, b in zip(exact, exact[1:])])
    assert ((t[1:] > t[:-1]) == rises).all() and ((t[1:] == t[:-1]) == ~rises).all()
    key = np.uint32(0x3F800000) - t.view(np.uint32)
    assert (key[1:] <= key[:-1]).all() and ((key[1:] == key[:-1]) == ~rises).all() and key.min() == 0
