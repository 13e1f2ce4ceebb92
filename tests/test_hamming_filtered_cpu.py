"""Filtered Hamming search, CPU tier (include/mvf_gpu_hamming_filtered.h; DESIGN.md §3 "Filtered Hamming search", §5 "HG"): the
header's functions against the library, the refusals that need no device in their order, and the properties of the route rule
and of the list route's form."""
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
NAMES = {"mvfgpu_search_hamming_filtered", "mvfgpu_search_hamming_filtered_device", "mvfgpu_selftest_hamming_filtered_form",
         "mvfgpu_selftest_hamming_filtered_stage_ms"}


def test_gpu_library_exports_the_header_s_symbols():
    text = open(os.path.join(ROOT, "include", "mvf_gpu_hamming_filtered.h")).read()
    assert set(re.findall(r"^\s*int\s+(mvfgpu_\w+)\s*\(", text, re.M)) == NAMES
    for name in NAMES:
        assert hasattr(_lib.gpu(), name), f"libmvf_gpu.so does not export {name}"
    assert '#include "mvf_gpu.h"' in text
    for name in ("find_top_k_hamming_filtered", "hamming_filtered_form", "HammingFilteredForm"):
        assert name in M.__all__ and hasattr(M, name)


def _call(fn, flt=True, q=True, nq=1, k=2, sc=True, idx=True, ms=True):
    buf = np.zeros(64, np.uint8)
    p = lambda on: buf.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    args = [None, p(flt), p(q), G.UINT8, 4, nq, k, p(sc), p(idx), None]  # (a filter that is not NULL is never read before the handle)
    if fn == "host":
        rc = lib.mvfgpu_search_hamming_filtered(*args)
    elif fn == "device":
        rc = lib.mvfgpu_search_hamming_filtered_device(*args, None)
    else:
        rc = lib.mvfgpu_selftest_hamming_filtered_stage_ms(*args, None, p(ms))
    return rc, lib.mvfgpu_last_error_message().decode()


@pytest.mark.parametrize("fn", ["host", "device", "timer"])
def test_refusals_precede_any_device_call_in_their_order(fn):
    """the handle-free checks with the Hamming search's messages, then k above one pass, then the filter, then the handle"""
    assert _call(fn, nq=0, flt=False) == (INV, "nq must be > 0")
    for k in (0, 2**31 + 1):
        assert _call(fn, k=k, flt=False) == (INV, "k must be in 1..2^31")
    for kw in (dict(q=False), dict(sc=False), dict(idx=False)):
        assert _call(fn, flt=False, **kw) == (INV, "NULL buffer"), kw
    rc, msg = _call(fn, k=1025, flt=False)
    assert rc == INV and "k above 1024 is not built for filtered Hamming search" in msg
    assert _call(fn, k=1024, flt=False) == (INV, "filter is NULL")
    assert _call(fn, k=1024) == (INV, "corpus is NULL")
    if fn == "timer":
        assert _call(fn, ms=False) == (INV, "NULL buffer")


def test_form_selftest_refusals():
    for dim, nq, k, rows, adm, has, forced in ((0, 1, 1, 1, 1, 1, 0), (33026, 1, 1, 1, 1, 1, 0), (16, 0, 1, 1, 1, 1, 0), (16, 1, 0, 1, 1, 1, 0),
                                               (16, 1, 1025, 1, 1, 1, 0), (16, 1, 1, 2**32, 1, 1, 0), (16, 1, 1, 5, 6, 1, 0),
                                               (16, 1, 1, 5, 5, 2, 0), (16, 1, 1, 5, 5, 1, 3), (16, 1, 1, 5, 5, 1, -1)):
        rc = _lib.gpu().mvfgpu_selftest_hamming_filtered_form(dim, nq, k, rows, adm, has, forced, 0, *[None] * 7)
        assert rc == INV, (dim, nq, k, rows, adm, has, forced)


DIMS = [1, 16, 17, 64, 65, 256, 257, 272, 512, 513, 4096, 33025]


def test_route_and_form_properties():
    rows = 10**7
    for dim in DIMS:
        pitch = (dim + 15) // 16 * 16
        for nq in (1, 16, 17, 33, 64, 65, 130, 1024, 5000):
            for k in (1, 100, 1024):
                for adm in (0, 1, 1023, 1024, 1025, 3001, 10**5, rows):
                    for forced in (0, 1, 2):
                        for cus in (0, 64, 256):
                            f = G.hamming_filtered_form(dim, nq, k, rows, adm, True, forced, cus)
                            where = (dim, nq, k, adm, forced, cus, f)
                            if pitch > 512 or adm == 0 or forced == 1:
                                assert f == (1, 0, 0, 0, 0, 0, 0), where
                                continue
                            assert G.hamming_filtered_form(dim, nq, k, rows, adm, False, forced, cus).route == 1, where  # no list
                            if forced == 2:
                                assert f.route == 2, where
                            if f.route == 1:
                                continue
                            wn = min(nq, 1024)
                            cap = 128 if pitch <= 256 else 64
                            assert f.query_tile == min(cap, max(16, 1 << (wn - 1).bit_length())), where
                            assert f.chunks == (pitch + 63) // 64, where
                            assert f.slice_entries >= 1024 and f.slice_entries % 256 == 0, where
                            assert f.list_slices * f.slice_entries >= adm > (f.list_slices - 1) * f.slice_entries, where
                            assert f.list_slices * (1 << (k - 1).bit_length()) <= 65536, where
                            assert f.lds_bytes <= 160 * 1024 and f.scratch_bytes <= 512 << 20, where
    assert G.hamming_filtered_form(128, 1, 100, rows, 2**20, True, 2, 256).list_slices == 256  # one slice per CU
    assert G.hamming_filtered_form(128, 1024, 100, rows, 2**20, True, 2, 256).list_slices == 32  # ... over the 8 query tiles


def test_the_automatic_rule_takes_the_list_only_where_it_was_measured_ahead():
    """profiles/r30_hamming_filtered.txt: 10M rows of 64 to 512 bytes, k = 100, every batch size, up to rows / 10 admitted; the
    mask outside each edge of that region"""
    rows = 10**7
    for dim in (49, 64, 128, 512):
        for nq in (1, 16, 128, 1024):
            assert [G.hamming_filtered_form(dim, nq, 100, rows, adm).route for adm in (1, 10**3, 10**6, 10**6 + 1, rows // 2, rows)] == \
                [2, 2, 2, 1, 1, 1], (dim, nq)
            assert [G.hamming_filtered_form(dim, nq, k, rows, 10**3).route for k in (1, 128, 129, 1024)] == [2, 2, 1, 1], (dim, nq)
            assert [G.hamming_filtered_form(dim, nq, 100, n, 10**3).route for n in (3001, 10**7 - 1, 10**7, 2**31)] == [1, 1, 2, 2], (dim, nq)
    assert {G.hamming_filtered_form(dim, 1, 100, rows, 10**3).route for dim in (1, 16, 48)} == {1}  # a pitch below 64 bytes
