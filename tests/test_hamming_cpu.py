"""Hamming search, CPU tier (include/mvf_gpu_hamming.h; DESIGN.md §3 "Hamming search"): the header's functions against the
library and the entry classes, the refusals that need no device, the form function's properties, the numpy reference pinned by
a bit-by-bit loop, and pack_sign_bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import gpu as G

import _hamming as H
import _streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT


def test_gpu_library_exports_the_hamming_header_s_symbols():
    text = open(os.path.join(ROOT, "include", "mvf_gpu_hamming.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mvfgpu_\w+)\s*\(", text, re.M))
    assert declared == set(H.ENTRY_CLASS), declared ^ set(H.ENTRY_CLASS)
    assert set(H.ENTRY_CLASS.values()) <= {S.NO_HANDLE, S.DEVICE_CALL}
    assert not declared & set(S.ENTRY_CLASS), "include/mvf_gpu.h declares none of them"
    for aid, form in H.TIMED_FORM_OF.items():
        assert H.ENTRY_CLASS[aid] == H.ENTRY_CLASS[form] == S.DEVICE_CALL
    for name in declared:
        assert hasattr(_lib.gpu(), name), f"libmvf_gpu.so does not export {name}"
    assert '#include "mvf_gpu.h"' in text
    assert callable(M.find_top_k_hamming) and "find_top_k_hamming" in M.__all__


def _call(fn, corpus=None, q=True, nq=1, k=2, sc=True, idx=True, ms=True):
    buf = np.zeros(64, np.uint8)
    p = lambda on: buf.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    args = [corpus, p(q), G.UINT8, 4, nq, k, p(sc), p(idx), None]
    if fn == "host":
        rc = lib.mvfgpu_search_hamming(*args)
    elif fn == "device":
        rc = lib.mvfgpu_search_hamming_device(*args, None)
    else:
        rc = lib.mvfgpu_selftest_hamming_stage_ms(*args, None, p(ms))
    return rc, lib.mvfgpu_last_error_message().decode()


@pytest.mark.parametrize("fn", ["host", "device", "timer"])
def test_refusals_precede_any_device_call(fn):
    """mvfgpu_search's handle-free checks with its messages, then k above one pass, then the handle"""
    assert _call(fn, nq=0) == (INV, "nq must be > 0")
    for k in (0, 2**31 + 1):
        assert _call(fn, k=k) == (INV, "k must be in 1..2^31")
    for kw in (dict(q=False), dict(sc=False), dict(idx=False)):
        assert _call(fn, **kw) == (INV, "NULL buffer"), kw
    rc, msg = _call(fn, k=1025)
    assert rc == INV and "k above 1024 is not built for Hamming search" in msg
    assert _call(fn, k=1024) == (INV, "corpus is NULL")
    if fn == "timer":
        assert _call(fn, ms=False) == (INV, "NULL buffer")


def test_form_selftest_refusals():
    for dim, nq, k, rows in ((0, 1, 1, 1), (33026, 1, 1, 1), (16, 0, 1, 1), (16, 1, 0, 1), (16, 1, 1025, 1), (16, 1, 1, 2**32)):
        rc = _lib.gpu().mvfgpu_selftest_hamming_form(dim, nq, k, rows, 0, None, None, None, None, None, None)
        assert rc == INV, (dim, nq, k, rows)


DIMS = [1, 15, 16, 17, 48, 100, 128, 255, 256, 257, 272, 512, 513, 1000, 4096, 33025]


def test_form_properties():
    forms = []
    for dim in DIMS:
        pitch = (dim + 15) // 16 * 16
        for nq in (1, 2, 5, 16, 70, 1024, 5000):
            for k in (1, 10, 100, 256, 257, 1000, 1024):
                for rows in (0, 1, 1000, 3001, 10**5, 10**7, 2**32 - 65536):
                    for cus in (0, 64, 256):
                        f = G.hamming_form(dim, nq, k, rows, cus)
                        where = (dim, nq, k, rows, cus, f)
                        kcap = 1 << (k - 1).bit_length()
                        assert f.form in (0, 1) and f.lanes_per_row in (1, 2, 4, 8, 16, 32, 64), where
                        if f.form == 0:
                            assert pitch <= f.lanes_per_row * 16 < 2 * pitch, where  # the group covers the pitch, no wider than needed
                        assert f.lds_bytes <= 160 * 1024, where
                        assert f.query_tile >= 1 and f.query_tile & (f.query_tile - 1) == 0 and f.query_tile <= max(1, 1 << (min(nq, 1024) - 1).bit_length()), where
                        assert f.row_slices * kcap <= f.merge_entries, where
                        assert (f.row_slices == 0) == (rows == 0) and f.row_slices <= max(rows, 1), where
                        assert f == G.hamming_form(dim, nq, k, rows, cus)
        forms.append(G.hamming_form(dim, 16, 10, 10**5).form)
        assert {G.hamming_form(dim, nq, k, rows).form for nq in (1, 1024) for k in (1, 1024) for rows in (1, 10**7)} == {forms[-1]}, dim
    assert forms == sorted(forms) and forms[0] == 0 and forms[-1] == 1, "the form switches once, with the dimension"
    assert G.hamming_form(1, 1, 10, 3001).row_slices >= 3 and G.hamming_form(128, 1, 100, 10**7, 256).row_slices >= 256


def test_the_reference_against_a_bit_loop():
    rng = np.random.default_rng(5)
    rows, qs = rng.integers(0, 256, (5, 3), np.uint8), rng.integers(0, 256, (2, 3), np.uint8)
    rows[3] = rows[1]  # a tie: position decides
    d = np.array([[sum(((int(a) ^ int(b)) >> bit) & 1 for a, b in zip(q, r) for bit in range(8)) for r in rows] for q in qs])
    assert (H.distances(qs, rows) == d).all()
    dead = np.array([False, False, True, False, False])
    sc, idx, raw = H.reference(qs, rows, 6, dead=dead, index_base=100)
    for q in range(2):
        want = sorted((int(d[q, r]), r) for r in range(5) if not dead[r])
        assert raw[q, :4].tolist() == [w[0] for w in want] and idx[q, :4].tolist() == [100 + w[1] for w in want]
        assert (sc[q, :4] == raw[q, :4]).all() and np.isinf(sc[q, 4:]).all() and (idx[q, 4:] == H.PAD).all() and (raw[q, 4:] == 0).all()


def test_pack_sign_bits():
    x = np.array([[0.5, -1.0, 0.0, 2.0, 3.0, -0.0, 1e-30, -7.0, 9.0, -9.0]], np.float32)
    assert G.pack_sign_bits(x).tolist() == [[0b01011001, 0b00000001]] and G.pack_sign_bits(x).dtype == np.uint8
    assert G.pack_sign_bits(x[0]).tolist() == [0b01011001, 1] and M.pack_sign_bits is G.pack_sign_bits
