"""Binary MaxSim, CPU tier (include/mvf_gpu_hamming_maxsim.h; DESIGN.md §3 "Binary MaxSim"): the header's functions against the
library, the refusals that need no device in their order, and the form function's properties."""
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
MAX_TOKENS = 1024


def test_gpu_library_exports_the_header_s_symbols():
    text = open(os.path.join(ROOT, "include", "mvf_gpu_hamming_maxsim.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mvfgpu_\w+)\s*\(", text, re.M))
    assert declared == {"mvfgpu_search_hamming_maxsim", "mvfgpu_search_hamming_maxsim_device", "mvfgpu_selftest_hamming_maxsim_form",
                        "mvfgpu_selftest_hamming_maxsim_stage_ms"}
    for name in declared:
        assert hasattr(_lib.gpu(), name), f"libmvf_gpu.so does not export {name}"
    assert '#include "mvf_gpu.h"' in text and "additions to ABI version 3" in text
    assert "mvfgpu_search_hamming_maxsim" not in open(os.path.join(ROOT, "include", "mvf_gpu.h")).read()
    for name in ("find_top_k_documents_hamming", "hamming_maxsim_form"):
        assert callable(getattr(M, name)) and name in M.__all__


def _call(fn, part=True, q=True, nq=1, n_tokens=4, k=2, sc=True, keys=True, ms=True):
    buf = np.zeros(64, np.uint8)
    p = lambda on: buf.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    # the corpus is NULL throughout; the partition, where given, is never read in front of that refusal
    args = [None, p(part), p(q), G.UINT8, 16, nq, n_tokens, k, p(sc), p(keys), None]
    if fn == "host":
        rc = lib.mvfgpu_search_hamming_maxsim(*args)
    elif fn == "device":
        rc = lib.mvfgpu_search_hamming_maxsim_device(*args, None)
    else:
        rc = lib.mvfgpu_selftest_hamming_maxsim_stage_ms(*args, None, p(ms))
    return rc, lib.mvfgpu_last_error_message().decode()


@pytest.mark.parametrize("fn", ["host", "device", "timer"])
def test_refusals_precede_any_device_call(fn):
    """the multi-vector search's handle-free checks with its messages, then n_tokens, then the partition, then the handle (what
    a handle is refused for needs one: tests/test_gpu_hamming_maxsim.py)"""
    assert _call(fn, nq=0, n_tokens=0, part=False) == (INV, "nq must be > 0")
    for k in (0, 2**31 + 1):
        assert _call(fn, k=k, n_tokens=0) == (INV, "k must be in 1..2^31")
    for kw in (dict(q=False), dict(sc=False), dict(keys=False)):
        assert _call(fn, n_tokens=0, **kw) == (INV, "NULL buffer"), kw
    for t in (0, MAX_TOKENS + 1):
        assert _call(fn, n_tokens=t, part=False) == (INV, f"n_tokens must be in 1..{MAX_TOKENS}, got {t}")
    assert _call(fn, part=False) == (INV, "partition is NULL")
    assert _call(fn, n_tokens=MAX_TOKENS) == (INV, "corpus is NULL")
    if fn == "timer":
        assert _call(fn, ms=False, nq=0) == (INV, "NULL buffer")


def test_form_properties():
    form = _lib.gpu().mvfgpu_selftest_hamming_maxsim_form
    for dim, nq, t, nk, held in ((0, 1, 1, 1, 1), (513, 1, 1, 1, 1), (16, 0, 1, 1, 1), (16, 1, 0, 1, 1), (16, 1, MAX_TOKENS + 1, 1, 1),
                                 (16, 1, 1, 1, 2**32), (16, 1, 1, 5, 4)):
        assert form(dim, nq, t, nk, held, 1 << 20, 0, None, None, None, None, None, None, None) == INV, (dim, nq, t, nk, held)
    for dim in (1, 16, 17, 64, 65, 128, 512):
        pitch = -(-dim // 16) * 16
        for nq in (1, 3, 1024, 5000):
            for t in (1, 3, 4, 33, 1024):
                for nk in (1, 600, 10**6):
                    for budget in (0, 10**5, 512 << 20):
                        f = G.hamming_maxsim_form(dim, nq, t, nk, max(nk, 1500), budget)
                        where = (dim, nq, t, nk, budget, f)
                        assert f.chunks == -(-pitch // 64) and f.lds_bytes <= 160 * 1024 and f.query_tile % 16 == 0, where
                        assert f.rows_in_registers == (1 if pitch <= 64 else 0), where
                        assert min(4, t) <= f.chunk_tokens <= min(32, t) and 1 <= f.window_sets <= min(nq, 1024), where
                        per_set = lambda chunk: nk * (4 * chunk + 20) + t * (256 * f.chunks + 4)  # noqa: E731
                        assert f.scratch_bytes == f.window_sets * per_set(f.chunk_tokens), where
                        if per_set(min(4, t)) <= budget:  # a one-group chunk of one set fits
                            assert f.scratch_bytes <= budget, where
    # the default budget holds whole chunks of 32 tokens and a ColPali batch of 16 sets in one window
    assert G.hamming_maxsim_form(16, 16, 32, 10**4, 10**7)[3:5] == (32, 16)
