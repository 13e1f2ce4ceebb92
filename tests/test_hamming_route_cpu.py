"""The Hamming search's MFMA route, CPU tier (include/mvf_gpu_hamming_route.h; DESIGN.md §5 "HQ / H2"): the header's functions
against the library, their refusals, the route function and the properties of the route's form."""
import ctypes as C
import os
import re

import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

import _hamming as H
import _streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT

# the stream class of every function the header declares, in tests/_streams.py's words
ENTRY_CLASS = {
    "mvfgpu_set_hamming_route": S.NO_DEVICE_WORK,
    "mvfgpu_selftest_hamming_route": S.NO_HANDLE,
    "mvfgpu_selftest_hamming_mfma_form": S.NO_HANDLE,
}


def test_gpu_library_exports_the_route_header_s_symbols():
    text = open(os.path.join(ROOT, "include", "mvf_gpu_hamming_route.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mvfgpu_\w+)\s*\(", text, re.M))
    assert declared == set(ENTRY_CLASS) and not declared & (set(S.ENTRY_CLASS) | set(H.ENTRY_CLASS))
    for name in declared:
        assert hasattr(_lib.gpu(), name), f"libmvf_gpu.so does not export {name}"
    for name in ("hamming_route", "hamming_mfma_form", "HammingMfmaForm"):
        assert name in M.__all__ and hasattr(M, name)


def test_refusals():
    lib, out = _lib.gpu(), C.c_uint32(0)
    assert lib.mvfgpu_set_hamming_route(None, 1) == INV
    assert lib.mvfgpu_selftest_hamming_route(16, 1, 1, 1, 0, None) == INV
    for forced in (-1, 3):
        assert lib.mvfgpu_selftest_hamming_route(16, 1, 1, 1, forced, C.byref(out)) == INV
    for dim, nq, k, rows in ((0, 1, 1, 1), (33026, 1, 1, 1), (16, 0, 1, 1), (16, 1, 0, 1), (16, 1, 1025, 1), (16, 1, 1, 2**32)):
        assert lib.mvfgpu_selftest_hamming_route(dim, nq, k, rows, 0, C.byref(out)) == INV, (dim, nq, k, rows)
    for dim, nq, k, rows in ((0, 1, 1, 1), (513, 1, 1, 1), (16, 0, 1, 1), (16, 1, 0, 1), (16, 1, 1025, 1), (16, 1, 1, 2**32)):
        assert lib.mvfgpu_selftest_hamming_mfma_form(dim, nq, k, rows, 0, *[None] * 8) == INV, (dim, nq, k, rows)
    with pytest.raises(E.InvalidArgument):
        G.hamming_route(16, 1, 1, 1, 3)


def test_route_function():
    for dim in (64, 128, 512):
        assert G.hamming_route(dim, 1024, 100, 10**7) == 2 and G.hamming_route(dim, 5000, 128, 10**8) == 2
        assert G.hamming_route(dim, 1023, 100, 10**7) == 1 and G.hamming_route(dim, 1024, 100, 10**7 - 1) == 1, "below a floor"
        assert G.hamming_route(dim, 63, 100, 10**7) == 1 and G.hamming_route(dim, 1024, 100, 131071) == 1, "below the floors of every rule"
        assert G.hamming_route(dim, 1024, 129, 10**7) == 1 and G.hamming_route(48, 1024, 100, 10**7) == 1, "long lists, short rows"
        assert G.hamming_route(dim, 1, 1, 1, 2) == 2 and G.hamming_route(dim, 1024, 100, 10**7, 1) == 1
    for dim in (513, 1000, 33025):
        assert {G.hamming_route(dim, 1024, 100, 10**7, forced) for forced in (0, 1, 2)} == {1}, "a pitch above 512 bytes"


def test_the_existing_hamming_tests_stay_on_route_1():
    import test_gpu_hamming as TG
    shapes = [(d, r, nq, k) for d, r, nq, k in TG.CASES] + [(d, H.cell_rows(d)[0], nq, k) for d, nq, k in H.FORM_CELLS]
    shapes += [(d, 4000, 5, k) for d in (16, 48, 300) for k in (1, 100, 1024)] + [(16, H.merge_world(n)[0].x.shape[0], 2, H.MERGE_K) for n in H.MERGE_CASES]
    shapes += [(d, 1100, 1030, 3) for d in (16, 300)] + [(33025, 300, 2, 300), (48, 3001, 20, 100), (17, 500, 6, 505)]
    for dim, rows, nq, k in shapes:
        for wn in {min(nq, 1024), max(nq - 1024, 1)}:
            assert G.hamming_route(dim, wn, k, rows) == 1, (dim, rows, nq, k)


def test_mfma_form_properties():
    for dim in (1, 16, 17, 100, 256, 257, 500, 512):
        for nq in (1, 63, 64, 65, 128, 129, 1024, 5000):
            for k in (1, 10, 100, 256, 257, 1024):
                for rows in (0, 1, 1100, 10**5, 10**7, 2**32 - 65536):
                    for cus in (0, 64, 256):
                        f = G.hamming_mfma_form(dim, nq, k, rows, cus)
                        where = (dim, nq, k, rows, cus, f)
                        assert f.query_tile == (128 if dim <= 256 else 64) and f.threads == 256 and f.rows_per_wave * f.threads // 64 == H.STEP_ROWS, where
                        assert f.lds_bytes <= 160 * 1024 and f.scratch_bytes <= 512 << 20 and f.prepared_bytes <= (2 << 20) + 4096, where
                        assert f.row_slices * H.next_pow2(k) <= H.MERGE_MAX, where
                        assert (f.row_slices == 0) == (rows == 0) and f.row_slices * f.slice_rows >= rows and (rows == 0 or (f.row_slices - 1) * f.slice_rows < rows), where
    assert G.hamming_mfma_form(128, 1024, 100, 10**7, 256).row_slices == 32 and G.hamming_mfma_form(128, 1024, 1024, 10**7, 256).row_slices == 32
