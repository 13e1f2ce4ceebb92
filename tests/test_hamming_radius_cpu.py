"""Hamming radius search, CPU tier (include/mvf_gpu_hamming_radius.h; DESIGN.md §3 "Hamming radius search"): the header's
functions against the library, the refusals that need no device in their order, the form function's bounds, and the GPU tier's
numpy reference against a second, independently written loop."""
import ctypes as C

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import gpu as G

INV = 12  # MVF_ERR_INVALID_ARGUMENT


def test_library_and_package_export_the_feature():
    for name in ("mvfgpu_search_hamming_radius", "mvfgpu_selftest_hamming_radius_form", "mvfgpu_selftest_hamming_radius_stage_ms"):
        assert hasattr(_lib.gpu(), name), f"libmvf_gpu.so does not export {name}"
    for name in ("find_within_hamming", "hamming_radius_form", "HammingRadiusForm"):
        assert callable(getattr(M, name)) and name in M.__all__
    assert callable(G.GpuCorpus.search_hamming_radius)


def _call(fn, q=True, nq=1, radii=True, m=2, counts=True, sc=True, idx=True, ms=True):
    buf = np.zeros(64, np.uint8)
    p = lambda on: buf.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    args = [None, p(q), G.UINT8, 32, nq, p(radii), m, p(counts), p(sc), p(idx), None]
    rc = lib.mvfgpu_search_hamming_radius(*args) if fn == "host" else lib.mvfgpu_selftest_hamming_radius_stage_ms(*args, None, p(ms))
    return rc, lib.mvfgpu_last_error_message().decode()


@pytest.mark.parametrize("fn", ["host", "timer"])
def test_refusals_precede_any_device_call(fn):
    """mvfgpu_search_radius' handle-free checks with its messages, then max_per_query above 1024, then the handle (what a handle
    is refused for needs one: tests/test_gpu_hamming_radius.py)"""
    assert _call(fn, nq=0) == (INV, "nq must be > 0")
    for kw in (dict(q=False), dict(radii=False), dict(counts=False)):
        assert _call(fn, **kw) == (INV, "NULL buffer"), kw
    for kw in (dict(sc=False), dict(idx=False), dict(sc=False, m=5000)):  # (before the limit on max_per_query)
        rc, msg = _call(fn, **kw)
        assert rc == INV and msg.startswith("NULL buffer (out_scores / out_indices are required"), kw
    rc, msg = _call(fn, m=1025)
    assert rc == INV and "max_per_query above 1024 is not built for Hamming radius search" in msg
    assert _call(fn, m=1024) == (INV, "corpus is NULL")
    assert _call(fn, m=0, sc=False, idx=False) == (INV, "corpus is NULL")  # counts only: the entry buffers may be NULL
    if fn == "timer":
        assert _call(fn, ms=False) == (INV, "NULL buffer")


def test_form_bounds():
    for dim, nq, rows in ((0, 1, 1), (513, 1, 1), (16, 0, 1), (16, 1, 2**32)):
        assert _lib.gpu().mvfgpu_selftest_hamming_radius_form(dim, nq, rows, 0, None, None, None, None, None, None) == INV, (dim, nq, rows)
    for dim in (1, 16, 17, 64, 65, 128, 129, 256, 257, 512):
        cap = 128 if dim <= 256 else 64
        for nq in (1, 16, 17, 33, 64, 65, 128, 129, 1024, 5000):
            for rows in (0, 1, 1100, 3001, 10**5, 10**7, 2**32 - 65536):
                for cus in (0, 64, 256):
                    f = G.hamming_radius_form(dim, nq, rows, cus)
                    where = (dim, nq, rows, cus, f)
                    tiles = -(-min(nq, 1024) // f.query_tile)
                    # the smallest of 16 .. 128 that holds the window's queries, capped by the prepared tile's LDS
                    assert f.query_tile == min(cap, max(16, 1 << (min(nq, 1024) - 1).bit_length())), where
                    # the staged tile and a u32 per query; as many blocks as share a CU's 160 KiB, 8 at most
                    assert f.chunks == -(-dim // 64) and f.lds_bytes == f.query_tile * (256 * f.chunks + 4), where
                    assert f.blocks_per_cu == min(8, 160 * 1024 // f.lds_bytes) >= 1 and f.blocks_per_cu * f.lds_bytes <= 160 * 1024, where
                    # a slice holds 1024 rows at least -- no more slices than started runs of 1024 rows -- and nothing else caps them
                    by_cus = -(-f.blocks_per_cu * (cus or 256) // tiles)
                    assert (f.row_slices == 0) == (rows == 0) and f.row_slices <= min(by_cus, max(1, -(-rows // 1024))), where
                    assert f.scratch_bytes >= min(nq, 1024) * 8192 * 8, where
    assert G.hamming_radius_form(16, 1, 10**7, 256).row_slices == 2048      # one query: eight small blocks per CU, no merge cap
    assert G.hamming_radius_form(128, 1024, 10**7, 256).row_slices == 64    # 128 queries x 128 bytes: 64.5 KiB, two per CU, 8 tiles
    assert G.hamming_radius_form(16, 17, 1100).row_slices == 2


def test_the_reference_agrees_with_a_plain_loop():
    from test_gpu_hamming_radius import PAD, reference
    rng = np.random.default_rng(5)
    x, q = rng.integers(0, 4, (9, 2), dtype=np.uint8), rng.integers(0, 4, (3, 2), dtype=np.uint8)
    dead = np.array([0, 1, 0, 0, 0, 0, 1, 0, 0], bool)
    radii, m = np.array([1, 2, 16], np.uint32), 4
    counts, sc, idx, raw = reference(q, x, radii, m, dead, index_base=50)
    for i in range(3):
        hits = []
        for r in range(9):
            d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(q[i], x[r]))
            if not dead[r] and d <= radii[i]:
                hits.append((d, r))
        hits.sort()
        assert counts[i] == len(hits)
        for j in range(m):
            want = (hits[j][0], 50 + hits[j][1], float(hits[j][0])) if j < len(hits) else (0, int(PAD), np.inf)
            assert (raw[i, j], int(idx[i, j]), sc[i, j]) == want
