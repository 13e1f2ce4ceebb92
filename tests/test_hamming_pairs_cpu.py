"""Hamming pair join, CPU tier (include/mvf_gpu_hamming_pairs.h; DESIGN.md §3 "Hamming pair join"): the header's functions against
the library, the refusals that need no device in their order, the form function's bounds, the triangular grid's exact cover
through the kernel's own decode function, and the GPU tier's numpy reference against a plain double loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import gpu as G

INV = 12  # MVF_ERR_INVALID_ARGUMENT
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
NAMES = {"mvfgpu_hamming_pairs", "mvfgpu_selftest_hamming_pairs_form", "mvfgpu_selftest_hamming_pairs_stage_ms"}


def declared(header):
    text = open(os.path.join(INCLUDE, header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    return set(re.findall(r"\b(mvfgpu_\w+)\s*\(", text))


def test_header_library_and_package_export_the_feature():
    assert declared("mvf_gpu_hamming_pairs.h") == NAMES and not (declared("mvf_gpu.h") & NAMES)
    for name in NAMES:
        assert hasattr(_lib.gpu(), name), f"libmvf_gpu.so does not export {name}"
    for name in ("find_duplicate_pairs", "hamming_pairs_form", "HammingPairsForm", "HammingPairs"):
        assert callable(getattr(M, name)) and name in M.__all__
    assert callable(G.GpuCorpus.hamming_pairs)


def _call(fn, m=2, total=True, first=True, second=True, listed=True, ms=True):
    buf = np.zeros(64, np.uint8)
    p = lambda on: buf.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    args = [None, 3, m, p(total), None, p(first), p(second), None, p(listed)]
    rc = lib.mvfgpu_hamming_pairs(*args) if fn == "host" else lib.mvfgpu_selftest_hamming_pairs_stage_ms(*args, None, p(ms))
    return rc, lib.mvfgpu_last_error_message().decode()


@pytest.mark.parametrize("fn", ["host", "timer"])
def test_refusals_precede_any_device_call(fn):
    """in the header's order, against a NULL handle (what a handle is refused for needs one: tests/test_gpu_hamming_pairs.py)"""
    for kw in (dict(total=False), dict(listed=False), dict(total=False, first=False, m=2**30)):
        assert _call(fn, **kw) == (INV, "NULL buffer"), kw
    for kw in (dict(first=False), dict(second=False), dict(first=False, m=2**24 + 1)):  # (before the limit on max_pairs)
        assert _call(fn, **kw) == (INV, "NULL buffer (out_first / out_second are required when max_pairs > 0)"), kw
    rc, msg = _call(fn, m=2**24 + 1)
    assert rc == INV and msg.startswith("max_pairs above 2^24 is not built for the Hamming pair join")
    assert _call(fn, m=2**24) == (INV, "corpus is NULL")
    assert _call(fn, m=0, first=False, second=False) == (INV, "corpus is NULL")  # total and degrees only: the entry buffers may be NULL
    if fn == "timer":
        assert _call(fn, ms=False) == (INV, "NULL buffer")


DIMS = (1, 16, 17, 64, 65, 256, 257, 512)
ROWS = (0, 1, 17, 300, 1100, 2300, 10**5, 10**7, 2**32 - 65536)


def test_form_refusals():
    form = _lib.gpu().mvfgpu_selftest_hamming_pairs_form
    for dim, rows, m in ((0, 1, 0), (513, 1, 0), (16, 2**32 - 65535, 0), (16, 10, 2**24 + 1)):
        assert form(dim, rows, 0, m, 0, *[None] * 10) == INV, (dim, rows, m)
    at = C.c_uint64(0)
    assert form(16, 2300, 0, 0, G.hamming_pairs_form(16, 2300).blocks, *[None] * 8, C.byref(at), None) == INV  # one behind the last block


@pytest.mark.parametrize("cus", [0, 64, 256])
@pytest.mark.parametrize("dim", DIMS)
def test_form_bounds(dim, cus):
    for rows in ROWS:
        f = G.hamming_pairs_form(dim, rows, cus, max_pairs=1000)
        where = (dim, rows, cus, f)
        # hamming_radius_form's tile rule with nq = rows
        assert f.query_tile == min(128 if dim <= 256 else 64, max(16, 1 << max(rows - 1, 0).bit_length())), where
        assert f.chunks == -(-dim // 64) and f.query_tile * 256 * f.chunks < f.lds_bytes <= 160 * 1024, where
        assert f.span_rows % 256 == 0 and 1024 <= f.span_rows <= 8192, where
        assert f.tiles == -(-rows // f.query_tile) and f.spans == -(-rows // f.span_rows), where
        # every tile with a row behind its first meets at least its own span; nothing beyond the rectangle's upper triangle
        active = -(-(rows - 1) // f.query_tile) if rows > 1 else 0
        assert active <= f.blocks <= active * max(f.spans, 1) and (f.blocks == 0) == (rows < 2), where
        listed = min(1000, rows * (rows - 1) // 2)
        assert f.scratch_bytes >= 16 + 4 * rows + 24 * listed, where
    assert G.hamming_pairs_form(dim, 10**6, cus).span_rows == 8192  # a 1M-row corpus: the longest spans, and still > 10^5 blocks
    assert G.hamming_pairs_form(dim, 10**6, cus).blocks > 10**5


@pytest.mark.parametrize("dim,rows", [(16, 2), (16, 17), (16, 129), (16, 1025), (16, 1100), (16, 2300), (48, 2049), (300, 4097), (512, 10**5),
                                      (16, 10**5)])
def test_the_grid_covers_the_upper_triangle_exactly_once(dim, rows):
    """block index -> (tile, span) through the kernel's decode: each pair whose span reaches above the tile's first row, once"""
    f = G.hamming_pairs_form(dim, rows)
    want = {(t, s) for t in range(f.tiles) for s in range(f.spans) if min((s + 1) * f.span_rows, rows) - 1 > t * f.query_tile}
    got = [G.hamming_pairs_form(dim, rows, block_index=b).block for b in range(f.blocks)]
    assert len(got) == len(want) and set(got) == want
    assert got == sorted(got)  # tiles ascending, each with its spans ascending


def test_the_reference_agrees_with_a_plain_loop():
    from test_gpu_hamming_pairs import reference
    rng = np.random.default_rng(5)
    x = rng.integers(0, 8, (9, 2), dtype=np.uint8)
    x[7] = x[2]
    dead = np.array([0, 1, 0, 0, 0, 0, 1, 0, 0], bool)
    ids = rng.permutation(9).astype(np.uint64) + np.uint64(100)
    for radius in (0, 2, 3, 16, 2**32 - 1):
        total, deg, first, second, raw = reference(x, radius, dead, ids)
        pairs, degree = [], [0] * 9
        for i in range(9):
            for j in range(i + 1, 9):
                d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(x[i], x[j]))
                if not dead[i] and not dead[j] and d <= radius:
                    pairs.append((int(ids[i]), int(ids[j]), d))
                    degree[i] += 1
                    degree[j] += 1
        assert total == len(pairs) and deg.tolist() == degree and list(zip(first.tolist(), second.tolist(), raw.tolist())) == pairs
        assert deg.dtype == np.uint32 and first.dtype == second.dtype == np.uint64 and raw.dtype == np.int32
    assert reference(x, 0, dead, None, index_base=50)[2].tolist() == [52]  # the copy planted above, by position
