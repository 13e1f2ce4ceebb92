"""Row writes, CPU tier (include/mvf_gpu_update.h; DESIGN.md §3 "Row writes"): the symbols are exported, the header compiles
as C99 and as C++17 and declares the struct the bindings mirror, the refusal that needs no handle works without a device, and
GpuCorpus.write_rows checks dtype and shape before any native call; and the worlds of the GPU tests (tests/_write_rows.py) have, under
the oracle alone, the properties that make a skipped row show."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
INV = 12  # MVF_ERR_INVALID_ARGUMENT
FUNCTIONS = ("mvfgpu_corpus_write_rows", "mvfgpu_corpus_write_rows_device")


def _message():
    return _lib.gpu().mvfgpu_last_error_message().decode()


def test_the_symbols_are_exported_and_the_header_declares_them():
    lib = _lib.gpu()
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
    text = open(os.path.join(INCLUDE, "mvf_gpu_update.h")).read()
    declared = set(re.findall(r"^\s*int\s+(mvfgpu_\w+)\s*\(", text, re.M))
    assert declared == set(FUNCTIONS), declared ^ set(FUNCTIONS)
    assert '#include "mvf_gpu.h"' in text
    main = open(os.path.join(INCLUDE, "mvf_gpu.h")).read()
    assert not any(name in main for name in FUNCTIONS), "additions to ABI version 3 live in their own header"
    assert lib.mvfgpu_abi_version() == 3


PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "mvf_gpu_update.h"
int main(void) {
    mvfgpu_write_report rep;
    MVFGPU_INIT(rep);
    printf("%u %u %u %u %u %u %u\n", (unsigned)sizeof(rep), (unsigned)rep.struct_size, (unsigned)offsetof(mvfgpu_write_report, launches),
           (unsigned)offsetof(mvfgpu_write_report, rows_written), (unsigned)offsetof(mvfgpu_write_report, bytes_written),
           (unsigned)offsetof(mvfgpu_write_report, refreshed), (unsigned)offsetof(mvfgpu_write_report, reserved));
    printf("%u %u %u %u\n", MVFGPU_WRITE_NORMS, MVFGPU_WRITE_SHADOW_F16, MVFGPU_WRITE_SHADOW_I8, MVFGPU_WRITE_SHADOW_6B);
    /* both link, and refuse a NULL corpus before anything else */
    return (mvfgpu_corpus_write_rows(NULL, NULL, 0, NULL, 0, &rep) != MVF_ERR_INVALID_ARGUMENT) +
           (mvfgpu_corpus_write_rows_device(NULL, NULL, 0, NULL, 0, NULL, NULL) != MVF_ERR_INVALID_ARGUMENT);
}
"""


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", ".c"), ("g++", "-std=c++17", ".cpp")])
def test_the_header_compiles_and_the_struct_is_as_declared(tmp_path, compiler, std, suffix):
    src = tmp_path / ("write_report" + suffix)
    src.write_text(PROGRAM)
    exe = str(tmp_path / "write_report")
    libdir = os.path.join(ROOT, "metrovector_amd")
    out = subprocess.run([compiler, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, str(src), "-L", libdir, "-lmvf_gpu",
                          f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    sizes, bits = run.stdout.splitlines()
    assert [int(x) for x in sizes.split()] == [32, 32, 4, 8, 16, 24, 28]
    assert [int(x) for x in bits.split()] == [1, 2, 4, 8]
    # the ctypes mirror and the Rust one
    assert C.sizeof(_lib.WriteReport) == 32
    for name, at in (("launches", 4), ("rows_written", 8), ("bytes_written", 16), ("refreshed", 24), ("reserved", 28)):
        assert getattr(_lib.WriteReport, name).offset == at, name
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in FUNCTIONS:
        assert f"fn {name}(" in rust, name
    assert "pub struct MvfGpuWriteReport" in rust


def test_the_mirror_includes_the_header():
    text = open(os.path.join(INCLUDE, "mvf.hpp")).read()
    assert '#include "mvf_gpu_update.h"' in text and "write_rows(" in text


def test_a_null_corpus_is_refused_without_a_device():
    lib = _lib.gpu()
    idx = np.zeros(2, np.uint64)
    rows = np.zeros((2, 4), np.float32)
    rep = _lib.WriteReport()
    for count in (0, 2):  # before everything else, count == 0 included
        rc = lib.mvfgpu_corpus_write_rows(None, idx.ctypes.data_as(C.c_void_p), count, rows.ctypes.data_as(C.c_void_p), 16, C.byref(rep))
        assert rc == INV and _message() == "corpus is NULL"
        rc = lib.mvfgpu_corpus_write_rows_device(None, idx.ctypes.data_as(C.c_void_p), count, rows.ctypes.data_as(C.c_void_p), 16, None,
                                                 C.byref(rep))
        assert rc == INV and _message() == "corpus is NULL"
    rc = lib.mvfgpu_corpus_write_rows(None, None, 0, None, 0, None)
    assert rc == INV and _message() == "corpus is NULL"


def test_python_layer_checks_dtype_and_shape_before_any_native_call():
    assert hasattr(G.GpuCorpus, "write_rows") and hasattr(G.GpuCorpus, "write_rows_device")
    assert callable(M.write_rows) and "write_rows" in M.__all__
    c = G.GpuCorpus(0)  # a NULL handle: nothing may reach the library
    c._h = C.c_void_p(None)
    c._shape = (10, 4, G.FLOAT32)
    good = np.zeros((2, 4), np.float32)
    for idx, rows in (([1, 2], good.astype(np.float64)), ([1, 2], good.astype(np.float16)), ([1, 2], good.astype(np.int8)),
                      ([1, 2], np.zeros((2, 5), np.float32)), ([1, 2], np.zeros((3, 4), np.float32)), ([1, 2], np.zeros(8, np.float32)),
                      ([1, 2, 3], good), ([1], np.zeros((1, 1, 4), np.float32))):
        with pytest.raises(E.InvalidArgument):
            c.write_rows(idx, rows)
        with pytest.raises(E.InvalidArgument):
            M.write_rows(c, idx, rows)
    c._shape = (10, 4, G.INT8)
    with pytest.raises(E.InvalidArgument):
        c.write_rows([0], np.zeros((1, 4), np.uint8))
    # what passes the checks reaches the library, which refuses the NULL handle
    with pytest.raises(E.InvalidArgument, match="corpus is NULL"):
        c.write_rows([0], np.zeros((1, 4), np.int8))


# ---- the worlds of tests/test_gpu_write_rows_edges.py, held with the oracle alone (tests/_write_rows.py) ---------------------------
def _world_cases():
    import _write_rows as W
    return ([("large", dt, dim) for dt, dims in W.LARGE_DIMS.items() for dim in dims] +
            [("wide", dt, dim) for dt, dims in W.WIDE_DIMS.items() for dim in dims])


@pytest.mark.parametrize("kind, dt, dim", _world_cases())
def test_a_skipped_list_entry_of_the_large_and_wide_worlds_would_show(oracle, kind, dt, dim):
    """every segment of the list -- the entries a wave serves first, second and third -- holds rows that are in their queries'
    top-k over the changed rows and not over the old ones"""
    import _write_rows as W
    w = (W.large_world if kind == "large" else W.wide_world)(oracle, dt, dim)
    (pos, rows), = w.writes
    lst = pos.astype(np.int64)
    es = np.dtype(W.NP[dt]).itemsize
    if kind == "large":
        assert w.rows0.shape == (16421, dim) and len(lst) == 16389 == 2 * 8192 + 5 and 16421 == 256 * 64 + 37
        assert set((0, 63, 64, 16383, 16384, 16420)) <= set(lst.tolist())
        assert w.segments == ((0, 8192), (8192, 16384), (16384, 16389))
        assert (rows[-5:] == w.q[:5].astype(W.NP[dt])).all(), "the last five entries hold the exact copies of the queries 0..4"
        assert dt != G.FLOAT32 or 16389 * (4 + (dim * es + 15) // 16 * 16) > 3 << 20, "the host call's blob is pageable"
    else:
        assert w.rows0.shape == (4133, dim) and len(lst) == 700
        assert (dim * es + 15) // 16 > 64, "more than 64 16-byte vectors to the row"
    assert len(set(lst.tolist())) == len(lst) and not (np.sort(lst) == lst).all(), "distinct positions, not in ascending order"
    assert (w.rows1[lst] == rows).all() and (np.sort(lst) == w.written).all()
    untouched = np.setdiff1d(np.arange(len(w.rows0)), lst)
    assert (w.rows1[untouched] == w.rows0[untouched]).all()
    for s, (a, b) in enumerate(w.segments):
        assert len(w.planted[s]) >= 5
        for i, mine in w.planted[s]:
            assert all(a <= int(np.nonzero(lst == p)[0][0]) < b for p in mine)
    W.planted_rows_show(oracle, w)


def test_the_outlier_rows_are_what_they_are_meant_to_be():
    """in numpy f32: the huge rows' sums of squares are finite, the overflowing row's elements are finite and their squares' sum is
    +inf, the non-finite rows hold one +Inf and one NaN"""
    import _write_rows as W
    like = np.ones((2, 256), np.float32)
    for dim in (50, 256):
        for dt in (G.FLOAT32, G.FLOAT16):
            huge = W.outlier_rows(dt, dim, "huge", like[:, :dim]).astype(np.float32)
            assert np.isfinite(huge).all() and (huge == (1e18 if dt == G.FLOAT32 else 60000.0)).all()
            s = np.float32(0)
            for x in huge[0]:
                s = np.float32(s + x * x)
            assert np.isfinite(s) and s < np.float32(3.0e38), "below the builders' own finiteness limit"
            bad = W.outlier_rows(dt, dim, "non-finite", like[:, :dim])
            assert np.isposinf(bad[0]).sum() == 1 and np.isnan(bad[1]).sum() == 1 and np.isfinite(bad).sum() == 2 * dim - 2
        over = W.outlier_rows(G.FLOAT32, dim, "overflowing", None)
        assert over.dtype == np.float32 and np.isfinite(over).all()
        with np.errstate(over="ignore"):
            assert np.isposinf(np.sum(over[0] * over[0], dtype=np.float32)) and np.isposinf(over[0, 0] * over[0, 0] * np.float32(dim))
    assert set(W.OUTLIER_KINDS) == {G.FLOAT32, G.FLOAT16} and "overflowing" not in W.OUTLIER_KINDS[G.FLOAT16]
    q = W.extreme_queries(G.FLOAT32, 50, np.arange(1, 51, dtype=np.float32))
    assert not q["zero"].any() and 0.5e-20 < np.linalg.norm(q["tiny"].astype(np.float64)) < 2e-20
    assert 0.5e15 < np.linalg.norm(q["big"].astype(np.float64)) < 2e15
