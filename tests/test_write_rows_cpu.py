"""Row writes, CPU tier (include/mvf_gpu_update.h; DESIGN.md §3 "Row writes"): the symbols are exported, the header compiles
as C99 and as C++17 and declares the struct the bindings mirror, the refusal that needs no handle works without a device, and
GpuCorpus.write_rows checks dtype and shape before any native call."""
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
