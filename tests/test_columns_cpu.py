"""Metadata columns and filters from predicates, CPU tier (DESIGN.md §3 "Column filters"): both libraries export the new
entry points and Python names them, the ctypes mirrors have the compiler's sizes, the host-side range normalisation agrees
with the numpy restatement (tests/_columns.py) over every operator, type and edge operand, refusals precede any device call,
and column data round-trips builder -> image -> reader byte for byte from blocks at odd offsets."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

from _columns import OP_CODE, OPS, TOP, U32, U64, clause_mask, range_of, where_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, BUILD = 12, 10  # MVF_ERR_INVALID_ARGUMENT, MVF_ERR_BUILD
EDGES = [0, 1, 2 ** 32 - 1, 2 ** 32, TOP]
RANGE_OPS = [op for op in OPS if op not in ("in", "not in")]


def _msg():
    return _lib.gpu().mvfgpu_last_error_message().decode()


def test_entry_points_and_python_names_exist():
    lib = _lib.gpu()
    for name in ("mvfgpu_column_create", "mvfgpu_column_create_device", "mvfgpu_column_destroy", "mvfgpu_column_get_info",
                 "mvfgpu_filter_create_where", "mvfgpu_selftest_predicate_range"):
        assert hasattr(lib, name), name
    for name in ("mvf_reader_metadata_column", "mvf_reader_metadata_column_at"):
        assert hasattr(_lib.host(), name), name
    for name in ("attach_column", "attach_column_device", "make_filter_where"):
        assert hasattr(G.GpuCorpus, name), name
    assert hasattr(G.GpuColumn, "info") and hasattr(G.GpuColumn, "__enter__") and hasattr(G.GpuColumn, "close")
    assert hasattr(M.MvfReader, "metadata_column")
    for name in ("find_top_k_where", "GpuColumn", "MetadataColumn"):
        assert name in M.__all__ and hasattr(M, name), name
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in ("mvfgpu_column_create", "mvfgpu_column_create_device", "mvfgpu_column_destroy", "mvfgpu_column_get_info",
                 "mvfgpu_filter_create_where"):
        assert f"fn {name}(" in rs, name
    hpp = open(os.path.join(ROOT, "include", "mvf.hpp")).read()
    assert "find_top_k_where" in hpp and "metadata_column(" in hpp
    assert _lib.gpu().mvfgpu_abi_version() == 3, "an additive change: the ABI version stays"


def test_ctypes_mirrors_have_the_compilers_sizes(tmp_path):
    want = {"mvf_metadata_column": _lib.CMetadataColumn, "mvfgpu_column_info": _lib.ColumnInfo, "mvfgpu_predicate": _lib.Predicate}
    body = "".join('printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in want)
    body += 'printf("ops %d %d %u %u %u %u\\n", MVFGPU_OP_EQ, MVFGPU_OP_NOT_IN, MVFGPU_WHERE_ALL, MVFGPU_WHERE_ANY, MVFGPU_WHERE_MAX_CLAUSES, MVFGPU_WHERE_MAX_SET_VALUES);'
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include "mvf_gpu.h"\n#include "mvf_file.h"\nint main(void){' + body + "return 0;}")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    lines = subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.splitlines()
    for line in lines[:-1]:
        name, size = line.split()
        assert C.sizeof(want[name]) == int(size), f"ctypes mirror of {name}: {C.sizeof(want[name])} bytes, header: {size}"
    assert C.sizeof(_lib.ColumnInfo) == 24 and C.sizeof(_lib.Predicate) == 40 and _lib.ColumnInfo().struct_size == 24
    assert lines[-1].split()[1:] == [str(x) for x in (_lib.OP_EQ, _lib.OP_NOT_IN, _lib.WHERE_ALL, _lib.WHERE_ANY, _lib.WHERE_MAX_CLAUSES,
                                                      _lib.WHERE_MAX_SET_VALUES)]
    assert [OP_CODE[op] for op in OPS] == list(range(9)) == [G._OP_OF[op] for op in OPS]


@pytest.mark.parametrize("data_type", [U32, U64])
@pytest.mark.parametrize("op", RANGE_OPS)
def test_the_range_normalisation_agrees_with_the_restatement(data_type, op):
    probe = np.array([v for v in EDGES + [2, 2 ** 32 - 2, 2 ** 32 + 1, TOP - 1] if data_type == U64 or v < 2 ** 32],
                     dtype=np.uint32 if data_type == U32 else np.uint64)
    for a, b in itertools.product(EDGES, EDGES):
        lo, hi, neg = G.predicate_range(data_type, op, a, b)
        assert (lo, hi, neg) == range_of(data_type, op, a, b), (op, a, b)
        # ... and the range means the comparison: on every edge value of the type
        inside = np.array([lo <= int(v) <= hi for v in probe]) ^ bool(neg)
        want = clause_mask(probe, op, (a, b) if op == "between" else a)
        assert (inside == want).all(), (op, a, b)


def test_the_range_normalisation_spot_cases():
    EMPTY = (1, 0, 0)
    for dt in (U32, U64):
        assert G.predicate_range(dt, "<", 0) == EMPTY
        assert G.predicate_range(dt, ">", TOP) == EMPTY
        assert G.predicate_range(dt, "between", 5, 4) == EMPTY
        for a in EDGES:
            eq, ne = G.predicate_range(dt, "==", a), G.predicate_range(dt, "!=", a)
            assert eq[:2] == ne[:2] and (eq[2], ne[2]) == (0, 1), "NE is the negation of EQ"
    assert G.predicate_range(U32, "==", 2 ** 32) == EMPTY
    assert G.predicate_range(U64, "==", 2 ** 32) == (2 ** 32, 2 ** 32, 0)
    assert G.predicate_range(U32, "<", 2 ** 32) == (0, 2 ** 32 - 1, 0), "everything"
    assert G.predicate_range(U32, ">", 2 ** 32 - 1) == EMPTY and G.predicate_range(U64, ">", 2 ** 32 - 1) == (2 ** 32, TOP, 0)
    lib = _lib.gpu()
    lo, hi, neg = C.c_uint64(), C.c_uint64(), C.c_uint32()
    for op in (_lib.OP_IN, _lib.OP_NOT_IN, 99):
        assert lib.mvfgpu_selftest_predicate_range(U32, op, 0, 0, C.byref(lo), C.byref(hi), C.byref(neg)) == INV
    assert lib.mvfgpu_selftest_predicate_range(6, 0, 0, 0, C.byref(lo), C.byref(hi), C.byref(neg)) == BUILD    # StringRef
    assert lib.mvfgpu_selftest_predicate_range(U32, 0, 0, 0, None, C.byref(hi), C.byref(neg)) == INV


def test_the_restatement_on_a_hand_made_column():
    v = np.array([0, 5, 7, 7, 9, 2 ** 32 - 1], np.uint32)
    t = np.array([10, 20, 30, 40, 50, TOP], np.uint64)
    assert where_mask([(v, "==", 7), (t, ">=", 40)]).tolist() == [False, False, False, True, False, False]
    assert where_mask([(v, "==", 7), (t, ">=", 40)], any=True).tolist() == [False, False, True, True, True, True]
    assert where_mask([(v, "in", [9, 0, 9])]).tolist() == [True, False, False, False, True, False]
    assert not where_mask([(v, "in", [])]).any() and where_mask([(v, "not in", [])]).all()
    assert not where_mask([(v, "between", (8, 6))]).any() and not where_mask([(v, "==", 2 ** 32)]).any()
    assert where_mask([(v, "<", 2 ** 32)]).all() and where_mask([(t, "==", TOP)]).tolist() == [False] * 5 + [True]
    dead, base = np.array([0, 0, 1, 0, 0, 0], bool), np.array([1, 1, 1, 1, 0, 1], bool)
    assert where_mask([(v, ">=", 7)], base=base, dead=dead).tolist() == [False, False, False, True, False, True]


def _where(corpus, clauses, n, combine=0, base=None, out=True):
    h = C.c_void_p()
    arr = None
    if clauses is not None:
        arr = (_lib.Predicate * max(len(clauses), 1))()
        for i, (col, op, vals) in enumerate(clauses):
            arr[i].column, arr[i].op = col, op
            if vals is not None:
                arr[i].n_values, arr[i].values = vals.size, vals.ctypes.data
    rc = _lib.gpu().mvfgpu_filter_create_where(corpus, arr, n, combine, base, C.byref(h) if out else None)
    return rc, _msg()


def test_where_refuses_bad_arguments_before_any_device_call():
    """None of these needs a handle: the fake handle and the fake column are never dereferenced."""
    fake, fcol = C.c_void_p(1), C.c_void_p(1)
    one = [(None, _lib.OP_EQ, None)]
    rc, msg = _where(None, one, 1)
    assert rc == INV and "corpus is NULL" in msg
    rc, msg = _where(fake, None, 1)
    assert rc == INV and "NULL" in msg
    rc, msg = _where(fake, one, 1, out=False)
    assert rc == INV and "NULL" in msg
    for n in (0, 9):
        rc, msg = _where(fake, one * 9, n)
        assert rc == INV and "n_clauses" in msg
    rc, msg = _where(fake, [(None, 99, None)], 1)
    assert rc == INV and "unknown predicate op 99" in msg
    rc, msg = _where(fake, one, 1, combine=2)
    assert rc == INV and "combine" in msg
    # the cap counts distinct values: 4097 are refused and pointed to the bitmap form ...
    rc, msg = _where(fake, [(fcol, _lib.OP_IN, np.arange(4097, dtype=np.uint64))], 1)
    assert rc == INV and "4096" in msg and "mvfgpu_filter_create" in msg
    halves = np.arange(2049, dtype=np.uint64)
    rc, msg = _where(fake, [(fcol, _lib.OP_IN, halves), (fcol, _lib.OP_NOT_IN, halves + np.uint64(10 ** 6))], 2)
    assert rc == INV and "4096" in msg, "the cap is over all clauses of a call"
    # ... 5000 given values of which 4096 are distinct pass that check: the next one (a NULL column) answers
    rep = (np.arange(5000, dtype=np.uint64)[::-1] % np.uint64(4096)).copy()
    assert np.unique(rep).size == 4096
    rc, msg = _where(fake, [(None, _lib.OP_IN, rep)], 1)
    assert rc == INV and "column is NULL" in msg
    three = [(None, _lib.OP_IN, halves[:2048].copy()), (None, _lib.OP_NOT_IN, np.zeros(1, np.uint64)),
             (None, _lib.OP_IN, halves[:2047] + np.uint64(10 ** 6))]
    rc, msg = _where(fake, three, 3, combine=1)               # 2048 + 1 + 2047: the cap exactly, over three clauses
    assert rc == INV and "column is NULL" in msg
    rc, msg = _where(fake, [(None, _lib.OP_IN, None)], 1)     # an empty set is legal
    assert rc == INV and "column is NULL" in msg
    arr = (_lib.Predicate * 1)()
    arr[0].op, arr[0].n_values = _lib.OP_IN, 3                # values NULL with n_values > 0
    h = C.c_void_p()
    assert _lib.gpu().mvfgpu_filter_create_where(fake, arr, 1, 0, None, C.byref(h)) == INV and "values is NULL" in _msg()


def test_column_calls_refuse_bad_arguments_before_any_device_call():
    lib = _lib.gpu()
    fake = C.c_void_p(1)
    vals = np.zeros(4, np.uint32)
    out = C.c_void_p()
    p = vals.ctypes.data_as(C.c_void_p)
    assert lib.mvfgpu_column_create(None, p, U32, 0, 4, C.byref(out)) == INV and "corpus is NULL" in _msg()
    assert lib.mvfgpu_column_create(fake, None, U32, 0, 4, C.byref(out)) == INV and "NULL" in _msg()
    assert lib.mvfgpu_column_create(fake, p, U32, 0, 4, None) == INV and "NULL" in _msg()
    assert lib.mvfgpu_column_create_device(None, C.c_void_p(64), U32, None, C.byref(out)) == INV and "corpus is NULL" in _msg()
    assert lib.mvfgpu_column_create_device(fake, None, U32, None, C.byref(out)) == INV and "NULL" in _msg()
    assert lib.mvfgpu_column_create_device(fake, C.c_void_p(64), U32, None, None) == INV and "NULL" in _msg()
    for dt in (0, 1, 2, 3, 6, 7):  # the vector types, StringRef, an unknown code
        assert lib.mvfgpu_column_create(fake, p, dt, 0, 4, C.byref(out)) == BUILD and "Unsupported metadata column data type" in _msg()
        assert lib.mvfgpu_column_create_device(fake, C.c_void_p(64), dt, None, C.byref(out)) == BUILD
    assert lib.mvfgpu_column_create_device(fake, C.c_void_p(68), U64, None, C.byref(out)) == INV and "aligned" in _msg()
    info = _lib.ColumnInfo()
    assert lib.mvfgpu_column_get_info(None, C.byref(info)) == INV and "column is NULL" in _msg()
    assert lib.mvfgpu_column_get_info(fake, None) == INV and "NULL" in _msg()
    info.struct_size = 0
    assert lib.mvfgpu_column_get_info(fake, C.byref(info)) == INV and "struct_size not set" in _msg()
    lib.mvfgpu_column_destroy(None)  # allowed


def test_python_layer_refuses_malformed_columns_and_clauses():
    c = G.GpuCorpus(0)
    c._h = C.c_void_p(None)   # a NULL handle: nothing may reach the library's device calls
    c._shape = (100, 4, 0)
    for bad in (np.zeros(100, np.int32), np.zeros(100, np.float32), np.zeros((10, 10), np.uint32), [1] * 100, np.zeros(99, np.uint32)):
        with pytest.raises(E.InvalidArgument):
            c.attach_column(bad)
    with pytest.raises(E.InvalidArgument):
        c.attach_column(np.zeros(104, np.uint64), first_value=5)
    with pytest.raises(E.InvalidArgument):
        c.attach_column(np.zeros(104, np.uint64), first_value=-1)
    with pytest.raises(E.InvalidArgument):
        c.attach_column_device(0, U32)
    col = G.GpuColumn(1, c)
    for bad in ([(col, "=", 3)], [(col, "==")], [("tenant", "==", 3)], [(col, "==", -1)], [(col, "in", [1, 2 ** 64])], [(col, 0, 3)]):
        with pytest.raises(E.InvalidArgument):
            c.make_filter_where(bad)
    with pytest.raises(E.InvalidArgument):
        c.make_filter_where([(col, "==", 3)], base="not a filter")
    col._h = None
    c._h = None


# ---- reader ------------------------------------------------------------------------------------------------------------

def _image_with_columns():
    """Two spaces with ids and tombstones (7 and 5 rows of 3 and 1 floats, bitmaps of 1 and 2 bytes) in front of four columns, so
    every column block starts at an odd file offset."""
    b = M.MvfBuilder()
    b.add_vector_space("a", 3, 0, 0, 0)
    b.add_vectors("a", np.arange(21, dtype=np.float32).reshape(7, 3))
    b.set_vector_ids("a", np.arange(7) + 100)
    b.set_tombstones("a", 1, bytes([0b0000101]), 2)
    b.add_vector_space("b", 1, 0, 0, 1)
    b.add_vectors("b", np.arange(5, dtype=np.float32).reshape(5, 1))
    b.set_vector_ids("b", np.arange(5) + 7)
    b.set_tombstones("b", 1, bytes([0b10000, 0]), 1)
    cols = {"tenant": (U32, np.array([7, 2 ** 32 - 1, 0], "<u4").tobytes()),
            "ts": (U64, np.array([1, 2 ** 32, TOP, 0, 5, 6, 7], "<u8").tobytes()),
            "label": (6, b"\x00\x01raw string refs\xff"),
            "short": (U32, b"\x01\x02\x03\x04\x05")}
    for name, (dt, data) in cols.items():
        b.add_metadata_column(name, dt, data)
    return b.build(), cols


def _check_columns(r, cols):
    assert r.has_metadata() and r.metadata_column_names() == list(cols)
    blocks = r.blocks()
    assert len(blocks) == 6 + len(cols)
    for i, (name, (dt, data)) in enumerate(cols.items()):
        for mc in (r.metadata_column(name), r.metadata_column_at(i)):
            assert mc.name == name and int(mc.data_type) == dt and mc.data_block_index == 6 + i and mc.null_count == 0
            assert mc.size == len(data) and mc.as_bytes() == data
            assert blocks[mc.data_block_index].size == len(data)
    assert all((4 + blocks[6 + i].offset) % 2 == 1 for i in range(len(cols))), "every column block lies at an odd file offset"
    assert r.metadata_column("tenant").values().tolist() == [7, 2 ** 32 - 1, 0] and r.metadata_column("tenant").values().dtype == np.uint32
    ts = r.metadata_column("ts").values()
    assert ts.dtype == np.uint64 and ts.tolist() == [1, 2 ** 32, TOP, 0, 5, 6, 7] and ts.flags.writeable
    with pytest.raises(E.BuildError, match="Unsupported metadata column data type"):
        r.metadata_column("label").values()
    with pytest.raises(E.BuildError, match="5 bytes"):
        r.metadata_column("short").values()
    with pytest.raises(E.VectorSpaceNotFound, match="Metadata column not found: nope"):
        r.metadata_column("nope")
    with pytest.raises(E.IndexOutOfBounds, match="4 >= 4"):
        r.metadata_column_at(4)
    # the spaces beside them read as before
    assert r.vector_space("a").total_vectors() == 7 and r.vector_space("b").vector_ids().tolist() == [7, 8, 9, 10, 11]
    r.validate_with_checksum()


def test_columns_round_trip_through_the_image(tmp_path):
    built, cols = _image_with_columns()
    image = built.to_bytes()
    with M.MvfReader.from_bytes(image) as r:
        _check_columns(r, cols)
    path = str(tmp_path / "cols.mvf")
    built.save(path)
    with M.MvfReader.open(path) as r:
        _check_columns(r, cols)
        mc = r.metadata_column("ts")
    with pytest.raises(E.InvalidArgument):
        mc.as_bytes()  # the reader is closed: the view dangles


def test_a_column_whose_block_index_is_wrong_still_opens_and_is_refused_by_the_accessor():
    built, cols = _image_with_columns()
    image = bytearray(built.to_bytes())
    with M.MvfReader.from_bytes(bytes(image)) as r:
        want = r.metadata_column("short").data_block_index
    # the footer stores the index as a u32 next to the column's type byte: patch the one u32 that holds it
    footer_len = int.from_bytes(image[-8:-4], "little")
    fs = len(image) - 8 - footer_len
    hits = [i for i in range(fs, len(image) - 12) if int.from_bytes(image[i:i + 4], "little") == want and i % 4 == fs % 4]
    opened = 0
    for i in hits:
        bad = bytearray(image)
        bad[i:i + 4] = (200).to_bytes(4, "little")
        try:
            r = M.MvfReader.from_bytes(bytes(bad))
        except E.MvfError:
            continue  # the patch hit another field of the footer
        with r:
            try:
                mc = r.metadata_column("short")
            except E.CorruptedData:
                opened += 1  # open() accepted the file, the accessor refused the column
                assert r.metadata_column_names() == list(cols) and r.metadata_column("ts").size == 56
            except E.MvfError:
                pass  # the patch hit another field of the footer
    assert opened == 1


def test_files_without_columns_still_open_and_report_none():
    b = M.MvfBuilder()
    b.add_vector_space("a", 2, 0, 0, 0)
    b.add_vectors("a", np.zeros((3, 2), np.float32))
    with M.MvfReader.from_bytes(b.build().to_bytes()) as r:
        assert not r.has_metadata() and r.metadata_column_names() == []
        with pytest.raises(E.VectorSpaceNotFound):
            r.metadata_column("tenant")
        with pytest.raises(E.IndexOutOfBounds, match="0 >= 0"):
            r.metadata_column_at(0)


def test_find_top_k_where_refuses_a_files_bad_columns_before_anything_is_uploaded():
    n = 6
    b = M.MvfBuilder()
    b.add_vector_space("s", 2, 0, 0, 0)
    b.add_vectors("s", np.zeros((n, 2), np.float32))
    b.add_metadata_column("few", U32, np.arange(n - 1, dtype="<u4").tobytes())
    b.add_metadata_column("label", 6, b"x" * (8 * n))
    with M.MvfReader.from_bytes(b.build().to_bytes()) as r:
        space = r.vector_space("s")
        q = np.zeros(2, np.float32)
        with pytest.raises(E.BuildError, match="holds 5 values, the space has 6 vectors"):
            M.find_top_k_where(space, q, 3, {"few": ("==", 1)})
        with pytest.raises(E.BuildError, match="Unsupported metadata column data type"):
            M.find_top_k_where(space, q, 3, {"label": ("==", 1)})
        with pytest.raises(E.VectorSpaceNotFound, match="Metadata column not found: nope"):
            M.find_top_k_where(space, q, 3, {"nope": ("==", 1)})
        with pytest.raises(E.BuildError, match="Unsupported distance metric"):
            M.find_top_k_where(space, q, 3, {"few": ("==", 1)}, metric=9)
