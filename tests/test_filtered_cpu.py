"""Filtered search, CPU tier: the C ABI entry points and the Python names exist, the info mirror has the header's size,
refusals precede any device call, the Python layer refuses malformed masks, the route rule holds its properties, and the
oracle restatement of the semantics (tests/_filtered.py) is pinned on hand-made masks -- including that two row-range shards
split at a row that is no multiple of 8, given the same whole-space bitmap, merge into the whole."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

from _filtered import PAD, admitted_mask, device_words, oracle_filtered, shard_bitmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT


def _msg():
    return _lib.gpu().mvfgpu_last_error_message().decode()


def _search(device=False, corpus=None, flt=None, metric=0, q=True, nq=1, k=2, sc=True, idx=True):
    qa, s, i = np.zeros(4, np.float32), np.zeros(max(nq * k, 1), np.float32), np.zeros(max(nq * k, 1), np.uint64)
    p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    lib = _lib.gpu()
    if device:
        rc = lib.mvfgpu_search_filtered_device(corpus, flt, metric, p(qa, q), 0, 4, nq, k, p(s, sc), p(i, idx), None, None)
    else:
        rc = lib.mvfgpu_search_filtered(corpus, flt, metric, p(qa, q), 0, 4, nq, k, p(s, sc), p(i, idx), None)
    return rc, _msg()


def test_entry_points_and_python_names_exist():
    lib = _lib.gpu()
    for name in ("mvfgpu_filter_create", "mvfgpu_filter_create_device", "mvfgpu_filter_destroy", "mvfgpu_filter_get_info",
                 "mvfgpu_search_filtered", "mvfgpu_search_filtered_device", "mvfgpu_selftest_filter_route"):
        assert hasattr(lib, name), name
    for name in ("make_filter", "make_filter_device", "search_filtered", "search_filtered_device"):
        assert hasattr(G.GpuCorpus, name), name
    assert hasattr(G.GpuFilter, "admitted") and hasattr(G.GpuFilter, "info") and hasattr(G.GpuFilter, "__enter__")
    assert callable(M.find_top_k_filtered) and "find_top_k_filtered" in M.__all__ and "GpuFilter" in M.__all__


def test_filter_info_mirror_has_the_headers_size(tmp_path):
    src = '#include <stdio.h>\n#include "mvf_gpu.h"\nint main(void){printf("%zu\\n", sizeof(mvfgpu_filter_info));return 0;}'
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    size = int(subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout)
    assert C.sizeof(_lib.FilterInfo) == size == 32
    assert _lib.FilterInfo().struct_size == 32


def test_the_abi_version_stays_3():
    assert _lib.gpu().mvfgpu_abi_version() == 3


def test_filter_calls_refuse_null_arguments_before_any_device_call():
    lib = _lib.gpu()
    bits = np.zeros(4, np.uint8)
    out = C.c_void_p()
    assert lib.mvfgpu_filter_create(None, bits.ctypes.data_as(C.c_void_p), 0, 32, C.byref(out)) == INV and "corpus is NULL" in _msg()
    assert lib.mvfgpu_filter_create_device(None, C.c_void_p(64), None, C.byref(out)) == INV and "corpus is NULL" in _msg()
    fake = C.c_void_p(1)  # never dereferenced: the NULL checks come first
    assert lib.mvfgpu_filter_create(fake, None, 0, 32, C.byref(out)) == INV and "NULL" in _msg()
    assert lib.mvfgpu_filter_create(fake, bits.ctypes.data_as(C.c_void_p), 0, 32, None) == INV and "NULL" in _msg()
    assert lib.mvfgpu_filter_create_device(fake, None, None, C.byref(out)) == INV and "NULL" in _msg()
    assert lib.mvfgpu_filter_create_device(fake, C.c_void_p(64), None, None) == INV and "NULL" in _msg()
    info = _lib.FilterInfo()
    assert lib.mvfgpu_filter_get_info(None, C.byref(info)) == INV and "filter is NULL" in _msg()
    lib.mvfgpu_filter_destroy(None)  # allowed
    assert lib.mvfgpu_selftest_filter_route(10, 4, 0, 1, 1, 5, None) == INV


@pytest.mark.parametrize("device", [False, True])
def test_searches_refuse_bad_arguments_before_any_device_call(device):
    fake = C.c_void_p(1)
    rc, msg = _search(device, corpus=None, flt=fake)
    assert rc == INV and "corpus is NULL" in msg
    rc, msg = _search(device, corpus=fake, flt=None)
    assert rc == INV and "filter is NULL" in msg
    rc, msg = _search(device, metric=7)
    assert rc == INV and "metric" in msg
    rc, msg = _search(device, k=0)
    assert rc == INV and "k must be" in msg
    rc, msg = _search(device, k=2**31 + 1)
    assert rc == INV and "k must be" in msg
    rc, msg = _search(device, nq=0)
    assert rc == INV and "nq" in msg
    for kw in ({"q": False}, {"sc": False}, {"idx": False}):
        rc, msg = _search(device, corpus=fake, flt=fake, **kw)
        assert rc == INV and "NULL" in msg


def test_python_layer_refuses_malformed_masks():
    c = G.GpuCorpus(0)
    c._h = C.c_void_p(None)   # a NULL handle: nothing may reach the library's device calls
    c._shape = (100, 4, 0)    # ... a shard of 100 rows
    for bad in (np.ones(99, bool),                 # one entry per row
                np.ones(101, bool),
                np.ones((10, 10), bool),           # 1-D
                np.ones(100, np.int32),            # neither bool nor packed uint8
                np.ones(100, np.float32),
                np.zeros(12, np.uint8),            # 96 bits for 100 rows
                [1] * 100):                        # a list of ints
        with pytest.raises(E.InvalidArgument):
            c.make_filter(bad)
    with pytest.raises(E.InvalidArgument):
        c.make_filter(np.zeros(13, np.uint8), first_bit=5)   # 104 bits, 105 needed
    with pytest.raises(E.InvalidArgument):
        c.make_filter(np.zeros(13, np.uint8), first_bit=-1)
    with pytest.raises(E.InvalidArgument):
        c.make_filter(np.ones(100, bool), first_bit=3)       # a bool mask has no first_bit
    with pytest.raises(E.InvalidArgument):
        c.make_filter_device(0)
    with pytest.raises(E.InvalidArgument):
        c.search_filtered(np.zeros((1, 4), np.float32), 3, G.L2, None)
    with pytest.raises(E.InvalidArgument):
        c.search_filtered(np.zeros((1, 4), np.float32), 3, G.L2, "not a filter")
    c._h = None


SHAPES = [(1_000_000, 768, 0), (10_000_000, 768, 0), (50_000_000, 768, 2), (1_000_000, 8, 0), (20_011, 96, 1), (3_000_000, 128, 3),
          (1_000_000, 33025, 2), (65_569, 8, 0)]


@pytest.mark.parametrize("rows,dim,dtype", SHAPES)
@pytest.mark.parametrize("nq", [1, 2, 5, 16, 300, 1024])
@pytest.mark.parametrize("k", [1, 100, 2048])
def test_the_route_rule_is_a_threshold_in_the_admitted_count(rows, dim, dtype, nq, k):
    """Properties, not constants: the list at and below some count, the mask above it; everything admitted is the mask."""
    counts = sorted({0, 1, 2, 1000, 1024, 1025, rows // 10000, rows // 1000, rows // 100, rows // 10, rows // 4, rows // 3, rows // 2,
                     rows - rows // 4, rows - 1, rows} | {int(rows * 2.0 ** -e) for e in range(1, 24)})
    routes = [G.filter_route(rows, dim, dtype, nq, k, a) for a in counts]
    assert set(routes) <= {1, 2}
    assert routes[-1] == 1, "a filter that admits every row takes the mask route"
    flips = [i for i in range(1, len(routes)) if routes[i] != routes[i - 1]]
    assert len(flips) <= 1 and (not flips or routes[flips[0]] == 1), f"not monotone in admitted: {list(zip(counts, routes))}"
    if nq == 1 and rows >= 1_000_000:
        assert all(r == 2 for a, r in zip(counts, routes) if a <= 1024), "a selective filter takes the list route"


def test_the_route_self_test_refuses_bad_shapes():
    lib = _lib.gpu()
    out = C.c_uint32(0)
    assert lib.mvfgpu_selftest_filter_route(10, 4, 0, 1, 1, 11, C.byref(out)) == INV      # more admitted than rows
    assert lib.mvfgpu_selftest_filter_route(10, 0, 0, 1, 1, 5, C.byref(out)) == INV
    assert lib.mvfgpu_selftest_filter_route(10, 4, 9, 1, 1, 5, C.byref(out)) == INV
    assert lib.mvfgpu_selftest_filter_route(10, 4, 0, 0, 1, 5, C.byref(out)) == INV
    assert lib.mvfgpu_selftest_filter_route(10, 4, 0, 1, 0, 5, C.byref(out)) == INV


def test_bitmap_helpers():
    allow = np.array([1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 1], bool)
    for fb in (0, 1, 7, 8, 13, 37):
        bits = shard_bitmap(allow, fb)
        assert (admitted_mask(bits, fb, allow.size) == allow).all()
        outside = np.unpackbits(bits, bitorder="little").astype(bool)
        outside[fb:fb + allow.size] = True
        assert outside.all(), "every bit outside the shard's range is set"
    dead = np.zeros(allow.size, bool)
    dead[[0, 1]] = True
    assert admitted_mask(shard_bitmap(allow, 5), 5, allow.size, dead).tolist() == (allow & ~dead).tolist()
    w = device_words(allow)
    assert w.dtype == np.uint32 and w.size == 1 and w[0] == (0xFFFFFFFF & ~0x7FF) | int(sum(1 << i for i in np.nonzero(allow)[0]))


@pytest.mark.parametrize("dtype", [G.FLOAT32, G.INT8])
@pytest.mark.parametrize("metric", [G.L2, G.INNER_PRODUCT, G.COSINE])
def test_oracle_restatement_on_hand_made_masks(oracle, dtype, metric):
    n, dim, k = 14, 5, 8
    rows = oracle.synth_rows(7, 0, n, dim, dtype)
    if dtype == G.FLOAT32:
        rows[6, 2] = np.nan  # a NaN row ranks last among the admitted
    q = oracle.synth_queries(8, 1, dim, dtype)
    sc, keys, raw = oracle.scores(rows, dtype, metric, q[0])
    dead = np.zeros(n, bool)
    dead[5] = True
    allow = np.zeros(n, bool)
    allow[[0, 3, 5, 6, 11]] = True                    # 5 is deleted: four rows admitted, k = 8 pads
    admit = admitted_mask(shard_bitmap(allow, 3), 3, n, dead)
    assert np.nonzero(admit)[0].tolist() == [0, 3, 6, 11]
    S, I, R = oracle_filtered(oracle, rows, dtype, metric, q, k, admit, index_base=100)
    live = np.array([0, 3, 6, 11])
    order = live[np.lexsort((live, keys[live]))]
    assert I[0][:4].tolist() == (order + 100).tolist() and (I[0][4:] == PAD).all()
    assert (S[0][:4].view(np.uint32) == sc[order].view(np.uint32)).all() and (R[0][:4] == raw[order]).all()
    assert (S[0][4:] == (np.inf if metric == G.L2 else -np.inf)).all()
    if dtype == G.FLOAT32 and metric != G.COSINE:
        assert I[0][3] == 106 and np.isnan(S[0][3]), "the NaN row ranks last"
    # everything admitted reproduces the oracle's search; nothing admitted is all padding
    osc, oidx, oraw = oracle.search(rows, dtype, metric, q, k)
    S, I, R = oracle_filtered(oracle, rows, dtype, metric, q, k, np.ones(n, bool))
    assert (I == oidx).all() and (R == oraw).all() and (S.view(np.uint32) == osc.view(np.uint32)).all()
    S, I, R = oracle_filtered(oracle, rows, dtype, metric, q, k, np.zeros(n, bool))
    assert (I == PAD).all() and (R == 0).all() and np.isinf(S).all()
    # ids are reported where attached
    ids = np.arange(n, dtype=np.uint64) * 3 + 1000
    S, I, R = oracle_filtered(oracle, rows, dtype, metric, q, k, admit, ids=ids)
    assert sorted(I[0][:4].tolist()) == [1000, 1009, 1018, 1033]


@pytest.mark.parametrize("dtype", [G.FLOAT32, G.UINT8])
@pytest.mark.parametrize("metric", [G.L2, G.COSINE])
def test_two_shards_given_the_whole_bitmap_merge_into_the_whole(oracle, dtype, metric):
    n, dim, nq, k, cut = 61, 6, 4, 9, 27   # the split row is no multiple of 8
    rows = oracle.synth_rows(11, 0, n, dim, dtype)
    qs = oracle.synth_queries(12, nq, dim, dtype)
    rng = np.random.default_rng(3)
    allow = rng.random(n) < 0.4
    dead = rng.random(n) < 0.2
    bits = np.packbits(allow, bitorder="little")   # ONE bitmap over the whole space
    whole = oracle_filtered(oracle, rows, dtype, metric, qs, k, admitted_mask(bits, 0, n, dead))
    per = []
    for a, b in ((0, cut), (cut, n)):
        admit = admitted_mask(bits, a, b - a, dead[a:b])
        assert (admit == (allow & ~dead)[a:b]).all()
        per.append(oracle_filtered(oracle, rows[a:b], dtype, metric, qs, k, admit, index_base=a))
    merged = G.merge_topk_host(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), metric, dtype)
    assert (merged.indices == whole[1]).all() and (merged.raw == whole[2]).all()
    assert (merged.scores.view(np.uint32) == whole[0].view(np.uint32)).all()
