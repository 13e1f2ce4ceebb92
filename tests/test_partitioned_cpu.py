"""Partitioned search, CPU tier (DESIGN.md §3 "Partitioned search"): the library exports the new entry points and Python
names them, the ctypes mirror of mvfgpu_partition_info has the compiler's size, the plan is the pure function the contract
states, every refusal that needs no handle precedes any device call, and the test layout (tests/_partitioned.py) is what the
GPU tests take it for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import metrovector_amd as M
from metrovector_amd import _lib
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

import _partitioned as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 12  # MVF_ERR_INVALID_ARGUMENT


def _msg():
    return _lib.gpu().mvfgpu_last_error_message().decode()


def test_entry_points_and_python_names_exist():
    lib = _lib.gpu()
    for name in ("mvfgpu_partition_create", "mvfgpu_partition_destroy", "mvfgpu_partition_get_info", "mvfgpu_partition_lookup",
                 "mvfgpu_partition_keys", "mvfgpu_search_partitioned", "mvfgpu_search_partitioned_device",
                 "mvfgpu_selftest_partition_plan"):
        assert hasattr(lib, name), name
    for name in ("make_partition", "search_partitioned", "search_partitioned_device"):
        assert hasattr(G.GpuCorpus, name), name
    for name in ("info", "lookup", "keys", "close", "__enter__", "__exit__"):
        assert hasattr(G.GpuPartition, name), name
    for name in ("find_top_k_per_key", "GpuPartition"):
        assert name in M.__all__ and hasattr(M, name), name
    assert "find_top_k_per_key" in open(os.path.join(ROOT, "include", "mvf.hpp")).read()
    assert _lib.gpu().mvfgpu_abi_version() == 3, "an additive change: the ABI version stays"


def test_the_ctypes_mirror_has_the_compilers_size(tmp_path):
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include "mvf_gpu.h"\nint main(void){'
                                  'printf("%zu\\n", sizeof(mvfgpu_partition_info));return 0;}')
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    size = int(subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout)
    assert C.sizeof(_lib.PartitionInfo) == size == 56 and _lib.PartitionInfo().struct_size == 56


def test_the_plan_is_the_contracts_function_of_counts_and_k():
    counts, keys = [0, 1, 1024, 1025], [10, 11, 12, 13]
    tier, groups = G.partition_plan(counts, keys, 1024)
    assert tier.tolist() == [0, 1, 1, 2] and groups == 1
    tier, groups = G.partition_plan(counts, keys, 1025)
    assert tier.tolist() == [0, 2, 2, 2] and groups == 3
    tier, groups = G.partition_plan(counts, keys, 1)
    assert tier.tolist() == [0, 1, 1, 2] and groups == 1


def test_the_large_tier_makes_one_group_per_distinct_key():
    # seven queries on three large keys (one of them repeated four times, not adjacent), two small, one absent
    counts = [3000, 5, 3000, 2000, 0, 3000, 1025, 3000, 1024, 2000]
    keys = [7, 1, 7, 9, 4, 7, 2 ** 63, 7, 3, 9]
    tier, groups = G.partition_plan(counts, keys, 10)
    assert tier.tolist() == [2, 1, 2, 2, 0, 2, 2, 2, 1, 2]
    assert groups == 3, "distinct large keys, not large queries"
    tier, groups = G.partition_plan(counts, keys, 1025)  # beyond one pass every scored query is large: keys 7, 1, 9, 2^63, 3
    assert tier.tolist() == [2, 2, 2, 2, 0, 2, 2, 2, 2, 2] and groups == 5
    tier, groups = G.partition_plan([0, 0], [1, 1], 10)
    assert tier.tolist() == [0, 0] and groups == 0
    # keys that differ only in the high half are different groups
    assert G.partition_plan([2000, 2000], [(5 << 32) | 77, (6 << 32) | 77], 10)[1] == 2


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.gpu()
    h, inf = C.c_void_p(), _lib.PartitionInfo()
    one = np.zeros(4, np.uint64)
    p1 = one.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(16)  # never dereferenced: the NULL argument is found first
    calls = {
        "create(corpus)": lambda: lib.mvfgpu_partition_create(None, fake, C.byref(h)),
        "get_info(partition)": lambda: lib.mvfgpu_partition_get_info(None, C.byref(inf)),
        "lookup(partition)": lambda: lib.mvfgpu_partition_lookup(None, p1, 1, p1),
        "keys(partition)": lambda: lib.mvfgpu_partition_keys(None, 0, 1, p1, p1),
        "search(metric first, then nq, k, buffers)": lambda: lib.mvfgpu_search_partitioned(None, None, 0, None, 0, 4, 1, p1, 1, None, None, None),
        "search(keys)": lambda: lib.mvfgpu_search_partitioned(None, None, 0, p1, 0, 4, 1, None, 1, p1, p1, None),
        "search(partition)": lambda: lib.mvfgpu_search_partitioned(None, None, 0, p1, 0, 4, 1, p1, 1, p1, p1, None),
        "search_device(keys)": lambda: lib.mvfgpu_search_partitioned_device(None, None, 0, p1, 0, 4, 1, None, 1, p1, p1, None, None),
        "search_device(partition)": lambda: lib.mvfgpu_search_partitioned_device(None, None, 0, p1, 0, 4, 1, p1, 1, p1, p1, None, None),
        "plan(counts)": lambda: lib.mvfgpu_selftest_partition_plan(None, p1, 1, 1, p1, p1),
        "plan(keys)": lambda: lib.mvfgpu_selftest_partition_plan(p1, None, 1, 1, p1, p1),
        "plan(out_tier)": lambda: lib.mvfgpu_selftest_partition_plan(p1, p1, 1, 1, None, p1),
        "plan(out_groups)": lambda: lib.mvfgpu_selftest_partition_plan(p1, p1, 1, 1, p1, None),
    }
    for what, call in calls.items():
        assert call() == INV, what
        assert _msg(), what
    lib.mvfgpu_partition_destroy(None)  # allowed
    assert lib.mvfgpu_search_partitioned(None, None, 0, p1, 0, 4, 1, None, 1, p1, p1, None) == INV and "keys" in _msg()
    assert lib.mvfgpu_search_partitioned(None, None, 0, p1, 0, 4, 1, p1, 1, p1, p1, None) == INV and "partition is NULL" in _msg()
    assert lib.mvfgpu_search_partitioned(None, None, 9, p1, 0, 4, 1, p1, 1, p1, p1, None) == INV and "metric" in _msg()
    assert lib.mvfgpu_search_partitioned(None, None, 0, p1, 0, 4, 0, p1, 1, p1, p1, None) == INV and "nq" in _msg()
    assert lib.mvfgpu_search_partitioned(None, None, 0, p1, 0, 4, 1, p1, 0, p1, p1, None) == INV and "k must be" in _msg()
    with pytest.raises(E.InvalidArgument):
        G.partition_plan([1, 2], [1], 10)


@pytest.mark.parametrize("flavour", ["u32", "u64"])
def test_the_layout_is_what_the_gpu_tests_take_it_for(flavour):
    lay = P.layout(flavour)
    assert lay["col"].dtype == P.NP_OF[flavour] and lay["col"].size == P.N
    assert [P.reference_rows(lay, k).size for k in lay["keys"]] == list(P.LIVE_SIZES)
    assert P.reference_rows(lay, lay["dead_key"]).size == 0 and (lay["col"] == lay["dead_key"]).sum() > 100
    assert P.reference_rows(lay, lay["absent_key"]).size == 0 and not (lay["col"] == lay["absent_key"]).any()
    keys, counts = P.group_by(lay)
    assert keys.size == len(P.LIVE_SIZES) + P.FURTHER and int(counts.sum()) == int((~lay["dead"]).sum()) == P.N - 820
    assert lay["dead_key"] not in keys.tolist()
    for v in P.SPECIAL[flavour]:
        assert v in keys.tolist(), hex(v)
    big = P.reference_rows(lay, lay["keys"][0])
    assert big[0] < 64 and big[-1] > P.N - 64, "a partition is scattered over the whole position range"
    assert (lay["dead"] & (lay["col"] == lay["keys"][0])).any(), "deleted rows inside a live partition"
    mk = P.mixed_keys(lay, 64)
    assert set(lay["keys"]) | {lay["absent_key"], lay["dead_key"]} <= set(mk.tolist()) and len(set(mk.tolist())) < 64
