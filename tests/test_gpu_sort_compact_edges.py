"""-m gpu tests that hold the device-wide ordering blocks at the sizes where they change their path (the radix
pass of radix_pass.h under sort_topk.hip, the block compaction of mvf_common.h under F1 and B0 / B2).

The entry sort, forced (MVF_LARGE_K = 2) and with k = n so that all n entries are sorted: 2048 | 2049 entries (one block's
LDS | the radix passes), 32 768 | 32 769 (16 tiles, whose scatter sums the tiles' counts itself | the scan launch), 131 072 |
131 073 (64 tiles of 11-bit digits | 8-bit digits).  Int8 rows of 16 small values: every score is shared by thousands of
rows, so the position order of equal keys -- the stability of every pass -- decides most of the result.

The compaction: filters (list route) and partition indexes over one row less than, exactly and one row more than a block of
each kind covers, with no row, every row and only the last row admitted."""
import os
import re

import numpy as np
import pytest

from metrovector_amd import gpu as G

from _filtered import PAD, oracle_filtered
from _util import assert_exact

pytestmark = pytest.mark.gpu
I8 = 2
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metrovector_amd", "csrc")


# ---- the entry sort at its switch points -------------------------------------------------------------------------------

SORT_N = (2048, 2049, 32_768, 32_769, 131_072, 131_073)
_TIES = {}


def _ties():
    if not _TIES:
        rng = np.random.default_rng(20)
        _TIES.update(rows=rng.integers(-3, 4, (max(SORT_N), 16)).astype(np.int8), q=rng.integers(-3, 4, (2, 16)).astype(np.int8))
    return _TIES["rows"], _TIES["q"]


def _sorted_search(oracle, monkeypatch, n, k):
    rows, q = _ties()
    monkeypatch.setenv("MVF_LARGE_K", "2")
    with G.GpuCorpus.from_array(rows[:n]) as c:
        c.set_profiling(True)
        res = c.search(q, k, G.L2)
        assert c.last_timing().scan_kernel == 8, "not the whole-shard sort"
    osc, oidx, oraw = oracle.search(rows[:n], I8, G.L2, q, k)
    ties = k - np.unique(oraw[0]).size
    assert ties > k // 2, "most entries share their key with another"
    assert_exact(res, osc, oidx, oraw)


@pytest.mark.parametrize("n", SORT_N)
def test_the_sort_of_all_entries_at_every_switch_of_its_path(oracle, monkeypatch, n):
    _sorted_search(oracle, monkeypatch, n, n)


def test_the_select_in_front_of_the_sort(oracle, monkeypatch):
    """k < n / 2: the radix select leaves 40 000 survivors (20 tiles) of 131 073 entries to the sort"""
    _sorted_search(oracle, monkeypatch, 131_073, 40_000)


# ---- the block compaction at its blocks' edges -------------------------------------------------------------------------

def _constant(header, name):
    with open(os.path.join(CSRC, header)) as fh:
        return int(re.search(rf"constexpr uint32_t {name} = (\d+);", fh.read()).group(1))


FILTER_BLOCK, PART_BLOCK = _constant("scan_filter.h", "kFilterBlockRows"), _constant("scan_partition.h", "kPartBlockRows")
EDGE_N = sorted({b + d for b in (8192, FILTER_BLOCK, PART_BLOCK) for d in (-1, 0, 1)})
ADMIT = ("none", "all", "last")


def test_the_edge_sizes_are_the_blocks_of_the_kernels():
    assert PART_BLOCK == 8192 and FILTER_BLOCK == 32_768  # a filter block is four partition blocks: both sets of edges run
    assert EDGE_N == [8191, 8192, 8193, 32_767, 32_768, 32_769]


def _admit(n, pattern):
    a = np.zeros(n, bool) if pattern != "all" else np.ones(n, bool)
    if pattern == "last":
        a[n - 1] = True
    return a


_EDGE = {}


def _edge_rows(oracle):
    if not _EDGE:
        _EDGE.update(rows=oracle.synth_rows(71, 0, max(EDGE_N), 32, I8), q=oracle.synth_queries(72, 3, 32, I8))
    return _EDGE["rows"], _EDGE["q"]


@pytest.mark.parametrize("n", EDGE_N)
def test_a_filters_row_list_at_the_block_edges(oracle, monkeypatch, n):
    rows, q = _edge_rows(oracle)
    monkeypatch.setenv("MVF_FILTER_ROUTE", "2")  # the list route: F1 compacts the admitted rows
    with G.GpuCorpus.from_array(rows[:n]) as c:
        for pattern in ADMIT:
            allow = _admit(n, pattern)
            with c.make_filter(allow) as f:
                assert f.admitted == int(allow.sum()) and f.info().has_row_list == (1 if allow.any() else 0), pattern
                res = c.search_filtered(q, 12, G.L2, f)
            assert_exact(res, *oracle_filtered(oracle, rows[:n], I8, G.L2, q, 12, allow))
            assert (res.indices != PAD).sum() == 3 * min(12, int(allow.sum())), pattern


@pytest.mark.parametrize("n", EDGE_N)
def test_a_partition_index_at_the_block_edges(oracle, n):
    rows, q = _edge_rows(oracle)
    col = (np.arange(n) % 3).astype(np.uint32)
    with G.GpuCorpus.from_array(rows[:n]) as c, c.attach_column(col) as column:
        for pattern in ADMIT:
            live = _admit(n, pattern)
            c.set_tombstones(np.packbits(~live, bitorder="little"))
            keys, counts = np.unique(col[live].astype(np.uint64), return_counts=True)
            with c.make_partition(column) as part:
                inf = part.info()
                assert (inf.live_rows, inf.n_keys, inf.largest) == (int(live.sum()), keys.size, int(counts.max(initial=0))), pattern
                gk, gc = part.keys()
                assert (gk == keys).all() and (gc == counts.astype(np.uint64)).all(), pattern
                res = c.search_partitioned(q, [0, 1, 2], 12, G.L2, part)
            for j in range(3):
                want = oracle_filtered(oracle, rows[:n], I8, G.L2, q[j], 12, live & (col == j))
                assert_exact(G.SearchResult(res.scores[j:j + 1], res.indices[j:j + 1], res.raw[j:j + 1]), *want)
