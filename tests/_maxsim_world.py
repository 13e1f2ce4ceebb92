"""What the multi-vector search's GPU test files share (tests/test_gpu_maxsim.py, tests/test_gpu_maxsim_forms.py): a corpus with
its column and partition index, and the yardstick of identity "the recipe the call replaces" -- every token through
search_grouped(per_key = 1, k = n_keys), the hits' keys from GpuColumn.gather, the per-key sum in numpy f32 in token order, the
keys ordered by (order key, key value).  Needs the binding; tests/_maxsim.py holds what needs numpy alone."""
import numpy as np

import _grouped as GR
import _maxsim as MS
import _partitioned as P
from _util import PAD
from metrovector_amd import gpu as G


class World:
    """one corpus with its column and partition index"""

    def __init__(self, dt, dim, lay, rows=None):
        self.dt, self.dim, self.lay = dt, dim, lay
        self.rows = P.make_rows(len(lay["col"]), dim, dt) if rows is None else rows
        self.c = G.GpuCorpus.from_array(self.rows)
        self.c.set_tombstones(np.packbits(lay["dead"], bitorder="little"))
        self.col = self.c.attach_column(lay["col"])
        self.part = self.c.make_partition(self.col)
        self.live = GR.live_rows(lay)
        self.keys = self.part.keys()[0] if self.live.size else np.zeros(0, np.uint64)
        self.nk = int(self.keys.size)

    def close(self):
        self.part.close()
        self.col.close()
        self.c.close()


def recipe(w, sets, metric):
    """b(t, g) of every query set, f32 [T, n_keys] in ascending key order, from the existing API: one grouped search per token"""
    nq, T, dim = sets.shape
    res = w.c.search_grouped(np.ascontiguousarray(sets.reshape(nq * T, dim)), w.nk, 1, metric, w.part)
    assert (res.indices != PAD).all(), "per_key = 1 and k = n_keys: every key's best row"
    keys = w.col.gather(res.indices)
    order = np.argsort(keys, axis=1, kind="stable")
    assert (np.take_along_axis(keys, order, 1) == w.keys[None, :]).all()
    return np.take_along_axis(res.scores, order, 1).reshape(nq, T, w.nk)


def expected(w, best, metric, k):
    """the result rows of the query sets from their b(t, g): the f32 sum in token order, (order key, key value), padding"""
    rows = [MS.rank_keys(b, w.keys, metric, k) for b in best]
    return G.MaxSimResult(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.uint32))


def same_bytes(got, want, what):
    assert got.scores.shape == want.scores.shape and got.keys.shape == want.keys.shape, what
    assert (got.keys == want.keys).all(), f"{what}: keys"
    assert (got.scores.view(np.uint32) == want.scores.view(np.uint32)).all(), f"{what}: score bits"
    assert (got.counts == want.counts).all(), f"{what}: counts"


def ks_of(w):
    return (1, 10, w.nk, w.nk + 3)


def check_sets(w, sets, metric, what, ks=None):
    """search_maxsim at every k against the recipe; -> the recipe's b(t, g)"""
    best = recipe(w, sets, metric)
    for k in ks or ks_of(w):
        got = w.c.search_maxsim(sets, k, metric, w.part)
        same_bytes(got, expected(w, best, metric, k), f"{what}, k {k}")
        assert (got.counts == min(k, w.nk)).all()
    return best
