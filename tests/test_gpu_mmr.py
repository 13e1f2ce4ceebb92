"""Diversified re-ranking on the GPU (mvfgpu_search_mmr[_device], include/mvf_gpu_mmr.h; DESIGN.md §3 "Diversified
re-ranking", §5 "D0"): every output byte -- score bits, picks, raw, objective bits, counts -- against the recipe of
tests/_mmr.py (the library's own candidate searches of the query and of the candidates' rows as queries, then the walk in numpy
float32), the identities of the contract, the oracle on the integer types, and a planted world where diversification shows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from metrovector_amd import _lib
from metrovector_amd import gpu as G

import _mmr as MM
import _stream_scenarios as SC
import _streams as S
from _candidates import PAD, candidate_rows
from _children import RUNNER

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DTYPES = [G.FLOAT32, G.FLOAT16, G.INT8, G.UINT8]
METRICS = [G.L2, G.INNER_PRODUCT, G.COSINE]
DIMS = [20, 128, 770]           # a row that is no multiple of 16 bytes, one lane-group step, several steps
MS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024]   # the wave and block edges of the argmax and of the ownership
LAMBDAS = [0.0, 0.3, 0.5, 1.0]
N = 3001
INV = 12


@pytest.fixture(scope="module")
def worlds(oracle):
    """(rows, handle) per (data type, dimension), made on first use and closed with the module"""
    made = {}

    def get(dtype, dim):
        if (dtype, dim) not in made:
            rows = oracle.synth_rows(1900 + dim + dtype, 0, N, dim, dtype)
            made[(dtype, dim)] = (rows, G.GpuCorpus.from_array(rows))
        return made[(dtype, dim)]

    yield get
    for _, c in made.values():
        c.close()


def _lists(rng, n, nq, m):
    """query 0: m distinct live rows (count = m, the edge itself); the others: foreign entries, repeats and pads"""
    lists = rng.integers(0, n + n // 10, size=(nq, m)).astype(np.uint64)
    if m > 4:
        lists[:, ::7] = PAD
    lists[0] = rng.permutation(n)[:m]
    return lists


def _ks(m):
    return [1, 5, m, m + 3]


def _check(c, metric, qs, lists, k, lam, res=None, which=None, what=""):
    res = c.search_mmr(qs, lists, k, lam, metric) if res is None else res
    assert res.scores.shape == res.indices.shape == res.raw.shape == res.objective.shape == (qs.shape[0], k)
    for j in (range(qs.shape[0]) if which is None else which):
        MM.assert_rows_equal(res, MM.recipe(c, metric, qs[j], lists[j], k, lam), j, what)
    return res


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_matrix(oracle, worlds, dtype, dim):
    """Identity 1.  Every m with every data type and dimension; the metric, k, lambda and nq rotate so that each (data type, m)
    meets all three metrics over the three dimensions, and each m all four k and lambda."""
    rows, c = worlds(dtype, dim)
    di = DIMS.index(dim)
    rng = np.random.default_rng(dim * 31 + dtype)
    for mi, m in enumerate(MS):
        metric = METRICS[(mi + di) % 3]
        k = _ks(m)[(mi + di + dtype) % 4]
        lam = LAMBDAS[(mi + 2 * di + dtype) % 4]
        nq = 5 if (mi + di) % 2 else 1
        qs = oracle.synth_queries(2000 + mi + 16 * di, nq, dim, dtype)
        lists = _lists(rng, N, nq, m)
        res = _check(c, metric, qs, lists, k, lam, what=f"m {m} metric {metric} k {k} lambda {lam}")
        assert int(res.counts[0]) == m


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_k_and_lambda_at_one_shape(oracle, worlds, dtype, metric):
    """every k and lambda of the matrix for each data type and metric, m = 257 (two positions in a thread's set)"""
    rows, c = worlds(dtype, 128)
    m, nq = 257, 2
    rng = np.random.default_rng(5 + dtype + 4 * metric)
    qs = oracle.synth_queries(2100 + dtype, nq, 128, dtype)
    lists = _lists(rng, N, nq, m)
    for i, k in enumerate(_ks(m)):
        for lam in (LAMBDAS if i == 1 else [LAMBDAS[i]]):
            _check(c, metric, qs, lists, k, lam, what=f"k {k} lambda {lam}")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lambda_one_reproduces_the_candidate_search(oracle, worlds, dtype, metric):
    """Identity 2 (finite scores)"""
    for dim in (20, 128):
        rows, c = worlds(dtype, dim)
        nq, m, k = 4, 300, 40
        qs = oracle.synth_queries(2200 + dim, nq, dim, dtype)
        lists = _lists(np.random.default_rng(dim + metric), N, nq, m)
        got = c.search_mmr(qs, lists, k, 1.0, metric)
        want = c.search_candidates(qs, lists, k, metric)
        assert np.isfinite(want.scores).all()
        for name in ("scores", "indices", "raw", "counts"):
            assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_permutations_and_repeats_change_no_byte(oracle, worlds, dtype):
    """Identity 3"""
    rows, c = worlds(dtype, 128)
    nq, m, k = 3, 500, 60
    rng = np.random.default_rng(33 + dtype)
    qs = oracle.synth_queries(2300, nq, 128, dtype)
    lists = _lists(rng, N, nq, m)
    perm = np.stack([np.concatenate([l[rng.permutation(m)], l[rng.integers(0, m, 300)]]) for l in lists])
    for metric in METRICS:
        a = c.search_mmr(qs, lists, k, 0.3, metric)
        for other in (c.search_mmr(qs, lists, k, 0.3, metric), c.search_mmr(qs, perm, k, 0.3, metric)):
            for name in ("scores", "indices", "raw", "counts", "objective"):
                assert getattr(other, name).tobytes() == getattr(a, name).tobytes(), (metric, name)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", [G.INT8, G.UINT8])
def test_the_walk_on_the_oracle_s_scores(oracle, worlds, dtype, metric):
    """Identity 4: the integer types against the oracle, which is bit-exact there"""
    rows, c = worlds(dtype, 128)
    nq, m, k, lam = 2, 150, 30, 0.3
    qs = oracle.synth_queries(2400 + metric, nq, 128, dtype)
    lists = _lists(np.random.default_rng(44 + metric), N, nq, m)
    res = c.search_mmr(qs, lists, k, lam, metric)
    for j in range(nq):
        sel = candidate_rows(lists[j], N)
        sc, keys, raw = oracle.scores(rows, dtype, metric, qs[j])
        first = int(np.lexsort((sel, keys[sel]))[0])
        sim = np.stack([oracle.scores(rows, dtype, metric, rows[s])[0][sel] for s in sel])
        order, obj = MM.numpy_walk(metric, sc[sel], sim, lam, k, first=first)
        raws = raw[sel] if metric != G.COSINE else np.zeros(sel.size, np.int32)
        MM.assert_rows_equal(res, MM.format_picks(metric, k, order, obj, sc[sel], sel.astype(np.uint64), raws, sel.size), j, "oracle")


def test_planted_copies():
    """What the feature is for: 8 exact copies of the best row among 64 candidates.  Relevance alone ranks the copies 0..7;
    lambda = 0.5 keeps one and fills the other 15 ranks with other rows."""
    rows, q, lst, copies = MM.planted_world()
    k = 16
    with G.GpuCorpus.from_array(rows) as c:
        plain = c.search_candidates(q[None, :], lst[None, :], k, G.COSINE)
        one = c.search_mmr(q[None, :], lst[None, :], k, 1.0, G.COSINE)
        half = c.search_mmr(q[None, :], lst[None, :], k, 0.5, G.COSINE)
        assert sorted(plain.indices[0][:8].tolist()) == copies.tolist()
        assert one.indices.tobytes() == plain.indices.tobytes() and one.scores.tobytes() == plain.scores.tobytes()
        assert np.nonzero(np.isin(one.indices[0], copies))[0].tolist() == list(range(8)), "lambda = 1: the copies hold ranks 0..7"
        assert np.nonzero(np.isin(half.indices[0], copies))[0].tolist() == [0], "lambda = 0.5: exactly one copy, at rank 0"
        assert int((half.indices[0] != plain.indices[0]).sum()) == 15, "15 of 16 ranks differ from the candidate search's"
        assert len(set(half.indices[0].tolist())) == k and np.isin(half.indices[0], lst).all()
        MM.assert_rows_equal(half, MM.recipe(c, G.COSINE, q, lst, k, 0.5), 0, "planted")


def test_edge_lists(oracle):
    """pads, entries outside the shard, deleted rows and index_base != 0 (host and device call); k beyond the count"""
    import torch
    n, dim, base = 3001, 24, 1_000_000
    rows = oracle.synth_rows(2501, 0, n, dim, G.FLOAT32)
    dead = np.zeros(n, bool)
    dead[[13, 500, 2000]] = True
    qs = oracle.synth_queries(2502, 3, dim, G.FLOAT32)
    rng = np.random.default_rng(25)
    m = 200
    lists = (rng.integers(0, n, size=(3, m)) + base).astype(np.uint64)
    lists[:, 5:11] = np.array([13, 500, 2000, 13, 7, 7], np.uint64) + np.uint64(base)
    lists[:, 20:60] = PAD
    lists[:, 60:80] = np.uint64(base + n) + np.arange(20, dtype=np.uint64)        # past the shard
    lists[:, 80:90] = np.uint64(base - 5) + np.arange(10, dtype=np.uint64) % 5    # in front of it
    lists[2, :] = PAD
    lists[2, 3] = base + 13                                                       # a deleted row only: count 0
    with G.GpuCorpus.from_array(rows, index_base=base) as c:
        c.set_tombstones(np.packbits(dead, bitorder="little"))
        for metric in METRICS:
            for k in (7, m + 3):
                res = _check(c, metric, qs, lists, k, 0.3, what=f"metric {metric} k {k}")
                cnt = [candidate_rows(l, n, index_base=base, dead=dead).size for l in lists]
                assert res.counts.tolist() == cnt and cnt[2] == 0
                assert (res.indices[2] == PAD).all() and (res.objective[2] == MM.pad_score(metric)).all()
                assert not np.isin(res.indices, np.array([13, 500, 2000], np.uint64) + np.uint64(base)).any()
                dq, dl = torch.from_numpy(qs).cuda(), torch.from_numpy(lists.view(np.int64)).cuda()
                ds, do = (torch.empty((3, k), dtype=torch.float32, device="cuda") for _ in range(2))
                di = torch.empty((3, k), dtype=torch.int64, device="cuda")
                dr = torch.empty((3, k), dtype=torch.int32, device="cuda")
                dc = torch.empty(3, dtype=torch.int64, device="cuda")
                st = torch.cuda.Stream()
                c.search_mmr_device(dq.data_ptr(), G.FLOAT32, dim, 3, dl.data_ptr(), m, k, 0.3, metric, ds.data_ptr(), di.data_ptr(),
                                    dr.data_ptr(), do.data_ptr(), dc.data_ptr(), st.cuda_stream)
                st.synchronize()
                assert di.cpu().numpy().view(np.uint64).tobytes() == res.indices.tobytes()
                assert ds.cpu().numpy().tobytes() == res.scores.tobytes() and do.cpu().numpy().tobytes() == res.objective.tobytes()
                assert dr.cpu().numpy().tobytes() == res.raw.tobytes() and dc.cpu().numpy().view(np.uint64).tobytes() == res.counts.tobytes()
                # the nullable outputs left out: the same picks
                ds2, di2 = torch.empty_like(ds), torch.empty_like(di)
                c.search_mmr_device(dq.data_ptr(), G.FLOAT32, dim, 3, dl.data_ptr(), m, k, 0.3, metric, ds2.data_ptr(), di2.data_ptr(),
                                    stream=st.cuda_stream)
                st.synchronize()
                assert torch.equal(di2, di) and ds2.cpu().numpy().tobytes() == res.scores.tobytes()


def test_ids_nothing_listed_and_null_outputs(oracle):
    n, dim = 3001, 24
    rows = oracle.synth_rows(2601, 0, n, dim, G.INT8)
    ids = np.arange(n, dtype=np.uint64) * 11 + 7
    qs = oracle.synth_queries(2602, 4, dim, G.INT8)
    rng = np.random.default_rng(26)
    pos = rng.integers(0, n, size=(4, 300)).astype(np.uint64)
    pos[:, :4] = PAD
    lists = np.where(pos == PAD, PAD, ids[np.minimum(pos, np.uint64(n - 1)).astype(np.int64)])
    lists[:, 1] = 3            # an id nobody holds
    with G.GpuCorpus.from_array(rows) as c, G.GpuCorpus.from_array(rows) as plain:
        c.set_vector_ids(ids)
        for metric in METRICS:
            got = c.search_mmr(qs, lists, 50, 0.5, metric)
            want = _check(plain, metric, qs, pos, 50, 0.5, what="positions")
            real = want.indices != PAD
            assert (got.indices[real] == ids[want.indices[real].astype(np.int64)]).all() and (got.indices[~real] == PAD).all()
            for name in ("scores", "raw", "counts", "objective"):
                assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), (metric, name)
        # m = 0: padding and counts 0
        empty = c.search_mmr(qs, np.zeros((4, 0), np.uint64), 3, 0.5, G.L2)
        assert (empty.counts == 0).all() and (empty.indices == PAD).all() and (empty.scores == np.inf).all()
        assert (empty.raw == 0).all() and (empty.objective == np.inf).all()
        assert int(c.search_mmr(qs[:1], np.full((1, 8), PAD, np.uint64), 3, 0.5, G.INNER_PRODUCT).counts[0]) == 0
        # out_raw, out_objective and out_counts NULL in the host call
        full = plain.search_mmr(qs, pos, 9, 0.5, G.L2)
        sc, idx = np.empty((4, 9), np.float32), np.empty((4, 9), np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        q = np.ascontiguousarray(qs)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_mmr(plain._h, G.L2, p(q), G.INT8, dim, 4, p(pos), pos.shape[1], 9, 0.5, p(sc), p(idx),
                                                    None, None, None))
        assert sc.tobytes() == full.scores.tobytes() and idx.tobytes() == full.indices.tobytes()


def test_edge_values(oracle):
    """a candidate row holding NaN, a NaN query, zero rows under Cosine, a picked row holding inf: the rules via the recipe"""
    n, dim = 3001, 40
    for dtype in (G.FLOAT32, G.FLOAT16):
        rows = oracle.synth_rows(2701, 0, n, dim, dtype)
        rows[10, 3] = np.nan
        rows[11] = 0
        rows[12] = 0
        rows[14, :] = np.abs(rows[14, :])
        rows[14, 0] = np.inf      # under InnerProduct with a positive query element: score +inf, picked first
        qs = np.abs(oracle.synth_queries(2702, 3, dim, dtype)) + np.float32(0.01)
        qs[2, 5] = np.nan         # a NaN query: every rel is NaN
        lists = np.random.default_rng(27).integers(0, n, size=(3, 120)).astype(np.uint64)
        lists[:, :5] = [10, 11, 12, 14, 10]
        with G.GpuCorpus.from_array(rows) as c:
            for metric in METRICS:
                for lam in (0.0, 0.5, 1.0):
                    res = _check(c, metric, qs, lists, 122, lam, what=f"dtype {dtype} metric {metric} lambda {lam}")
                    assert res.counts.tolist() == [candidate_rows(l, n).size for l in lists]
            res = c.search_mmr(qs[:1], lists[:1], 5, 0.5, G.INNER_PRODUCT)
            assert res.indices[0][0] == 14 and np.isposinf(res.scores[0][0]), "the row holding inf is picked first"


@pytest.mark.parametrize("dtype", [G.FLOAT32, G.FLOAT16])
def test_a_query_larger_than_lds(oracle, dtype):
    """dimension 20000 (tests/test_gpu_candidates.py test_a_query_larger_than_lds): the padded picked row takes 80 KiB, beyond the
    40 KiB the kernels keep in LDS -- D0 reads it back from the query's scratch row.  70 candidates are 70 lane groups of 64
    lanes: every wave scores, in two passes of its loop, and 12 picks rewrite the scratch row eleven times while other waves have
    read it (tests/test_gpu_mmr_forms.py holds both sides of the switch itself)"""
    n, dim, m, k = 300, 20000, 70, 12
    rows = oracle.synth_rows(2801, 0, n, dim, dtype)
    qs = oracle.synth_queries(2802, 2, dim, dtype)
    lists = np.stack([np.random.default_rng(28 + j).permutation(n)[:m] for j in range(2)]).astype(np.uint64)
    with G.GpuCorpus.from_array(rows) as c:
        for metric in METRICS:
            _check(c, metric, qs, lists, k, 0.5, what=f"metric {metric}")


def test_a_second_window_of_queries(oracle):
    """mmr.hip windows a call's queries at min(1024, 512 MiB / (12 m + 4)) = 1024 for m = 1024 on a dim-16 corpus: 1025 queries
    are windows of 1024 and 1"""
    n, dim, m, k, nq = 3001, 16, 1024, 3, 1025
    assert min(1024, (512 << 20) // (12 * m + 4)) == 1024 < nq
    rows = oracle.synth_rows(2901, 0, n, dim, G.FLOAT32)
    qs = oracle.synth_queries(2902, nq, dim, G.FLOAT32)
    lists = np.random.default_rng(29).integers(0, n, size=(nq, m)).astype(np.uint64)
    with G.GpuCorpus.from_array(rows) as c:
        res = _check(c, G.L2, qs, lists, k, 0.5, which=(0, 1023, 1024))
        assert (res.indices != PAD).all() and (res.counts > 800).all()


@pytest.fixture(scope="module")
def streams(oracle):
    """(s1, s2) for which both controls of tests/_streams.py hold"""
    rows = np.ascontiguousarray(oracle.synth_rows(7, 0, 4000, SC.DIM[SC.F32], SC.F32))
    q = np.ascontiguousarray(oracle.synth_queries(8, 1, SC.DIM[SC.F32], SC.F32))
    try:
        return S.pick_streams(lambda: G.GpuCorpus.from_array(rows), q)
    except S.ControlFailed as e:
        pytest.skip(str(e))


class MmrDev(SC.CandHost):
    entry, is_async = "mvfgpu_search_mmr_device", True

    def __init__(self, q, cand, k, metric, lam):
        super().__init__(q, cand, k, metric)
        self.lam = lam

    def prepare(self, ctx):
        import torch
        nq = self.q.shape[0]
        self.t = (SC._dev(self.q), SC._dev(self.cand)) + SC._outs(nq, self.k) + (
            torch.zeros((nq, self.k), dtype=torch.float32, device="cuda"), torch.zeros(nq, dtype=torch.int64, device="cuda"))

    def issue(self, ctx, stream):
        dq, dc, ds, di, dr, do, dn = self.t
        ctx.c.search_mmr_device(dq.data_ptr(), G.query_dtype_code(ctx.c.data_type), self.q.shape[1], self.q.shape[0], dc.data_ptr(),
                                self.cand.shape[1], self.k, self.lam, self.metric, ds.data_ptr(), di.data_ptr(), dr.data_ptr(),
                                do.data_ptr(), dn.data_ptr(), stream=SC._sp(stream))
        return lambda: dict(SC._read(ds, di, dr), objective=do.cpu().numpy().view(np.uint32), counts=dn.cpu().numpy().view(np.uint64))


def test_stream_order_behind_a_pending_batched_search(oracle, streams):
    """The device call on a second stream while a batched mvfgpu_search_device of the same handle (it builds the row norms) is
    pending behind a stall: S.run_pair asserts the stall pending when the call is issued and when it returns -- the call is
    asynchronous --, and both calls give the bytes of a run with a full synchronise between them."""
    sid = "entry:f32:mmr:dev"
    seed = SC._seed_of(sid)
    dim = SC.DIM[SC.F32]
    rows = np.ascontiguousarray(oracle.synth_rows(seed, 0, SC.N, dim, SC.F32))
    producer = SC.SearchDev(np.ascontiguousarray(oracle.synth_queries(seed + 3, 128, dim, SC.F32)), 2 * SC.K, SC.IP, 2, SC.KERNEL[(2, SC.F32)])
    qb = np.ascontiguousarray(oracle.synth_queries(seed + 2, 5, dim, SC.F32))
    cand = np.random.default_rng(seed).integers(0, SC.N, (5, 300)).astype(np.uint64)
    consumer = MmrDev(qb, cand, SC.K, SC.IP, 0.5)
    sc = SC.Scenario(sid, SC.F32, seed, producer, consumer, rows=rows)
    gp, gc, rp, rc = SC.run(sc, streams)
    for got, ref, what in ((gp, rp, "the producer"), (gc, rc, "the consumer")):
        assert sorted(got) == sorted(ref)
        for name in ref:
            assert np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(ref[name]).tobytes(), f"{what}: {name}"
    with G.GpuCorpus.from_array(rows) as c:
        res = G.MmrResult(rc["scores"].view(np.float32), rc["indices"], rc["raw"], rc["counts"], rc["objective"].view(np.float32))
        for j in (0, 4):
            MM.assert_rows_equal(res, MM.recipe(c, SC.IP, qb[j], cand[j], SC.K, 0.5), j, "reference")


def test_a_fresh_poisoned_process(tmp_path):
    """tests/_mmr.py as a child whose first search is the diversified re-ranking, with every allocation of the library poisoned
    with 0x00 and with 0xFF: the bytes of this process' call and of the recipe; one child at a time, none after a fault"""
    rows, queries, lists = MM.fresh_inputs()
    with G.GpuCorpus.from_array(rows) as c:
        want = _check(c, MM.FP_METRIC, queries, lists, MM.FP_K, MM.FP_LAMBDA, which=(0, MM.FP_NQ - 1))
    for poison in (0, 255):
        env = {k: v for k, v in os.environ.items() if k != "MVF_DEBUG_POISON"}
        env["MVF_DEBUG_POISON"] = str(poison)
        path = str(tmp_path / f"poison{poison}.npz")
        out = RUNNER.run([sys.executable, os.path.join(HERE, "_mmr.py"), path], env=env)
        assert out.returncode == 0, f"poison {poison}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
        with np.load(path) as z:
            assert z["poison"].tolist() == [poison], "the child ran poisoned (mvfgpu_selftest_poison)"
            for name in ("scores", "indices", "raw", "objective", "counts"):
                assert z[name].tobytes() == getattr(want, name).tobytes(), f"poison {poison}: {name}"


def _raw_call(c, device, lam=0.5, m=3):
    qa, ca = np.zeros(4, np.float32), np.zeros(max(m, 1), np.uint64)
    s, i = np.zeros(2, np.float32), np.zeros(2, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lib = _lib.gpu()
    if device:
        rc = lib.mvfgpu_search_mmr_device(c._h, 0, p(qa), 0, 4, 1, p(ca), m, 2, lam, p(s), p(i), None, None, None, None)
    else:
        rc = lib.mvfgpu_search_mmr(c._h, 0, p(qa), 0, 4, 1, p(ca), m, 2, lam, p(s), p(i), None, None, None)
    return rc, lib.mvfgpu_last_error_message().decode()


@pytest.mark.parametrize("device", [False, True])
def test_refusals_on_a_live_handle(device):
    """behind the candidate search's checks: lambda, then the list length -- host pointers even in the device form: a refusal
    reads nothing and leaves no device error"""
    import torch
    rows = np.arange(32, dtype=np.float32).reshape(8, 4)
    with G.GpuCorpus.from_array(rows) as c:
        for lam in (float("nan"), -0.25, 1.5):
            rc, msg = _raw_call(c, device, lam=lam, m=5000)
            assert rc == INV and "lambda" in msg, (lam, msg)
        rc, msg = _raw_call(c, device, m=1025)
        assert rc == INV and "MVFGPU_MMR_MAX_CANDIDATES" in msg and "1025" in msg
        torch.cuda.synchronize()   # raises where a refusal left an error on the device
        res = c.search_mmr(rows[:1], np.array([[0, 1, 2, 3]], np.uint64), 2, 0.5, G.L2)
        assert res.indices[0][0] == 0 and int(res.counts[0]) == 4


def _space(rows, metric):
    from metrovector_amd import MvfBuilder, MvfReader
    from metrovector_amd.reader import VectorType
    b = MvfBuilder()
    b.add_vector_space("emb", rows.shape[1], VectorType.Dense, metric, G.FLOAT32)
    b.add_vectors_raw("emb", rows)
    return MvfReader.from_bytes(b.build().to_bytes()).vector_space("emb")


def test_find_top_k_diverse_is_its_two_call_composition():
    from metrovector_amd import diversify_top_k, find_top_k_diverse, find_top_k_similar_batch
    rows, q, lst, copies = MM.planted_world(n=600)
    space = _space(rows, G.COSINE)
    qs = np.stack([q, rows[5]])
    got = find_top_k_diverse(space, qs, 10, 40, 0.5, with_vectors=True)
    top = find_top_k_similar_batch(space, qs, 40)
    cand = np.array([[h.index for h in hits] for hits in top], np.uint64)
    want = diversify_top_k(space, qs, cand, 10, 0.5)
    for a, b in zip(got, want):
        assert [h.index for h in a] == [h.index for h in b] and len(a) == 10
        assert [np.float32(h.score).view(np.uint32) for h in a] == [np.float32(h.score).view(np.uint32) for h in b]
        assert all((h.vector == rows[h.index]).all() for h in a)
    assert sum(int(h.index) in set(copies.tolist()) for h in got[0]) == 1, "one of the planted copies among the diverse ten"
    assert [h.index for h in got[0]] != [h.index for h in top[0][:10]]


CPP = r'''
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "mvf.hpp"
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    auto reader = mvf::MvfReader::open(argv[1]);
    auto space = reader.vector_space(reader.vector_space_names()[0]);
    mvf::GpuVectorSpace gs(space);
    std::vector<float> q = {1.0f, 1.0f, 1.0f, 1.0f};
    std::vector<uint64_t> cand = {5, 3, 3, 59, 58, 1000, ~0ull, 0, 17, 20, 21, 40, 41};
    for (const auto& h : gs.diversify_top_k(q, cand, 6, 0.3f)) {
        uint32_t b;
        std::memcpy(&b, &h.score, 4);
        std::printf("%llu:%08x\n", (unsigned long long)h.index, b);
    }
    std::printf("--\n");
    for (const auto& h : gs.find_top_k_diverse(q, 5, 20, 0.3f)) std::printf("%llu\n", (unsigned long long)h.index);
    return 0;
}
'''


def test_cpp_diversify_top_k(tmp_path, golden_dir):
    from metrovector_amd import MvfReader, diversify_top_k, find_top_k_diverse
    src = tmp_path / "diversify.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "diversify_cpp")
    libdir = os.path.join(ROOT, "metrovector_amd")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                          "-L", libdir, "-lmvf_gpu", "-lmvf_host", f"-Wl,-rpath,{libdir}", "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    path = os.path.join(golden_dir, "clusters_60x4_f32.mvf")
    run = RUNNER.run([exe, path], timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    first, second = run.stdout.split("--\n")
    got = [(int(a), int(b, 16)) for a, b in (l.split(":") for l in first.split())]
    r = MvfReader.open(path)
    space = r.vector_space(r.vector_space_names()[0])
    cand = np.array([[5, 3, 3, 59, 58, 1000, int(PAD), 0, 17, 20, 21, 40, 41]], np.uint64)
    want = diversify_top_k(space, np.ones((1, 4), np.float32), cand, 6, 0.3)[0]
    assert got == [(h.index, int(np.float32(h.score).view(np.uint32))) for h in want] and len(got) == 6
    want2 = find_top_k_diverse(space, np.ones((1, 4), np.float32), 5, 20, 0.3)[0]
    assert [int(x) for x in second.split()] == [h.index for h in want2]
