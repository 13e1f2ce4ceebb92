"""-m gpu tests of the multi-vector search's MFMA selection route (DESIGN.md §3 "Multi-vector search: the MFMA route", §5
"A0 / P0").  The yardstick is route 1 on the same handle and partition: every case runs both routes and asserts equal score
bits, keys and counts, from the host call and from the device call.  Route 1 itself is held to the recipe of grouped searches
by tests/test_gpu_maxsim.py and tests/test_gpu_maxsim_forms.py.
World A: tests/_maxsim.py's form layout on 2048 rows (keys of 300 / 129 / 128 / 127 / 64 / 2 / 1 rows, tombstones, keys across
block edges); world B: 8192 rows, 1007 keys.  Beside the identity: that the selection really selects (candidate and block
counts of the stage timer), planted twins, ties, non-finite and zero values, subnormal f16 rows, ineligible handles, a fresh
process that takes the route from the environment, two calls on one stream.
Run time on an MI355X: see DESIGN.md §6; every case takes a few seconds at the most."""
import os
import sys

import numpy as np
import pytest

import _edges as ED
import _maxsim as MS
import _maxsim_mfma as MM
import _partitioned as P
from _children import RUNNER
from _maxsim_world import World, same_bytes
from metrovector_amd import errors as E
from metrovector_amd import gpu as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
L2, IP, COS = 0, 1, 2
SHAPES = [("f32", 3), ("f32", 100), ("f32", 129), ("f32", 768), ("f16", 8), ("f16", 20), ("f16", 200), ("f16", 768)]
TOKENS = (1, 5, 32, 33, 70)
NQS = (1, 3)


def device_call(w, sets, metric, k, stream=None, counts=True):
    """search_maxsim_device through torch's allocations -> (MaxSimResult, the tensors that keep the memory alive)"""
    import torch
    nq, T, dim = sets.shape
    dq = torch.from_numpy(np.ascontiguousarray(sets)).cuda()
    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    dk = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    dc = torch.zeros((nq,), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    qcode = {"float32": 0, "int8": 2, "uint8": 3}[sets.dtype.name]
    w.c.search_maxsim_device(w.part, dq.data_ptr(), qcode, dim, nq, T, k, metric, ds.data_ptr(), dk.data_ptr(), dc.data_ptr() if counts else 0, s)
    return (ds, dk, dc), dq


def fetch(t):
    import torch
    torch.cuda.synchronize()
    return G.MaxSimResult(t[0].cpu().numpy(), t[1].cpu().numpy().view(np.uint64), t[2].cpu().numpy().view(np.uint32))


def both_routes(w, sets, metric, k, what):
    """route 2 against route 1, host call and device call; -> route 1's result"""
    w.c.set_maxsim_route(1)
    want = w.c.search_maxsim(sets, k, metric, w.part)
    w.c.set_maxsim_route(2)
    try:
        same_bytes(w.c.search_maxsim(sets, k, metric, w.part), want, f"{what}, k {k}: host call")
        t, _ = device_call(w, sets, metric, k)
        same_bytes(fetch(t), want, f"{what}, k {k}: device call")
    finally:
        w.c.set_maxsim_route(0)
    assert (want.counts == min(k, w.nk)).all()
    return want


def stage(w, sets, metric, k):
    """the stage timer of route 2 -> (ms, candidates per set, blocks per set, its result)"""
    import torch
    nq, T, dim = sets.shape
    dq = torch.from_numpy(np.ascontiguousarray(sets)).cuda()
    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    dk = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ms, cand, blocks = w.c.maxsim_mfma_stage_ms(w.part, dq.data_ptr(), 0, dim, nq, T, k, metric, ds.data_ptr(), dk.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
    assert len(ms) == 6 and all(0.0 <= x < 1000.0 for x in ms) and ms[1] > 0.0
    return ms, cand, blocks, (ds.cpu().numpy(), dk.cpu().numpy().view(np.uint64))


def list_blocks(w):
    return -(-w.live.size // 128)


@pytest.fixture(scope="module")
def world_a():
    made = {}

    def get(dt, dim):
        if (dt, dim) not in made:
            made[dt, dim] = World(dt, dim, MS.form_layout(2048))
        return made[dt, dim]
    yield get
    for w in made.values():
        w.close()


@pytest.fixture(scope="module")
def world_b():
    made = {}

    def get(dt, dim):
        if (dt, dim) not in made:
            made[dt, dim] = World(dt, dim, MM.world_b())
        return made[dt, dim]
    yield get
    for w in made.values():
        w.close()


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=[f"{dt}d{dim}" for dt, dim in SHAPES])
def test_world_a_every_shape_token_count_and_k(world_a, case):
    dt, dim = SHAPES[case]
    w = world_a(dt, dim)
    assert MS.spans_block_edge(w.lay)
    pool = MS.token_pool(dt, dim, 3, 70)
    for metric in (IP, COS):
        for T in TOKENS:
            for nq in NQS:
                for k in (1, 10, w.nk, w.nk + 5):
                    both_routes(w, pool[:nq, :T], metric, k, f"{dt} x {dim}, metric {metric}, T {T}, nq {nq}")


@pytest.mark.parametrize("dt,dim", [("f32", 100), ("f16", 200)])
def test_world_b_is_the_same_bytes_and_the_selection_selects(world_b, dt, dim):
    """1007 keys, random rows, k = 10: at least 10 and at most n_keys / 2 candidates per set, fewer blocks than the list has --
    conditions of the rule (tests/test_maxsim_mfma_cpu.py holds the emulation inside them on these rows), not measurements"""
    w = world_b(dt, dim)
    assert w.nk >= 1000
    for metric in (IP, COS):
        for T, nq in ((5, 3), (33, 1), (70, 3)):
            sets = MS.make_sets(nq, T, dim, dt)
            for k in (1, 10, w.nk, w.nk + 5):
                want = both_routes(w, sets, metric, k, f"world B {dt} x {dim}, metric {metric}, T {T}, nq {nq}")
            want10 = w.c.search_maxsim(sets, 10, metric, w.part)
            _, cand, blocks, (sc, ky) = stage(w, sets, metric, 10)
            assert (ky == want10.keys).all() and (sc.view(np.uint32) == want10.scores.view(np.uint32)).all(), "the stage timer is the search"
            assert ((cand >= 10) & (cand <= w.nk // 2)).all(), f"metric {metric}, T {T}: candidates {cand} of {w.nk} keys"
            assert ((blocks >= 1) & (blocks < list_blocks(w))).all(), f"metric {metric}, T {T}: blocks {blocks} of {list_blocks(w)}"
            _, cand, blocks, _ = stage(w, sets, metric, w.nk)
            assert (cand == w.nk).all() and (blocks == list_blocks(w)).all(), "k = n_keys: every key is a candidate"


def test_a_small_scratch_budget_gives_several_windows_and_chunks(world_a, monkeypatch):
    for dt, dim, metric in (("f32", 100, COS), ("f16", 200, IP)):
        w = world_a(dt, dim)
        budget = w.nk * (8 * 4 + MS.KEY_BYTES)
        chunk, window = G.maxsim_plan(w.nk, 33, 3, 16, budget)
        assert -(-33 // chunk) >= 3 and -(-3 // window) >= 2, "route 2's window can only be shorter"
        monkeypatch.setenv("MVF_MAXSIM_SCRATCH_BYTES", str(budget))
        small = World(dt, dim, w.lay)
        monkeypatch.delenv("MVF_MAXSIM_SCRATCH_BYTES")
        try:
            sets = MS.make_sets(3, 33, dim, dt)
            w.c.set_maxsim_route(1)
            for k in (1, 10, w.nk + 5):
                whole = w.c.search_maxsim(sets, k, metric, w.part)
                same_bytes(both_routes(small, sets, metric, k, f"{dt}: small budget"), whole, f"{dt}, k {k}: chunked against unchunked")
        finally:
            w.c.set_maxsim_route(0)
            small.close()


def next_after(x, up):
    b = x.view(np.uint32 if x.dtype == np.float32 else np.uint16).copy()
    b += np.where((x > 0) == up, 1, -1).astype(b.dtype)
    return b.view(x.dtype)


@pytest.mark.parametrize("dt,dim", [("f32", 100), ("f16", 200)])
def test_planted_twins_equal_keys_and_equal_rows(dt, dim):
    lay = MS.form_layout(2048)
    live, keys, starts, values = MS.key_order(lay)
    rows = P.make_rows(2048, dim, dt)
    ends = np.concatenate([starts[1:], [keys.size]])
    sizes = ends - starts
    # twins: pairs of keys with equally many rows; the second's rows are the first's with one element moved by one ulp
    # equal keys: a third key of the same size holds the first's rows exactly
    done = 0
    for size in np.unique(sizes):
        same = np.nonzero(sizes == size)[0]
        if same.size < 3:
            continue
        a, b, c = same[:3]
        ra, rb, rc = (live[starts[g]:ends[g]] for g in (a, b, c))
        rows[rb] = rows[ra]
        rows[rc] = rows[ra]
        col = (done * 7) % dim
        rows[rb[0], col] = next_after(rows[rb[0], col:col + 1], up=done % 2 == 0)[0]
        done += 1
    assert done >= 2
    w = World(dt, dim, lay, rows=rows)
    try:
        for metric in (IP, COS):
            for T, nq in ((5, 3), (33, 1)):
                for k in (1, 10, w.nk + 5):
                    both_routes(w, MS.make_sets(nq, T, dim, dt), metric, k, f"twins {dt}, metric {metric}, T {T}")
    finally:
        w.close()
    # all rows equal: every sum ties, the keys rank by value, every key is a candidate
    rows = np.broadcast_to(P.make_rows(1, dim, dt), (2048, dim)).copy()
    w = World(dt, dim, lay, rows=rows)
    try:
        for metric in (IP, COS):
            sets = MS.make_sets(3, 5, dim, dt)
            for k in (1, 10, w.nk + 5):
                got = both_routes(w, sets, metric, k, f"equal rows {dt}, metric {metric}")
                assert (got.keys[:, :min(k, w.nk)] == w.keys[None, :min(k, w.nk)]).all()
            _, cand, blocks, _ = stage(w, sets, metric, 10)
            assert (cand == w.nk).all() and (blocks == list_blocks(w)).all()
    finally:
        w.close()


@pytest.mark.parametrize("dt,dim", [("f32", 100), ("f16", 200)])
def test_non_finite_huge_and_zero_values(dt, dim):
    """NaN, +-Inf, 1e30 (Float16 rows: 60000) and zero rows planted in keys of every size; NaN and zero tokens"""
    lay = MS.form_layout(2048)
    live, keys, starts, values = MS.key_order(lay)
    rows = P.make_rows(2048, dim, dt)
    big = 60000.0 if dt == "f16" else 1e30
    rng = np.random.default_rng(P._seed("mfma edges", dt, dim))
    at = rng.choice(live, 40, replace=False)
    for i, r in enumerate(at):
        kind = i % 8
        if kind == 0:
            rows[r, i % dim] = np.nan
        elif kind == 1:
            rows[r, i % dim] = np.inf
        elif kind == 2:
            rows[r, i % dim] = -np.inf
        elif kind == 3:
            rows[r, 0], rows[r, dim - 1] = np.inf, -np.inf
        elif kind == 4:
            rows[r] = big
        elif kind == 5:
            rows[r, i % dim] = -big
        else:
            rows[r] = 0
    # whole keys of special rows: a key of zero rows only, a key of NaN rows only
    small = np.nonzero((np.concatenate([starts[1:], [keys.size]]) - starts) <= 3)[0]
    rows[live[starts[small[0]]:starts[small[0] + 1]]] = 0
    rows[live[starts[small[1]]:starts[small[1] + 1]]] = np.nan
    w = World(dt, dim, lay, rows=rows)
    try:
        base = MS.make_sets(3, 5, dim, dt)
        token_edges = {"ordinary": None, "nan": np.full(dim, np.nan, np.float32), "zero": np.zeros(dim, np.float32),
                       "inf": None, "huge": None}
        for name, token in token_edges.items():
            sets = base.copy()
            if name == "inf":
                sets[1, 2, 0] = np.inf
            elif name == "huge":
                sets[1, 2] *= np.float32(1e30)
                sets[2, 0] *= np.float32(1e-30)
            elif token is not None:
                sets[0, 1], sets[2, 4] = token, token
            for metric in (IP, COS):
                for k in (1, 10, w.nk, w.nk + 5):
                    both_routes(w, sets, metric, k, f"edges {dt}, {name} tokens, metric {metric}")
    finally:
        w.close()


@pytest.mark.parametrize("kind", ["S", "R", "T"])
def test_subnormal_f16_rows(oracle, kind):
    """tests/_edges.py's Float16 corpora: S every non-zero value subnormal, R normal to fully subnormal rows side by side, T
    values up to 32736"""
    case = ED.get_case(oracle, "d96", ED.F16)
    rows = case.rows(kind)
    n = rows.shape[0]
    dead = case.dead if case.dead is not None else np.zeros(n, bool)
    col = ((np.arange(n) * 2654435761) % 211).astype(np.uint32)
    w = World("f16", case.dim, dict(col=col, dead=dead), rows=rows)
    try:
        pool = case.pool[:15].reshape(3, 5, case.dim).astype(np.float32)
        for metric in (IP, COS):
            for sets in (pool, np.ldexp(pool, -20).astype(np.float32), np.ldexp(pool, 20).astype(np.float32)):
                for k in (1, 10, w.nk + 5):
                    both_routes(w, sets, metric, k, f"f16 corpus {kind}, metric {metric}")
    finally:
        w.close()


def test_ineligible_handles_and_metrics_take_route_1(world_a):
    """the forced route on Int8 rows and under L2 is route 1; the route's stage timer refuses them"""
    import torch
    w = World("i8", 64, MS.form_layout(2048))
    try:
        sets = MS.make_sets(3, 5, 64, "i8")
        for metric in (L2, IP, COS):
            both_routes(w, sets, metric, 10, f"i8, metric {metric}")
        dq = torch.from_numpy(sets).cuda()
        ds, dk = torch.empty((3, 10), dtype=torch.float32, device="cuda"), torch.empty((3, 10), dtype=torch.int64, device="cuda")
        with pytest.raises(E.InvalidArgument, match="Float32 / Float16 rows under InnerProduct / Cosine"):
            w.c.maxsim_mfma_stage_ms(w.part, dq.data_ptr(), 2, 64, 3, 5, 10, IP, ds.data_ptr(), dk.data_ptr())
        with pytest.raises(E.InvalidArgument, match="route must be 0, 1 or 2"):
            w.c.set_maxsim_route(3)
        with pytest.raises(E.InvalidArgument, match="route must be 0, 1 or 2"):
            w.c.set_maxsim_route(-1)
    finally:
        w.close()
    f = world_a("f32", 100)
    sets = MS.make_sets(3, 5, 100, "f32")
    for k in (1, 10, f.nk + 5):
        both_routes(f, sets, L2, k, "f32 under L2")
    dq = torch.from_numpy(sets).cuda()
    ds, dk = torch.empty((3, 10), dtype=torch.float32, device="cuda"), torch.empty((3, 10), dtype=torch.int64, device="cuda")
    with pytest.raises(E.InvalidArgument, match="Float32 / Float16 rows under InnerProduct / Cosine"):
        f.c.maxsim_mfma_stage_ms(f.part, dq.data_ptr(), 0, 100, 3, 5, 10, L2, ds.data_ptr(), dk.data_ptr())
    torch.cuda.synchronize()  # the refusals left no device error behind
    # the route 1 timer times route 1 whatever the handle's route
    f.c.set_maxsim_route(2)
    try:
        ms = f.c.maxsim_stage_ms(f.part, dq.data_ptr(), 0, 100, 3, 5, 10, COS, ds.data_ptr(), dk.data_ptr())
        assert len(ms) == 4 and ms[1] > 0.0
    finally:
        f.c.set_maxsim_route(0)


def test_a_second_call_enqueued_behind_the_first_gives_the_same_bytes(world_b):
    """two device calls on one stream, the second enqueued without waiting for the first: each call's scratch is its own"""
    import torch
    w = world_b("f32", 100)
    a, b = MS.make_sets(3, 33, 100, "f32"), MS.make_sets(2, 5, 100, "f32")
    w.c.set_maxsim_route(1)
    want_a, want_b = w.c.search_maxsim(a, 10, COS, w.part), w.c.search_maxsim(b, 7, IP, w.part)
    w.c.set_maxsim_route(2)
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            ta, qa = device_call(w, a, COS, 10, stream.cuda_stream)
            tb, qb = device_call(w, b, IP, 7, stream.cuda_stream)
            ta2, qa2 = device_call(w, a, COS, 10, stream.cuda_stream, counts=False)
        same_bytes(fetch(ta), want_a, "first call")
        same_bytes(fetch(tb), want_b, "second call")
        got = fetch(ta2)
        assert (got.keys == want_a.keys).all() and (got.scores.view(np.uint32) == want_a.scores.view(np.uint32)).all(), "third call"
    finally:
        w.c.set_maxsim_route(0)


def test_a_fresh_process_takes_the_route_from_the_environment(tmp_path):
    """tests/_maxsim_mfma.py as a child: MVF_MAXSIM_ROUTE=2 with every allocation of the library poisoned gives the bytes of a
    child on route 1; one child at a time, none after a fault"""
    results = {}
    for tag, route, poison in (("route1", "1", None), ("route2", "2", None), ("route2 poison00", "2", 0), ("route2 poisonFF", "2", 255)):
        env = {k: v for k, v in os.environ.items() if k not in ("MVF_DEBUG_POISON", "MVF_MAXSIM_SCRATCH_BYTES", "MVF_MAXSIM_ROUTE")}
        env["MVF_MAXSIM_ROUTE"] = route
        if poison is not None:
            env["MVF_DEBUG_POISON"] = str(poison)
        path = str(tmp_path / f"{tag.replace(' ', '_')}.npz")
        out = RUNNER.run([sys.executable, os.path.join(HERE, "_maxsim_mfma.py"), path], env=env)
        assert out.returncode == 0, f"{tag}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}"
        with np.load(path) as z:
            assert z["poison"].tolist() == [-1 if poison is None else poison] and z["route"].tolist() == [int(route)]
            results[tag] = {call: G.MaxSimResult(z[call + ".scores"], z[call + ".keys"], z[call + ".counts"]) for call in ("host", "device")}
            assert (z["candidates"] >= MS.FP_K).all() and (z["blocks"] >= 1).all()
    for tag, res in results.items():
        for call in ("host", "device"):
            same_bytes(res[call], results["route1"]["host"], f"{tag}: the {call} call")
