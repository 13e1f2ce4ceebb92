"""The calls and scenarios of tests/test_gpu_stream_order.py, and -- run as a program,
`python tests/_stream_scenarios.py <id> ...` -- the child process that runs scenarios under MVF_DEBUG_POISON and prints one digest
per scenario.  No pytest in here.

A scenario: rows, a producer call and a consumer call of one handle, and how the handle is set up.  `run` does what every
scenario does: a decoy handle of other rows (negated, times 3) runs both calls and is destroyed, so that recycled memory holds
plausible but wrong norms, shadows and lists; a fresh handle runs the producer on the stalled stream and the consumer at once;
a third handle runs both with a full synchronise in between -- the reference, taken afterwards."""
import contextlib
import hashlib
import os
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _streams as S

L2, IP, COS = 0, 1, 2
F32, F16, I8 = 0, 1, 2
N = 20_000
DIM = {F32: 96, F16: 128, I8: 64}
K = 10
# mvfgpu_timing::scan_kernel of a forced scan path, by the stored type
KERNEL = {(2, F32): 2, (2, F16): 3, (2, I8): 3, (3, F32): 4, (4, F32): 5, (5, F32): 6, (5, F16): 6, (6, F32): 7, (7, F32): 7,
          (1, F32): 1, (1, I8): 1, (1, F16): 1}


def _G():
    from metrovector_amd import gpu as G
    return G


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _outs(nq, k):
    import torch
    return (torch.zeros((nq, k), dtype=torch.float32, device="cuda"), torch.zeros((nq, k), dtype=torch.int64, device="cuda"),
            torch.zeros((nq, k), dtype=torch.int32, device="cuda"))


def _sp(stream):
    return stream.cuda_stream if stream is not None else 0


def _read(ds, di, dr, **more):
    out = dict(scores=ds.cpu().numpy().view(np.uint32), indices=di.cpu().numpy().view(np.uint64), raw=dr.cpu().numpy())
    out.update({k: v.cpu().numpy() for k, v in more.items()})
    return out


def _res(r):
    out = dict(scores=r.scores.view(np.uint32), indices=r.indices, raw=r.raw)
    if hasattr(r, "counts"):
        out["counts"] = r.counts
    return out


def _maxsim_res(r):
    return dict(scores=r.scores.view(np.uint32), keys=r.keys, counts=r.counts)


class Ctx:
    """one handle and what was made of it"""

    def __init__(self, c, rows):
        self.c, self.rows, self.owned = c, rows, []  # owned: closed before the handle, newest first

    def own(self, obj):
        self.owned.append(obj)
        return obj

    def close(self):
        for o in reversed(self.owned):
            o.close()
        self.owned = []
        self.c.close()


class Call:
    entry = ""        # the C function (tests/_streams.py ENTRY_CLASS)
    is_async = False  # returns without waiting for the device
    path = None       # the scan path it forces
    kernel = None     # mvfgpu_timing::scan_kernel it must report (None: the route reports none)
    scan_bytes = None

    def handle(self, ctx):
        return ctx.c

    def force(self, ctx):
        if self.path is not None:
            self.handle(ctx).set_scan_path(self.path)

    def prepare(self, ctx):
        pass

    def issue(self, ctx, stream):
        raise NotImplementedError

    def after(self, ctx):
        """with the device idle behind this call: the route it took"""
        if self.kernel is not None:
            t = self.handle(ctx).last_timing()
            assert t.scan_kernel == self.kernel, f"{self.entry} on path {self.path}: scan_kernel {t.scan_kernel}, expected {self.kernel}"
            if self.scan_bytes is not None:
                assert t.scan_bytes == self.scan_bytes, f"{self.entry}: scan_bytes {t.scan_bytes}, expected {self.scan_bytes}"


class _Search(Call):
    def __init__(self, q, k, metric, path=None, kernel=None, scan_bytes=None):
        self.q, self.k, self.metric, self.path, self.kernel, self.scan_bytes = np.ascontiguousarray(q), k, metric, path, kernel, scan_bytes


class SearchDev(_Search):
    entry, is_async = "mvfgpu_search_device", True

    def prepare(self, ctx):
        self.t = (_dev(self.q),) + _outs(self.q.shape[0], self.k)

    def issue(self, ctx, stream):
        dq, ds, di, dr = self.t
        c = self.handle(ctx)
        c.search_device(dq.data_ptr(), _G().query_dtype_code(c.data_type), self.q.shape[1], self.q.shape[0], self.k, self.metric,
                        ds.data_ptr(), di.data_ptr(), dr.data_ptr(), stream=_sp(stream))
        return lambda: _read(ds, di, dr)


class SearchHost(_Search):
    entry = "mvfgpu_search"

    def issue(self, ctx, stream):
        r = self.handle(ctx).search(self.q, self.k, self.metric)
        return lambda: _res(r)


class SearchOnQueryHandle(SearchHost):
    def handle(self, ctx):
        return ctx.qc


class RadiusHost(Call):
    entry = "mvfgpu_search_radius"

    def __init__(self, q, radii, m, metric, path=None):
        self.q, self.radii, self.m, self.metric, self.path = np.ascontiguousarray(q), np.asarray(radii, np.float32), m, metric, path

    def issue(self, ctx, stream):
        r = ctx.c.search_radius(self.q, self.radii, self.m, self.metric)
        return lambda: _res(r)


class FilteredHost(_Search):
    entry = "mvfgpu_search_filtered"

    def issue(self, ctx, stream):
        r = ctx.c.search_filtered(self.q, self.k, self.metric, ctx.flt)
        return lambda: _res(r)


class FilteredDev(SearchDev):
    entry = "mvfgpu_search_filtered_device"

    def issue(self, ctx, stream):
        dq, ds, di, dr = self.t
        ctx.c.search_filtered_device(ctx.flt, dq.data_ptr(), _G().query_dtype_code(ctx.c.data_type), self.q.shape[1], self.q.shape[0],
                                     self.k, self.metric, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), stream=_sp(stream))
        return lambda: _read(ds, di, dr)


class JoinHost(Call):
    entry = "mvfgpu_knn_join"

    def __init__(self, first, count, k, metric, other=False, path=None):
        self.first, self.count, self.k, self.metric, self.other, self.path = first, count, k, metric, other, path

    def issue(self, ctx, stream):
        r = ctx.c.knn_join(self.k, self.metric, first=self.first, count=self.count, queries_from=ctx.qc if self.other else None)
        return lambda: _res(r)


class JoinDev(JoinHost):
    entry, is_async = "mvfgpu_knn_join_device", True

    def prepare(self, ctx):
        self.t = _outs(self.count, self.k)

    def issue(self, ctx, stream):
        ds, di, dr = self.t
        ctx.c.knn_join_device(self.k, self.metric, self.first, self.count, ds.data_ptr(), di.data_ptr(), dr.data_ptr(),
                              queries_from=ctx.qc if self.other else None, stream=_sp(stream))
        return lambda: _read(ds, di, dr)


class CandHost(_Search):
    entry = "mvfgpu_search_candidates"

    def __init__(self, q, cand, k, metric):
        super().__init__(q, k, metric)
        self.cand = np.ascontiguousarray(cand, np.uint64)

    def issue(self, ctx, stream):
        r = ctx.c.search_candidates(self.q, self.cand, self.k, self.metric)
        return lambda: _res(r)


class CandDev(CandHost):
    entry, is_async = "mvfgpu_search_candidates_device", True

    def prepare(self, ctx):
        import torch
        self.t = (_dev(self.q), _dev(self.cand)) + _outs(self.q.shape[0], self.k) + (torch.zeros(self.q.shape[0], dtype=torch.int64, device="cuda"),)

    def issue(self, ctx, stream):
        dq, dc, ds, di, dr, dn = self.t
        ctx.c.search_candidates_device(dq.data_ptr(), _G().query_dtype_code(ctx.c.data_type), self.q.shape[1], self.q.shape[0], dc.data_ptr(),
                                       self.cand.shape[1], self.k, self.metric, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), dn.data_ptr(),
                                       stream=_sp(stream))
        return lambda: dict(_read(ds, di, dr), counts=dn.cpu().numpy().view(np.uint64))


class PartHost(_Search):
    entry = "mvfgpu_search_partitioned"

    def __init__(self, q, keys, k, metric):
        super().__init__(q, k, metric)
        self.keys = np.ascontiguousarray(keys, np.uint64)

    def issue(self, ctx, stream):
        r = ctx.c.search_partitioned(self.q, self.keys, self.k, self.metric, ctx.part)
        return lambda: _res(r)


class PartDev(PartHost):
    entry, is_async = "mvfgpu_search_partitioned_device", True
    prepare = SearchDev.prepare

    def issue(self, ctx, stream):
        dq, ds, di, dr = self.t
        ctx.c.search_partitioned_device(ctx.part, dq.data_ptr(), _G().query_dtype_code(ctx.c.data_type), self.q.shape[1], self.q.shape[0],
                                        self.keys, self.k, self.metric, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), stream=_sp(stream))
        return lambda: _read(ds, di, dr)


class GroupedHost(_Search):
    entry = "mvfgpu_search_grouped"

    def __init__(self, q, k, per_key, metric):
        super().__init__(q, k, metric)
        self.per_key = per_key

    def issue(self, ctx, stream):
        r = ctx.c.search_grouped(self.q, self.k, self.per_key, self.metric, ctx.part)
        return lambda: _res(r)


class GroupedDev(GroupedHost):
    entry, is_async = "mvfgpu_search_grouped_device", True
    prepare = SearchDev.prepare

    def issue(self, ctx, stream):
        dq, ds, di, dr = self.t
        ctx.c.search_grouped_device(ctx.part, dq.data_ptr(), _G().query_dtype_code(ctx.c.data_type), self.q.shape[1], self.q.shape[0], self.k,
                                    self.per_key, self.metric, ds.data_ptr(), di.data_ptr(), dr.data_ptr(), stream=_sp(stream))
        return lambda: _read(ds, di, dr)


class MaxsimHost(Call):
    entry = "mvfgpu_search_maxsim"

    def __init__(self, sets, k, metric, cand=None):
        self.sets, self.k, self.metric = np.ascontiguousarray(sets), k, metric
        self.cand = None if cand is None else np.ascontiguousarray(cand, np.uint64)

    def issue(self, ctx, stream):
        r = ctx.c.search_maxsim(self.sets, self.k, self.metric, ctx.part)
        return lambda: _maxsim_res(r)


class MaxsimDev(MaxsimHost):
    entry, is_async = "mvfgpu_search_maxsim_device", True

    def prepare(self, ctx):
        import torch
        nq = self.sets.shape[0]
        self.t = (_dev(self.sets), torch.zeros((nq, self.k), dtype=torch.float32, device="cuda"),
                  torch.zeros((nq, self.k), dtype=torch.int64, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda"))

    def _got(self):
        dq, ds, dk, dn = self.t
        return lambda: dict(scores=ds.cpu().numpy().view(np.uint32), keys=dk.cpu().numpy().view(np.uint64), counts=dn.cpu().numpy().view(np.uint32))

    def issue(self, ctx, stream):
        dq, ds, dk, dn = self.t
        nq, T, dim = self.sets.shape
        ctx.c.search_maxsim_device(ctx.part, dq.data_ptr(), _G().query_dtype_code(ctx.c.data_type), dim, nq, T, self.k, self.metric,
                                   ds.data_ptr(), dk.data_ptr(), dn.data_ptr(), stream=_sp(stream))
        return self._got()


class MaxsimCandHost(MaxsimHost):
    entry = "mvfgpu_search_maxsim_candidates"

    def issue(self, ctx, stream):
        r = ctx.c.search_maxsim_candidates(self.sets, self.cand, self.k, self.metric, ctx.part)
        return lambda: _maxsim_res(r)


class MaxsimCandDev(MaxsimDev):
    entry = "mvfgpu_search_maxsim_candidates_device"

    def issue(self, ctx, stream):
        dq, ds, dk, dn = self.t
        nq, T, dim = self.sets.shape
        ctx.c.search_maxsim_candidates_device(ctx.part, dq.data_ptr(), _G().query_dtype_code(ctx.c.data_type), dim, nq, T, self.cand, self.k,
                                              self.metric, ds.data_ptr(), dk.data_ptr(), dn.data_ptr(), stream=_sp(stream))
        return self._got()


# ---- scenarios ------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def decoy_of(rows):
    """other rows of the same shape: negated and scaled by 3 (integers wrap)"""
    if rows.dtype.kind == "f":
        return (rows.astype(np.float32) * -3.0).astype(rows.dtype)
    return (rows.astype(np.int32) * -3).astype(rows.dtype)


def column_values(n):
    """a UInt32 key per row: 37 keys scattered over all positions"""
    return ((np.arange(n, dtype=np.uint64) * 2654435761 + 12345) % 1000003 % 37).astype(np.uint32)


def allow_mask(n, every=3):
    m = np.zeros(n, bool)
    m[::every] = True
    return m


class Scenario:
    def __init__(self, sid, dtype, seed, producer, consumer, env=None, needs=(), rows=None):
        self.id, self.dtype, self.seed, self.producer, self.consumer = sid, dtype, seed, producer, consumer
        self.env, self.needs = dict(env or {}), tuple(needs)
        self.rows = rows
        self.probe = None  # one query of the handle's space: the own-stream control's

    def make_ctx(self, rows):
        G = _G()
        with _environment(self.env):  # the switches are read once, when the handle is created
            ctx = Ctx(G.GpuCorpus.from_array(rows), rows)
        ctx.c.set_profiling(True)  # mvfgpu_last_timing carries the route (scan_kernel) of a profiled search
        n = rows.shape[0]
        if "filter" in self.needs:
            ctx.flt = ctx.own(ctx.c.make_filter(allow_mask(n)))
        if "partition" in self.needs:
            ctx.col = ctx.own(ctx.c.attach_column(column_values(n)))
            ctx.part = ctx.own(ctx.c.make_partition(ctx.col))
        if "query_handle" in self.needs:
            with _environment(self.env):
                ctx.qc = ctx.own(G.GpuCorpus.from_array(np.ascontiguousarray(rows[::-1][:600]), index_base=1_000_000))
        return ctx


def run(sc, streams, reference=True):
    """-> (stalled producer, stalled consumer, reference producer, reference consumer), dicts of arrays (the last two None
    without a reference)"""
    S.run_pair(lambda: sc.make_ctx(decoy_of(sc.rows)), sc.producer, sc.consumer, None)
    gp, gc = S.run_pair(lambda: sc.make_ctx(sc.rows), sc.producer, sc.consumer, streams, query=sc.probe)
    if not reference:
        return gp, gc, None, None
    rp, rc = S.run_pair(lambda: sc.make_ctx(sc.rows), sc.producer, sc.consumer, None)
    return gp, gc, rp, rc


def digest(*results):
    h = hashlib.sha256()
    for r in results:
        for k in sorted(r):
            h.update(k.encode())
            h.update(np.ascontiguousarray(r[k]).tobytes())
    return h.hexdigest()


def _seed_of(sid):
    import zlib
    return zlib.crc32(sid.encode()) & 0x7FFFFFFF


def radius_between(scores64, metric, rank):
    """a radius strictly between the rank-th and the (rank+1)-th best float64 score"""
    s = np.sort(scores64)
    if metric != L2:
        s = s[::-1]
    return float(np.float32((s[rank - 1] + s[rank]) / 2))


def scores64(rows, q, metric):
    x, v = rows.astype(np.float64), np.asarray(q, np.float64)
    if metric == L2:
        return np.sqrt(((x - v) ** 2).sum(1))
    d = x @ v
    if metric == IP:
        return d
    return d / np.maximum(np.linalg.norm(x, axis=1) * np.linalg.norm(v), 1e-300)


def build(sid, oracle):
    """the scenario `sid` of tests/_streams.py SCENARIOS"""
    G = _G()
    kind, *rest = sid.split(":")
    seed = _seed_of(sid)
    dtype = {"f32": F32, "f16": F16, "i8": I8}[rest[0]]
    dim = DIM[dtype]
    rows = np.ascontiguousarray(oracle.synth_rows(seed, 0, N, dim, dtype))

    def queries(tag, nq):
        return np.ascontiguousarray(oracle.synth_queries(seed + tag, nq, dim, dtype))

    def kern(path):
        return KERNEL[(path, dtype)]

    env, needs = {}, []
    if kind == "lazy":  # lazy:<dtype>:<producer path>:<metric>:<consumer>
        path, metric, cons = int(rest[1]), {"l2": L2, "ip": IP, "cos": COS}[rest[2]], rest[3]
        nq = 1 if path in (6, 7) else 64 if dtype == I8 else 32
        k = K
        sbytes = None
        if path == 6:
            env["MVF_STREAM_I8"] = "1"
        if path == 7:
            sbytes = G.shadow6_bytes(N, dim)
        if path == 1:  # lazy:f32:1:<metric>:<consumer>:<passes|sort>
            k, nq = 3000, 2
            env["MVF_LARGE_K"] = {"passes": "1", "sort": "2"}[rest[4]]
            large_k_kernel = {"passes": 1, "sort": 8}[rest[4]]  # 8: the streaming kernel as a dump + the whole-shard sort
        q = queries(1, nq)
        pk = large_k_kernel if path == 1 else kern(path)
        producer = SearchDev(q, k, metric, path, pk, sbytes)
        producer.waits_for_its_stream = path == 7  # once per 6-bit shadow: its bound maxima are read back (api.hip search_locked)
        if cons == "dev":
            consumer = SearchDev(q, k, metric, path, pk, sbytes)
        elif cons == "host":
            consumer = SearchHost(q, k, metric, path, pk, sbytes)
        elif cons == "hostother":
            consumer = SearchHost(queries(2, nq), k, metric, path, pk)
        elif cons.startswith("radius"):
            rq = queries(3, int(cons[6:]))
            if dtype == I8:
                sc_all = [oracle.scores(rows, dtype, metric, v)[0].astype(np.float64) for v in rq]
            else:
                sc_all = [scores64(rows, v, metric) for v in rq]
            radii = [radius_between(s, metric, 40 + 7 * j) for j, s in enumerate(sc_all)]
            if metric == COS:
                assert min(radii) > 0
            # (a forced batched path sends every Float32 radius call through the batched route: four queries on path 0 stream, R1)
            consumer = RadiusHost(rq, radii, 64, metric, 0 if len(rq) < 16 and dtype == F32 else path)
        elif cons in ("filtermask", "filterlist"):
            env["MVF_FILTER_ROUTE"] = "1" if cons == "filtermask" else "2"
            needs.append("filter")
            consumer = FilteredHost(queries(4, 32), k, metric, path)
        elif cons == "filterdev":
            needs.append("filter")
            consumer = FilteredDev(queries(4, 32), k, metric, path)
        elif cons == "join":
            consumer = JoinHost(1000, 512, k, metric, path=path)
        elif cons == "cand":
            cq = queries(5, 6)
            cand = np.random.default_rng(seed).integers(0, N, (6, 200)).astype(np.uint64)
            consumer = CandHost(cq, cand, k, metric)
        elif cons.startswith("p"):  # another forced path on the host: p4x1 = path 4, one query
            cpath, cnq = int(cons[1]), int(cons.split("x")[1])
            consumer = SearchHost(queries(6, cnq), k, metric, cpath, kern(cpath))
        elif cons == "batch5":
            consumer = SearchDev(queries(7, 32), k, metric, 5, kern(5))
            consumer.grows_scratch = True  # the one-query search's candidate buffer is freed for the batch's: hipFree waits
        else:
            raise KeyError(sid)
    elif kind == "scratch":  # scratch:<dtype>:<path>: two different batches share the handle's query matrix and candidate regions
        path = int(rest[1])
        producer = SearchDev(queries(1, 64), K, L2, path, kern(path))
        consumer = SearchDev(queries(2, 48), K, L2, path, kern(path))
    elif kind == "entry":  # entry:<dtype>:<name>:<form>: a *_device entry on the stalled stream and its host form; or (dev) a batched
        # search that builds the norms on the stalled stream and the *_device entry on the other stream
        name, form = rest[1], rest[2]
        metric = IP
        qa, qb = queries(1, 6), queries(2, 5)
        rng = np.random.default_rng(seed)
        col = column_values(N).astype(np.uint64)
        if name == "candidates":
            mk = lambda dev, q: (CandDev if dev else CandHost)(q, rng.integers(0, N, (q.shape[0], 300)).astype(np.uint64), K, metric)  # noqa: E731
        elif name == "filtered":
            needs.append("filter")
            mk = lambda dev, q: (FilteredDev if dev else FilteredHost)(q, K, metric)  # noqa: E731
        elif name == "partitioned":
            needs.append("partition")
            mk = lambda dev, q: (PartDev if dev else PartHost)(q, col[rng.integers(0, N, q.shape[0])], K, metric)  # noqa: E731
        elif name == "grouped":
            needs.append("partition")
            mk = lambda dev, q: (GroupedDev if dev else GroupedHost)(q, K, 2, metric)  # noqa: E731
        elif name in ("maxsim", "maxsimcand"):
            needs.append("partition")
            cls = {("maxsim", True): MaxsimDev, ("maxsim", False): MaxsimHost, ("maxsimcand", True): MaxsimCandDev,
                   ("maxsimcand", False): MaxsimCandHost}
            mk = lambda dev, q: cls[(name, dev)](np.stack([q, q[::-1]]), 5, metric, cand=np.arange(3, 30, 2, dtype=np.uint64))  # noqa: E731
        elif name in ("join", "join2"):
            if name == "join2":
                needs.append("query_handle")
            # (behind the batched search: fewer queries and a shorter list than its, so that the handle's scratch does not grow)
            mk = lambda dev, q: (JoinDev if dev else JoinHost)(37 if dev else 90, 100 if form == "dev" else 300, K, metric,  # noqa: E731
                                                               other=name == "join2")
        else:
            raise KeyError(sid)
        producer = SearchDev(queries(3, 128), 2 * K, metric, 2, kern(2)) if form == "dev" else mk(True, qa)
        if form == "search":  # join2: a host search on the query handle follows
            consumer = SearchOnQueryHandle(qb, K, metric)
        else:
            consumer = mk(form == "dev", qb)
    else:
        raise KeyError(sid)
    sc = Scenario(sid, dtype, seed, producer, consumer, env=env, needs=needs, rows=rows)
    sc.probe = queries(99, 1)
    return sc


COLUMN_CLAUSE = ("between", (5, 20))


def column_inputs(oracle):
    seed = _seed_of("column")
    rows = np.ascontiguousarray(oracle.synth_rows(seed, 0, N, DIM[F32], F32))
    positions = np.random.default_rng(seed).integers(0, N, 100).astype(np.uint64)
    return dict(rows=rows, values=column_values(N), positions=positions, probe=np.ascontiguousarray(oracle.synth_queries(seed + 99, 1, DIM[F32], F32)))


def _column_run(rows, values, positions, probe, streams):
    """A column created from device values (streams given: written on the stalled stream behind the stall, the column created there
    with no host wait), then a where-filter, a partition index and a gather of it at once -> dict of arrays"""
    import torch
    G = _G()

    def attempt():
        c = G.GpuCorpus.from_array(rows)
        try:
            src = _dev(values)
            dv = torch.zeros_like(src)
            torch.cuda.synchronize()
            if streams is None:
                dv.copy_(src)
                torch.cuda.synchronize()
                col = c.attach_column_device(dv.data_ptr(), G.UINT32)
                torch.cuda.synchronize()
            else:
                s2 = streams[1]
                ev = S.stall(s2)
                with torch.cuda.stream(s2):
                    dv.copy_(src)
                col = c.attach_column_device(dv.data_ptr(), G.UINT32, stream=s2.cuda_stream)
                S.require_pending(ev, "when mvfgpu_column_create_device had returned and mvfgpu_filter_create_where was issued")
            flt = c.make_filter_where([(col,) + COLUMN_CLAUSE])
            part = c.make_partition(col)
            gathered = col.gather(positions)
            keys, counts = part.keys()
            out = dict(admitted=np.array([flt.admitted], np.uint64), keys=keys, counts=counts, gathered=gathered)
            torch.cuda.synchronize()
            part.close(), flt.close(), col.close()
            return out, c, c.close
        except BaseException:
            c.close()
            raise

    if streams is None:
        out, _, close = attempt()
        close()
        return out
    return S.on_an_independent_handle(attempt, probe, streams[1])


def column_scenario(oracle, streams):
    """decoy (other rows, other values), then the stalled run -> what it returned"""
    inp = column_inputs(oracle)
    _column_run(decoy_of(inp["rows"]), inp["values"] + np.uint32(1000), inp["positions"], inp["probe"], None)
    return _column_run(inp["rows"], inp["values"], inp["positions"], inp["probe"], streams)


def main(argv):
    """the child: every scenario named, decoy and stalled run only; one line `<id> <digest>` each"""
    from oracle import mvf_oracle
    mvf_oracle.build()
    G = _G()
    first = build(next(a for a in argv[1:] if a != "column"), mvf_oracle)
    try:
        streams = S.pick_streams(lambda: G.GpuCorpus.from_array(first.rows), first.probe)
    except S.ControlFailed as e:
        print(f"CONTROL {e}")
        return 3
    print(f"poison {G.selftest_poison()}")
    for sid in argv[1:]:
        if sid == "column":
            print(f"column {digest(column_scenario(mvf_oracle, streams))}", flush=True)
            continue
        sc = build(sid, mvf_oracle)
        gp, gc, _, _ = run(sc, streams, reference=False)
        print(f"{sid} {digest(gp, gc)}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
