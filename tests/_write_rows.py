"""The worlds and the comparison rule of the row-write tests (tests/test_gpu_write_rows.py, tests/test_gpu_write_rows_edges.py,
tests/test_write_rows_cpu.py; DESIGN.md §3 "Row writes", §8 "Row writes").  Nothing here needs a GPU until a handle is made.

* `world`: the ORIGINAL world -- n = 4133, three writes of 1, 37 and 700 rows.
* `large_world`: n = 16421, ONE write of 16389 = 2 x 8192 + 5 rows, so that every wave of a list kernel (at most 8192 per
  launch) takes a second row and five waves a third; the list is arranged in three segments, each holding planted rows.
* `wide_world`: n = 4133, one write of 700 rows whose pitch is more than 64 16-byte vectors.
* `outlier_rows`: the rows that raise a maximum which is never lowered.

The planting, per query: an exact copy, a copy scaled by 1e3 (integer spaces: saturated) and the negation of the row that was
rank 1 before the write."""
import dataclasses

import numpy as np

from _util import assert_exact, assert_float_topk
from metrovector_amd import gpu as G

N, K, NQ = 4133, 10, 64
FIXED = (0, 63, 64, 4095, 4096, 4132)
COUNTS = (1, 37, 700)
SEED = 0x57524954
L2, IP, COS = G.L2, G.INNER_PRODUCT, G.COSINE
METRICS = (L2, IP, COS)
F32, F16, I8, U8 = G.FLOAT32, G.FLOAT16, G.INT8, G.UINT8
NP = {F32: np.float32, F16: np.float16, I8: np.int8, U8: np.uint8}
NORMS, S_F16, S_I8, S_6B = 1, 2, 4, 8  # mvfgpu_write_report::refreshed


# ---- the worlds: rows, queries, the changed rows and the three writes that change them --------------------------------------
def _scaled(q, dt):
    if dt in (F32, F16):
        return (q.astype(np.float32) * np.float32(1e3)).astype(NP[dt])
    lo, hi = (-128, 127) if dt == I8 else (0, 255)
    return np.clip(q.astype(np.int64) * 1000, lo, hi).astype(NP[dt])


def _negated(x, dt):
    if dt in (F32, F16):
        return -x
    if dt == I8:
        return np.clip(-x.astype(np.int64), -128, 127).astype(np.int8)
    return (255 - x.astype(np.int64)).astype(np.uint8)


@dataclasses.dataclass
class World:
    dt: int
    dim: int
    rows0: np.ndarray    # before the writes
    rows1: np.ndarray    # behind them
    q: np.ndarray        # [NQ, dim], the query dtype
    writes: list         # [(positions u64, rows)] of 1, 37 and 700 rows
    written: np.ndarray  # every written position
    tag: str = ""        # which world (the key of the cached oracle scores)
    planted: dict = dataclasses.field(default_factory=dict)  # large / wide: segment -> [(query, [planted positions of it there])]
    segments: tuple = ()  # large / wide: the list entries [a, b) of each segment


_WORLDS, _SCORES = {}, {}


def world(oracle, dt, dim):
    key = (dt, dim)
    if key in _WORLDS:
        return _WORLDS[key]
    rows0 = np.ascontiguousarray(oracle.synth_rows(SEED + 16 * dim + dt, 0, N, dim, dt))
    q = np.ascontiguousarray(oracle.synth_queries(SEED + 16 * dim + dt + 7, NQ, dim, dt))
    fresh = oracle.synth_rows(SEED + 16 * dim + dt + 11, 0, sum(COUNTS), dim, dt)
    rank1 = oracle.search(rows0, dt, IP, q, 1)[1][:, 0].astype(np.int64)
    rng = np.random.default_rng(SEED + dim + dt)
    spare = [int(p) for p in rng.permutation(N) if int(p) not in FIXED and int(p) not in set(rank1.tolist())]
    new = {}  # position -> row

    def put(row, pos=None):
        pos = spare.pop() if pos is None else pos
        assert pos not in new
        new[pos] = row
        return pos

    for i, p in enumerate(FIXED):  # the fixed positions hold the first queries' copies
        put(q[i].astype(NP[dt]), p)
    first = list(FIXED)  # the positions of the writes of 1 and 37 rows: the fixed ones, and what the first three queries need
    for i in range(NQ):
        if i >= len(FIXED):
            put(q[i].astype(NP[dt]))
        s = put(_scaled(q[i], dt))
        r = int(rank1[i])
        if r not in new:  # (a rank-1 row that is a fixed position, or another query's too, is overwritten already)
            new[r] = _negated(rows0[r], dt)
        first += [s, r] if i < 3 else []
    first = list(dict.fromkeys(first))
    while len(new) < sum(COUNTS):
        put(fresh[len(new)])
    while len(first) < COUNTS[0] + COUNTS[1]:
        p = next(p for p in new if p not in first)
        first.append(p)
    rest = [p for p in new if p not in first]
    assert first[0] == 0 and len(rest) == COUNTS[2]
    rows1 = rows0.copy()
    for p, row in new.items():
        rows1[p] = row
    writes = []
    for pos in (first[:1], first[1:], rest):
        pos = np.array(pos, np.uint64)
        writes.append((pos, np.ascontiguousarray(rows1[pos.astype(np.int64)])))
    assert [len(w[0]) for w in writes] == list(COUNTS)
    w = World(dt, dim, rows0, rows1, q, writes, np.array(sorted(new), np.int64))
    assert set(FIXED) <= set(w.written.tolist())
    # a property of the reference alone: a write that forgets a shadow or a norm cannot go unseen
    for metric in METRICS:
        top = oracle.search(rows1, dt, metric, q, K)[1].astype(np.int64)
        hit = np.isin(top, w.written).any(axis=1)
        assert hit.all(), f"dtype {dt} dim {dim} metric {metric}: no written row in the top-{K} of queries {np.nonzero(~hit)[0][:5]}"
    _WORLDS[key] = w
    return w


def all_scores(oracle, w, metric, qi):
    """the oracle's score of every changed row for query qi (float spaces), computed once"""
    key = (w.tag, w.dt, w.dim, metric, qi)
    if key not in _SCORES:
        _SCORES[key] = oracle.scores(w.rows1, w.dt, metric, w.q[qi])[0]
    return _SCORES[key]


_F32ROWS = {}


def rows_f32(w):
    key = (w.tag, w.dt, w.dim)
    if key not in _F32ROWS:
        _F32ROWS[key] = w.rows1.astype(np.float32)
    return _F32ROWS[key]


def same(a, b, what):
    """every array of two results, byte for byte (NaN scores included)"""
    assert type(a) is type(b)
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {f.name} differs from the twin's"


def expect_refreshed(shadows):
    """mvfgpu_corpus_info::shadows -> the bits of mvfgpu_write_report::refreshed those shadows need"""
    return (S_I8 if shadows & 5 else 0) | (S_F16 if shadows & 2 else 0) | (S_6B if shadows & 8 else 0)


def check_against_oracle(oracle, w, metric, nq, res, what):
    if w.dt in (I8, U8) and metric != COS:
        assert_exact(res, *oracle.search(w.rows1, w.dt, metric, w.q[:nq], K))
        return
    for qi in range(nq):
        assert_float_topk(metric, res.scores[qi], res.indices[qi], all_scores(oracle, w, metric, qi), rows_f32(w),
                          w.q[qi].astype(np.float32), K)


def bits_promised(dt, path, nq):
    return dt in (I8, U8) or (dt == F32 and nq == 1 and path in (0, 1, 6, 7))


# (data type, scan path, MVF_STREAM_5P1); path 4 streams the f16 shadow for one or two Float32 queries (route_nqs)
ROUTES = ([(F32, p, None) for p in (1, 2, 3, 4, 5, 6)] + [(F32, 7, "0"), (F32, 7, "1")] + [(F16, p, None) for p in (1, 2, 5, 6)] +
          [(I8, 1, None), (I8, 2, None), (U8, 1, None), (U8, 2, None)])
ROUTE_IDS = [f"dt{dt}-path{p}" + (f"-5p1={e}" if e else "") for dt, p, e in ROUTES]


def _handle(rows, path, **kw):
    c = G.GpuCorpus.from_array(rows, **kw)
    c.set_scan_path(path)
    return c


# ---- the comparison rule, for any rows and queries -----------------------------------------------------------------------------
def check_rows_against_oracle(oracle, dt, rows, q, metric, res, what, rows32=None):
    """`res` = a search of the queries `q` over `rows`, against the oracle over those rows: exact integers, the tolerance
    criterion of tests/_util.py elsewhere (what check_against_oracle does for a world's changed rows and its own queries)"""
    if dt in (I8, U8) and metric != COS:
        assert_exact(res, *oracle.search(rows, dt, metric, q, res.scores.shape[1]))
        return
    rows32 = rows.astype(np.float32) if rows32 is None else rows32
    for qi in range(len(q)):
        ref = oracle.scores(rows, dt, metric, q[qi])[0]
        try:
            assert_float_topk(metric, res.scores[qi], res.indices[qi], ref, rows32, q[qi].astype(np.float32), res.scores.shape[1])
        except AssertionError as e:
            raise AssertionError(f"{what}, query {qi}: {e}") from e


def compare(oracle, w, dt, path, metric, nq, got, want, what):
    """the rule of every row-write test: the twin's bytes where the library promises bits, else handle AND twin against the oracle
    over the changed rows"""
    if bits_promised(dt, path, nq):
        same(got, want, what)
    else:
        check_against_oracle(oracle, w, metric, nq, want, what + " (twin)")
    check_against_oracle(oracle, w, metric, nq, got, what)


def route_nqs(path):
    """the batch sizes a route is searched at: scan path 4 streams the f16 shadow for one or two queries and is path 0 beyond"""
    return (1, 2) if path == 4 else (1, 3, NQ)


def row_cost(inf, dt, dim, refreshed):
    """bytes_written per written row of a write that refreshed `refreshed` (include/mvf_gpu_update.h; the whole int8 shadow)"""
    per_row = inf.pitch_bytes
    per_row += (4 if dt == I8 else 8) if refreshed & NORMS else 0
    per_row += ((2 * dim + 15) // 16 * 16 + 4) if refreshed & S_F16 else 0
    per_row += ((dim + 15) // 16 * 16 + 4) if refreshed & S_I8 else 0
    if refreshed & S_6B:
        p51 = dim % 128 == 0 or dim % 128 > 64
        per_row += (96 * ((dim + 127) // 128) if p51 else 48 * ((dim + 63) // 64)) + 4
    return per_row


# ---- the large and the wide world: ONE write, its list in segments ---------------------------------------------------------------
LARGE_N, LARGE_COUNT = 16421, 16389  # 256 whole 6-bit tiles and one of 37; 2 x 8192 + 5 listed rows
LARGE_FIXED = (0, 63, 64, 16383, 16384, 16420)
LARGE_SEGMENTS = ((0, 8192), (8192, 16384), (16384, 16389))
LARGE_DIMS = {F32: (50, 256), F16: (50,), I8: (50,), U8: (50,)}
WIDE_COUNT = 700
WIDE_SEGMENTS = ((0, WIDE_COUNT),)
WIDE_DIMS = {F32: (260, 1030), F16: (520, 1030), I8: (1030,), U8: (1030,)}  # every pitch is more than 64 16-byte vectors


def _planted_world(oracle, tag, dt, dim, n, count, fixed, segments):
    """One write of `count` rows.  Query i's exact copy, 1e3 copy and negated old rank 1 lie together in one segment of the list
    -- the queries are dealt to the whole segments in turn --, except that the LAST five entries are the exact copies of the
    queries 0..4 where the last segment is that short (their other two rows lie in the first segment)."""
    seed = SEED + {"large": 0x10000, "wide": 0x20000}[tag] + 16 * dim + dt
    rows0 = np.ascontiguousarray(oracle.synth_rows(seed, 0, n, dim, dt))
    q = np.ascontiguousarray(oracle.synth_queries(seed + 7, NQ, dim, dt))
    rank1 = oracle.search(rows0, dt, IP, q, 1)[1][:, 0].astype(np.int64)
    rng = np.random.default_rng(seed)
    taken = set(fixed) | set(rank1.tolist())
    spare = [int(p) for p in rng.permutation(n) if int(p) not in taken]
    tail = segments[-1][1] - segments[-1][0] == 5 and len(segments) > 1  # the large world's last segment
    whole = len(segments) - (1 if tail else 0)
    new, seg_of, planted = {}, {}, {s: [] for s in range(len(segments))}

    def put(row, seg, pos=None):
        pos = spare.pop() if pos is None else pos
        assert pos not in new
        new[pos], seg_of[pos] = row, seg
        return pos

    segs = [(i - 5) % whole if tail and i >= 5 else 0 if tail else i % whole for i in range(NQ)]
    copies = [put(q[i].astype(NP[dt]), len(segments) - 1 if tail else segs[i], fixed[i]) for i in range(5)]  # at fixed positions
    # The 1e3 copies' positions ascend through the queries dealt segment by segment in turn: the saturated copies of a UInt8
    # space are one and the same row for most queries, which every query then ranks by position alone.
    by_seg = [[i for i in range(NQ) if segs[i] == s] for s in range(whole)]
    deal = [by_seg[s][r] for r in range(NQ) for s in reversed(range(whole)) if r < len(by_seg[s])]
    scaled_at = dict(zip(deal, sorted(spare.pop() for _ in range(NQ))))
    for i in range(NQ):
        seg = segs[i]
        e = copies[i] if i < 5 else put(q[i].astype(NP[dt]), seg)
        s = put(_scaled(q[i], dt), seg, scaled_at[i])
        mine = [s] if tail and i < 5 else [e, s]
        r = int(rank1[i])
        if r not in new:
            new[r], seg_of[r] = _negated(rows0[r], dt), seg
            mine.append(r)
        planted[seg].append((i, mine))
        if tail and i < 5:
            planted[len(segments) - 1].append((i, [e]))
    put(oracle.synth_rows(seed + 11, 0, 1, dim, dt)[0], None, fixed[-1])
    fresh = oracle.synth_rows(seed + 11, 1, count, dim, dt)
    while len(new) < count:
        put(fresh[len(new)], None)
    # the list: a fixed pseudo-random permutation, then every planted row moved into its segment
    order = [int(p) for p in rng.permutation(np.array(sorted(new), np.int64))]
    last = [p for p in order if seg_of[p] == len(segments) - 1] if tail else []
    order = [p for p in order if p not in set(last)]
    cells = [[p for p in order if seg_of[p] == s] for s in range(whole)]
    free = [p for p in order if seg_of[p] is None]
    lst = []
    for s in range(whole):
        room = segments[s][1] - segments[s][0] - len(cells[s])
        part = cells[s] + [free.pop() for _ in range(room)]
        lst += [part[j] for j in rng.permutation(len(part))]
    lst += sorted(last, key=lambda p: [i for i, m in planted[len(segments) - 1] if p in m][0]) if tail else []
    assert not free and len(lst) == count == len(set(lst)) and set(fixed) <= set(lst)
    pos = np.array(lst, np.uint64)
    for s, (a, b) in enumerate(segments):
        for i, mine in planted[s]:
            assert all(a <= lst.index(p) < b for p in mine)
    rows1 = rows0.copy()
    for p, row in new.items():
        rows1[p] = row
    return World(dt, dim, rows0, rows1, q, [(pos, np.ascontiguousarray(rows1[pos.astype(np.int64)]))], np.array(sorted(new), np.int64),
                 tag, planted, tuple(segments))


def large_world(oracle, dt, dim):
    key = ("large", dt, dim)
    if key not in _WORLDS:
        _WORLDS[key] = _planted_world(oracle, "large", dt, dim, LARGE_N, LARGE_COUNT, LARGE_FIXED, LARGE_SEGMENTS)
    return _WORLDS[key]


def wide_world(oracle, dt, dim):
    key = ("wide", dt, dim)
    if key not in _WORLDS:
        _WORLDS[key] = _planted_world(oracle, "wide", dt, dim, N, WIDE_COUNT, FIXED, WIDE_SEGMENTS)
    return _WORLDS[key]


def planted_rows_show(oracle, w):
    """The property of the reference alone that makes a skipped list entry SHOW: in every segment of the list and under every
    metric, at least five queries have a planted row of that segment in their top-k over the changed rows that is not in their
    top-k over the old rows.  The large world's last segment holds exact copies only: they are rank 1 under L2 and Cosine, and
    under InnerProduct they cannot be in a top-10 -- about half of the other 63 queries' 1e3 copies score higher --, so that
    segment is held under L2 and Cosine (the derived state a write refreshes does not depend on the metric)."""
    for metric in METRICS:
        top0 = oracle.search(w.rows0, w.dt, metric, w.q, K)[1].astype(np.int64)
        top1 = oracle.search(w.rows1, w.dt, metric, w.q, K)[1].astype(np.int64)
        for s, (a, b) in enumerate(w.segments):
            if b - a == 5 and metric == IP:
                continue
            shows = [i for i, mine in w.planted[s] if any(p in top1[i] and p not in top0[i] for p in mine)]
            need = len(w.planted[s]) if b - a == 5 else 5
            assert len(shows) >= need, (f"{w.tag} world dtype {w.dt} dim {w.dim} metric {metric}: list entries [{a}, {b}) show in the "
                                        f"top-{K} of the queries {shows} only")


# ---- rows that raise a maximum ------------------------------------------------------------------------------------------------
OUTLIER_AT = (64, 4100)
OUTLIER_KINDS = {F32: ("huge", "overflowing", "non-finite"), F16: ("huge", "non-finite")}


def outlier_rows(dt, dim, kind, like):
    """two rows of a float space for the positions OUTLIER_AT.  huge: every element 1e18 (Float16: 60000), the sum of squares
    finite in f32; overflowing (Float32): every element 3e19, each finite and their squares' sum +inf; non-finite: the rows
    `like` [2, dim] with one +Inf and one NaN element."""
    t = NP[dt]
    if kind == "huge":
        return np.full((2, dim), 1e18 if dt == F32 else 60000.0, t)
    if kind == "overflowing":
        assert dt == F32
        return np.full((2, dim), 3e19, t)
    bad = np.array(like, t, copy=True)
    bad[0, 3], bad[1, dim - 1] = np.inf, np.nan
    return bad


def extreme_queries(dt, dim, q):
    """the all-zero query, one of norm about 1e-20 and one of norm about 1e15 (Float16 rows: 1e3), along the query q"""
    unit = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))
    return {"zero": np.zeros(dim, np.float32), "tiny": (unit * 1e-20).astype(np.float32),
            "big": (unit * (1e15 if dt == F32 else 1e3)).astype(np.float32)}


# ---- device sources -------------------------------------------------------------------------------------------------------------
def device_source(rows, stride, offset=0):
    """-> (a device tensor holding `rows` at `stride` bytes from byte `offset` on, 0xFF between them; the address of the first)"""
    import torch
    row_bytes = rows.shape[1] * rows.itemsize
    host = np.full(offset + len(rows) * stride, 0xFF, np.uint8)
    flat = np.ascontiguousarray(rows).view(np.uint8).reshape(len(rows), row_bytes)
    for i in range(len(rows)):
        host[offset + i * stride:offset + i * stride + row_bytes] = flat[i]
    dev = torch.from_numpy(host).cuda()
    return dev, dev.data_ptr() + offset
