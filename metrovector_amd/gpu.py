"""GpuCorpus — Python face of one HBM-resident row-range shard
(`mvfgpu_corpus`, include/mvf_gpu.h).

The search replaces the reference's `find_top_k_similar`
(examples/similarity_search.rs:140-176).  Everything numeric happens in
libmvf_gpu.so (HIP, gfx950); this module only marshals pointers.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _lib
from .errors import BuildError, InvalidArgument

# schema/types.fbs codes
FLOAT32, FLOAT16, INT8, UINT8 = 0, 1, 2, 3
L2, INNER_PRODUCT, COSINE = 0, 1, 2

_NP_OF = {FLOAT32: np.float32, FLOAT16: np.float16, INT8: np.int8, UINT8: np.uint8}
_CODE_OF = {np.dtype(np.float32): FLOAT32, np.dtype(np.float16): FLOAT16,
            np.dtype(np.int8): INT8, np.dtype(np.uint8): UINT8}


def query_dtype_code(space_dtype: int) -> int:
    """Float32 queries for Float32/Float16 spaces (Vector::as_f32 widens,
    src/vectors/vector.rs:81-89); Int8/UInt8 spaces take their own type."""
    return FLOAT32 if space_dtype in (FLOAT32, FLOAT16) else space_dtype


def device_count() -> int:
    n = C.c_int(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_device_count(C.byref(n)))
    return n.value


@dataclass
class SearchResult:
    scores: np.ndarray   # f32 [nq, k]
    indices: np.ndarray  # u64 [nq, k]
    raw: np.ndarray      # i32 [nq, k] (exact integer score on Int8/UInt8 spaces)


@dataclass
class MaxSimResult:
    scores: np.ndarray   # f32 [nq, k]: a key's sum over the query's vectors of that vector's best score among the key's rows
    keys: np.ndarray     # u64 [nq, k]: the column values, best first (UINT64_MAX pads -- `counts` tells it from a real key)
    counts: np.ndarray   # u32 [nq]: min(k, keys of the partition), the entries of a row that are no padding


@dataclass
class MaxSimAlignment:
    """Each listed key's best row per query token (`GpuCorpus.maxsim_align`), in list order; padding where a key is not held."""
    rows: np.ndarray     # u64 [nq, m, n_tokens]: the row as every search reports it (UINT64_MAX pads)
    scores: np.ndarray   # f32 [nq, m, n_tokens]: its score for the token; summed in token order, the key's MaxSim score
    raw: np.ndarray      # i32 [nq, m, n_tokens] (exact integer score on Int8/UInt8 spaces)


@dataclass
class MaxSimSelection:
    """What the MFMA selection route held on the device for one call (`GpuCorpus.maxsim_mfma_selection`); keys in ascending value."""
    sums: np.ndarray        # f32 [nq, n_keys]: the approximate sums as the candidate rule read them
    forced: np.ndarray      # bool [nq, n_keys]: keys the scoring kernel forced, before the rule
    candidates: np.ndarray  # bool [nq, n_keys]: the candidates, behind the rule
    delta: np.ndarray       # f64 [nq]: the bound the device computed
    theta: np.ndarray       # f32 [nq]: the min(k, n_keys)-th best approximate sum the rule compared with
    theta_nan: np.ndarray   # bool [nq]: that entry was the live NaN entry
    xxmax: float            # the largest sum of squares of a stored row, as the rule read it


@dataclass
class RadiusResult:
    counts: np.ndarray   # u64 [nq]: exact number of matches per query (also beyond max_per_query)
    scores: np.ndarray   # f32 [nq, max_per_query]: the best min(count, max_per_query) matches, best first, then padding
    indices: np.ndarray  # u64 [nq, max_per_query] (UINT64_MAX = padding)
    raw: np.ndarray      # i32 [nq, max_per_query] (exact integer score on Int8/UInt8 spaces)

    @property
    def overflowed(self) -> np.ndarray:
        """Queries whose matches did not fit the device list (MVFGPU_RADIUS_LIST_CAP) and that the library completed
        through the top-k search (only when max_per_query > 0)."""
        return self.counts > RADIUS_LIST_CAP if self.scores.shape[1] > 0 else np.zeros(self.counts.shape, bool)


RADIUS_LIST_CAP = 8192  # include/mvf_gpu.h MVFGPU_RADIUS_LIST_CAP
JOIN_WINDOW = 1024      # include/mvf_gpu.h MVFGPU_JOIN_WINDOW
JOIN_EXCLUDE_SELF = 1   # include/mvf_gpu.h MVFGPU_JOIN_EXCLUDE_SELF


@dataclass
class CandidateResult(SearchResult):
    counts: np.ndarray   # u64 [nq]: distinct live in-shard candidates per query; the first min(count, k) entries are real


MMR_MAX_CANDIDATES = 1024  # include/mvf_gpu_mmr.h MVFGPU_MMR_MAX_CANDIDATES


@dataclass
class MmrResult(CandidateResult):
    objective: np.ndarray  # f32 [nq, k]: lambda * rel of pick 0, the objective of the later picks, the padding score behind them


def mmr_walk(rel_scores, sim_scores, metric: int, lambda_mult: float, k: int) -> tuple[np.ndarray, np.ndarray, int]:
    """The greedy walk of the diversified re-ranking on the host, with the device's arithmetic
    (`mvfgpu_selftest_mmr_walk`, include/mvf_gpu_mmr.h; no GPU needed): `rel_scores` [m] and `sim_scores` [m, m]
    (`sim_scores[s, d]`: row s as the query) in score form -> (the picks' positions [k], UINT32_MAX behind them; the
    objective [k]; the number of picks)."""
    rel = np.ascontiguousarray(rel_scores, np.float32).reshape(-1)
    m = rel.size
    sim = np.ascontiguousarray(sim_scores, np.float32)
    if sim.size != m * m:
        raise InvalidArgument(f"sim_scores must hold {m} x {m} scores, got shape {sim.shape}")
    k = int(k)
    if k < 0:
        raise InvalidArgument("k must be >= 0")
    order = np.empty(max(k, 1), np.uint32)
    obj = np.empty(max(k, 1), np.float32)
    n = _lib.gpu().mvfgpu_selftest_mmr_walk(rel.ctypes.data_as(C.c_void_p) if m else None, sim.ctypes.data_as(C.c_void_p) if m else None,
                                            m, metric, float(lambda_mult), k, order.ctypes.data_as(C.c_void_p),
                                            obj.ctypes.data_as(C.c_void_p))
    if n < 0:
        _lib.gpu_check(-n)
    return order[:k], obj[:k], int(n)


class MmrForm(NamedTuple):
    G: int      # lanes per row
    J: int      # 16-byte steps per lane
    qlds: bool  # the picked row is staged as a query in LDS; False: through the query's f32 scratch row and the cache


def mmr_form(dtype: int, dim: int, forced_g: int = 0) -> MmrForm:
    """The instantiation of the diversified re-ranking's walk kernel for rows of `dim` elements of `dtype` (a data type code),
    under the library's lane-group rule or the width `MVF_K1_G` = `forced_g` forces: `mvfgpu_selftest_mmr_form`; no GPU needed."""
    out = [C.c_uint32(0) for _ in range(3)]
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_mmr_form(dtype, dim, forced_g, *[C.byref(o) for o in out]))
    return MmrForm(out[0].value, out[1].value, bool(out[2].value))


def radius_bound(data_type: int, metric: int, radius: float) -> tuple[int, int]:
    """(largest matching order key, exact i32 bound of Int8/UInt8 L2/InnerProduct spaces) of a radius --
    `mvfgpu_selftest_radius_bound`; no GPU needed."""
    key, raw = C.c_uint32(0), C.c_int32(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_radius_bound(data_type, metric, float(radius), C.byref(key), C.byref(raw)))
    return key.value, raw.value


def radius_route(data_type: int, nq: int, scan_path: int = 0) -> int:
    """0: the streaming radius kernel serves the batch, 1: one thresholded batched MFMA pass + exact re-scoring --
    `mvfgpu_selftest_radius_route`; no GPU needed."""
    out = C.c_uint32(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_radius_route(data_type, nq, scan_path, C.byref(out)))
    return out.value


def stream_rows(rows: int, dim: int, data_type: int, metric: int, nq: int, k: int) -> int:
    """1: on scan path 0 the search streams the int8 shadow of the Float32 rows (re-scored with K1's arithmetic: the
    same bits as the stored rows), 0: K1 reads the stored rows -- the shape part of the rule, default tuning;
    `mvfgpu_selftest_stream_rows`; no GPU needed."""
    out = C.c_uint32(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_stream_rows(rows, dim, data_type, metric, nq, k, C.byref(out)))
    return out.value


def stream_bits(rows: int, dim: int, data_type: int, metric: int, nq: int, k: int) -> int:
    """Which rows ONE search on scan path 0 streams: 0 the stored rows, 8 the int8 shadow, 6 the 6-bit shadow -- the shape part
    of the rule, default tuning; `mvfgpu_selftest_stream_bits`; no GPU needed."""
    out = C.c_uint32(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_stream_bits(rows, dim, data_type, metric, nq, k, C.byref(out)))
    return out.value


def selftest_poison() -> int:
    """The byte MVF_DEBUG_POISON makes this process fill every allocation of the library with before its first use, or -1
    where the switch is unset -- `mvfgpu_selftest_poison`; no GPU needed."""
    return int(_lib.gpu().mvfgpu_selftest_poison())


def shadow6_bytes(rows: int, dim: int) -> int:
    """Bytes of the 6-bit shadow of `rows` x `dim` (64-row tiles of 64-element units: csrc/shadow_6b.h); no GPU needed."""
    return int(_lib.gpu().mvfgpu_selftest_shadow6_bytes(rows, dim))


def shadow51_bytes(rows: int, dim: int) -> int:
    """Bytes of the 5+1 layout of the 6-bit shadow of `rows` x `dim` (64-row tiles of 128-element units: csrc/shadow_5p1.h); no
    GPU needed."""
    return int(_lib.gpu().mvfgpu_selftest_shadow51_bytes(rows, dim))


def shadow51_pack(codes: np.ndarray) -> np.ndarray:
    """`codes` (rows x dim int8 in [-31, 31]) in the 5+1 layout, as the build kernel packs them; no GPU needed."""
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    rows, dim = codes.shape
    out = np.empty(shadow51_bytes(rows, dim), np.uint8)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_shadow51_pack(codes.ctypes.data, rows, dim, out.ctypes.data, out.size))
    return out


def shadow51_unpack(shadow: np.ndarray, rows: int, dim: int) -> np.ndarray:
    """The codes (rows x dim int8) held by a shadow in the 5+1 layout; no GPU needed."""
    shadow = np.ascontiguousarray(shadow, dtype=np.uint8)
    out = np.empty((rows, dim), np.int8)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_shadow51_unpack(shadow.ctypes.data, shadow.size, rows, dim, out.ctypes.data))
    return out


def shadow6_pack(codes: np.ndarray) -> np.ndarray:
    """`codes` (rows x dim int8 in [-31, 31]) in the 6-bit shadow's layout, as the build kernel packs them; no GPU needed."""
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    rows, dim = codes.shape
    out = np.empty(shadow6_bytes(rows, dim), np.uint8)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_shadow6_pack(codes.ctypes.data, rows, dim, out.ctypes.data, out.size))
    return out


def shadow6_unpack(shadow: np.ndarray, rows: int, dim: int) -> np.ndarray:
    """The codes (rows x dim int8) held by a 6-bit shadow; no GPU needed."""
    shadow = np.ascontiguousarray(shadow, dtype=np.uint8)
    out = np.empty((rows, dim), np.int8)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_shadow6_unpack(shadow.ctypes.data, shadow.size, rows, dim, out.ctypes.data))
    return out


def filter_route(rows: int, dim: int, data_type: int, nq: int, k: int, admitted: int) -> int:
    """1: a filtered search of this shape takes the mask route (the plain search's kernels under the filter's deny mask),
    2: the list route (only the admitted rows are read) -- default tuning; `mvfgpu_selftest_filter_route`; no GPU needed."""
    out = C.c_uint32(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_filter_route(rows, dim, data_type, nq, k, admitted, C.byref(out)))
    return out.value


def _query_args(queries) -> tuple[np.ndarray, int, int, int]:
    """(the queries as a contiguous 2-D array -- a 1-D array is one query --, their data type's code, nq, their dimension)"""
    q = np.asarray(queries)
    if q.ndim == 1:
        q = q[None, :]
    qcode = _CODE_OF.get(q.dtype)
    if qcode is None:
        raise BuildError(f"unsupported query dtype {q.dtype}")
    q = np.ascontiguousarray(q)
    return q, qcode, q.shape[0], q.shape[1]


def _result_arrays(nq: int, k: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(scores, indices, raw) of a search, for the library to fill"""
    return np.empty((nq, k), np.float32), np.empty((nq, k), np.uint64), np.empty((nq, k), np.int32)


def _opt(p: int):
    """an optional device pointer or stream: 0 is NULL"""
    return C.c_void_p(p) if p else None


class _OwnedHandle:
    """What a GpuCorpus made and what is closed before it: the handle, the corpus it belongs to, and `_destroy`, the name of
    the library function that frees it.  A context manager."""
    _destroy = ""

    def __init__(self, handle: int, corpus: "GpuCorpus"):
        self._h = C.c_void_p(handle)
        self._corpus = corpus  # keeps the handle it belongs to alive

    def close(self) -> None:
        if self._h is not None and self._h.value and self._corpus._h is not None:
            getattr(_lib.gpu(), self._destroy)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _open_handle(obj, cls: type, what: str) -> C.c_void_p:
    """the handle of `obj`, which must be an open `cls`"""
    if not isinstance(obj, cls) or obj._h is None:
        raise InvalidArgument(f"{what} must be an open {cls.__name__} of this corpus")
    return obj._h


def pack_allow_mask(allow, rows: int | None = None) -> np.ndarray:
    """The packed uint8 bitmap (`bitorder="little"`) of a filter's rows: a bool array has one entry per row and is packed;
    a uint8 array is taken as already packed.  `rows` (a bool mask's required length) is checked when given.  Anything else
    is refused with InvalidArgument."""
    a = allow if isinstance(allow, np.ndarray) else np.asarray(allow)
    if a.ndim != 1:
        raise InvalidArgument(f"the allow mask must be 1-D, got shape {a.shape}")
    if a.dtype == np.bool_:
        if rows is not None and a.size != rows:
            raise InvalidArgument(f"the allow mask holds {a.size} entries for {rows} rows")
        return np.packbits(a, bitorder="little")
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    raise InvalidArgument(f"the allow mask must be a bool array over rows or a packed uint8 bitmap, got {a.dtype}")


class GpuFilter(_OwnedHandle):
    """An immutable set of admitted rows of one GpuCorpus (`mvfgpu_filter`): made once by `GpuCorpus.make_filter`, used by
    any number of `search_filtered` calls, closed before its corpus.  A context manager."""

    _destroy = "mvfgpu_filter_destroy"

    def info(self) -> _lib.FilterInfo:
        out = _lib.FilterInfo()
        _lib.gpu_check(_lib.gpu().mvfgpu_filter_get_info(self._h, C.byref(out)))
        return out

    @property
    def admitted(self) -> int:
        return self.info().admitted


UINT32, UINT64 = 4, 5  # schema/types.fbs: the data types of a device column
_COLUMN_CODE_OF = {np.dtype(np.uint32): UINT32, np.dtype(np.uint64): UINT64}
_OP_OF = {"==": _lib.OP_EQ, "!=": _lib.OP_NE, "<": _lib.OP_LT, "<=": _lib.OP_LE, ">": _lib.OP_GT, ">=": _lib.OP_GE,
          "between": _lib.OP_BETWEEN, "in": _lib.OP_IN, "not in": _lib.OP_NOT_IN}


def predicate_range(data_type: int, op: str | int, a: int = 0, b: int = 0) -> tuple[int, int, int]:
    """(lo, hi, negate) of a comparison after the host-side normalisation: lo <= v <= hi, negated where negate is 1; an
    empty range is (1, 0) -- `mvfgpu_selftest_predicate_range`; no GPU needed."""
    lo, hi, neg = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    code = _OP_OF[op] if isinstance(op, str) else int(op)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_predicate_range(data_type, code, a, b, C.byref(lo), C.byref(hi), C.byref(neg)))
    return lo.value, hi.value, neg.value


class GpuColumn(_OwnedHandle):
    """One UInt32 / UInt64 value per row of one GpuCorpus, resident next to the rows (`mvfgpu_column`): made by
    `GpuCorpus.attach_column`, used by any number of `make_filter_where` calls, closed before its corpus.  A context manager."""

    _destroy = "mvfgpu_column_destroy"

    def info(self) -> _lib.ColumnInfo:
        out = _lib.ColumnInfo()
        _lib.gpu_check(_lib.gpu().mvfgpu_column_get_info(self._h, C.byref(out)))
        return out

    def gather(self, indices) -> np.ndarray:
        """The column's values, as uint64, of the rows `indices` name -- what a search on the column's corpus reports (global
        positions, or vector ids where attached), in any shape (`mvfgpu_column_gather`).  Padding (UINT64_MAX) gives 0."""
        if self._h is None:
            raise InvalidArgument("the column is closed")
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        out = np.zeros(idx.shape, np.uint64)
        _lib.gpu_check(_lib.gpu().mvfgpu_column_gather(self._h, idx.ctypes.data_as(C.c_void_p), idx.size, out.ctypes.data_as(C.c_void_p)))
        return out


class GpuPartition(_OwnedHandle):
    """The live rows of one GpuCorpus grouped by a column's value (`mvfgpu_partition`): made once by
    `GpuCorpus.make_partition`, used by any number of `search_partitioned` calls, closed before its corpus.  A context manager."""

    _destroy = "mvfgpu_partition_destroy"

    def info(self) -> _lib.PartitionInfo:
        out = _lib.PartitionInfo()
        _lib.gpu_check(_lib.gpu().mvfgpu_partition_get_info(self._h, C.byref(out)))
        return out

    def lookup(self, keys) -> np.ndarray:
        """The live rows carrying each of `keys` (0 for an unknown key), from the host mirror: no device work."""
        kk = _keys_u64(keys)
        out = np.zeros(kk.size, np.uint64)
        _lib.gpu_check(_lib.gpu().mvfgpu_partition_lookup(self._h, kk.ctypes.data_as(C.c_void_p), kk.size, out.ctypes.data_as(C.c_void_p)))
        return out

    def keys(self) -> tuple[np.ndarray, np.ndarray]:
        """(the distinct keys in ascending order, their row counts): the column's group-by over the live rows."""
        n = self.info().n_keys
        kk, cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        _lib.gpu_check(_lib.gpu().mvfgpu_partition_keys(self._h, 0, n, kk.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
        return kk, cnt


def partition_plan(counts, keys, k: int) -> tuple[np.ndarray, int]:
    """(tier per query: 0 padding / 1 small / 2 large, gathered searches of the large tier) of a partitioned search whose
    queries' keys hold `counts` live rows -- `mvfgpu_selftest_partition_plan`; no GPU needed."""
    cc, kk = _keys_u64(counts), _keys_u64(keys)
    if cc.size != kk.size:
        raise InvalidArgument("counts and keys must have one entry per query")
    tier, groups = np.zeros(max(cc.size, 1), np.uint32), C.c_uint32(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_partition_plan(cc.ctypes.data_as(C.c_void_p), kk.ctypes.data_as(C.c_void_p), cc.size, k,
                                                             tier.ctypes.data_as(C.c_void_p), C.byref(groups)))
    return tier[:cc.size], groups.value


def group_plan(run_lengths, crossing, per_key: int) -> np.ndarray:
    """The tier (0 all kept / 1 ranked by counting / 2 one wave's running best) of every run -- what one 1024-entry tile of a
    grouped search's key-ordered list holds of one key -- of `run_lengths` entries whose key does (`crossing`) or does not go
    on in another tile: `mvfgpu_selftest_group_plan`; no GPU needed."""
    ll = _keys_u64(run_lengths)
    cr = np.ascontiguousarray(np.asarray(crossing).reshape(-1), dtype=np.uint8)
    if ll.size != cr.size:
        raise InvalidArgument("run_lengths and crossing must have one entry per run")
    tier = np.zeros(max(ll.size, 1), np.uint32)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_group_plan(ll.ctypes.data_as(C.c_void_p), cr.ctypes.data_as(C.c_void_p), ll.size, per_key,
                                                         tier.ctypes.data_as(C.c_void_p)))
    return tier[:ll.size]


def maxsim_plan(n_keys: int, n_tokens: int, nq: int, token_bytes: int, budget_bytes: int) -> tuple[int, int]:
    """(tokens per chunk, query sets per window) of a multi-vector search over `n_keys` keys with `n_tokens` tokens per set,
    `nq` sets, padded tokens of `token_bytes` and a scratch budget: `mvfgpu_selftest_maxsim_plan`; no GPU needed."""
    chunk, window = C.c_uint32(0), C.c_uint32(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_plan(n_keys, n_tokens, nq, token_bytes, budget_bytes, C.byref(chunk), C.byref(window)))
    return chunk.value, window.value


def maxsim_align_plan(n_keys: int, n_tokens: int, nq: int, token_bytes: int, budget_bytes: int) -> tuple[int, int]:
    """(tokens per chunk, query sets per window) of an alignment call (`GpuCorpus.maxsim_align`) whose windows hold up to `n_keys`
    distinct keys per set, inside what the scratch budget leaves beside the list and the slot map:
    `mvfgpu_selftest_maxsim_align_plan`; no GPU needed."""
    chunk, window = C.c_uint32(0), C.c_uint32(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_align_plan(n_keys, n_tokens, nq, token_bytes, budget_bytes, C.byref(chunk), C.byref(window)))
    return chunk.value, window.value


class MaxSimForm(NamedTuple):
    G: int              # lanes per row
    J: int              # 16-byte steps per lane
    token_bytes: int    # a padded token
    form: int           # 0 rows in registers, 1 rows read again per token group, 2 .. and float tokens read through the cache
    lds_chunk_cap: int  # tokens per chunk for 1024 tokens and an unbounded budget


def maxsim_form(dtype: int, dim: int, forced_g: int = 0) -> MaxSimForm:
    """The instantiation of the multi-vector search's scoring kernel for rows of `dim` elements of `dtype` (a data type code),
    under the library's lane-group rule or the width `MVF_K1_G` = `forced_g` forces: `mvfgpu_selftest_maxsim_form`; no GPU needed."""
    out = [C.c_uint32(0) for _ in range(5)]
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_form(dtype, dim, forced_g, *[C.byref(o) for o in out]))
    return MaxSimForm(*[o.value for o in out])


def maxsim_route(held_rows: int, n_keys: int, dim: int, dtype: int, metric: int, nq: int, n_tokens: int, k: int, forced: int = 0) -> int:
    """The route of a full multi-vector search -- 1: the one-pass route, 2: the MFMA selection route -- for `forced` = 0 (automatic),
    1 or 2 (`GpuCorpus.set_maxsim_route`, `MVF_MAXSIM_ROUTE`): `mvfgpu_selftest_maxsim_route`; no GPU needed."""
    out = C.c_uint32(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_route(held_rows, n_keys, dim, dtype, metric, nq, n_tokens, k, forced, C.byref(out)))
    return out.value


def maxsim_margin(dtype: int, metric: int, dim: int, token_norms, xxmax: float) -> float:
    """The bound of |approximate sum - exact sum| the MFMA selection route holds for one query set whose tokens have the f32
    norms `token_norms`, over rows whose largest sum of squares is `xxmax`: `mvfgpu_selftest_maxsim_margin`; no GPU needed."""
    tn = np.ascontiguousarray(np.asarray(token_norms).reshape(-1), dtype=np.float32)
    out = C.c_double(0.0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_margin(dtype, metric, dim, tn.ctypes.data_as(C.c_void_p) if tn.size else None, tn.size,
                                                            float(np.float32(xxmax)), C.byref(out)))
    return out.value


def maxsim_candidates_plan(candidate_keys, held_counts) -> tuple[np.ndarray, int, int]:
    """(slot ordinals [m], distinct held candidates, the rows they hold) of ONE query set's candidate list, given every entry's
    held row count (`GpuPartition.lookup`'s): `mvfgpu_selftest_maxsim_candidates_plan`; no GPU needed.  A slot of UINT32_MAX
    marks an entry that is skipped (no held row) or repeats an earlier one."""
    ck = _keys_u64(candidate_keys)
    hc = np.ascontiguousarray(np.asarray(held_counts).reshape(-1), dtype=np.uint64)
    if ck.size != hc.size:
        raise InvalidArgument("candidate_keys and held_counts must have one entry per candidate")
    slot = np.zeros(max(ck.size, 1), np.uint32)
    distinct, rows = C.c_uint32(0), C.c_uint64(0)
    _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_candidates_plan(ck.ctypes.data_as(C.c_void_p), hc.ctypes.data_as(C.c_void_p), ck.size,
                                                                     slot.ctypes.data_as(C.c_void_p), C.byref(distinct), C.byref(rows)))
    return slot[:ck.size], distinct.value, rows.value


def _candidate_lists(candidate_keys, nq: int) -> np.ndarray:
    """[nq, m] uint64 from one list [m] (shared by every set) or [nq, m]"""
    if candidate_keys is None:
        return np.zeros((nq, 0), np.uint64)
    a = np.asarray(candidate_keys)
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[0] != nq):
        raise InvalidArgument(f"candidate_keys must be [m] or [{nq}, m], got shape {a.shape}")
    m = a.shape[-1]
    flat = _keys_u64(a).reshape(-1, m) if m else np.zeros((a.shape[0] if a.ndim == 2 else 1, 0), np.uint64)
    return np.ascontiguousarray(np.broadcast_to(flat, (nq, m)))


def _keys_u64(keys) -> np.ndarray:
    if isinstance(keys, np.ndarray) and keys.dtype.kind == "u":
        return np.ascontiguousarray(keys.reshape(-1), dtype=np.uint64)
    return np.array([_u64(x, "key") for x in np.asarray(keys, dtype=object).reshape(-1)], dtype=np.uint64)


def _u64(x, what: str) -> int:
    v = int(x)
    if v < 0 or v >= 1 << 64:
        raise InvalidArgument(f"{what} {v} is no unsigned 64-bit value")
    return v


def _pack_clauses(clauses) -> tuple[C.Array, list]:
    """(mvfgpu_predicate array, the arrays it points into) of [(column, op, operand), ...]"""
    clauses = list(clauses)
    arr = (_lib.Predicate * max(len(clauses), 1))()
    keep = []
    for i, cl in enumerate(clauses):
        if not isinstance(cl, (tuple, list)) or len(cl) != 3:
            raise InvalidArgument("a clause is (column, op, operand)")
        col, op, operand = cl
        hcol = _open_handle(col, GpuColumn, "a clause's column")
        code = _OP_OF.get(op) if isinstance(op, str) else None
        if code is None:
            raise InvalidArgument(f"unknown predicate op {op!r}: one of {', '.join(_OP_OF)}")
        arr[i].column, arr[i].op = hcol, code
        if code in (_lib.OP_IN, _lib.OP_NOT_IN):
            if isinstance(operand, np.ndarray) and operand.dtype == np.uint64 and operand.ndim == 1:
                vals = np.ascontiguousarray(operand)
            else:
                vals = np.array([_u64(x, "set value") for x in operand], dtype=np.uint64)
            keep.append(vals)
            arr[i].n_values = vals.size
            arr[i].values = vals.ctypes.data if vals.size else None
        elif code == _lib.OP_BETWEEN:
            lo, hi = operand
            arr[i].a, arr[i].b = _u64(lo, "operand"), _u64(hi, "operand")
        else:
            arr[i].a = _u64(operand, "operand")
    return arr, keep


def _write_report(rep: "_lib.WriteReport") -> dict:
    return {"launches": rep.launches, "rows_written": rep.rows_written, "bytes_written": rep.bytes_written, "refreshed": rep.refreshed}


class GpuCorpus:
    """One shard of a vector space, resident in HBM on one MI355X."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)
        self._shape = None  # (rows, dimension, data_type): fixed for the life of the handle, asked for once

    # ---- construction ------------------------------------------------------
    @classmethod
    def from_pointer(cls, ptr: int, rows: int, dimension: int, data_type: int, stride_bytes: int,
                     device: int = 0, index_base: int = 0, prepare_batched: bool = False, pinned_staging: bool | None = None,
                     chunk_mib: int = 0) -> "GpuCorpus":
        """What a Rust caller passes: VectorSlice::as_ptr / stride / count
        (src/vectors/mem.rs:75-77, vector_space.rs:155-188).  `prepare_batched` builds the row norms and (Float32
        spaces) the f16 shadow chunk by chunk beside the copy (`mvfgpu_corpus_create_ex`)."""
        h = C.c_void_p()
        flags = _lib.UPLOAD_EAGER_SHADOW if prepare_batched else 0
        if pinned_staging is not None:  # None: the library's choice (pinned staging from 256 MiB up)
            flags |= _lib.UPLOAD_PINNED_STAGING if pinned_staging else _lib.UPLOAD_PAGEABLE
        opts = _lib.UploadOptions(C.sizeof(_lib.UploadOptions), flags, chunk_mib, 0)
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_create_ex(C.c_void_p(ptr), rows, dimension, data_type, stride_bytes,
                                                          device, index_base, C.byref(opts), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_array(cls, rows: np.ndarray, device: int = 0, index_base: int = 0, **upload) -> "GpuCorpus":
        if rows.ndim != 2:
            raise InvalidArgument("rows must be a 2-D array")
        code = _CODE_OF.get(rows.dtype)
        if code is None:
            raise BuildError("Unsupported vector data type")
        if rows.shape[0] and rows.strides[1] != rows.itemsize:
            rows = np.ascontiguousarray(rows)
        stride = rows.strides[0] if rows.shape[0] else rows.shape[1] * rows.itemsize
        return cls.from_pointer(rows.ctypes.data, rows.shape[0], rows.shape[1], code, stride, device, index_base, **upload)

    @classmethod
    def synthetic(cls, rows: int, dimension: int, data_type: int, seed: int, row0: int = 0,
                  device: int = 0) -> "GpuCorpus":
        h = C.c_void_p()
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_create_synthetic(rows, dimension, data_type, seed, row0, device,
                                                                 C.byref(h)))
        return cls(h.value)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            _lib.gpu().mvfgpu_corpus_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- deletions / ids (schema/core.fbs:35-39, :54) ---------------------------
    def set_tombstones(self, bitmap: np.ndarray | None, first_bit: int = 0) -> None:
        """Mask deleted rows: bit (first_bit + r) of `bitmap` (uint8, LSB first) = local row r is deleted."""
        if bitmap is None:
            _lib.gpu_check(_lib.gpu().mvfgpu_corpus_set_tombstones(self._h, None, 0, 0))
            return
        b = np.ascontiguousarray(bitmap, np.uint8)
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_set_tombstones(self._h, b.ctypes.data_as(C.c_void_p), first_bit, b.size * 8))

    def set_vector_ids(self, ids: np.ndarray | None) -> None:
        """Report ids[row] instead of index_base + row."""
        if ids is None:
            _lib.gpu_check(_lib.gpu().mvfgpu_corpus_set_vector_ids(self._h, None, 0))
            return
        a = np.ascontiguousarray(ids, np.uint64)
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_set_vector_ids(self._h, a.ctypes.data_as(C.c_void_p), a.size))

    # ---- introspection -------------------------------------------------------
    def info(self) -> _lib.CorpusInfo:
        out = _lib.CorpusInfo()
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_get_info(self._h, C.byref(out)))
        return out

    def _fixed(self) -> tuple[int, int, int]:
        if self._shape is None:
            inf = self.info()
            self._shape = (inf.rows, inf.dimension, inf.data_type)
        return self._shape

    @property
    def rows(self) -> int:
        return self._fixed()[0]

    @property
    def dimension(self) -> int:
        return self._fixed()[1]

    @property
    def data_type(self) -> int:
        return self._fixed()[2]

    def read_rows(self, first: int, count: int) -> np.ndarray:
        _, dim, dt = self._fixed()
        out = np.empty((count, dim), _NP_OF[dt])
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_read_rows(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def gather_rows(self, indices) -> np.ndarray:
        """Rows by GLOBAL index, in the order given (`mvfgpu_corpus_gather_rows`): the payload of the
        reference's ScoredVector.vector, served from HBM."""
        _, dim, dt = self._fixed()
        idx = np.ascontiguousarray(np.asarray(indices).reshape(-1), np.uint64)
        out = np.empty((idx.size, dim), _NP_OF[dt])
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_gather_rows(self._h, idx.ctypes.data_as(C.c_void_p), idx.size,
                                                            out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- row writes (include/mvf_gpu_update.h) ---------------------------------------
    def write_rows(self, indices, rows: np.ndarray) -> dict:
        """New bytes into row positions (`mvfgpu_corpus_write_rows`; DESIGN.md §3 "Row writes"): `rows` [m, dimension] of the
        stored dtype go to `indices` [m] -- global positions, or vector ids where ids are attached --, every derived array
        that is resident (norms, shadows) is refreshed for exactly those rows, and the call returns when the write is
        complete.  A row named twice is refused.  Returns the report: launches, rows_written, bytes_written, refreshed
        (bit 0 norms, 1 f16 shadow, 2 int8 shadow, 3 6-bit shadow)."""
        _, dim, dt = self._fixed()
        rows = np.asarray(rows)
        if rows.dtype != _NP_OF[dt]:
            raise InvalidArgument(f"rows must have the space's stored dtype {np.dtype(_NP_OF[dt]).name}, got {rows.dtype.name}")
        idx = np.ascontiguousarray(np.asarray(indices).reshape(-1), np.uint64)
        if rows.ndim != 2 or rows.shape != (idx.size, dim):
            raise InvalidArgument(f"rows must be [{idx.size}, {dim}] (one row per index), got shape {rows.shape}")
        if rows.shape[0] and rows.strides[1] != rows.itemsize:
            rows = np.ascontiguousarray(rows)
        stride = rows.strides[0] if rows.shape[0] > 1 else dim * rows.itemsize
        if stride < dim * rows.itemsize:  # a broadcast or reversed view
            rows = np.ascontiguousarray(rows)
            stride = dim * rows.itemsize
        rep = _lib.WriteReport()
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_write_rows(self._h, idx.ctypes.data_as(C.c_void_p) if idx.size else None, idx.size,
                                                           rows.ctypes.data_as(C.c_void_p) if idx.size else None, stride, C.byref(rep)))
        return _write_report(rep)

    def write_rows_device(self, positions, d_rows: int, stride_bytes: int, stream: int = 0) -> dict:
        """Device-pointer row write (`mvfgpu_corpus_write_rows_device`), asynchronous on `stream`: `positions` [m] are GLOBAL
        positions in host memory (never ids), `d_rows` m rows of the stored dtype in device memory, `stride_bytes` apart."""
        pos = np.ascontiguousarray(np.asarray(positions).reshape(-1), np.uint64)
        rep = _lib.WriteReport()
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_write_rows_device(self._h, pos.ctypes.data_as(C.c_void_p) if pos.size else None, pos.size,
                                                                  C.c_void_p(d_rows), stride_bytes, C.c_void_p(stream), C.byref(rep)))
        return _write_report(rep)

    # ---- search ----------------------------------------------------------------
    def search(self, queries: np.ndarray, k: int, metric: int = L2) -> SearchResult:
        """Host-buffer search (`mvfgpu_search`)."""
        q, qcode, nq, qdim = _query_args(queries)
        sc, idx, raw = _result_arrays(nq, k)
        _lib.gpu_check(_lib.gpu().mvfgpu_search(self._h, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq, k,
                                                sc.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                                raw.ctypes.data_as(C.c_void_p)))
        return SearchResult(sc, idx, raw)

    def search_fetch(self, queries: np.ndarray, k: int, metric: int = L2) -> tuple[SearchResult, np.ndarray]:
        """Search + payload in one call (`mvfgpu_search_fetch`): the results and the rows they name, [nq, k, dimension] in
        the stored type (zero rows behind a short result list)."""
        q, qcode, nq, qdim = _query_args(queries)
        _, dim, dt = self._fixed()
        sc, idx, raw = _result_arrays(nq, k)
        vec = np.zeros((nq, k, dim), _NP_OF[dt])  # zeros, not empty: the library writes min(k, rows) rows per query; untouched pages stay unmapped
        _lib.gpu_check(_lib.gpu().mvfgpu_search_fetch(self._h, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq, k,
                                                      sc.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                                      raw.ctypes.data_as(C.c_void_p), vec.ctypes.data_as(C.c_void_p)))
        return SearchResult(sc, idx, raw), vec

    def search_radius(self, queries: np.ndarray, radius, max_per_query: int, metric: int = L2) -> RadiusResult:
        """Every row within `radius` of each query (`mvfgpu_search_radius`): L2 distance <= radius, InnerProduct /
        Cosine score >= radius.  `radius` is a scalar or one value per query; `max_per_query` = 0 asks for counts only."""
        q, qcode, nq, qdim = _query_args(queries)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32), (nq,)), np.float32)
        m = int(max_per_query)
        if m < 0:
            raise InvalidArgument("max_per_query must be >= 0")
        counts = np.zeros(nq, np.uint64)
        sc, idx, raw = _result_arrays(nq, m)
        ptr = (lambda a: a.ctypes.data_as(C.c_void_p)) if m else (lambda a: None)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_radius(self._h, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq,
                                                       r.ctypes.data_as(C.c_void_p), m, counts.ctypes.data_as(C.c_void_p),
                                                       ptr(sc), ptr(idx), ptr(raw)))
        return RadiusResult(counts, sc, idx, raw)

    def search_candidates(self, queries: np.ndarray, candidates: np.ndarray, k: int, metric: int = L2) -> CandidateResult:
        """The exact top-k of each query over its own list of rows (`mvfgpu_search_candidates`): `candidates` is a 2-D
        [nq, m] uint64 array of global positions, or vector ids when ids are attached; UINT64_MAX pads a short list.
        Entries this shard does not hold and deleted rows are skipped, a row listed twice counts once."""
        q, qcode, nq, qdim = _query_args(queries)
        cand = candidates if isinstance(candidates, np.ndarray) else np.asarray(candidates)
        if cand.ndim != 2 or cand.dtype != np.uint64:
            raise InvalidArgument(f"candidates must be a 2-D uint64 array [nq, m], got {cand.dtype} of shape {cand.shape}")
        if cand.shape[0] != nq:
            raise InvalidArgument(f"candidates holds {cand.shape[0]} lists for {nq} queries")
        if cand.shape[1] > 0xFFFFFFFF:
            raise InvalidArgument("at most 2^32 - 1 candidates per query")
        cand = np.ascontiguousarray(cand)
        m = cand.shape[1]
        sc, idx, raw = _result_arrays(nq, k)
        counts = np.zeros(nq, np.uint64)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_candidates(self._h, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq,
                                                           cand.ctypes.data_as(C.c_void_p) if m else None, m, k,
                                                           sc.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                                           raw.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
        return CandidateResult(sc, idx, raw, counts)

    def search_candidates_device(self, d_queries: int, query_dtype: int, query_dim: int, nq: int, d_candidates: int, m: int,
                                 k: int, metric: int, d_scores: int, d_indices: int, d_raw: int = 0, d_counts: int = 0,
                                 stream: int = 0) -> None:
        """Device-pointer candidate search (`mvfgpu_search_candidates_device`), asynchronous on `stream`; the lists are
        global positions."""
        _lib.gpu_check(_lib.gpu().mvfgpu_search_candidates_device(self._h, metric, C.c_void_p(d_queries), query_dtype, query_dim,
                                                                  nq, _opt(d_candidates), m, k, C.c_void_p(d_scores),
                                                                  C.c_void_p(d_indices), _opt(d_raw), _opt(d_counts), _opt(stream)))

    def search_mmr(self, queries: np.ndarray, candidates: np.ndarray, k: int, lambda_mult: float = 0.5, metric: int = L2) -> MmrResult:
        """Diversified re-ranking (`mvfgpu_search_mmr`, include/mvf_gpu_mmr.h): of each query's candidate rows -- `candidates`
        as `search_candidates` takes them, at most MMR_MAX_CANDIDATES per query -- the k picks of the greedy maximal-marginal-
        relevance walk, in pick order; `lambda_mult` in [0, 1] weighs relevance against the similarity to the rows already
        picked (1: the candidate search's order)."""
        q, qcode, nq, qdim = _query_args(queries)
        cand = candidates if isinstance(candidates, np.ndarray) else np.asarray(candidates)
        if cand.ndim != 2 or cand.dtype != np.uint64:
            raise InvalidArgument(f"candidates must be a 2-D uint64 array [nq, m], got {cand.dtype} of shape {cand.shape}")
        if cand.shape[0] != nq:
            raise InvalidArgument(f"candidates holds {cand.shape[0]} lists for {nq} queries")
        if cand.shape[1] > 0xFFFFFFFF:
            raise InvalidArgument("at most 2^32 - 1 candidates per query")
        cand = np.ascontiguousarray(cand)
        m = cand.shape[1]
        sc, idx, raw = _result_arrays(nq, k)
        obj = np.empty((nq, k), np.float32)
        counts = np.zeros(nq, np.uint64)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_mmr(self._h, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq,
                                                    cand.ctypes.data_as(C.c_void_p) if m else None, m, k, float(lambda_mult),
                                                    sc.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                                    raw.ctypes.data_as(C.c_void_p), obj.ctypes.data_as(C.c_void_p),
                                                    counts.ctypes.data_as(C.c_void_p)))
        return MmrResult(sc, idx, raw, counts, obj)

    def search_mmr_device(self, d_queries: int, query_dtype: int, query_dim: int, nq: int, d_candidates: int, m: int, k: int,
                          lambda_mult: float, metric: int, d_scores: int, d_indices: int, d_raw: int = 0, d_objective: int = 0,
                          d_counts: int = 0, stream: int = 0) -> None:
        """Device-pointer diversified re-ranking (`mvfgpu_search_mmr_device`), asynchronous on `stream`; the lists are
        global positions."""
        _lib.gpu_check(_lib.gpu().mvfgpu_search_mmr_device(self._h, metric, C.c_void_p(d_queries), query_dtype, query_dim, nq,
                                                           _opt(d_candidates), m, k, float(lambda_mult), C.c_void_p(d_scores),
                                                           C.c_void_p(d_indices), _opt(d_raw), _opt(d_objective), _opt(d_counts),
                                                           _opt(stream)))

    def mmr_stage_ms(self, d_queries: int, query_dtype: int, query_dim: int, nq: int, d_candidates: int, m: int, k: int,
                     lambda_mult: float, metric: int, d_scores: int, d_indices: int, stream: int = 0) -> tuple[float, float]:
        """(C0 + relevance, D0) milliseconds of one device call (`mvfgpu_selftest_mmr_stage_ms`); waits for the stream."""
        ms = (C.c_float * 2)()
        _lib.gpu_check(_lib.gpu().mvfgpu_selftest_mmr_stage_ms(self._h, metric, C.c_void_p(d_queries), query_dtype, query_dim, nq,
                                                               _opt(d_candidates), m, k, float(lambda_mult), C.c_void_p(d_scores),
                                                               C.c_void_p(d_indices), None, None, None, _opt(stream), ms))
        return float(ms[0]), float(ms[1])

    @staticmethod
    def mmr_walk(rel_scores, sim_scores, metric: int, lambda_mult: float, k: int) -> tuple[np.ndarray, np.ndarray, int]:
        """The walk of `search_mmr` on the host (`mvfgpu_selftest_mmr_walk`; no GPU needed): `rel_scores` [m] and
        `sim_scores` [m, m] (row s as the query) in score form -> (the picks' positions [k], UINT32_MAX behind them; the
        objective [k]; the number of picks)."""
        return mmr_walk(rel_scores, sim_scores, metric, lambda_mult, k)

    def knn_join(self, k: int, metric: int = L2, first: int = 0, count: int | None = None,
                 queries_from: "GpuCorpus | None" = None, exclude_self: bool = True) -> SearchResult:
        """The exact top-k of rows [first, first + count) of `queries_from` (None: this corpus, the k-NN graph) among this
        corpus' rows (`mvfgpu_knn_join`): the queries are staged on the device from the stored rows, `exclude_self` leaves
        the row at the query row's own global position out.  `count` None = to the end of the query corpus."""
        src = self if queries_from is None else queries_from
        if count is None:
            count = src.rows - first
        if first < 0 or count < 0:
            raise InvalidArgument("first and count must be >= 0")
        sc, idx, raw = _result_arrays(count, k)
        _lib.gpu_check(_lib.gpu().mvfgpu_knn_join(self._h, None if queries_from is None else queries_from._h, metric, first, count, k,
                                                  JOIN_EXCLUDE_SELF if exclude_self else 0, sc.ctypes.data_as(C.c_void_p),
                                                  idx.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p)))
        return SearchResult(sc, idx, raw)

    def knn_join_device(self, k: int, metric: int, first: int, count: int, d_scores: int, d_indices: int, d_raw: int = 0,
                        queries_from: "GpuCorpus | None" = None, exclude_self: bool = True, stream: int = 0) -> None:
        """Device-pointer join (`mvfgpu_knn_join_device`): [count, k] results in device memory, every window enqueued on
        `stream` without a host wait."""
        _lib.gpu_check(_lib.gpu().mvfgpu_knn_join_device(self._h, None if queries_from is None else queries_from._h, metric, first,
                                                         count, k, JOIN_EXCLUDE_SELF if exclude_self else 0, _opt(d_scores),
                                                         _opt(d_indices), _opt(d_raw), _opt(stream)))

    # ---- filtered search ---------------------------------------------------------
    def make_filter(self, allow, first_bit: int = 0) -> GpuFilter:
        """A reusable filter (`mvfgpu_filter_create`): `allow` is a bool array over this shard's rows, or a packed uint8
        bitmap (`bitorder="little"`) in which bit (first_bit + r) admits local row r -- a row-range shard passes the whole
        space's bitmap and its first row.  Rows deleted now are never admitted."""
        a = allow if isinstance(allow, np.ndarray) else np.asarray(allow)
        if first_bit < 0:
            raise InvalidArgument("first_bit must be >= 0")
        if a.dtype == np.bool_ and first_bit:
            raise InvalidArgument("a bool mask covers this shard's rows only: first_bit applies to packed bitmaps")
        b = pack_allow_mask(a, self.rows)
        if b.size * 8 < first_bit + self.rows:
            raise InvalidArgument(f"the allow bitmap holds {b.size * 8} bits, the shard needs {first_bit + self.rows}")
        h = C.c_void_p()
        _lib.gpu_check(_lib.gpu().mvfgpu_filter_create(self._h, b.ctypes.data_as(C.c_void_p), first_bit, b.size * 8, C.byref(h)))
        return GpuFilter(h.value, self)

    def make_filter_device(self, d_words: int, stream: int = 0) -> GpuFilter:
        """A filter from u32 words over local rows in device memory (`mvfgpu_filter_create_device`): bit r & 31 of word
        r >> 5, ceil(rows / 32) words, read on `stream`."""
        if not d_words:
            raise InvalidArgument("d_words is a NULL device pointer")
        h = C.c_void_p()
        _lib.gpu_check(_lib.gpu().mvfgpu_filter_create_device(self._h, C.c_void_p(d_words), _opt(stream),
                                                              C.byref(h)))
        return GpuFilter(h.value, self)

    # ---- metadata columns and filters from predicates -------------------------------------
    def attach_column(self, values: np.ndarray, first_value: int = 0) -> GpuColumn:
        """A device column (`mvfgpu_column_create`): `values` is a 1-D uint32 / uint64 array in which entry
        (first_value + r) belongs to local row r -- a row-range shard passes the whole space's column and its first row."""
        if not isinstance(values, np.ndarray) or values.ndim != 1 or values.dtype not in _COLUMN_CODE_OF:
            raise InvalidArgument("a column is a 1-D numpy array of uint32 or uint64 values")
        if first_value < 0:
            raise InvalidArgument("first_value must be >= 0")
        if values.size < first_value + self.rows:
            raise InvalidArgument(f"the column holds {values.size} values, the shard needs {first_value + self.rows}")
        a = np.ascontiguousarray(values)
        h = C.c_void_p()
        _lib.gpu_check(_lib.gpu().mvfgpu_column_create(self._h, a.ctypes.data_as(C.c_void_p), _COLUMN_CODE_OF[a.dtype], first_value,
                                                       a.size, C.byref(h)))
        return GpuColumn(h.value, self)

    def attach_column_pointer(self, ptr: int, data_type: int, first_value: int, n_values: int) -> GpuColumn:
        """`attach_column` from an address of little-endian values of ANY alignment -- a file's column block in place
        (`MetadataColumn.as_ptr`)."""
        if not ptr:
            raise InvalidArgument("ptr is NULL")
        h = C.c_void_p()
        _lib.gpu_check(_lib.gpu().mvfgpu_column_create(self._h, C.c_void_p(ptr), int(data_type), first_value, n_values, C.byref(h)))
        return GpuColumn(h.value, self)

    def attach_column_device(self, ptr: int, data_type: int, stream: int = 0) -> GpuColumn:
        """A device column from values over local rows in device memory (`mvfgpu_column_create_device`), copied on `stream`."""
        if not ptr:
            raise InvalidArgument("ptr is a NULL device pointer")
        h = C.c_void_p()
        _lib.gpu_check(_lib.gpu().mvfgpu_column_create_device(self._h, C.c_void_p(ptr), int(data_type),
                                                              _opt(stream), C.byref(h)))
        return GpuColumn(h.value, self)

    def make_filter_where(self, clauses, any: bool = False, base: GpuFilter | None = None) -> GpuFilter:  # noqa: A002
        """A filter from predicates over this corpus' columns, evaluated on the device (`mvfgpu_filter_create_where`).  A
        clause is (column, op, operand): op "==", "!=", "<", "<=", ">", ">=" with an integer, "between" with (lo, hi),
        inclusive, "in" / "not in" with a sequence of integers.  All clauses hold (`any`: at least one), `base` admits the
        row where given, and rows deleted now are never admitted.  The result is an ordinary GpuFilter."""
        clauses = list(clauses)
        arr, keep = _pack_clauses(clauses)
        hbase = None if base is None else _open_handle(base, GpuFilter, "base")
        h = C.c_void_p()
        _lib.gpu_check(_lib.gpu().mvfgpu_filter_create_where(self._h, arr, len(clauses),
                                                             _lib.WHERE_ANY if any else _lib.WHERE_ALL,
                                                             hbase, C.byref(h)))
        del keep
        return GpuFilter(h.value, self)

    def where_kernel_ms(self, clauses, any: bool = False, base: GpuFilter | None = None, repeats: int = 8) -> np.ndarray:  # noqa: A002
        """Milliseconds of `repeats` launches of the predicate kernel alone (`mvfgpu_selftest_where_kernel_ms`): a
        measurement aid, no filter is built."""
        clauses = list(clauses)
        arr, keep = _pack_clauses(clauses)
        out = np.zeros(repeats, np.float32)
        _lib.gpu_check(_lib.gpu().mvfgpu_selftest_where_kernel_ms(self._h, arr, len(clauses), _lib.WHERE_ANY if any else _lib.WHERE_ALL,
                                                                  None if base is None else base._h, repeats,
                                                                  out.ctypes.data_as(C.c_void_p)))
        del keep
        return out

    def search_filtered(self, queries: np.ndarray, k: int, metric: int, flt: GpuFilter) -> SearchResult:
        """The exact top-k among the rows `flt` admits (`mvfgpu_search_filtered`): `search`'s results in every respect."""
        hflt = _open_handle(flt, GpuFilter, "flt")
        q, qcode, nq, qdim = _query_args(queries)
        sc, idx, raw = _result_arrays(nq, k)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_filtered(self._h, hflt, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq, k,
                                                         sc.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                                         raw.ctypes.data_as(C.c_void_p)))
        return SearchResult(sc, idx, raw)

    def search_filtered_device(self, flt: GpuFilter, d_queries: int, query_dtype: int, query_dim: int, nq: int, k: int, metric: int,
                               d_scores: int, d_indices: int, d_raw: int = 0, stream: int = 0) -> None:
        """Device-pointer filtered search (`mvfgpu_search_filtered_device`), asynchronous on `stream`."""
        hflt = _open_handle(flt, GpuFilter, "flt")
        _lib.gpu_check(_lib.gpu().mvfgpu_search_filtered_device(self._h, hflt, metric, C.c_void_p(d_queries), query_dtype, query_dim,
                                                                nq, k, C.c_void_p(d_scores), C.c_void_p(d_indices),
                                                                _opt(d_raw), _opt(stream)))

    # ---- partitioned search: one key per query -------------------------------------------
    def make_partition(self, column: GpuColumn) -> GpuPartition:
        """The index of this corpus' live rows grouped by `column`'s value (`mvfgpu_partition_create`); rows deleted now are
        not in it, and a later `set_tombstones` makes it stale."""
        h = C.c_void_p()
        _lib.gpu_check(_lib.gpu().mvfgpu_partition_create(self._h, _open_handle(column, GpuColumn, "column"), C.byref(h)))
        return GpuPartition(h.value, self)

    def search_partitioned(self, queries: np.ndarray, keys, k: int, metric: int, part: GpuPartition) -> SearchResult:
        """The exact top-k of every query among the live rows whose column value equals the query's own key
        (`mvfgpu_search_partitioned`): `search`'s results in every respect; a key no live row carries gives padding."""
        hpart = _open_handle(part, GpuPartition, "part")
        q, qcode, nq, qdim = _query_args(queries)
        kk = _keys_u64(keys)
        if kk.size != nq:
            raise InvalidArgument(f"{kk.size} keys for {nq} queries: a partitioned search takes one key per query")
        sc, idx, raw = _result_arrays(nq, k)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_partitioned(self._h, hpart, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq,
                                                            kk.ctypes.data_as(C.c_void_p), k, sc.ctypes.data_as(C.c_void_p),
                                                            idx.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p)))
        return SearchResult(sc, idx, raw)

    def search_partitioned_device(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, keys, k: int,
                                  metric: int, d_scores: int, d_indices: int, d_raw: int = 0, stream: int = 0) -> None:
        """Device-pointer partitioned search (`mvfgpu_search_partitioned_device`), asynchronous on `stream`; `keys` is a host
        array, read before the call returns."""
        hpart = _open_handle(part, GpuPartition, "part")
        kk = _keys_u64(keys)
        if kk.size != nq:
            raise InvalidArgument(f"{kk.size} keys for {nq} queries: a partitioned search takes one key per query")
        _lib.gpu_check(_lib.gpu().mvfgpu_search_partitioned_device(self._h, hpart, metric, C.c_void_p(d_queries), query_dtype,
                                                                   query_dim, nq, kk.ctypes.data_as(C.c_void_p), k,
                                                                   C.c_void_p(d_scores), C.c_void_p(d_indices),
                                                                   _opt(d_raw), _opt(stream)))

    # ---- grouped search: at most per_key results per key ----------------------------------
    def search_grouped(self, queries: np.ndarray, k: int, per_key: int, metric: int, part: GpuPartition) -> SearchResult:
        """The exact top-k of every query with at most `per_key` rows of any one key of `part` (`mvfgpu_search_grouped`):
        `search`'s results in every respect over the rows the partition holds; `GpuColumn.gather` gives the hits' keys."""
        hpart = _open_handle(part, GpuPartition, "part")
        q, qcode, nq, qdim = _query_args(queries)
        sc, idx, raw = _result_arrays(nq, k)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_grouped(self._h, hpart, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq, k,
                                                        per_key, sc.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                                        raw.ctypes.data_as(C.c_void_p)))
        return SearchResult(sc, idx, raw)

    def search_grouped_device(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, k: int,
                              per_key: int, metric: int, d_scores: int, d_indices: int, d_raw: int = 0, stream: int = 0) -> None:
        """Device-pointer grouped search (`mvfgpu_search_grouped_device`), asynchronous on `stream`."""
        hpart = _open_handle(part, GpuPartition, "part")
        _lib.gpu_check(_lib.gpu().mvfgpu_search_grouped_device(self._h, hpart, metric, C.c_void_p(d_queries), query_dtype, query_dim,
                                                               nq, k, per_key, C.c_void_p(d_scores), C.c_void_p(d_indices),
                                                               _opt(d_raw), _opt(stream)))

    def grouped_stage_ms(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, k: int, per_key: int,
                         metric: int, d_scores: int, d_indices: int, stream: int = 0) -> tuple[float, float, float, float]:
        """(segment bounds, G0, G1, tail) in ms of one grouped search that fits one window (`mvfgpu_selftest_grouped_stage_ms`);
        waits for the stream."""
        out = (C.c_float * 4)()
        _lib.gpu_check(_lib.gpu().mvfgpu_selftest_grouped_stage_ms(self._h, part._h, metric, C.c_void_p(d_queries), query_dtype, query_dim,
                                                                   nq, k, per_key, C.c_void_p(d_scores), C.c_void_p(d_indices),
                                                                   _opt(stream), out))
        return tuple(float(x) for x in out)

    # ---- multi-vector search: top-k keys by summed per-token best --------------------------
    def search_maxsim(self, query_sets: np.ndarray, k: int, metric: int, part: GpuPartition) -> MaxSimResult:
        """The k best keys of `part` for every SET of query vectors (`mvfgpu_search_maxsim`; late interaction): `query_sets` is
        [nq, n_tokens, dim] (a 2-D array is one set), a key's score the sum over the set's vectors, in their order, of that
        vector's best score among the key's rows; ties by ascending key."""
        hpart = _open_handle(part, GpuPartition, "part")
        q = np.asarray(query_sets)
        if q.ndim == 2:
            q = q[None, :, :]
        if q.ndim != 3:
            raise InvalidArgument(f"query sets must be [nq, n_tokens, dim], got shape {q.shape}")
        qcode = _CODE_OF.get(q.dtype)
        if qcode is None:
            raise BuildError(f"unsupported query dtype {q.dtype}")
        q = np.ascontiguousarray(q)
        nq, n_tokens, qdim = q.shape
        sc, keys, cnt = np.empty((nq, k), np.float32), np.empty((nq, k), np.uint64), np.zeros(nq, np.uint32)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_maxsim(self._h, hpart, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq, n_tokens, k,
                                                       sc.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p),
                                                       cnt.ctypes.data_as(C.c_void_p)))
        return MaxSimResult(sc, keys, cnt)

    def search_maxsim_device(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, n_tokens: int, k: int,
                             metric: int, d_scores: int, d_keys: int, d_counts: int = 0, stream: int = 0) -> None:
        """Device-pointer multi-vector search (`mvfgpu_search_maxsim_device`), asynchronous on `stream`."""
        hpart = _open_handle(part, GpuPartition, "part")
        _lib.gpu_check(_lib.gpu().mvfgpu_search_maxsim_device(self._h, hpart, metric, C.c_void_p(d_queries), query_dtype, query_dim,
                                                              nq, n_tokens, k, C.c_void_p(d_scores), C.c_void_p(d_keys),
                                                              _opt(d_counts), _opt(stream)))

    def maxsim_stage_ms(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, n_tokens: int, k: int,
                        metric: int, d_scores: int, d_keys: int, stream: int = 0) -> tuple[float, float, float, float]:
        """(key ordinals, M0, M1, tail) in ms of one multi-vector search, summed over its chunks and windows
        (`mvfgpu_selftest_maxsim_stage_ms`); waits for the stream."""
        out = (C.c_float * 4)()
        _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_stage_ms(self._h, part._h, metric, C.c_void_p(d_queries), query_dtype, query_dim,
                                                                  nq, n_tokens, k, C.c_void_p(d_scores), C.c_void_p(d_keys),
                                                                  _opt(stream), out))
        return tuple(float(x) for x in out)

    def set_maxsim_route(self, route: int) -> None:
        """0: the library's rule, 1: multi-vector searches always by the one-pass route, 2: by the MFMA selection route where it
        is eligible (Float32 / Float16 rows, InnerProduct / Cosine); the answers are the same bytes (`mvfgpu_set_maxsim_route`)."""
        _lib.gpu_check(_lib.gpu().mvfgpu_set_maxsim_route(self._h, route))

    def maxsim_mfma_stage_ms(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, n_tokens: int, k: int,
                             metric: int, d_scores: int, d_keys: int, stream: int = 0) -> tuple[tuple[float, ...], np.ndarray, np.ndarray]:
        """((preparation, A0, approximate sums + kth best + P0, M0 over the candidates' blocks, M1 + mask, tail) in ms, candidate
        keys per set, blocks scored again per set) of one multi-vector search by the MFMA selection route
        (`mvfgpu_selftest_maxsim_mfma_stage_ms`); waits for the stream."""
        out = (C.c_float * 6)()
        cand, blocks = np.zeros(max(nq, 1), np.uint32), np.zeros(max(nq, 1), np.uint32)
        _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_mfma_stage_ms(
            self._h, part._h, metric, C.c_void_p(d_queries), query_dtype, query_dim, nq, n_tokens, k, C.c_void_p(d_scores), C.c_void_p(d_keys),
            _opt(stream), out, cand.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p)))
        return tuple(float(x) for x in out), cand[:nq], blocks[:nq]

    def maxsim_mfma_selection(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, n_tokens: int, k: int,
                              metric: int, d_scores: int, d_keys: int, stream: int = 0) -> MaxSimSelection:
        """The selection of one multi-vector search by the MFMA selection route, read out of the device: approximate sums, forced
        keys, candidates, the bound, the kth best approximate sum (`mvfgpu_selftest_maxsim_mfma_selection`); waits for the stream."""
        hpart = _open_handle(part, GpuPartition, "part")
        nk = int(part.info().n_keys)
        shape = (max(nq, 1), max(nk, 1))  # never an empty buffer: the library refuses nq 0 and a partition without keys itself
        sums, forced, cands = np.zeros(shape, np.float32), np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
        delta, theta, tnan = np.zeros(shape[0], np.float64), np.zeros(shape[0], np.float32), np.zeros(shape[0], np.uint8)
        xxmax = C.c_float(0.0)
        _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_mfma_selection(
            self._h, hpart, metric, C.c_void_p(d_queries), query_dtype, query_dim, nq, n_tokens, k, C.c_void_p(d_scores), C.c_void_p(d_keys),
            _opt(stream), *(a.ctypes.data_as(C.c_void_p) for a in (sums, forced, cands, delta, theta, tnan)), C.byref(xxmax)))
        return MaxSimSelection(sums[:nq], forced[:nq].astype(bool), cands[:nq].astype(bool), delta[:nq], theta[:nq], tnan[:nq].astype(bool),
                               float(xxmax.value))

    def search_maxsim_candidates(self, query_sets: np.ndarray, candidate_keys, k: int, metric: int, part: GpuPartition) -> MaxSimResult:
        """`search_maxsim` among every set's own candidate keys (`mvfgpu_search_maxsim_candidates`; re-ranking): `candidate_keys`
        is [m] (one list for every set) or [nq, m]; entries the partition does not hold -- unknown keys, wholly deleted keys,
        UINT64_MAX pads -- are skipped, repeats count once.  counts[q] = min(k, distinct held candidates of set q)."""
        hpart = _open_handle(part, GpuPartition, "part")
        q = np.asarray(query_sets)
        if q.ndim == 2:
            q = q[None, :, :]
        if q.ndim != 3:
            raise InvalidArgument(f"query sets must be [nq, n_tokens, dim], got shape {q.shape}")
        qcode = _CODE_OF.get(q.dtype)
        if qcode is None:
            raise BuildError(f"unsupported query dtype {q.dtype}")
        q = np.ascontiguousarray(q)
        nq, n_tokens, qdim = q.shape
        cand = _candidate_lists(candidate_keys, nq)
        m = cand.shape[1]
        sc, keys, cnt = np.empty((nq, k), np.float32), np.empty((nq, k), np.uint64), np.zeros(nq, np.uint32)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_maxsim_candidates(self._h, hpart, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq,
                                                                  n_tokens, cand.ctypes.data_as(C.c_void_p) if cand.size else None, m, k,
                                                                  sc.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p),
                                                                  cnt.ctypes.data_as(C.c_void_p)))
        return MaxSimResult(sc, keys, cnt)

    def search_maxsim_candidates_device(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, n_tokens: int,
                                        candidate_keys, k: int, metric: int, d_scores: int, d_keys: int, d_counts: int = 0,
                                        stream: int = 0) -> None:
        """Device-pointer candidate multi-vector search (`mvfgpu_search_maxsim_candidates_device`), asynchronous on `stream`;
        `candidate_keys` ([m] or [nq, m]) stays on the host and is read before the call returns."""
        hpart = _open_handle(part, GpuPartition, "part")
        cand = _candidate_lists(candidate_keys, nq)
        _lib.gpu_check(_lib.gpu().mvfgpu_search_maxsim_candidates_device(
            self._h, hpart, metric, C.c_void_p(d_queries), query_dtype, query_dim, nq, n_tokens,
            cand.ctypes.data_as(C.c_void_p) if cand.size else None, cand.shape[1], k, C.c_void_p(d_scores), C.c_void_p(d_keys),
            _opt(d_counts), _opt(stream)))

    def maxsim_candidates_stage_ms(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, n_tokens: int,
                                   candidate_keys, k: int, metric: int, d_scores: int, d_keys: int,
                                   stream: int = 0) -> tuple[float, float, float, float]:
        """(plan upload + E0, M0, M1, tail) in ms of one candidate multi-vector search, summed over its chunks and windows
        (`mvfgpu_selftest_maxsim_candidates_stage_ms`); waits for the stream."""
        out = (C.c_float * 4)()
        cand = _candidate_lists(candidate_keys, nq)
        _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_candidates_stage_ms(
            self._h, part._h, metric, C.c_void_p(d_queries), query_dtype, query_dim, nq, n_tokens,
            cand.ctypes.data_as(C.c_void_p) if cand.size else None, cand.shape[1], k, C.c_void_p(d_scores), C.c_void_p(d_keys),
            _opt(stream), out))
        return tuple(float(x) for x in out)

    # ---- alignments: each listed key's best row per query token ----------------------------
    def maxsim_align(self, query_sets: np.ndarray, keys, metric: int, part: GpuPartition) -> MaxSimAlignment:
        """Which row of every listed key scored best for every query token (`mvfgpu_maxsim_align`): `query_sets` is
        [nq, n_tokens, dim] (a 2-D array is one set), `keys` [m] (one list for every set) or [nq, m] -- usually the keys a
        multi-vector search just returned: for a full search, `search_maxsim` and then this call on its keys.  Rows, scores and raw
        are [nq, m, n_tokens] in list order; element (q, i, t) is `search_partitioned`'s single result for token t of set q with
        key keys[q, i] and k = 1, padding where the partition does not hold the key; a key's scores summed in token order are its
        `search_maxsim_candidates` score."""
        hpart = _open_handle(part, GpuPartition, "part")
        q = np.asarray(query_sets)
        if q.ndim == 2:
            q = q[None, :, :]
        if q.ndim != 3:
            raise InvalidArgument(f"query sets must be [nq, n_tokens, dim], got shape {q.shape}")
        qcode = _CODE_OF.get(q.dtype)
        if qcode is None:
            raise BuildError(f"unsupported query dtype {q.dtype}")
        q = np.ascontiguousarray(q)
        nq, n_tokens, qdim = q.shape
        kk = _candidate_lists(keys, nq)
        m = kk.shape[1]
        shape = (nq, m, n_tokens)
        sc, rows, raw = np.empty(shape, np.float32), np.empty(shape, np.uint64), np.empty(shape, np.int32)
        # never a NULL output: the library checks the buffers before it looks at m
        out = [(a if a.size else np.empty(1, a.dtype)).ctypes.data_as(C.c_void_p) for a in (sc, rows, raw)]
        _lib.gpu_check(_lib.gpu().mvfgpu_maxsim_align(self._h, hpart, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq, n_tokens,
                                                      kk.ctypes.data_as(C.c_void_p) if kk.size else None, m, *out))
        return MaxSimAlignment(rows, sc, raw)

    def maxsim_align_device(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, n_tokens: int, keys,
                            metric: int, d_scores: int, d_rows: int, d_raw: int = 0, stream: int = 0) -> None:
        """Device-pointer alignments (`mvfgpu_maxsim_align_device`), asynchronous on `stream`: the three outputs are
        [nq, m, n_tokens] in device memory; `keys` ([m] or [nq, m]) stays on the host and is read before the call returns."""
        hpart = _open_handle(part, GpuPartition, "part")
        kk = _candidate_lists(keys, nq)
        _lib.gpu_check(_lib.gpu().mvfgpu_maxsim_align_device(
            self._h, hpart, metric, C.c_void_p(d_queries), query_dtype, query_dim, nq, n_tokens,
            kk.ctypes.data_as(C.c_void_p) if kk.size else None, kk.shape[1], C.c_void_p(d_scores), C.c_void_p(d_rows), _opt(d_raw),
            _opt(stream)))

    def maxsim_align_stage_ms(self, part: GpuPartition, d_queries: int, query_dtype: int, query_dim: int, nq: int, n_tokens: int, keys,
                              metric: int, d_scores: int, d_rows: int, d_raw: int = 0, stream: int = 0) -> tuple[float, float, float]:
        """(plan upload + E0, M0-arg, writer) in ms of one alignment call, summed over its chunks and windows
        (`mvfgpu_selftest_maxsim_align_stage_ms`); waits for the stream."""
        out = (C.c_float * 3)()
        kk = _candidate_lists(keys, nq)
        _lib.gpu_check(_lib.gpu().mvfgpu_selftest_maxsim_align_stage_ms(
            self._h, part._h, metric, C.c_void_p(d_queries), query_dtype, query_dim, nq, n_tokens,
            kk.ctypes.data_as(C.c_void_p) if kk.size else None, kk.shape[1], C.c_void_p(d_scores), C.c_void_p(d_rows), _opt(d_raw),
            _opt(stream), out))
        return tuple(float(x) for x in out)

    def search_device(self, d_queries: int, query_dtype: int, query_dim: int, nq: int, k: int, metric: int,
                      d_scores: int, d_indices: int, d_raw: int = 0, stream: int = 0) -> None:
        """Device-pointer search (`mvfgpu_search_device`), asynchronous on `stream`."""
        _lib.gpu_check(_lib.gpu().mvfgpu_search_device(self._h, metric, C.c_void_p(d_queries), query_dtype, query_dim,
                                                       nq, k, C.c_void_p(d_scores), C.c_void_p(d_indices),
                                                       _opt(d_raw), _opt(stream)))

    # ---- profiling -------------------------------------------------------------
    def set_profiling(self, enabled: bool) -> None:
        _lib.gpu_check(_lib.gpu().mvfgpu_set_profiling(self._h, int(enabled)))

    def last_timing(self) -> _lib.Timing:
        t = _lib.Timing()
        _lib.gpu_check(_lib.gpu().mvfgpu_last_timing(self._h, C.byref(t)))
        return t

    def stream_lo_lines(self):
        """(fetched, total) 128-byte lines of the low-bit planes the newest one-query search over the 6-bit shadow requested / held
        in the rows it scanned; (0, 0) where it read the 6-bit layout -- `mvfgpu_debug_stream_lo_lines`."""
        f, t = C.c_uint64(0), C.c_uint64(0)
        _lib.gpu_check(_lib.gpu().mvfgpu_debug_stream_lo_lines(self._h, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    def set_scan_path(self, path: int) -> None:
        _lib.gpu_check(_lib.gpu().mvfgpu_set_scan_path(self._h, path))

    def reload_tuning(self) -> None:
        """Re-read the MVF_* tuning switches of the environment (they are read once, when the handle is created)."""
        _lib.gpu_check(_lib.gpu().mvfgpu_corpus_reload_tuning(self._h))


class ShardSet:
    """Several GPUs in ONE process (`mvfgpu_shardset_*`): per-shard searches on every device, one packed RCCL
    all-gather of the top-k lists, merge on the first shard's device.  The shards are borrowed."""

    def __init__(self, shards: list[GpuCorpus]):
        self._shards = list(shards)  # keeps them alive
        arr = (C.c_void_p * len(shards))(*[s._h for s in shards])
        h = C.c_void_p()
        _lib.gpu_check(_lib.gpu().mvfgpu_shardset_create(arr, len(shards), C.byref(h)))
        self._h = h

    def close(self) -> None:
        if self._h is not None and self._h.value:
            _lib.gpu().mvfgpu_shardset_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self) -> _lib.ShardsetInfo:
        out = _lib.ShardsetInfo()
        _lib.gpu_check(_lib.gpu().mvfgpu_shardset_get_info(self._h, C.byref(out)))
        return out

    def last_timing(self) -> _lib.ShardsetTiming:
        out = _lib.ShardsetTiming()
        _lib.gpu_check(_lib.gpu().mvfgpu_shardset_last_timing(self._h, C.byref(out)))
        return out

    def search(self, queries: np.ndarray, k: int, metric: int = L2) -> SearchResult:
        q, qcode, nq, qdim = _query_args(queries)
        sc, idx, raw = _result_arrays(nq, k)
        _lib.gpu_check(_lib.gpu().mvfgpu_shardset_search(self._h, metric, q.ctypes.data_as(C.c_void_p), qcode, qdim, nq, k,
                                                         sc.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                                         raw.ctypes.data_as(C.c_void_p)))
        return SearchResult(sc, idx, raw)


def merge_topk_host(scores: np.ndarray, indices: np.ndarray, raw: np.ndarray | None, metric: int,
                    data_type: int) -> SearchResult:
    """Merge per-shard results [nlists, nq, k] (host) — `mvfgpu_merge_topk_host`."""
    scores = np.ascontiguousarray(scores, np.float32)
    indices = np.ascontiguousarray(indices, np.uint64)
    nl, nq, k = scores.shape
    if raw is not None:
        raw = np.ascontiguousarray(raw, np.int32)
    sc, idx, rw = _result_arrays(nq, k)
    _lib.gpu_check(_lib.gpu().mvfgpu_merge_topk_host(
        scores.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
        raw.ctypes.data_as(C.c_void_p) if raw is not None else None, nl, nq, k, metric, data_type,
        sc.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), rw.ctypes.data_as(C.c_void_p)))
    return SearchResult(sc, idx, rw)
