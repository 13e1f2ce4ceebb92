"""find_top_k_similar — the GPU drop-in for the reference's hot loop
(examples/similarity_search.rs:140-176), same name and argument meaning.

    reference:  find_top_k_similar(space: &VectorSpace, query: &[f32], k) -> Vec<ScoredVector>
    here:       find_top_k_similar(space, query, k) -> list[ScoredVector]

Differences, all deliberate and documented in DESIGN.md §3:
  * returns the k NEAREST (the reference as written keeps the k farthest,
    SURVEY.md F5; its comments and examples/simple.rs:90 intend nearest);
  * the metric defaults to the space's stored `distance_metric()` (the
    reference ignores it and always computes L2);
  * a query whose length differs from the space's dimension raises
    DimensionMismatch (the reference's zip silently truncates);
  * Int8/UInt8 spaces are searchable (the reference errors in as_f32).
The scan itself runs in libmvf_gpu.so; nothing here computes a distance.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .errors import BuildError, InvalidVectorType
from .gpu import COSINE, INNER_PRODUCT, L2, GpuCorpus, MaxSimAlignment, MaxSimResult, SearchResult, pack_allow_mask, query_dtype_code
from .reader import VectorSpace

_NP_OF = {0: np.float32, 1: np.float16, 2: np.int8, 3: np.uint8}


@dataclass
class ScoredVector:
    """reference examples/similarity_search.rs:14-19"""
    index: int
    score: float
    vector: np.ndarray  # decoded like Vector::as_f32 for float spaces; raw ints for Int8/UInt8


def upload_space(space: VectorSpace, device: int = 0, first: int = 0, count: int | None = None,
                 prepare_batched: bool = False, verify_checksum: bool = False) -> GpuCorpus:
    """HBM-resident copy of rows [first, first+count) of a space, via the
    reference's own hand-off: map_vector_range(..).as_ptr() + stride + count
    (vector_space.rs:155-188, mem.rs:75-77).  The space's deletions and vector ids (schema/core.fbs:35-39, :54) travel
    with it; compressed blocks and Sparse spaces are refused.  `prepare_batched`: norms / f16 shadow are built chunk
    by chunk beside the copy.  `verify_checksum`: the file's CRC32s (what the reference's validate_with_checksum
    leaves as todo!(), src/reader.rs:220) are checked on a second thread WHILE the rows upload; a mismatch raises
    CorruptedData and nothing stays resident."""
    if int(space.vector_type()) != 0:
        raise InvalidVectorType("Invalid vector type: expected Dense, got Sparse")
    total = space.total_vectors()
    if count is None:
        count = total - first
    sl = space.map_vector_range(first, count)
    ids = space.vector_ids()
    tomb = space.tombstone_bitmap()
    check_err: list[BaseException] = []
    th = None
    if verify_checksum:
        import threading

        def _check():
            try:
                space._reader.validate_with_checksum()  # ctypes releases the GIL: runs beside the upload
            except BaseException as e:  # noqa: BLE001 - re-raised below
                check_err.append(e)

        th = threading.Thread(target=_check)
        th.start()
    corpus = None
    try:
        corpus = GpuCorpus.from_pointer(sl.as_ptr(), sl.count, space.dimension(), int(space.data_type()), sl.stride,
                                        device=device, index_base=first, prepare_batched=prepare_batched)
        if tomb is not None:
            corpus.set_tombstones(tomb, first_bit=first)
        if ids is not None:
            corpus.set_vector_ids(ids[first:first + count])
    finally:
        if th is not None:
            th.join()
    if check_err:
        corpus.close()
        raise check_err[0]
    return corpus


def find_top_k_similar(space: VectorSpace, query, k: int, metric: int | None = None, corpus: GpuCorpus | None = None,
                       device: int = 0) -> list[ScoredVector]:
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        qd = _NP_OF[query_dtype_code(int(space.data_type()))]
        res, vec = corpus.search_fetch(np.asarray(query, dtype=qd), k, metric)  # the k best + their payload straight from HBM
        valid = res.indices[0] != np.uint64(0xFFFFFFFFFFFFFFFF)  # fewer than k rows: the reference returns fewer items
        rows = vec[0][valid]
    finally:
        if own:
            corpus.close()
    dt = int(space.data_type())
    out = []
    for idx, score, row in zip(res.indices[0][valid], res.scores[0][valid], rows):
        payload = row.astype(np.float32) if dt in (0, 1) else row.copy()  # as Vector::as_f32 for float spaces
        out.append(ScoredVector(int(idx), float(score), payload))
    return out


def find_top_k_similar_batch(space: VectorSpace, queries, k: int, metric: int | None = None,
                             corpus: GpuCorpus | None = None, device: int = 0,
                             with_vectors: bool = False) -> list[list[ScoredVector]]:
    """The batched form: one call for many queries ([nq, dimension]) -- on large spaces two or more queries take the
    MFMA path (include/mvf_gpu.h).  Same semantics per query as `find_top_k_similar`; the row payloads are fetched only
    when `with_vectors` is set (nq * k rows)."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    dt = int(space.data_type())
    q = np.asarray(queries, dtype=_NP_OF[query_dtype_code(dt)])
    if q.ndim != 2:
        raise BuildError("queries must be a 2-D array [nq, dimension]")
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        if with_vectors:
            res, vec = corpus.search_fetch(q, k, metric)
        else:
            res, vec = corpus.search(q, k, metric), None
        valid = res.indices != np.uint64(0xFFFFFFFFFFFFFFFF)
        rows = vec[valid] if with_vectors else None
    finally:
        if own:
            corpus.close()
    out, r = [], 0
    for i in range(q.shape[0]):
        hits = []
        for idx, score in zip(res.indices[i][valid[i]], res.scores[i][valid[i]]):
            payload = None
            if rows is not None:
                payload = rows[r].astype(np.float32) if dt in (0, 1) else rows[r].copy()
                r += 1
            hits.append(ScoredVector(int(idx), float(score), payload))
        out.append(hits)
    return out


def rerank_top_k(space: VectorSpace, queries, candidates, k: int, metric: int | None = None, corpus: GpuCorpus | None = None,
                 device: int = 0, with_vectors: bool = False) -> list[list[ScoredVector]]:
    """Exact re-ranking (`mvfgpu_search_candidates`; DESIGN.md §3 "Candidate search"): for each query ([nq, dimension]) the
    k best of ITS candidate rows -- `candidates` [nq, m] uint64, the positions (or vector ids) an index, a filter or several
    retrievers proposed, UINT64_MAX padding a short list.  Rows the space does not hold and deleted rows are skipped, a row
    listed twice counts once; each query's list holds min(k, distinct live candidates) results, shaped and scored like
    `find_top_k_similar_batch`'s.  The row payloads are fetched only when `with_vectors` is set."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    dt = int(space.data_type())
    q = np.asarray(queries, dtype=_NP_OF[query_dtype_code(dt)])
    if q.ndim != 2:
        raise BuildError("queries must be a 2-D array [nq, dimension]")
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        res = corpus.search_candidates(q, candidates, k, metric)
        n = np.minimum(res.counts, np.uint64(k)).astype(np.int64)
        rows = None
        if with_vectors and int(n.sum()):
            rows = corpus.gather_rows(np.concatenate([res.indices[i][:n[i]] for i in range(q.shape[0])]))
    finally:
        if own:
            corpus.close()
    out, r = [], 0
    for i in range(q.shape[0]):
        hits = []
        for j in range(int(n[i])):
            payload = None
            if rows is not None:
                payload = rows[r].astype(np.float32) if dt in (0, 1) else rows[r].copy()
                r += 1
            hits.append(ScoredVector(int(res.indices[i][j]), float(res.scores[i][j]), payload))
        out.append(hits)
    return out


def write_rows(corpus: GpuCorpus, indices, rows) -> dict:
    """Replace resident rows (`mvfgpu_corpus_write_rows`; DESIGN.md §3 "Row writes"): `rows` [m, dimension] go to `indices` [m]
    of a corpus `upload_space` made -- global positions, or vector ids where the space has them -- and every later search of the
    corpus answers as one uploaded from the changed rows would.  `rows` must hold the space's stored dtype (nothing is
    converted: a Float16 space takes float16).  Together with tombstones this is the fixed-capacity upsert: upload with spare
    rows kept deleted, write a new vector into a free slot, then clear its bit with `GpuCorpus.set_tombstones`.  The file
    behind the space is not changed.  Returns the write's report (`GpuCorpus.write_rows`)."""
    return corpus.write_rows(indices, rows)


def diversify_top_k(space: VectorSpace, queries, candidates, k: int, lambda_mult: float = 0.5, metric: int | None = None,
                    corpus: GpuCorpus | None = None, device: int = 0, with_vectors: bool = False) -> list[list[ScoredVector]]:
    """Diversified re-ranking by maximal marginal relevance (`mvfgpu_search_mmr`; DESIGN.md §3 "Diversified re-ranking"): of
    each query's candidate rows -- `candidates` [nq, m] uint64 as `rerank_top_k` takes them, at most 1024 per query -- k that
    are relevant and not near-copies of each other, in pick order.  `lambda_mult` in [0, 1]: 1 ranks by relevance alone
    (`rerank_top_k`'s order), 0 by dissimilarity to the rows already picked.  Each hit's score is the query's score of the
    row, as `rerank_top_k` reports it.  The row payloads are fetched only when `with_vectors` is set."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    dt = int(space.data_type())
    q = np.asarray(queries, dtype=_NP_OF[query_dtype_code(dt)])
    if q.ndim != 2:
        raise BuildError("queries must be a 2-D array [nq, dimension]")
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        res = corpus.search_mmr(q, candidates, k, lambda_mult, metric)
        n = np.minimum(res.counts, np.uint64(k)).astype(np.int64)
        rows = None
        if with_vectors and int(n.sum()):
            rows = corpus.gather_rows(np.concatenate([res.indices[i][:n[i]] for i in range(q.shape[0])]))
    finally:
        if own:
            corpus.close()
    out, r = [], 0
    for i in range(q.shape[0]):
        hits = []
        for j in range(int(n[i])):
            payload = None
            if rows is not None:
                payload = rows[r].astype(np.float32) if dt in (0, 1) else rows[r].copy()
                r += 1
            hits.append(ScoredVector(int(res.indices[i][j]), float(res.scores[i][j]), payload))
        out.append(hits)
    return out


def find_top_k_diverse(space: VectorSpace, queries, k: int, fetch_k: int, lambda_mult: float = 0.5, metric: int | None = None,
                       corpus: GpuCorpus | None = None, device: int = 0, with_vectors: bool = False) -> list[list[ScoredVector]]:
    """The usual one-call form ("max marginal relevance search"): `find_top_k_similar_batch` with `fetch_k` (at most 1024),
    then `diversify_top_k` over the rows it found."""
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        top = find_top_k_similar_batch(space, queries, fetch_k, metric, corpus=corpus)
        cand = np.full((len(top), max(fetch_k, 1)), 0xFFFFFFFFFFFFFFFF, np.uint64)
        for i, hits in enumerate(top):
            cand[i, :len(hits)] = [h.index for h in hits]
        return diversify_top_k(space, queries, cand, k, lambda_mult, metric, corpus=corpus, with_vectors=with_vectors)
    finally:
        if own:
            corpus.close()


def find_top_k_filtered(space: VectorSpace, query, k: int, allow, metric: int | None = None, corpus: GpuCorpus | None = None,
                        device: int = 0) -> list[ScoredVector]:
    """`find_top_k_similar` among the rows a predicate admits (`mvfgpu_search_filtered`; DESIGN.md §3 "Filtered search"):
    `allow` covers the WHOLE space -- a bool array with one entry per vector, or the packed uint8 bitmap of one
    (`bitorder="little"`) -- and a `corpus` that holds a row range of the space reads its own part of it.  Deleted rows are
    never returned; fewer than k admitted rows give fewer items.  The filter lives for this call: a caller with many
    queries per predicate makes one with `GpuCorpus.make_filter` and calls `GpuCorpus.search_filtered`.  The row payloads
    are fetched behind the search (`gather_rows`)."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    bits = pack_allow_mask(allow, space.total_vectors())  # malformed masks are refused before anything is uploaded
    dt = int(space.data_type())
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        with corpus.make_filter(bits, first_bit=int(corpus.info().index_base)) as flt:
            res = corpus.search_filtered(np.asarray(query, dtype=_NP_OF[query_dtype_code(dt)]), k, metric, flt)
        valid = res.indices[0] != np.uint64(0xFFFFFFFFFFFFFFFF)
        rows = corpus.gather_rows(res.indices[0][valid]) if int(valid.sum()) else np.empty((0, space.dimension()), _NP_OF[dt])
    finally:
        if own:
            corpus.close()
    out = []
    for idx, score, row in zip(res.indices[0][valid], res.scores[0][valid], rows):
        payload = row.astype(np.float32) if dt in (0, 1) else row.copy()
        out.append(ScoredVector(int(idx), float(score), payload))
    return out


def find_top_k_where(space: VectorSpace, query, k: int, where, any: bool = False, metric: int | None = None,  # noqa: A002
                     corpus: GpuCorpus | None = None, device: int = 0) -> list[ScoredVector]:
    """`find_top_k_filtered` with the predicate evaluated on the device from the file's metadata columns
    (`mvfgpu_filter_create_where`; DESIGN.md §3 "Column filters"): `where` maps column names of the space's file to
    (op, operand) -- op "==", "!=", "<", "<=", ">", ">=" with an integer, "between" with (lo, hi), "in" / "not in" with a
    sequence of integers; every clause holds, or with `any` at least one.  A column holds one UInt32 / UInt64 value per vector
    of the WHOLE space; a `corpus` that holds a row range reads its own part.  The columns and the filter live for this call:
    a caller with many predicates attaches the columns once (`GpuCorpus.attach_column`, `make_filter_where`)."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    total = space.total_vectors()
    cols = {}
    for name in where:  # everything about the file's columns is refused before anything is uploaded
        mc = space._reader.metadata_column(name)
        es = {4: 4, 5: 8}.get(int(mc.data_type))
        if es is None:
            raise BuildError("Unsupported metadata column data type")
        if mc.size // es < total:
            raise BuildError(f"metadata column '{name}' holds {mc.size // es} values, the space has {total} vectors")
        cols[name] = (mc, mc.size // es)
    dt = int(space.data_type())
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    attached = []
    try:
        base = int(corpus.info().index_base)
        clauses = []
        for name, (op, operand) in where.items():
            mc, count = cols[name]
            attached.append(corpus.attach_column_pointer(mc.as_ptr(), int(mc.data_type), base, count))
            clauses.append((attached[-1], op, operand))
        with corpus.make_filter_where(clauses, any=any) as flt:
            res = corpus.search_filtered(np.asarray(query, dtype=_NP_OF[query_dtype_code(dt)]), k, metric, flt)
        valid = res.indices[0] != np.uint64(0xFFFFFFFFFFFFFFFF)
        rows = corpus.gather_rows(res.indices[0][valid]) if int(valid.sum()) else np.empty((0, space.dimension()), _NP_OF[dt])
    finally:
        for col in attached:
            col.close()
        if own:
            corpus.close()
    out = []
    for idx, score, row in zip(res.indices[0][valid], res.scores[0][valid], rows):
        payload = row.astype(np.float32) if dt in (0, 1) else row.copy()
        out.append(ScoredVector(int(idx), float(score), payload))
    return out


def find_top_k_per_key(space: VectorSpace, queries, keys, k: int, column: str, metric: int | None = None,
                       corpus: GpuCorpus | None = None, device: int = 0) -> SearchResult:
    """The top-k of every query among the vectors whose value in the file's metadata column `column` equals the query's own
    key (`mvfgpu_search_partitioned`; DESIGN.md §3 "Partitioned search"): `keys` holds one unsigned integer per query, a key
    no live vector carries gives a row of padding.  The column is read as `find_top_k_where` reads it -- one UInt32 / UInt64
    value per vector of the WHOLE space, a `corpus` that holds a row range reads its own part -- with the same refusals.
    Returns [nq, k] arrays like a search.  The column and the index live for this call: a caller with many batches attaches
    the column and builds the index once (`GpuCorpus.attach_column`, `make_partition`, `search_partitioned`)."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    total = space.total_vectors()
    mc = space._reader.metadata_column(column)  # everything about the file's column is refused before anything is uploaded
    es = {4: 4, 5: 8}.get(int(mc.data_type))
    if es is None:
        raise BuildError("Unsupported metadata column data type")
    if mc.size // es < total:
        raise BuildError(f"metadata column '{column}' holds {mc.size // es} values, the space has {total} vectors")
    dt = int(space.data_type())
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        base = int(corpus.info().index_base)
        with corpus.attach_column_pointer(mc.as_ptr(), int(mc.data_type), base, mc.size // es) as col:
            with corpus.make_partition(col) as part:
                return corpus.search_partitioned(np.asarray(queries, dtype=_NP_OF[query_dtype_code(dt)]), keys, k, metric, part)
    finally:
        if own:
            corpus.close()


def find_top_k_grouped(space: VectorSpace, queries, k: int, column: str, per_key: int = 1, metric: int | None = None,
                       corpus: GpuCorpus | None = None, device: int = 0) -> tuple[SearchResult, np.ndarray]:
    """The top-k of every query with at most `per_key` vectors of any one value of the file's metadata column `column`
    (`mvfgpu_search_grouped`; DESIGN.md §3 "Grouped search"): the k best documents of a corpus of passages (`per_key` 1), or
    the k best passages with at most `per_key` per document.  The column is read as `find_top_k_per_key` reads it, with the
    same refusals.  Returns ([nq, k] arrays like a search, the hits' keys as uint64 [nq, k]; a padding entry's key is 0).
    The column and the index live for this call: a caller with many batches attaches the column and builds the index once
    (`GpuCorpus.attach_column`, `make_partition`, `search_grouped`, `GpuColumn.gather`)."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    total = space.total_vectors()
    mc = space._reader.metadata_column(column)  # everything about the file's column is refused before anything is uploaded
    es = {4: 4, 5: 8}.get(int(mc.data_type))
    if es is None:
        raise BuildError("Unsupported metadata column data type")
    if mc.size // es < total:
        raise BuildError(f"metadata column '{column}' holds {mc.size // es} values, the space has {total} vectors")
    dt = int(space.data_type())
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        base = int(corpus.info().index_base)
        with corpus.attach_column_pointer(mc.as_ptr(), int(mc.data_type), base, mc.size // es) as col:
            with corpus.make_partition(col) as part:
                res = corpus.search_grouped(np.asarray(queries, dtype=_NP_OF[query_dtype_code(dt)]), k, per_key, metric, part)
            return res, col.gather(res.indices)
    finally:
        if own:
            corpus.close()


def find_top_k_documents(space: VectorSpace, query_vectors, k: int, column: str, metric: int | None = None,
                         corpus: GpuCorpus | None = None, device: int = 0) -> MaxSimResult:
    """The k best values of the file's metadata column `column` -- documents of a corpus of token or passage vectors -- for a
    SET of query vectors (`mvfgpu_search_maxsim`; DESIGN.md §3 "Multi-vector search"): late interaction, a document's score
    being the sum over the query's vectors of that vector's best score among the document's vectors.  `query_vectors` is
    [n_tokens, dim] for one query or [nq, n_tokens, dim].  The column is read as `find_top_k_per_key` reads it, with the same
    refusals.  Returns scores [nq, k], keys [nq, k] (UINT64_MAX pads) and counts [nq].  The column and the index live for this
    call: a caller with many batches attaches the column and builds the index once (`GpuCorpus.attach_column`,
    `make_partition`, `search_maxsim`)."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    total = space.total_vectors()
    mc = space._reader.metadata_column(column)  # everything about the file's column is refused before anything is uploaded
    es = {4: 4, 5: 8}.get(int(mc.data_type))
    if es is None:
        raise BuildError("Unsupported metadata column data type")
    if mc.size // es < total:
        raise BuildError(f"metadata column '{column}' holds {mc.size // es} values, the space has {total} vectors")
    dt = int(space.data_type())
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        base = int(corpus.info().index_base)
        with corpus.attach_column_pointer(mc.as_ptr(), int(mc.data_type), base, mc.size // es) as col:
            with corpus.make_partition(col) as part:
                return corpus.search_maxsim(np.asarray(query_vectors, dtype=_NP_OF[query_dtype_code(dt)]), k, metric, part)
    finally:
        if own:
            corpus.close()


def rerank_top_k_documents(space: VectorSpace, query_vectors, candidate_keys, k: int, column: str, metric: int | None = None,
                           corpus: GpuCorpus | None = None, device: int = 0) -> MaxSimResult:
    """`find_top_k_documents` among CANDIDATE documents (`mvfgpu_search_maxsim_candidates`; DESIGN.md §3 "Candidate keys"): the
    exact late-interaction scores of the documents a first stage proposed, best k first.  `candidate_keys` holds values of the
    column, [m] for every query or [nq, m]; values no live vector carries (UINT64_MAX pads among them) are skipped, repeats
    count once, and counts[q] = min(k, the distinct candidates found).  The column is read as `find_top_k_per_key` reads it,
    with the same refusals; it and the index live for this call (`GpuCorpus.search_maxsim_candidates` for many batches)."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    total = space.total_vectors()
    mc = space._reader.metadata_column(column)  # everything about the file's column is refused before anything is uploaded
    es = {4: 4, 5: 8}.get(int(mc.data_type))
    if es is None:
        raise BuildError("Unsupported metadata column data type")
    if mc.size // es < total:
        raise BuildError(f"metadata column '{column}' holds {mc.size // es} values, the space has {total} vectors")
    dt = int(space.data_type())
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        base = int(corpus.info().index_base)
        with corpus.attach_column_pointer(mc.as_ptr(), int(mc.data_type), base, mc.size // es) as col:
            with corpus.make_partition(col) as part:
                return corpus.search_maxsim_candidates(np.asarray(query_vectors, dtype=_NP_OF[query_dtype_code(dt)]), candidate_keys, k,
                                                       metric, part)
    finally:
        if own:
            corpus.close()


def align_documents(space: VectorSpace, query_vectors, keys, column: str, metric: int | None = None,
                    corpus: GpuCorpus | None = None, device: int = 0) -> MaxSimAlignment:
    """Which vector of every listed document scored best for every query vector (`mvfgpu_maxsim_align`; DESIGN.md §3
    "Alignments"): the tokens or passages behind a late-interaction score.  `keys` holds values of the column, [m] for every
    query or [nq, m] -- usually the keys `find_top_k_documents` or `rerank_top_k_documents` just returned; alignments are not part
    of those searches: the recipe is the search, then this call on its keys.  Returns rows, scores and raw [nq, m, n_tokens] in list
    order, padding (row UINT64_MAX) for values no live vector carries; a document's scores summed in token order are its
    `rerank_top_k_documents` score.  The column is read as `find_top_k_per_key` reads it, with the same refusals; it and the
    index live for this call (`GpuCorpus.maxsim_align` for many batches)."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    total = space.total_vectors()
    mc = space._reader.metadata_column(column)  # everything about the file's column is refused before anything is uploaded
    es = {4: 4, 5: 8}.get(int(mc.data_type))
    if es is None:
        raise BuildError("Unsupported metadata column data type")
    if mc.size // es < total:
        raise BuildError(f"metadata column '{column}' holds {mc.size // es} values, the space has {total} vectors")
    dt = int(space.data_type())
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        base = int(corpus.info().index_base)
        with corpus.attach_column_pointer(mc.as_ptr(), int(mc.data_type), base, mc.size // es) as col:
            with corpus.make_partition(col) as part:
                return corpus.maxsim_align(np.asarray(query_vectors, dtype=_NP_OF[query_dtype_code(dt)]), keys, metric, part)
    finally:
        if own:
            corpus.close()


def build_knn_graph(space: VectorSpace, k: int, metric: int | None = None, corpus: GpuCorpus | None = None, first: int = 0,
                    count: int | None = None, device: int = 0) -> SearchResult:
    """The k-NN graph of a space (`mvfgpu_knn_join`; DESIGN.md §3 "Join"): for rows [first, first + count) (local rows of
    the corpus; None: to its end) the k nearest OTHER rows -- a row is never its own neighbour (decided by position; its exact
    duplicates are), deleted rows neither appear nor get neighbours (their result rows are padding).  The rows never leave the
    device.  Returns [count, k] arrays like a search: indices (positions, or vector ids where the space has them; UINT64_MAX
    pads), scores, raw.  `first` / `count` let a caller stream a graph that does not fit in host memory."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        return corpus.knn_join(k, metric, first=first, count=count, exclude_self=True)
    finally:
        if own:
            corpus.close()


def find_within_radius(space: VectorSpace, query, radius: float, max_results: int | None = None, metric: int | None = None,
                       corpus: GpuCorpus | None = None, device: int = 0, with_vectors: bool = True) -> list[ScoredVector]:
    """Every row within `radius` of `query` (`mvfgpu_search_radius`), best first like `find_top_k_similar`: L2 distance
    <= radius, InnerProduct / Cosine score >= radius (inclusive).  `max_results` keeps the best that many
    (None: all of them).  Deleted rows never match; ids and the payload as in `find_top_k_similar`."""
    if metric is None:
        metric = int(space.distance_metric())
    if metric not in (L2, INNER_PRODUCT, COSINE):
        raise BuildError(f"Unsupported distance metric {metric}")
    if max_results is not None and max_results < 0:
        raise BuildError("max_results must be >= 0")
    dt = int(space.data_type())
    q = np.asarray(query, dtype=_NP_OF[query_dtype_code(dt)])
    own = corpus is None
    if own:
        corpus = upload_space(space, device)
    try:
        want = max_results
        if want is None:  # all matches: the count first (no lists), then one call for exactly that many
            want = int(corpus.search_radius(q, radius, 0, metric).counts[0])
        res = corpus.search_radius(q, radius, want, metric)
        count = int(res.counts[0])
        n = min(count, res.indices.shape[1])
        idx, sc = res.indices[0][:n], res.scores[0][:n]
        rows = corpus.gather_rows(idx) if (with_vectors and n) else None
    finally:
        if own:
            corpus.close()
    out = []
    for i in range(n):
        payload = None
        if rows is not None:
            payload = rows[i].astype(np.float32) if dt in (0, 1) else rows[i].copy()
        out.append(ScoredVector(int(idx[i]), float(sc[i]), payload))
    return out
