"""metrovector_amd — MI355X-native brute-force similarity search for MVF files.

Host-side mirror of the reference's reader API (MvfReader / VectorSpace /
Vector) plus the GPU search path that replaces
examples/similarity_search.rs::find_top_k_similar.  The numeric work lives in
the in-tree native libraries (metrovector_amd/csrc); there is no CPU fallback.
"""
from .errors import (BuildError, CorruptedData, DeviceError, DimensionMismatch, IndexOutOfBounds,  # noqa: F401
                     InvalidArgument, InvalidFormat, IoError, MvfError, UnsupportedVersion, VectorSpaceNotFound)

from .reader import MetadataColumn, MvfReader, Vector, VectorSlice, VectorSpace  # noqa: F401,E402  (reference: src/reader.rs, src/vectors/*)
from .builder import BuiltMvf, MvfBuilder  # noqa: F401,E402                      (reference: src/builder.rs)
from .gpu import (CandidateResult, GpuColumn, GpuCorpus, GpuFilter, GpuPartition, MaxSimAlignment, MaxSimResult, MmrResult, RadiusResult, SearchResult,  # noqa: F401,E402
                  maxsim_margin, maxsim_route, mmr_walk)
from .search import (ScoredVector, align_documents, build_knn_graph, diversify_top_k, find_top_k_diverse, find_top_k_documents, find_top_k_filtered, find_top_k_grouped, find_top_k_per_key, find_top_k_similar, find_top_k_where, find_top_k_similar_batch,  # noqa: F401,E402
                     find_within_radius, rerank_top_k, rerank_top_k_documents, upload_space, write_rows)  # examples/similarity_search.rs:140-176; find_within_radius, rerank_top_k, build_knn_graph, find_top_k_filtered, find_top_k_where, find_top_k_per_key, find_top_k_grouped, find_top_k_documents, rerank_top_k_documents, align_documents, diversify_top_k, find_top_k_diverse, write_rows: DESIGN.md §3

__all__ = ["MvfError", "MvfReader", "VectorSpace", "Vector", "VectorSlice", "MvfBuilder", "BuiltMvf", "GpuCorpus",
           "GpuFilter", "GpuColumn", "GpuPartition", "MetadataColumn", "SearchResult", "RadiusResult", "CandidateResult", "MmrResult", "MaxSimResult", "MaxSimAlignment", "ScoredVector", "find_top_k_similar",
           "find_top_k_similar_batch", "find_within_radius", "rerank_top_k", "build_knn_graph", "find_top_k_filtered", "find_top_k_where", "find_top_k_per_key", "find_top_k_grouped", "find_top_k_documents", "rerank_top_k_documents", "align_documents",
           "diversify_top_k", "find_top_k_diverse", "upload_space", "write_rows", "maxsim_route", "maxsim_margin", "mmr_walk"]
