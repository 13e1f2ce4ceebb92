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
from .gpu import (CandidateResult, GpuColumn, GpuCorpus, GpuFilter, GpuPartition, HammingFilteredForm, HammingForm, HammingMaxsimForm, HammingMfmaForm, HammingPairs, HammingPairsForm, HammingRadiusForm, MaxSimAlignment, MaxSimResult, MmrResult, RadiusResult, SearchResult, SignbitsForm, TanimotoForm,  # noqa: F401,E402
                  hamming_filtered_form, hamming_form, hamming_maxsim_form, hamming_mfma_form, hamming_pairs_form, hamming_radius_form, hamming_route, maxsim_margin, maxsim_route, mmr_walk, pack_sign_bits, quantize_queries_int8, signbits_form, tanimoto_form)
from .search import (ScoredVector, align_documents, build_knn_graph, diversify_top_k, find_duplicate_pairs, find_top_k_diverse, find_top_k_documents, find_top_k_documents_hamming, find_top_k_filtered, find_top_k_grouped, find_top_k_hamming, find_top_k_hamming_filtered, find_top_k_per_key, find_top_k_signbits, find_top_k_similar, find_top_k_tanimoto, find_top_k_where, find_top_k_similar_batch,  # noqa: F401,E402
                     find_within_hamming, find_within_radius, rerank_top_k, rerank_top_k_documents, upload_space, write_rows)  # examples/similarity_search.rs:140-176; find_within_radius, rerank_top_k, build_knn_graph, find_top_k_filtered, find_top_k_where, find_top_k_per_key, find_top_k_grouped, find_top_k_documents, rerank_top_k_documents, align_documents, diversify_top_k, find_top_k_diverse, write_rows, find_top_k_hamming, find_top_k_signbits, find_within_hamming, find_top_k_tanimoto, find_top_k_documents_hamming, find_top_k_hamming_filtered, find_duplicate_pairs: DESIGN.md §3

__all__ = ["MvfError", "MvfReader", "VectorSpace", "Vector", "VectorSlice", "MvfBuilder", "BuiltMvf", "GpuCorpus",
           "GpuFilter", "GpuColumn", "GpuPartition", "MetadataColumn", "SearchResult", "RadiusResult", "CandidateResult", "MmrResult", "MaxSimResult", "MaxSimAlignment", "ScoredVector", "find_top_k_similar",
           "find_top_k_similar_batch", "find_within_radius", "rerank_top_k", "build_knn_graph", "find_top_k_filtered", "find_top_k_where", "find_top_k_per_key", "find_top_k_grouped", "find_top_k_documents", "rerank_top_k_documents", "align_documents",
           "diversify_top_k", "find_top_k_diverse", "upload_space", "write_rows", "maxsim_route", "maxsim_margin", "mmr_walk", "find_top_k_hamming",
           "HammingForm", "hamming_form", "pack_sign_bits", "HammingMfmaForm", "hamming_mfma_form", "hamming_route",
           "find_top_k_signbits", "SignbitsForm", "signbits_form", "quantize_queries_int8",
           "find_within_hamming", "HammingRadiusForm", "hamming_radius_form",
           "find_duplicate_pairs", "HammingPairs", "HammingPairsForm", "hamming_pairs_form",
           "find_top_k_tanimoto", "TanimotoForm", "tanimoto_form",
           "find_top_k_documents_hamming", "HammingMaxsimForm", "hamming_maxsim_form",
           "find_top_k_hamming_filtered", "HammingFilteredForm", "hamming_filtered_form"]
