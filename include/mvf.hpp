// mvf.hpp — header-only C++17 mirror of the reference's host API for the search path, over the two C ABIs
// (include/mvf_file.h -> libmvf_host.so, include/mvf_gpu.h -> libmvf_gpu.so).
//
// The reference is a Rust crate; no Rust toolchain exists in this image, so the host side above the C ABI is written
// in C++ with the reference's names, argument meaning and error behaviour:
//
//   reference (Rust)                                          here
//   MvfError (src/errors.rs:8-40)                             mvf::MvfError (one code per variant, mvf_status.h)
//   MvfReader::open / version / num_vector_spaces /           mvf::MvfReader (src/reader.rs:45-172)
//     vector_space_names / vector_space / file_size /
//     has_metadata / metadata_column_names / validate /       (+ metadata_column: the column's type and bytes)
//     validate_with_checksum
//   VectorSpace::name / dimension / total_vectors /           mvf::VectorSpace (src/vectors/vector_space.rs:62-188)
//     vector_type / distance_metric / data_type /
//     get_vector / map_vector_range
//   Vector::dimension / data_type / as_bytes / as_f32         mvf::Vector (src/vectors/vector.rs:51-92)
//   VectorSlice (as_ptr, stride, count)                       mvf::VectorSlice (src/vectors/mem.rs:24-77)
//   MvfBuilder::new / add_vector_space / add_vectors /        mvf::MvfBuilder, mvf::BuiltMvf (src/builder.rs:93-558)
//     build -> BuiltMvf::save / to_bytes
//   ScoredVector, find_top_k_similar(&space, &query, k)       mvf::ScoredVector, mvf::find_top_k_similar
//     (examples/similarity_search.rs:14-37, :140-176)           -- the scan runs on the GPU (mvfgpu_search)
//
// find_top_k_similar(space, query, k) uploads the space's rows on every call, as the reference's function walks the file
// on every call; a caller with more than one query keeps a mvf::GpuVectorSpace (upload once, search many).
// Results follow the INTENDED semantics of the example (the k nearest for L2, best first; UPSTREAM.md F5) with the metric
// the space declares, not the example's hard-wired Euclidean distance.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mvf_file.h"
#include "mvf_gpu.h"
#include "mvf_gpu_maxsim_align.h"
#include "mvf_gpu_maxsim_route.h"
#include "mvf_gpu_mmr.h"
#include "mvf_gpu_update.h"
#include "mvf_status.h"

namespace mvf {

enum class DataType : uint8_t { Float32 = 0, Float16 = 1, Int8 = 2, UInt8 = 3 };       // schema/types.fbs:3-11 (vector types)
enum class VectorType : uint8_t { Dense = 0, Sparse = 1 };                              // schema/types.fbs:14-17
enum class DistanceMetric : uint8_t { L2 = 0, InnerProduct = 1, Cosine = 2, Custom = 255 };  // schema/types.fbs:20-25

// MvfError (src/errors.rs:8-40): code() is the variant, what() the reference's message text.
class MvfError : public std::runtime_error {
public:
    MvfError(int code, const std::string& msg) : std::runtime_error(msg), code_(code) {}
    int code() const noexcept { return code_; }

private:
    int code_;
};

namespace detail {
inline void check_host(int rc) {
    if (rc != MVF_OK) throw MvfError(rc, std::string(mvf_strerror(rc)) + ": " + mvf_last_error_message());
}
inline void check_gpu(int rc) {
    if (rc != MVF_OK) throw MvfError(rc, std::string(mvfgpu_strerror(rc)) + ": " + mvfgpu_last_error_message());
}
}  // namespace detail

// VectorSlice<'a> (src/vectors/mem.rs:24-30): a borrowed, strided view of rows inside the mapping.
struct VectorSlice {
    const void* data = nullptr;
    uint64_t stride = 0;  // bytes between rows
    uint64_t count = 0;
    DataType data_type = DataType::Float32;
    template <class T> const T* as_ptr() const { return static_cast<const T*>(data); }  // mem.rs:75-77
};

// Vector<'a> (src/vectors/vector.rs:28-33): one row, borrowed from the mapping.
class Vector {
public:
    Vector(const void* data, uint64_t len, uint32_t dimension, DataType dt) : data_(data), len_(len), dim_(dimension), dt_(dt) {}
    uint32_t dimension() const { return dim_; }
    DataType data_type() const { return dt_; }
    std::pair<const uint8_t*, uint64_t> as_bytes() const { return {static_cast<const uint8_t*>(data_), len_}; }
    std::vector<float> as_f32() const {  // vector.rs:71-92 (Float32 / Float16; the integer types widen)
        std::vector<float> out(dim_);
        uint64_t n = 0;
        detail::check_host(mvf_vector_as_f32(data_, len_, (uint8_t)dt_, out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }

private:
    const void* data_;
    uint64_t len_;
    uint32_t dim_;
    DataType dt_;
};

class MvfReader;

// VectorSpace<'a> (src/vectors/vector_space.rs:34-39): valid while its reader lives.
class VectorSpace {
public:
    std::string name() const { return std::string(s_.name, s_.name_len); }
    uint32_t dimension() const { return s_.dimension; }
    uint64_t total_vectors() const { return s_.total_vectors; }
    VectorType vector_type() const { return (VectorType)s_.vector_type; }
    DistanceMetric distance_metric() const { return (DistanceMetric)s_.distance_metric; }
    DataType data_type() const { return (DataType)s_.data_type; }
    Vector get_vector(uint64_t index) const {  // :101-142: IndexOutOfBounds beyond total_vectors
        const void* d = nullptr;
        uint64_t len = 0;
        detail::check_host(mvf_space_get_vector(&s_, index, &d, &len));
        return Vector(d, len, s_.dimension, data_type());
    }
    VectorSlice map_vector_range(uint64_t start, uint64_t count) const {  // :155-188
        mvf_vector_slice v;
        detail::check_host(mvf_space_map_vector_range(&s_, start, count, &v));
        VectorSlice out;
        out.data = v.data, out.stride = v.stride, out.count = v.count, out.data_type = (DataType)v.data_type;
        return out;
    }
    const mvf_vector_space& raw() const { return s_; }

private:
    friend class MvfReader;
    explicit VectorSpace(const mvf_vector_space& s) : s_(s) {}
    mvf_vector_space s_;
};

// One metadata column of a file (MetadataColumn, schema/core.fbs:16-25): a borrowed view of its block, valid while the
// reader is open.  UInt32 / UInt64 columns hold one little-endian value per row; `data` may be unaligned.
struct MetadataColumn {
    std::string name;
    uint8_t data_type = 0;  // enum mvf_data_type as stored
    uint32_t data_block_index = 0;
    uint64_t null_count = 0;
    const void* data = nullptr;
    uint64_t size = 0;  // bytes
};

// One clause of GpuVectorSpace::find_top_k_where: `op` is MVFGPU_OP_*; EQ .. GE compare with `a`, BETWEEN takes a <= v <= b,
// IN / NOT_IN take `values` (any order, repeats allowed).
struct WhereClause {
    MetadataColumn column;
    uint32_t op = MVFGPU_OP_EQ;
    uint64_t a = 0, b = 0;
    std::vector<uint64_t> values;
};

// MvfReader (src/reader.rs:27-33): the mapping and the verified footer.
class MvfReader {
public:
    static MvfReader open(const std::string& path) {  // :45-79
        mvf_reader* r = nullptr;
        detail::check_host(mvf_reader_open(path.c_str(), &r));
        return MvfReader(r);
    }
    MvfReader(MvfReader&& o) noexcept : r_(o.r_) { o.r_ = nullptr; }
    MvfReader& operator=(MvfReader&& o) noexcept {
        if (this != &o) {
            if (r_) mvf_reader_close(r_);
            r_ = o.r_, o.r_ = nullptr;
        }
        return *this;
    }
    MvfReader(const MvfReader&) = delete;
    MvfReader& operator=(const MvfReader&) = delete;
    ~MvfReader() {
        if (r_) mvf_reader_close(r_);
    }
    uint16_t version() const {
        uint16_t v = 0;
        detail::check_host(mvf_reader_version(r_, &v));
        return v;
    }
    size_t num_vector_spaces() const {
        uint64_t n = 0;
        detail::check_host(mvf_reader_num_vector_spaces(r_, &n));
        return (size_t)n;
    }
    std::vector<std::string> vector_space_names() const {  // :92-98
        std::vector<std::string> out;
        for (uint64_t i = 0, n = num_vector_spaces(); i < n; i++) {
            const char* s = nullptr;
            uint32_t len = 0;
            detail::check_host(mvf_reader_vector_space_name(r_, i, &s, &len));
            out.emplace_back(s, len);
        }
        return out;
    }
    VectorSpace vector_space(const std::string& name) const {  // :104-119: VectorSpaceNotFound
        mvf_vector_space s;
        detail::check_host(mvf_reader_vector_space(r_, name.c_str(), &s));
        return VectorSpace(s);
    }
    uint64_t file_size() const {
        uint64_t n = 0;
        detail::check_host(mvf_reader_file_size(r_, &n));
        return n;
    }
    bool has_metadata() const {
        int b = 0;
        detail::check_host(mvf_reader_has_metadata(r_, &b));
        return b != 0;
    }
    std::vector<std::string> metadata_column_names() const {  // :132-143
        std::vector<std::string> out;
        uint64_t n = 0;
        detail::check_host(mvf_reader_num_metadata_columns(r_, &n));
        for (uint64_t i = 0; i < n; i++) {
            const char* s = nullptr;
            uint32_t len = 0;
            detail::check_host(mvf_reader_metadata_column_name(r_, i, &s, &len));
            out.emplace_back(s, len);
        }
        return out;
    }
    MetadataColumn metadata_column(const std::string& name) const {  // the first of that name; VectorSpaceNotFound-style error
        mvf_metadata_column c;
        detail::check_host(mvf_reader_metadata_column(r_, name.c_str(), &c));
        MetadataColumn out;
        out.name.assign(c.name, c.name_len);
        out.data_type = c.data_type, out.data_block_index = c.data_block_index, out.null_count = c.null_count;
        out.data = c.data, out.size = c.size;
        return out;
    }
    void validate() const { detail::check_host(mvf_reader_validate(r_)); }                              // :149-162
    void validate_with_checksum() const { detail::check_host(mvf_reader_validate_with_checksum(r_)); }  // :172-220 (todo!() upstream)

private:
    explicit MvfReader(mvf_reader* r) : r_(r) {}
    mvf_reader* r_;
};

// BuiltMvf (src/builder.rs:395-558)
class BuiltMvf {
public:
    void save(const std::string& path) const { detail::check_host(mvf_builder_save(b_, path.c_str(), 0)); }  // :408-411
    std::vector<uint8_t> to_bytes() const {                                                                  // :417-558
        uint8_t* p = nullptr;
        uint64_t len = 0;
        detail::check_host(mvf_builder_to_bytes(b_, 0, &p, &len));
        std::vector<uint8_t> out(p, p + len);
        mvf_free(p);
        return out;
    }
    BuiltMvf(BuiltMvf&& o) noexcept : b_(o.b_) { o.b_ = nullptr; }
    BuiltMvf(const BuiltMvf&) = delete;
    BuiltMvf& operator=(const BuiltMvf&) = delete;
    ~BuiltMvf() {
        if (b_) mvf_builder_free(b_);
    }

private:
    friend class MvfBuilder;
    explicit BuiltMvf(mvf_builder* b) : b_(b) {}
    mvf_builder* b_;
};

// MvfBuilder (src/builder.rs:44-308)
class MvfBuilder {
public:
    MvfBuilder() { detail::check_host(mvf_builder_new(&b_)); }  // :93-95
    MvfBuilder(const MvfBuilder&) = delete;
    MvfBuilder& operator=(const MvfBuilder&) = delete;
    ~MvfBuilder() {
        if (b_) mvf_builder_free(b_);
    }
    // :113-135 + VectorSpaceBuilderRef's setters (:339-357) in one call
    MvfBuilder& add_vector_space(const std::string& name, uint32_t dimension, VectorType vt = VectorType::Dense,
                                 DistanceMetric dm = DistanceMetric::L2, DataType dt = DataType::Float32) {
        detail::check_host(mvf_builder_add_vector_space(b_, name.c_str(), dimension, (uint8_t)vt, (uint8_t)dm, (uint8_t)dt, nullptr));
        return *this;
    }
    // :151-196: rows of `dimension` floats, stored as the space's type (Float32 / Float16; Build error otherwise);
    // DimensionMismatch names the offending row's length
    MvfBuilder& add_vectors(const std::string& space_name, const std::vector<std::vector<float>>& vectors) {
        if (vectors.empty()) return *this;
        const size_t dim = vectors.front().size();
        std::vector<float> flat;
        flat.reserve(vectors.size() * dim);
        for (const auto& v : vectors) {
            if (v.size() != dim)
                throw MvfError(MVF_ERR_DIMENSION_MISMATCH, "Dimension mismatch: expected " + std::to_string(dim) + ", got " + std::to_string(v.size()));
            flat.insert(flat.end(), v.begin(), v.end());
        }
        detail::check_host(mvf_builder_add_vectors_f32(b_, space_name.c_str(), flat.data(), vectors.size(), (uint32_t)dim));
        return *this;
    }
    // :211-236: the column's bytes as given; UInt32 / UInt64 columns are little-endian values, one per row
    MvfBuilder& add_metadata_column(const std::string& name, uint8_t data_type, const void* bytes, uint64_t len) {
        detail::check_host(mvf_builder_add_metadata_column(b_, name.c_str(), data_type, bytes, len));
        return *this;
    }
    MvfBuilder& add_metadata_column(const std::string& name, const std::vector<uint32_t>& values) {
        return add_metadata_column(name, MVF_DTYPE_UINT32, values.data(), (uint64_t)values.size() * 4);
    }
    MvfBuilder& add_metadata_column(const std::string& name, const std::vector<uint64_t>& values) {
        return add_metadata_column(name, MVF_DTYPE_UINT64, values.data(), (uint64_t)values.size() * 8);
    }
    BuiltMvf build() {  // :241-308 (consumes the builder)
        mvf_builder* b = b_;
        b_ = nullptr;
        return BuiltMvf(b);
    }

private:
    mvf_builder* b_ = nullptr;
};

// ScoredVector (examples/similarity_search.rs:14-19)
struct ScoredVector {
    uint64_t index;
    float score;
    std::vector<float> vector;
};

// A vector space resident in HBM: upload once (VectorSpace::map_vector_range -> mvfgpu_corpus_create), search many.
class GpuVectorSpace {
public:
    explicit GpuVectorSpace(const VectorSpace& space, int device = 0)
        : dim_(space.dimension()), metric_(space.distance_metric()), dt_(space.data_type()) {
        if (mvfgpu_abi_version() != MVFGPU_ABI_VERSION)  // a library built from another header: its structs may differ
            throw MvfError(MVF_ERR_INVALID_ARGUMENT, "libmvf_gpu speaks ABI version " + std::to_string(mvfgpu_abi_version()) +
                                                         ", this program was built against " + std::to_string(MVFGPU_ABI_VERSION));
        const VectorSlice s = space.map_vector_range(0, space.total_vectors());
        detail::check_gpu(mvfgpu_corpus_create(s.data, s.count, dim_, (uint8_t)s.data_type, s.stride, 0, device, &c_));
    }
    GpuVectorSpace(const GpuVectorSpace&) = delete;
    GpuVectorSpace& operator=(const GpuVectorSpace&) = delete;
    ~GpuVectorSpace() {
        if (c_) mvfgpu_corpus_destroy(c_);
    }
    // Row writes (mvfgpu_corpus_write_rows, mvf_gpu_update.h; DESIGN.md section 3, "Row writes"): rows.size() / (dimension x
    // element size) rows of the space's STORED type, back to back, into `indices` -- global positions, or vector ids when the
    // space carries them; a row named twice is refused.  Every later search answers as a space uploaded from the changed rows
    // would; the file behind the space is not changed.  With spare rows kept deleted this is the fixed-capacity upsert: write
    // into a free slot, then clear its bit (mvfgpu_corpus_set_tombstones on raw()).
    mvfgpu_write_report write_rows(const std::vector<uint64_t>& indices, const std::vector<uint8_t>& rows) {
        const size_t es = dt_ == DataType::Float32 ? 4 : dt_ == DataType::Float16 ? 2 : 1, row_bytes = (size_t)dim_ * es;
        if (rows.size() != indices.size() * row_bytes)
            throw MvfError(MVF_ERR_INVALID_ARGUMENT, "write_rows takes " + std::to_string(row_bytes) + " bytes per index, got " +
                                                         std::to_string(rows.size()) + " for " + std::to_string(indices.size()));
        mvfgpu_write_report rep{};
        rep.struct_size = sizeof rep;
        detail::check_gpu(mvfgpu_corpus_write_rows(c_, indices.empty() ? nullptr : indices.data(), indices.size(),
                                                   rows.empty() ? nullptr : rows.data(), row_bytes, &rep));
        return rep;
    }
    // a Float32 space's rows as floats
    mvfgpu_write_report write_rows(const std::vector<uint64_t>& indices, const std::vector<float>& rows) {
        if (dt_ != DataType::Float32) throw MvfError(MVF_ERR_BUILD, "write_rows(float) writes Float32 spaces: pass the stored bytes");
        const uint8_t* b = reinterpret_cast<const uint8_t*>(rows.data());
        return write_rows(indices, std::vector<uint8_t>(b, b + rows.size() * 4));
    }
    // examples/similarity_search.rs:140-176 with the metric the space declares; DimensionMismatch for a query of another
    // length (the reference's zip would truncate silently); the payload of every hit is fetched from HBM
    std::vector<ScoredVector> find_top_k_similar(const std::vector<float>& query, size_t k, bool with_vectors = true) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "find_top_k_similar takes f32 queries: Float32 / Float16 spaces");
        std::vector<float> scores(k);
        std::vector<uint64_t> idx(k);
        const size_t es = dt_ == DataType::Float32 ? 4 : 2;
        // one query: the library writes the first min(k, rows) payload rows only (include/mvf_gpu.h) -- any k, as the reference takes
        mvfgpu_corpus_info info{};
        info.struct_size = sizeof info;
        detail::check_gpu(mvfgpu_corpus_get_info(c_, &info));
        std::vector<uint8_t> rows(with_vectors ? std::min<uint64_t>(k, info.rows) * dim_ * es : 0);
        if (with_vectors)  // the k best and their rows in one call
            detail::check_gpu(mvfgpu_search_fetch(c_, (uint8_t)metric_, query.data(), MVF_DTYPE_FLOAT32, (uint32_t)query.size(), 1, (uint32_t)k,
                                                  scores.data(), idx.data(), nullptr, rows.data()));
        else
            detail::check_gpu(mvfgpu_search(c_, (uint8_t)metric_, query.data(), MVF_DTYPE_FLOAT32, (uint32_t)query.size(), 1, (uint32_t)k,
                                            scores.data(), idx.data(), nullptr));
        std::vector<ScoredVector> out;
        for (size_t i = 0; i < k && idx[i] != ~0ull; i++) {  // fewer than k rows: the tail is padding
            out.push_back({idx[i], scores[i], {}});
            if (with_vectors) out.back().vector = Vector(rows.data() + i * dim_ * es, dim_ * es, dim_, dt_).as_f32();
        }
        return out;
    }
    // Every row within `radius` of the query, best first (mvfgpu_search_radius): L2 distance <= radius,
    // InnerProduct / Cosine score >= radius, inclusive.  At most max_results hits (the best ones); the payload is not fetched.
    std::vector<ScoredVector> find_within_radius(const std::vector<float>& query, float radius, size_t max_results) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "find_within_radius takes f32 queries: Float32 / Float16 spaces");
        uint64_t count = 0;
        std::vector<float> scores(max_results);
        std::vector<uint64_t> idx(max_results);
        detail::check_gpu(mvfgpu_search_radius(c_, (uint8_t)metric_, query.data(), MVF_DTYPE_FLOAT32, (uint32_t)query.size(), 1, &radius,
                                               max_results, &count, max_results ? scores.data() : nullptr,
                                               max_results ? idx.data() : nullptr, nullptr));
        std::vector<ScoredVector> out;
        for (size_t i = 0; i < max_results && i < count; i++) out.push_back({idx[i], scores[i], {}});
        return out;
    }
    // Exact re-ranking (mvfgpu_search_candidates): the k best of the rows `candidates` names -- global
    // positions, or vector ids when the space carries them -- scored as find_top_k_similar scores them.  Entries the space
    // does not hold and deleted rows are skipped, a row listed twice counts once; fewer than k candidates give fewer hits.
    std::vector<ScoredVector> rerank_top_k(const std::vector<float>& query, const std::vector<uint64_t>& candidates, size_t k) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "rerank_top_k takes f32 queries: Float32 / Float16 spaces");
        if (k == 0) return {};
        uint64_t count = 0;
        std::vector<float> scores(k);
        std::vector<uint64_t> idx(k);
        detail::check_gpu(mvfgpu_search_candidates(c_, (uint8_t)metric_, query.data(), MVF_DTYPE_FLOAT32, (uint32_t)query.size(), 1,
                                                   candidates.empty() ? nullptr : candidates.data(), (uint32_t)candidates.size(),
                                                   (uint32_t)k, scores.data(), idx.data(), nullptr, &count));
        std::vector<ScoredVector> out;
        for (size_t i = 0; i < k && i < count; i++) out.push_back({idx[i], scores[i], {}});
        return out;
    }
    // Diversified re-ranking by maximal marginal relevance (mvfgpu_search_mmr, mvf_gpu_mmr.h): of the rows
    // `candidates` names (as rerank_top_k takes them, at most MVFGPU_MMR_MAX_CANDIDATES) k that are relevant and not near-copies
    // of each other, in pick order; lambda in [0, 1] -- 1 ranks by relevance alone.  Each hit's score is the query's score of
    // the row, as rerank_top_k reports it.
    std::vector<ScoredVector> diversify_top_k(const std::vector<float>& query, const std::vector<uint64_t>& candidates, size_t k,
                                              float lambda = 0.5f) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "diversify_top_k takes f32 queries: Float32 / Float16 spaces");
        if (k == 0) return {};
        uint64_t count = 0;
        std::vector<float> scores(k);
        std::vector<uint64_t> idx(k);
        detail::check_gpu(mvfgpu_search_mmr(c_, (uint8_t)metric_, query.data(), MVF_DTYPE_FLOAT32, (uint32_t)query.size(), 1,
                                            candidates.empty() ? nullptr : candidates.data(), (uint32_t)candidates.size(), (uint32_t)k,
                                            lambda, scores.data(), idx.data(), nullptr, nullptr, &count));
        std::vector<ScoredVector> out;
        for (size_t i = 0; i < k && i < count; i++) out.push_back({idx[i], scores[i], {}});
        return out;
    }
    // The usual one-call form: find_top_k_similar with fetch_k (at most MVFGPU_MMR_MAX_CANDIDATES), then diversify_top_k over
    // the rows it found.
    std::vector<ScoredVector> find_top_k_diverse(const std::vector<float>& query, size_t k, size_t fetch_k, float lambda = 0.5f) const {
        std::vector<uint64_t> candidates;
        for (const auto& h : find_top_k_similar(query, fetch_k, false)) candidates.push_back(h.index);
        return diversify_top_k(query, candidates, k, lambda);
    }
    // find_top_k_similar among the rows a predicate admits (mvfgpu_search_filtered; DESIGN.md section 3, "Filtered search"):
    // bit r of allow_bits (byte r >> 3, bit r & 7; at least one bit per row) admits row r.  Deleted rows are never returned;
    // fewer than k admitted rows give fewer hits.  The filter lives for this call; the payload is not fetched.
    std::vector<ScoredVector> find_top_k_filtered(const std::vector<float>& query, size_t k, const std::vector<uint8_t>& allow_bits) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "find_top_k_filtered takes f32 queries: Float32 / Float16 spaces");
        if (k == 0) return {};
        mvfgpu_filter* f = nullptr;
        detail::check_gpu(mvfgpu_filter_create(c_, allow_bits.data(), 0, (uint64_t)allow_bits.size() * 8, &f));
        std::vector<float> scores(k);
        std::vector<uint64_t> idx(k);
        const int rc = mvfgpu_search_filtered(c_, f, (uint8_t)metric_, query.data(), MVF_DTYPE_FLOAT32, (uint32_t)query.size(), 1, (uint32_t)k,
                                              scores.data(), idx.data(), nullptr);
        mvfgpu_filter_destroy(f);
        detail::check_gpu(rc);
        std::vector<ScoredVector> out;
        for (size_t i = 0; i < k && idx[i] != ~0ull; i++) out.push_back({idx[i], scores[i], {}});
        return out;
    }
    // find_top_k_filtered with the predicate evaluated on the device from a file's metadata columns (mvfgpu_column_create,
    // mvfgpu_filter_create_where; DESIGN.md section 3, "Column filters"): every clause holds, or with `any` at least one.  A
    // column holds one UInt32 / UInt64 value per vector of the space (Build error otherwise).  The columns and the filter live
    // for this call; the payload is not fetched.
    std::vector<ScoredVector> find_top_k_where(const std::vector<float>& query, size_t k, const std::vector<WhereClause>& where,
                                               bool any = false) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "find_top_k_where takes f32 queries: Float32 / Float16 spaces");
        if (k == 0) return {};
        mvfgpu_corpus_info inf;
        MVFGPU_INIT(inf);
        detail::check_gpu(mvfgpu_corpus_get_info(c_, &inf));
        std::vector<mvfgpu_column*> cols;
        std::vector<mvfgpu_predicate> preds;
        mvfgpu_filter* f = nullptr;
        std::vector<float> scores(k);
        std::vector<uint64_t> idx(k);
        int rc = MVF_OK;
        for (const WhereClause& w : where) {
            const uint64_t es = w.column.data_type == MVF_DTYPE_UINT32 ? 4 : w.column.data_type == MVF_DTYPE_UINT64 ? 8 : 0;
            mvfgpu_column* col = nullptr;
            if (!es || w.column.size / es < inf.rows) {
                for (mvfgpu_column* c : cols) mvfgpu_column_destroy(c);
                throw MvfError(MVF_ERR_BUILD, es ? "metadata column '" + w.column.name + "' holds fewer values than the space has vectors"
                                                 : "Unsupported metadata column data type");
            }
            rc = mvfgpu_column_create(c_, w.column.data, w.column.data_type, 0, w.column.size / es, &col);
            if (rc != MVF_OK) break;
            cols.push_back(col);
            preds.push_back({col, w.op, (uint32_t)w.values.size(), w.a, w.b, w.values.empty() ? nullptr : w.values.data()});
        }
        if (rc == MVF_OK)
            rc = mvfgpu_filter_create_where(c_, preds.data(), (uint32_t)preds.size(), any ? MVFGPU_WHERE_ANY : MVFGPU_WHERE_ALL, nullptr, &f);
        if (rc == MVF_OK)
            rc = mvfgpu_search_filtered(c_, f, (uint8_t)metric_, query.data(), MVF_DTYPE_FLOAT32, (uint32_t)query.size(), 1, (uint32_t)k,
                                        scores.data(), idx.data(), nullptr);
        mvfgpu_filter_destroy(f);
        for (mvfgpu_column* c : cols) mvfgpu_column_destroy(c);
        detail::check_gpu(rc);
        std::vector<ScoredVector> out;
        for (size_t i = 0; i < k && idx[i] != ~0ull; i++) out.push_back({idx[i], scores[i], {}});
        return out;
    }
    // The top-k of every query among the vectors whose value in `column` equals the query's own key (mvfgpu_partition_create,
    // mvfgpu_search_partitioned; DESIGN.md section 3, "Partitioned search"): queries.size() / dimension queries, one key each; a
    // key no live vector carries gives an empty list.  The column holds one UInt32 / UInt64 value per vector of the space
    // (Build error otherwise).  The column and the index live for this call; the payload is not fetched.
    std::vector<std::vector<ScoredVector>> find_top_k_per_key(const std::vector<float>& queries, const std::vector<uint64_t>& keys, size_t k,
                                                              const MetadataColumn& column) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "find_top_k_per_key takes f32 queries: Float32 / Float16 spaces");
        const size_t nq = keys.size();
        if (queries.size() != nq * (size_t)dim_) throw MvfError(MVF_ERR_DIMENSION_MISMATCH, "find_top_k_per_key takes one key per query");
        std::vector<std::vector<ScoredVector>> out(nq);
        if (k == 0 || nq == 0) return out;
        mvfgpu_corpus_info inf;
        MVFGPU_INIT(inf);
        detail::check_gpu(mvfgpu_corpus_get_info(c_, &inf));
        const uint64_t es = column.data_type == MVF_DTYPE_UINT32 ? 4 : column.data_type == MVF_DTYPE_UINT64 ? 8 : 0;
        if (!es || column.size / es < inf.rows)
            throw MvfError(MVF_ERR_BUILD, es ? "metadata column '" + column.name + "' holds fewer values than the space has vectors"
                                             : "Unsupported metadata column data type");
        mvfgpu_column* col = nullptr;
        mvfgpu_partition* part = nullptr;
        std::vector<float> scores(nq * k);
        std::vector<uint64_t> idx(nq * k);
        int rc = mvfgpu_column_create(c_, column.data, column.data_type, 0, column.size / es, &col);
        if (rc == MVF_OK) rc = mvfgpu_partition_create(c_, col, &part);
        if (rc == MVF_OK)
            rc = mvfgpu_search_partitioned(c_, part, (uint8_t)metric_, queries.data(), MVF_DTYPE_FLOAT32, dim_, (uint32_t)nq, keys.data(),
                                           (uint32_t)k, scores.data(), idx.data(), nullptr);
        mvfgpu_partition_destroy(part);
        mvfgpu_column_destroy(col);
        detail::check_gpu(rc);
        for (size_t i = 0; i < nq; i++)
            for (size_t j = 0; j < k && idx[i * k + j] != ~0ull; j++) out[i].push_back({idx[i * k + j], scores[i * k + j], {}});
        return out;
    }
    // The top-k of every query with at most per_key vectors of any one value of `column` (mvfgpu_search_grouped; DESIGN.md
    // section 3, "Grouped search"): the k best documents of a corpus of passages (per_key 1), or the k best passages with at
    // most per_key per document.  queries.size() / dimension queries; the column as in find_top_k_per_key.  hit_keys, where
    // given, receives every hit's column value (mvfgpu_column_gather).  The column and the index live for this call; the
    // payload is not fetched.
    std::vector<std::vector<ScoredVector>> find_top_k_grouped(const std::vector<float>& queries, size_t k, size_t per_key,
                                                              const MetadataColumn& column,
                                                              std::vector<std::vector<uint64_t>>* hit_keys = nullptr) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "find_top_k_grouped takes f32 queries: Float32 / Float16 spaces");
        if (dim_ == 0 || queries.size() % (size_t)dim_)
            throw MvfError(MVF_ERR_DIMENSION_MISMATCH, "find_top_k_grouped takes whole queries of the space's dimension");
        const size_t nq = queries.size() / (size_t)dim_;
        std::vector<std::vector<ScoredVector>> out(nq);
        if (hit_keys) hit_keys->assign(nq, {});
        if (k == 0 || nq == 0) return out;
        mvfgpu_corpus_info inf;
        MVFGPU_INIT(inf);
        detail::check_gpu(mvfgpu_corpus_get_info(c_, &inf));
        const uint64_t es = column.data_type == MVF_DTYPE_UINT32 ? 4 : column.data_type == MVF_DTYPE_UINT64 ? 8 : 0;
        if (!es || column.size / es < inf.rows)
            throw MvfError(MVF_ERR_BUILD, es ? "metadata column '" + column.name + "' holds fewer values than the space has vectors"
                                             : "Unsupported metadata column data type");
        mvfgpu_column* col = nullptr;
        mvfgpu_partition* part = nullptr;
        std::vector<float> scores(nq * k);
        std::vector<uint64_t> idx(nq * k), vals(nq * k);
        int rc = mvfgpu_column_create(c_, column.data, column.data_type, 0, column.size / es, &col);
        if (rc == MVF_OK) rc = mvfgpu_partition_create(c_, col, &part);
        if (rc == MVF_OK)
            rc = mvfgpu_search_grouped(c_, part, (uint8_t)metric_, queries.data(), MVF_DTYPE_FLOAT32, dim_, (uint32_t)nq, (uint32_t)k,
                                       (uint32_t)per_key, scores.data(), idx.data(), nullptr);
        if (rc == MVF_OK && hit_keys) rc = mvfgpu_column_gather(col, idx.data(), idx.size(), vals.data());
        mvfgpu_partition_destroy(part);
        mvfgpu_column_destroy(col);
        detail::check_gpu(rc);
        for (size_t i = 0; i < nq; i++)
            for (size_t j = 0; j < k && idx[i * k + j] != ~0ull; j++) {
                out[i].push_back({idx[i * k + j], scores[i * k + j], {}});
                if (hit_keys) (*hit_keys)[i].push_back(vals[i * k + j]);
            }
        return out;
    }
    // The route of find_top_k_documents (mvfgpu_set_maxsim_route): 0 the library's rule, 1 always the one-pass route, 2 the MFMA
    // selection route where it is eligible (Float32 / Float16 spaces, InnerProduct / Cosine).  The answers are the same bytes.
    void set_maxsim_route(int route) { detail::check_gpu(mvfgpu_set_maxsim_route(c_, route)); }
    // The k best values of `column` -- documents of a corpus of token or passage vectors -- for ONE query of n_tokens vectors
    // (mvfgpu_search_maxsim; DESIGN.md section 3, "Multi-vector search"): late interaction, a document's score being the sum
    // over the query's vectors, in their order, of that vector's best score among the document's vectors.  query_vectors holds
    // n_tokens x dimension floats; the column as in find_top_k_per_key.  -> (column value, score), best first, ties by
    // ascending value; fewer than k where the column has fewer values among the live vectors.  The column and the index live
    // for this call.
    std::vector<std::pair<uint64_t, float>> find_top_k_documents(const std::vector<float>& query_vectors, size_t k,
                                                                 const MetadataColumn& column) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "find_top_k_documents takes f32 queries: Float32 / Float16 spaces");
        if (dim_ == 0 || query_vectors.empty() || query_vectors.size() % (size_t)dim_)
            throw MvfError(MVF_ERR_DIMENSION_MISMATCH, "find_top_k_documents takes whole query vectors of the space's dimension");
        const size_t n_tokens = query_vectors.size() / (size_t)dim_;
        std::vector<std::pair<uint64_t, float>> out;
        if (k == 0) return out;
        mvfgpu_corpus_info inf;
        MVFGPU_INIT(inf);
        detail::check_gpu(mvfgpu_corpus_get_info(c_, &inf));
        const uint64_t es = column.data_type == MVF_DTYPE_UINT32 ? 4 : column.data_type == MVF_DTYPE_UINT64 ? 8 : 0;
        if (!es || column.size / es < inf.rows)
            throw MvfError(MVF_ERR_BUILD, es ? "metadata column '" + column.name + "' holds fewer values than the space has vectors"
                                             : "Unsupported metadata column data type");
        mvfgpu_column* col = nullptr;
        mvfgpu_partition* part = nullptr;
        std::vector<float> scores(k);
        std::vector<uint64_t> keys(k);
        uint32_t count = 0;
        int rc = mvfgpu_column_create(c_, column.data, column.data_type, 0, column.size / es, &col);
        if (rc == MVF_OK) rc = mvfgpu_partition_create(c_, col, &part);
        if (rc == MVF_OK)
            rc = mvfgpu_search_maxsim(c_, part, (uint8_t)metric_, query_vectors.data(), MVF_DTYPE_FLOAT32, dim_, 1,
                                      (uint32_t)std::min<size_t>(n_tokens, UINT32_MAX), (uint32_t)k, scores.data(), keys.data(), &count);
        mvfgpu_partition_destroy(part);
        mvfgpu_column_destroy(col);
        detail::check_gpu(rc);
        for (uint32_t i = 0; i < count; i++) out.emplace_back(keys[i], scores[i]);
        return out;
    }
    // find_top_k_documents among CANDIDATE documents (mvfgpu_search_maxsim_candidates; DESIGN.md section 3, "Candidate keys"):
    // the exact late-interaction scores of the values of `column` a first stage proposed, the best k first.  Values no live
    // vector carries (UINT64_MAX pads among them) are skipped and a value listed twice counts once, so fewer than k come back
    // where fewer distinct candidates are found.  The column and the index live for this call.
    std::vector<std::pair<uint64_t, float>> rerank_top_k_documents(const std::vector<float>& query_vectors,
                                                                   const std::vector<uint64_t>& candidate_keys, size_t k,
                                                                   const MetadataColumn& column) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "rerank_top_k_documents takes f32 queries: Float32 / Float16 spaces");
        if (dim_ == 0 || query_vectors.empty() || query_vectors.size() % (size_t)dim_)
            throw MvfError(MVF_ERR_DIMENSION_MISMATCH, "rerank_top_k_documents takes whole query vectors of the space's dimension");
        if (candidate_keys.size() > UINT32_MAX) throw MvfError(MVF_ERR_INVALID_ARGUMENT, "more than 2^32 - 1 candidate keys");
        const size_t n_tokens = query_vectors.size() / (size_t)dim_;
        std::vector<std::pair<uint64_t, float>> out;
        if (k == 0) return out;
        mvfgpu_corpus_info inf;
        MVFGPU_INIT(inf);
        detail::check_gpu(mvfgpu_corpus_get_info(c_, &inf));
        const uint64_t es = column.data_type == MVF_DTYPE_UINT32 ? 4 : column.data_type == MVF_DTYPE_UINT64 ? 8 : 0;
        if (!es || column.size / es < inf.rows)
            throw MvfError(MVF_ERR_BUILD, es ? "metadata column '" + column.name + "' holds fewer values than the space has vectors"
                                             : "Unsupported metadata column data type");
        mvfgpu_column* col = nullptr;
        mvfgpu_partition* part = nullptr;
        std::vector<float> scores(k);
        std::vector<uint64_t> keys(k);
        uint32_t count = 0;
        int rc = mvfgpu_column_create(c_, column.data, column.data_type, 0, column.size / es, &col);
        if (rc == MVF_OK) rc = mvfgpu_partition_create(c_, col, &part);
        if (rc == MVF_OK)
            rc = mvfgpu_search_maxsim_candidates(c_, part, (uint8_t)metric_, query_vectors.data(), MVF_DTYPE_FLOAT32, dim_, 1,
                                                 (uint32_t)std::min<size_t>(n_tokens, UINT32_MAX), candidate_keys.data(),
                                                 (uint32_t)candidate_keys.size(), (uint32_t)k, scores.data(), keys.data(), &count);
        mvfgpu_partition_destroy(part);
        mvfgpu_column_destroy(col);
        detail::check_gpu(rc);
        for (uint32_t i = 0; i < count; i++) out.emplace_back(keys[i], scores[i]);
        return out;
    }
    // Which vector of every listed document scored best for every query vector (mvfgpu_maxsim_align; DESIGN.md section 3,
    // "Alignments").  `keys` holds values of `column` -- usually the documents find_top_k_documents or rerank_top_k_documents
    // just returned; alignments are not part of those searches: the recipe is the search, then this call on its keys.
    // -> [keys.size()][n_tokens] (vector index, score) in list order: the document's best vector for the token and its score; a
    // document's scores summed in token order are its rerank_top_k_documents score.  A value no live vector carries gets
    // (UINT64_MAX, +inf under L2 / -inf otherwise) for every token.  The column and the index live for this call.
    std::vector<std::vector<std::pair<uint64_t, float>>> align_documents(const std::vector<float>& query_vectors,
                                                                         const std::vector<uint64_t>& keys,
                                                                         const MetadataColumn& column) const {
        if (dt_ != DataType::Float32 && dt_ != DataType::Float16)
            throw MvfError(MVF_ERR_BUILD, "align_documents takes f32 queries: Float32 / Float16 spaces");
        if (dim_ == 0 || query_vectors.empty() || query_vectors.size() % (size_t)dim_)
            throw MvfError(MVF_ERR_DIMENSION_MISMATCH, "align_documents takes whole query vectors of the space's dimension");
        if (keys.size() > UINT32_MAX) throw MvfError(MVF_ERR_INVALID_ARGUMENT, "more than 2^32 - 1 keys");
        const size_t n_tokens = query_vectors.size() / (size_t)dim_;
        std::vector<std::vector<std::pair<uint64_t, float>>> out(keys.size());
        if (keys.empty()) return out;
        mvfgpu_corpus_info inf;
        MVFGPU_INIT(inf);
        detail::check_gpu(mvfgpu_corpus_get_info(c_, &inf));
        const uint64_t es = column.data_type == MVF_DTYPE_UINT32 ? 4 : column.data_type == MVF_DTYPE_UINT64 ? 8 : 0;
        if (!es || column.size / es < inf.rows)
            throw MvfError(MVF_ERR_BUILD, es ? "metadata column '" + column.name + "' holds fewer values than the space has vectors"
                                             : "Unsupported metadata column data type");
        mvfgpu_column* col = nullptr;
        mvfgpu_partition* part = nullptr;
        std::vector<float> scores(keys.size() * n_tokens);
        std::vector<uint64_t> rows(keys.size() * n_tokens);
        int rc = mvfgpu_column_create(c_, column.data, column.data_type, 0, column.size / es, &col);
        if (rc == MVF_OK) rc = mvfgpu_partition_create(c_, col, &part);
        if (rc == MVF_OK)
            rc = mvfgpu_maxsim_align(c_, part, (uint8_t)metric_, query_vectors.data(), MVF_DTYPE_FLOAT32, dim_, 1,
                                     (uint32_t)std::min<size_t>(n_tokens, UINT32_MAX), keys.data(), (uint32_t)keys.size(), scores.data(),
                                     rows.data(), nullptr);
        mvfgpu_partition_destroy(part);
        mvfgpu_column_destroy(col);
        detail::check_gpu(rc);
        for (size_t i = 0; i < keys.size(); i++)
            for (size_t t = 0; t < n_tokens; t++) out[i].emplace_back(rows[i * n_tokens + t], scores[i * n_tokens + t]);
        return out;
    }
    // The k-NN graph (mvfgpu_knn_join; DESIGN.md section 3, "Join"): for each of the rows [first, first + count) -- count
    // UINT64_MAX: to the end of the space -- its k nearest OTHER rows under the space's metric, best first.  A row is never its
    // own neighbour (decided by position: its exact duplicates are); a deleted row gets an empty list; fewer than k live
    // others give fewer hits.  The rows never leave the device.
    std::vector<std::vector<ScoredVector>> knn_graph(size_t k, uint64_t first = 0, uint64_t count = UINT64_MAX) const {
        if (count == UINT64_MAX) {
            mvfgpu_corpus_info inf;
            MVFGPU_INIT(inf);
            detail::check_gpu(mvfgpu_corpus_get_info(c_, &inf));
            count = inf.rows > first ? inf.rows - first : 0;
        }
        std::vector<std::vector<ScoredVector>> out((size_t)count);
        if (k == 0 || count == 0) return out;
        std::vector<float> scores((size_t)count * k);
        std::vector<uint64_t> idx((size_t)count * k);
        detail::check_gpu(mvfgpu_knn_join(c_, nullptr, (uint8_t)metric_, first, count, (uint32_t)k, MVFGPU_JOIN_EXCLUDE_SELF, scores.data(),
                                          idx.data(), nullptr));
        for (size_t i = 0; i < (size_t)count; i++)
            for (size_t j = 0; j < k && idx[i * k + j] != UINT64_MAX; j++) out[i].push_back({idx[i * k + j], scores[i * k + j], {}});
        return out;
    }
    mvfgpu_corpus* raw() const { return c_; }

private:
    mvfgpu_corpus* c_ = nullptr;
    uint32_t dim_;
    DistanceMetric metric_;
    DataType dt_;
};

// fn find_top_k_similar(space: &VectorSpace, query: &[f32], k: usize) -> Result<Vec<ScoredVector>, _>
inline std::vector<ScoredVector> find_top_k_similar(const VectorSpace& space, const std::vector<float>& query, size_t k) {
    return GpuVectorSpace(space).find_top_k_similar(query, k);
}

}  // namespace mvf
