// filter.hip — mvfgpu_filter_* and mvfgpu_search_filtered / mvfgpu_search_filtered_device: the exact top-k among the rows a
// reusable filter admits (include/mvf_gpu.h; DESIGN.md §3 "Filtered search", §5 "F0 / F1 / F2 — filtered search").
//
// A filter is built once, on the device: F0 (scan_filter.hip) re-bases the caller's allow bits to local rows and combines them
// with the handle's tombstones into a deny mask of the tombstone buffer's layout, counting the admitted rows per block; the
// total is read back (creation's one host wait); where the route rule could ever choose the list route, F1 then lays the
// admitted rows out as an ascending list.  A search takes one of two routes:
//   mask: api.hip's search with the deny mask in the tombstones' place -- the plain search's routes and kernels;
//   list: gather_topk (scan_gather.hip) -- F2, the gathered-row kernel, scores the listed rows chunk by chunk for groups of
//         queries with K1's one-query arithmetic, and the results are selected as the candidate search's are (candidates.hip).
// Both run under mvfgpu_search_device's stream discipline; the host call goes through search_host's staging.

#include "../../include/mvf_gpu.h"

#include "aux_kernels.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_candidates.h"
#include "scan_filter.h"

#include <algorithm>
#include <string>

using namespace mvf;

struct mvfgpu_filter {
    const mvfgpu_corpus* owner = nullptr;
    int device = 0;
    uint64_t tomb_gen = 0;  // the owner's tombstone generation the deny mask holds
    uint64_t rows = 0, admitted = 0;
    uint32_t dim = 0;
    uint8_t dtype = 0;
    int forced_route = 0;   // the owner's MVF_FILTER_ROUTE when the filter was created
    uint32_t* deny = nullptr;  // ceil(rows / 32) + 1 words
    uint32_t* list = nullptr;  // [admitted] ascending, or NULL
    size_t device_bytes = 0;
};

namespace {

// could any batch size send a filter of `admitted` rows down the list route?  (the rule falls with nq inside a route of the
// plain search and jumps where that route changes: one to four queries and the powers of two cover its steps)
bool list_possible(uint64_t rows, uint32_t dim, uint8_t dtype, uint64_t admitted) {
    for (uint32_t k : {1u, MVFGPU_K_PER_PASS + 1u})
        for (uint32_t nq : {1u, 2u, 3u, 4u, 8u, 16u, 32u, 64u, 128u, 256u, 1024u, 4096u, 65536u})
            if (filter_route_rule(rows, dim, dtype, nq, k, admitted) == 2u) return true;
    return false;
}

// F0 .. F1 on `s`, the allow bits already in device memory; waits once, for the admitted count
int build_filter(mvfgpu_filter* f, const CorpusView& v, const uint32_t* d_allow, uint32_t shift, hipStream_t s) {
    const uint64_t n = v.n;
    const size_t words = (size_t)((n + 31) / 32) + 1;
    const uint32_t nb = filter_blocks(n);
    MVF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&f->deny), words * 4));
    MVF_HIP_TRY(poison_fill(f->deny, words * 4));
    f->device_bytes = words * 4;
    AsyncBuf cnt, off, tot;
    MVF_HIP_TRY(cnt.alloc((size_t)nb * 4, s));
    MVF_HIP_TRY(off.alloc((size_t)nb * 8, s));
    MVF_HIP_TRY(tot.alloc(8, s));
    FilterMaskParams mp{};
    mp.allow = d_allow;
    mp.shift = shift;
    mp.n = n;
    mp.tomb = v.tomb;
    mp.deny = f->deny;
    mp.block_cnt = static_cast<uint32_t*>(cnt.p);
    MVF_HIP_TRY(filter_mask_launch(mp, s));
    MVF_HIP_TRY(filter_scan_launch(mp.block_cnt, nb, static_cast<uint64_t*>(off.p), static_cast<uint64_t*>(tot.p), s));
    uint64_t admitted = 0;
    MVF_HIP_TRY(hipMemcpyAsync(&admitted, tot.p, 8, hipMemcpyDeviceToHost, s));
    MVF_HIP_TRY(hipStreamSynchronize(s));
    f->admitted = admitted;
    const bool want_list = f->forced_route == 2 || (f->forced_route == 0 && list_possible(n, v.dim, v.dtype, admitted));
    if (want_list && admitted > 0) {
        MVF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&f->list), (size_t)admitted * 4));
        MVF_HIP_TRY(poison_fill(f->list, (size_t)admitted * 4));
        f->device_bytes += (size_t)admitted * 4;
        MVF_HIP_TRY(filter_compact_launch(f->deny, n, static_cast<const uint64_t*>(off.p), f->list, s));
    }
    return MVF_OK;
}

mvfgpu_filter* new_filter(const mvfgpu_corpus* c, const CorpusView& v) {
    mvfgpu_filter* f = new mvfgpu_filter();
    f->owner = c;
    f->device = v.device;
    f->tomb_gen = v.tomb_gen;
    f->rows = v.n;
    f->dim = v.dim;
    f->dtype = v.dtype;
    f->forced_route = v.filter_route;
    return f;
}

void free_filter(mvfgpu_filter* f) {
    if (f->deny) (void)hipFree(f->deny);
    if (f->list) (void)hipFree(f->list);
    delete f;
}

// the checks of both searches, none of which touches the device; then the route of this call
int check_filtered_args(const mvfgpu_corpus* c, const mvfgpu_filter* f, uint8_t metric, const void* queries, uint8_t query_dtype,
                        uint32_t query_dim, uint32_t nq, uint32_t k, const void* out_scores, const void* out_indices, FilterUse* use) {
    if (const int rc = check_search_scalars(metric, nq, k, queries, out_scores, out_indices)) return rc;
    if (!f) return set_fail(MVF_ERR_INVALID_ARGUMENT, "filter is NULL");
    const int rc = check_search_args(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices);
    if (rc != MVF_OK) return rc;
    if (f->owner != c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the filter was created for another corpus handle");
    const CorpusView v = corpus_view(c);
    if (f->tomb_gen != v.tomb_gen)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "stale filter: mvfgpu_corpus_set_tombstones changed the handle's tombstones after the filter was created");
    use->deny = f->deny;
    use->list = f->list;
    use->admitted = f->admitted;
    const uint32_t route = f->forced_route ? (uint32_t)f->forced_route : filter_route_rule(f->rows, f->dim, f->dtype, nq, k, f->admitted);
    use->by_list = route == 2u && f->list != nullptr;
    return MVF_OK;
}

}  // namespace

namespace mvf {

int filter_list_search(const CorpusView& v, const FilterUse& flt, uint8_t metric, const void* d_queries, uint32_t nq, uint32_t k,
                       float* d_scores, uint64_t* d_indices, int32_t* d_raw, hipStream_t s) {
    if (flt.admitted == 0 || v.n == 0) return fill_padding(metric, nq, k, d_scores, d_indices, d_raw, s);  // nothing admitted
    GatherSource src;
    src.m = (uint32_t)flt.admitted;  // a shard holds fewer than 2^32 rows
    src.qg = one_query_group(v).qg;
    src.list = flt.list;
    return gather_topk(v, metric, d_queries, nq, src, k, d_scores, d_indices, d_raw, s);
}

int filter_from_allow_words(const mvfgpu_corpus* c, const CorpusView& v, const uint32_t* d_allow, hipStream_t s, mvfgpu_filter** out) {
    mvfgpu_filter* f = new_filter(c, v);
    const int rc = build_filter(f, v, d_allow, 0u, s);
    if (rc != MVF_OK) {
        free_filter(f);
        return rc;
    }
    *out = f;
    return MVF_OK;
}

FilterOrigin filter_origin(const mvfgpu_filter* f) { return FilterOrigin{f->owner, f->tomb_gen, f->deny}; }

}  // namespace mvf

extern "C" {

int mvfgpu_filter_create(const mvfgpu_corpus* c, const uint8_t* allow_bitmap, uint64_t first_bit, uint64_t nbits, mvfgpu_filter** out) {
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (!allow_bitmap || !out) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    *out = nullptr;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));  // the handle's own stream belongs to the host-buffer calls
    mvfgpu_filter* f = nullptr;
    const int rc = [&]() -> int {
        const CorpusView v = corpus_view(c);
        if (first_bit + v.n > nbits || first_bit + v.n < first_bit)
            return set_fail(MVF_ERR_INVALID_ARGUMENT, "allow bitmap covers fewer rows than the shard holds");
        hipStream_t s = static_cast<hipStream_t>(v.stream);
        f = new_filter(c, v);
        // the bytes that hold the shard's bits go up from the 4-byte boundary in front of first_bit: F0 shifts by 0 .. 31
        const uint64_t byte0 = (first_bit >> 3) & ~3ull;
        const uint32_t shift = (uint32_t)(first_bit - byte0 * 8);
        const size_t nbytes = (size_t)((shift + v.n + 7) / 8);
        const size_t up_words = (nbytes + 3) / 4 + 2;  // F0 reads one word past the last it needs; zeros
        AsyncBuf up;
        return corpus_device_call(c, s, [&]() -> int {
            MVF_HIP_TRY(up.alloc(up_words * 4, s));
            MVF_HIP_TRY(hipMemsetAsync(up.p, 0, up_words * 4, s));
            if (nbytes) MVF_HIP_TRY(hipMemcpyAsync(up.p, allow_bitmap + byte0, nbytes, hipMemcpyHostToDevice, s));
            return build_filter(f, corpus_view(c), static_cast<const uint32_t*>(up.p), shift, s);
        });
    }();
    if (rc != MVF_OK) {
        if (f) free_filter(f);
        return rc;
    }
    *out = f;
    return MVF_OK;
}

int mvfgpu_filter_create_device(const mvfgpu_corpus* c, const uint32_t* d_allow_words, void* hip_stream, mvfgpu_filter** out) {
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (!d_allow_words || !out) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    *out = nullptr;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    mvfgpu_filter* f = new_filter(c, corpus_view(c));
    const int rc = corpus_device_call(c, s, [&]() -> int {
        const CorpusView v = corpus_view(c);
        f->tomb_gen = v.tomb_gen;
        return build_filter(f, v, d_allow_words, 0u, s);
    });
    if (rc != MVF_OK) {
        free_filter(f);
        return rc;
    }
    *out = f;
    return MVF_OK;
}

void mvfgpu_filter_destroy(mvfgpu_filter* f) {
    if (!f) return;
    DevScope guard(f->device);
    (void)corpus_wait_newest(f->owner);  // a search enqueued on the handle may still read the mask or the list
    free_filter(f);
}

int mvfgpu_filter_get_info(const mvfgpu_filter* f, mvfgpu_filter_info* out) {
    if (!f) return set_fail(MVF_ERR_INVALID_ARGUMENT, "filter is NULL");
    if (!out) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    mvfgpu_filter_info inf{};
    inf.has_row_list = f->list ? 1u : 0u;
    inf.rows = f->rows;
    inf.admitted = f->admitted;
    inf.device_bytes = f->device_bytes;
    return copy_out_struct(out, inf);
}

int mvfgpu_search_filtered(const mvfgpu_corpus* c, const mvfgpu_filter* f, uint8_t metric, const void* queries, uint8_t query_dtype,
                           uint32_t query_dim, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_indices, int32_t* out_raw) {
    FilterUse use;
    const int rc = check_filtered_args(c, f, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices, &use);
    if (rc != MVF_OK) return rc;
    return search_filtered_host(c, use, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices, out_raw);
}

int mvfgpu_search_filtered_device(const mvfgpu_corpus* c, const mvfgpu_filter* f, uint8_t metric, const void* d_queries,
                                  uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k, float* d_scores,
                                  uint64_t* d_indices, int32_t* d_raw, void* hip_stream) {
    FilterUse use;
    const int rc = check_filtered_args(c, f, metric, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices, &use);
    if (rc != MVF_OK) return rc;
    return search_filtered_device(c, use, metric, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices, d_raw, hip_stream);
}

}  // extern "C"
