// partition.hip — mvfgpu_partition_* and mvfgpu_search_partitioned / mvfgpu_search_partitioned_device: an index of a handle's
// live rows grouped by a column's value, and the exact top-k of every query among the rows that carry the query's own key
// (include/mvf_gpu.h; DESIGN.md §3 "Partitioned search", §5 "B0 / B1 / B2 / S1 — partitioned search").
//
// The index is built once, on the device (scan_partition.hip): B0 lays down the live rows' (key, row) pairs in position order,
// B1 sorts them by key -- stable, and only in the 8-bit digits the keys differ in --, B2 writes the table of distinct keys and
// their offsets, which is copied to a host mirror.  Creation waits twice (live count and differing bits; number of keys).
//
// A search plans on the host, from the mirror: every query is padding (no live row carries its key), small tier (its rows
// fit one chunk of the gathered-row kernel) or large tier.  The small tier is one launch of S1 and one of K3 per window of
// queries, whatever the number of keys; the large tier is one gather_topk (scan_gather.hip) per distinct key -- what the
// filtered search's list route runs for a filter whose list is that key's segment.  The results are computed in the plan's
// order and put into the caller's order, padding rows included, by one kernel.  The plan travels through a pinned buffer of
// the index; no host wait but for that buffer's previous upload (an event that has long passed when searches do not pile up).
// The host call runs the same device work per host window (host_staging.h).

#include "../../include/mvf_gpu.h"

#include "aux_kernels.h"
#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_filter.h"
#include "scan_gather.h"
#include "scan_partition.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace mvf;

struct mvfgpu_partition {
    const mvfgpu_corpus* owner = nullptr;
    int device = 0;
    uint64_t tomb_gen = 0;  // the owner's tombstone generation the index holds
    uint8_t key_type = 0;
    uint64_t rows = 0, live = 0, n_keys = 0, largest = 0;
    uint32_t* rows_by_key = nullptr;  // [live] local rows, grouped by key, ascending inside a key
    uint64_t* table = nullptr;        // device key table: keys[n_keys] ascending, then offsets[n_keys + 1]
    size_t device_bytes = 0;
    std::vector<uint64_t> mirror;     // the host mirror of the table, same layout
    // the plan's way to the device: pinned, reused by every search of the index (they run under the owner's lock); `copied`
    // follows the upload of the plan it holds
    mutable void* pin = nullptr;
    mutable size_t pin_bytes = 0;
    mutable hipEvent_t copied = nullptr;
    mutable bool pin_busy = false;

    const uint64_t* keys() const { return mirror.data(); }
    const uint64_t* offsets() const { return mirror.data() + n_keys; }
    // (offset, count) of `key`'s rows; count 0 for a key no live row carries.  from (nullable): keys looked up in ascending order
    // search only the table behind the previous one's place, which *from carries (0 at first)
    void find(uint64_t key, uint64_t* offset, uint64_t* count, uint64_t* from = nullptr) const {
        const uint64_t* k0 = keys();
        const uint64_t* it = std::lower_bound(k0 + (from ? std::min(*from, n_keys) : 0), k0 + n_keys, key);
        if (from) *from = (uint64_t)(it - k0);
        if (it == k0 + n_keys || *it != key) {
            *offset = 0, *count = 0;
            return;
        }
        const uint64_t j = (uint64_t)(it - k0);
        *offset = offsets()[j], *count = offsets()[j + 1] - offsets()[j];
    }
};

namespace {

constexpr uint32_t kSmallWindow = 1024;  // small-tier queries per launch of S1 and K3

// ---- the plan: a pure function of every query's row count and key
struct PartGroup {
    uint32_t first, nq;     // the group's entries of the plan
    uint64_t offset, count;
};
struct PartPlan {
    std::vector<PartQuery> entries;  // [nq]: the small tier's queries, the large tier's group by group, the padding queries
    std::vector<PartGroup> groups;   // the large tier: one per distinct key, ascending key, ascending query inside
    uint32_t n_small = 0, n_large = 0;
};

uint32_t tier_of(uint64_t count, uint32_t k, bool query_fits) {
    if (count == 0) return 0u;
    return query_fits && count <= kGatherChunk && k <= MVFGPU_K_PER_PASS ? 1u : 2u;
}

// query_fits: the padded query fits S1's LDS budget (kCandQueryLdsMax); beyond it every query goes to the large tier, whose
// kernel reads one float query through the cache.  tier (nullable) receives every query's case.
void plan_partitioned(const uint64_t* counts, const uint64_t* offsets, const uint64_t* keys, uint32_t nq, uint32_t k, bool query_fits,
                      uint32_t* tier, PartPlan* plan) {
    plan->entries.clear();
    plan->groups.clear();
    plan->entries.reserve(nq);
    std::vector<uint32_t> large, pad;
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t t = tier_of(counts[q], k, query_fits);
        if (tier) tier[q] = t;
        if (t == 1u) plan->entries.push_back(PartQuery{q, offsets ? (uint32_t)offsets[q] : 0u, (uint32_t)counts[q]});
        else (t == 2u ? large : pad).push_back(q);
    }
    plan->n_small = (uint32_t)plan->entries.size();
    std::stable_sort(large.begin(), large.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    for (size_t i = 0; i < large.size(); i++) {
        const uint32_t q = large[i];
        if (i == 0 || keys[q] != keys[large[i - 1]])
            plan->groups.push_back(PartGroup{(uint32_t)plan->entries.size(), 0u, offsets ? offsets[q] : 0u, counts[q]});
        plan->groups.back().nq++;
        plan->entries.push_back(PartQuery{q, offsets ? (uint32_t)offsets[q] : 0u, (uint32_t)std::min<uint64_t>(counts[q], 0xFFFFFFFFull)});
    }
    plan->n_large = (uint32_t)large.size();
    for (uint32_t q : pad) plan->entries.push_back(PartQuery{q, 0u, 0u});
}

void free_partition(mvfgpu_partition* p) {
    if (p->rows_by_key) (void)hipFree(p->rows_by_key);
    if (p->table) (void)hipFree(p->table);
    if (p->pin) (void)hipHostFree(p->pin);
    if (p->copied) (void)hipEventDestroy(p->copied);
    delete p;
}

// B0 .. B2 on `s`; waits twice
int build_partition(mvfgpu_partition* p, const CorpusView& v, const void* values, bool is_u64, hipStream_t s) {
    MVF_HIP_TRY(hipEventCreateWithFlags(&p->copied, hipEventDisableTiming));
    const uint64_t n = v.n;
    if (n == 0) return MVF_OK;
    // B0: live rows per block, the bits the live keys differ in
    const uint32_t nb = part_blocks(n);
    AsyncBuf cnt, off, stat;
    MVF_HIP_TRY(cnt.alloc((size_t)nb * 4, s));
    MVF_HIP_TRY(off.alloc((size_t)nb * 8, s));
    MVF_HIP_TRY(stat.alloc(24, s));  // live rows | OR of the live keys | AND of the live keys
    uint64_t* dstat = static_cast<uint64_t*>(stat.p);
    MVF_HIP_TRY(hipMemsetAsync(dstat, 0, 16, s));
    MVF_HIP_TRY(hipMemsetAsync(dstat + 2, 0xFF, 8, s));
    MVF_HIP_TRY(part_count_launch(values, is_u64, n, v.tomb, static_cast<uint32_t*>(cnt.p), dstat + 1, s));
    MVF_HIP_TRY(filter_scan_launch(static_cast<const uint32_t*>(cnt.p), nb, static_cast<uint64_t*>(off.p), dstat, s));
    uint64_t hstat[3] = {0, 0, 0};
    MVF_HIP_TRY(hipMemcpyAsync(hstat, dstat, 24, hipMemcpyDeviceToHost, s));
    MVF_HIP_TRY(hipStreamSynchronize(s));
    const uint64_t live = hstat[0], differ = hstat[1] ^ hstat[2];
    p->live = live;
    if (live == 0) return MVF_OK;

    MVF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->rows_by_key), (size_t)live * 4));
    MVF_HIP_TRY(poison_fill(p->rows_by_key, (size_t)live * 4));
    p->device_bytes = (size_t)live * 4;
    // B0: the pairs in position order; B1: sorted by key, only in the digits that differ
    const uint32_t NB = part_sort_tiles(live);
    AsyncBuf ka, kb, ra, rb, bh, tot;
    MVF_HIP_TRY(ka.alloc((size_t)live * 8, s));
    MVF_HIP_TRY(kb.alloc((size_t)live * 8, s));
    MVF_HIP_TRY(ra.alloc((size_t)live * 4, s));
    MVF_HIP_TRY(rb.alloc((size_t)live * 4, s));
    MVF_HIP_TRY(bh.alloc((size_t)256 * NB * 4, s));
    MVF_HIP_TRY(tot.alloc(256 * 4, s));
    uint64_t *kcur = static_cast<uint64_t*>(ka.p), *koth = static_cast<uint64_t*>(kb.p);
    uint32_t *rcur = static_cast<uint32_t*>(ra.p), *roth = static_cast<uint32_t*>(rb.p);
    MVF_HIP_TRY(part_compact_launch(values, is_u64, n, v.tomb, static_cast<const uint64_t*>(off.p), kcur, rcur, s));
    for (int shift = 0; shift < 64; shift += 8) {
        if (!((differ >> shift) & 0xFFull)) continue;
        MVF_HIP_TRY(part_sort_pass_launch(kcur, rcur, koth, roth, live, shift, static_cast<uint32_t*>(bh.p), static_cast<uint32_t*>(tot.p), s));
        std::swap(kcur, koth);
        std::swap(rcur, roth);
    }
    MVF_HIP_TRY(hipMemcpyAsync(p->rows_by_key, rcur, (size_t)live * 4, hipMemcpyDeviceToDevice, s));
    // B2: the distinct keys
    const uint32_t hb = part_blocks(live);
    AsyncBuf hcnt, hoff, htot;
    MVF_HIP_TRY(hcnt.alloc((size_t)hb * 4, s));
    MVF_HIP_TRY(hoff.alloc((size_t)hb * 8, s));
    MVF_HIP_TRY(htot.alloc(8, s));
    MVF_HIP_TRY(part_heads_count_launch(kcur, live, static_cast<uint32_t*>(hcnt.p), s));
    MVF_HIP_TRY(filter_scan_launch(static_cast<const uint32_t*>(hcnt.p), hb, static_cast<uint64_t*>(hoff.p), static_cast<uint64_t*>(htot.p), s));
    uint64_t n_keys = 0;
    MVF_HIP_TRY(hipMemcpyAsync(&n_keys, htot.p, 8, hipMemcpyDeviceToHost, s));
    MVF_HIP_TRY(hipStreamSynchronize(s));
    if (n_keys == 0 || n_keys > live) return set_fail(MVF_ERR_DEVICE, "partition build: the key table's size does not fit the live rows");
    const size_t table_bytes = (size_t)(2 * n_keys + 1) * 8;
    MVF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p->table), table_bytes));
    MVF_HIP_TRY(poison_fill(p->table, table_bytes));
    p->device_bytes += table_bytes;
    MVF_HIP_TRY(part_heads_write_launch(kcur, live, static_cast<const uint64_t*>(hoff.p), p->table, p->table + n_keys, s));
    p->mirror.resize((size_t)(2 * n_keys + 1));
    MVF_HIP_TRY(hipMemcpyAsync(p->mirror.data(), p->table, table_bytes, hipMemcpyDeviceToHost, s));
    MVF_HIP_TRY(hipStreamSynchronize(s));
    p->n_keys = n_keys;
    for (uint64_t j = 0; j < n_keys; j++) p->largest = std::max(p->largest, p->offsets()[j + 1] - p->offsets()[j]);
    return MVF_OK;
}

// the checks of both searches, none of which touches the device
int check_partitioned_args(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries, uint8_t query_dtype,
                           uint32_t query_dim, uint32_t nq, const uint64_t* keys, uint32_t k, const void* out_scores, const void* out_indices) {
    if (const int rc = check_search_scalars(metric, nq, k, queries, out_scores, out_indices)) return rc;
    if (!keys) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer (keys)");
    if (!part) return set_fail(MVF_ERR_INVALID_ARGUMENT, "partition is NULL");
    if (const int rc = check_search_args(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices)) return rc;
    return check_partition_use(c, part);
}

// The plan of `nq` queries to `dst` on `s`
int upload_plan(const mvfgpu_partition* part, const PartPlan& plan, void* dst, hipStream_t s) {
    return partition_upload(part, plan.entries.data(), plan.entries.size() * sizeof(PartQuery), dst, s);
}

}  // namespace

namespace mvf {
int partition_upload(const mvfgpu_partition* part, const void* src, size_t bytes, void* dst, hipStream_t s) {
    if (!bytes) return MVF_OK;
    if (part->pin_busy) {  // the previous search's upload still reads the buffer
        MVF_HIP_TRY(hipEventSynchronize(part->copied));
        part->pin_busy = false;
    }
    if (part->pin_bytes < bytes) {
        if (part->pin) (void)hipHostFree(part->pin);
        part->pin = nullptr, part->pin_bytes = 0;
        const size_t want = std::max<size_t>(bytes, 16u << 10);
        MVF_HIP_TRY(hipHostMalloc(&part->pin, want, hipHostMallocDefault));
        poison_fill_host(part->pin, want);
        part->pin_bytes = want;
    }
    std::memcpy(part->pin, src, bytes);
    MVF_HIP_TRY(hipMemcpyAsync(dst, part->pin, bytes, hipMemcpyHostToDevice, s));
    MVF_HIP_TRY(hipEventRecord(part->copied, s));
    part->pin_busy = true;
    return MVF_OK;
}
void partition_find(const mvfgpu_partition* part, uint64_t key, uint64_t* offset, uint64_t* count, uint64_t* from) {
    part->find(key, offset, count, from);
}
}  // namespace mvf

namespace {

// The device work of both calls: queries and results in device memory, `keys` on the host; everything on `s`.  Runs under
// corpus_device_call.
int partitioned_core(const CorpusView& v, const mvfgpu_partition* part, uint8_t metric, const void* d_queries, uint32_t nq,
                     const uint64_t* keys, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, hipStream_t s) {
    if (part->n_keys == 0) return fill_padding(metric, nq, k, d_scores, d_indices, d_raw, s);
    const OneQueryGroup g1 = one_query_group(v);
    std::vector<uint64_t> counts(nq), offsets(nq);
    for (uint32_t q = 0; q < nq; q++) part->find(keys[q], &offsets[q], &counts[q]);
    PartPlan plan;
    plan_partitioned(counts.data(), offsets.data(), keys, nq, k, g1.qbytes <= kCandQueryLdsMax, nullptr, &plan);
    const uint32_t n_scored = plan.n_small + plan.n_large;
    if (n_scored == 0) return fill_padding(metric, nq, k, d_scores, d_indices, d_raw, s);

    const size_t qrow = query_row_bytes(v);
    AsyncBuf dplan, csc, cidx, craw, dlists, dql;
    MVF_HIP_TRY(dplan.alloc((size_t)nq * sizeof(PartQuery), s));
    if (const int rc = upload_plan(part, plan, dplan.p, s)) return rc;
    const PartQuery* d_plan = static_cast<const PartQuery*>(dplan.p);
    // the results in the plan's order
    MVF_HIP_TRY(csc.alloc((size_t)n_scored * k * 4, s));
    MVF_HIP_TRY(cidx.alloc((size_t)n_scored * k * 8, s));
    if (d_raw) MVF_HIP_TRY(craw.alloc((size_t)n_scored * k * 4, s));
    float* c_scores = static_cast<float*>(csc.p);
    uint64_t* c_indices = static_cast<uint64_t*>(cidx.p);
    int32_t* c_raw = static_cast<int32_t*>(craw.p);

    if (plan.n_small) {  // S1 + K3 per window
        const uint32_t kcap = next_pow2(k);
        const uint32_t W = std::min(plan.n_small, kSmallWindow);
        MVF_HIP_TRY(dlists.alloc((size_t)W * kcap * 8, s));
        SegmentScoreParams sp{};
        sp.rows = v.rows;
        sp.queries = d_queries;
        sp.rows_by_key = part->rows_by_key;
        sp.dim = v.dim;
        sp.pitch = v.pitch;
        sp.V = v.V;
        sp.J = g1.J;
        sp.lists = static_cast<uint64_t*>(dlists.p);
        sp.kcap = kcap;
        SelectParams fp{};
        fp.k = k;
        fp.metric = metric;
        fp.dtype = v.dtype;
        fp.index_base = v.index_base;
        fp.ids = v.ids;
        fp.lists = sp.lists;
        fp.nlists = 1;
        fp.kcap = kcap;
        fp.heads = k;
        fp.P = 4096;
        for (uint32_t w0 = 0; w0 < plan.n_small; w0 += W) {
            const uint32_t wn = std::min(W, plan.n_small - w0);
            sp.plan = d_plan + w0;
            sp.n = wn;
            MVF_HIP_TRY(segment_score_launch(v.dtype, metric, g1.G, sp, s));
            fp.out_scores = c_scores + (size_t)w0 * k;
            fp.out_indices = c_indices + (size_t)w0 * k;
            fp.out_raw = c_raw ? c_raw + (size_t)w0 * k : nullptr;
            MVF_HIP_TRY(launch_select_final(fp, wn, s));
        }
    }
    if (plan.n_large) {  // per key, what the filtered search's list route runs for that key's segment
        MVF_HIP_TRY(dql.alloc((size_t)plan.n_large * qrow, s));
        MVF_HIP_TRY(part_gather_queries_launch(d_queries, d_plan + plan.n_small, plan.n_large, (uint32_t)qrow, dql.p, s));
        for (const PartGroup& g : plan.groups) {
            GatherSource src;
            src.m = (uint32_t)g.count;  // a shard holds fewer than 2^32 rows
            src.qg = g1.qg;
            src.list = part->rows_by_key + g.offset;
            const size_t l0 = g.first - plan.n_small;  // the group's first query among the gathered ones
            const int rc = gather_topk(v, metric, static_cast<const unsigned char*>(dql.p) + l0 * qrow, g.nq, src, k,
                                       c_scores + (size_t)g.first * k, c_indices + (size_t)g.first * k,
                                       c_raw ? c_raw + (size_t)g.first * k : nullptr, s);
            if (rc != MVF_OK) return rc;
        }
    }
    PartScatterParams ps{};
    ps.plan = d_plan;
    ps.nq = nq;
    ps.n_scored = n_scored;
    ps.k = k;
    ps.metric = metric;
    ps.c_scores = c_scores;
    ps.c_indices = c_indices;
    ps.c_raw = c_raw;
    ps.out_scores = d_scores;
    ps.out_indices = d_indices;
    ps.out_raw = d_raw;
    MVF_HIP_TRY(part_scatter_launch(ps, s));
    return MVF_OK;
}

}  // namespace

namespace mvf {
PartitionView partition_view(const mvfgpu_partition* part) {
    return PartitionView{part->owner, part->tomb_gen, part->rows_by_key, part->table, part->live, part->n_keys, part->largest};
}
int check_partition_use(const mvfgpu_corpus* c, const mvfgpu_partition* part) {
    if (part->owner != c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the partition was created for another corpus handle");
    if (part->tomb_gen != corpus_view(c).tomb_gen)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "stale partition: mvfgpu_corpus_set_tombstones changed the handle's tombstones after the partition was created");
    return MVF_OK;
}
}  // namespace mvf

extern "C" {

int mvfgpu_partition_create(const mvfgpu_corpus* c, const mvfgpu_column* column, mvfgpu_partition** out) {
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (!column) return set_fail(MVF_ERR_INVALID_ARGUMENT, "column is NULL");
    if (!out) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    *out = nullptr;
    const ColumnOrigin col = column_origin(column);
    if (col.owner != c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the column was created for another corpus handle");
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));  // the handle's own stream belongs to the host-buffer calls
    hipStream_t s = static_cast<hipStream_t>(corpus_view(c).stream);
    mvfgpu_partition* p = new mvfgpu_partition();
    const int rc = corpus_device_call(c, s, [&]() -> int {
        const CorpusView v = corpus_view(c);
        p->owner = c;
        p->device = v.device;
        p->tomb_gen = v.tomb_gen;
        p->key_type = col.dtype;
        p->rows = v.n;
        return build_partition(p, v, col.values, col.dtype == MVF_DTYPE_UINT64, s);
    });
    if (rc != MVF_OK) {
        (void)hipStreamSynchronize(s);  // nothing enqueued may still write what is freed
        free_partition(p);
        return rc;
    }
    *out = p;
    return MVF_OK;
}

void mvfgpu_partition_destroy(mvfgpu_partition* p) {
    if (!p) return;
    DevScope guard(p->device);
    (void)corpus_wait_newest(p->owner);  // a search enqueued on the handle may still read the rows or the plan buffer
    free_partition(p);
}

int mvfgpu_partition_get_info(const mvfgpu_partition* p, mvfgpu_partition_info* out) {
    if (!p) return set_fail(MVF_ERR_INVALID_ARGUMENT, "partition is NULL");
    if (!out) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    mvfgpu_partition_info inf{};
    inf.key_type = p->key_type;
    inf.rows = p->rows;
    inf.live_rows = p->live;
    inf.n_keys = p->n_keys;
    inf.largest = p->largest;
    inf.device_bytes = p->device_bytes;
    inf.host_bytes = p->mirror.size() * 8;
    return copy_out_struct(out, inf);
}

int mvfgpu_partition_lookup(const mvfgpu_partition* p, const uint64_t* keys, uint64_t n, uint64_t* out_counts) {
    if (!p) return set_fail(MVF_ERR_INVALID_ARGUMENT, "partition is NULL");
    if (n && (!keys || !out_counts)) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    for (uint64_t i = 0; i < n; i++) {
        uint64_t off;
        p->find(keys[i], &off, &out_counts[i]);
    }
    return MVF_OK;
}

int mvfgpu_partition_keys(const mvfgpu_partition* p, uint64_t first, uint64_t count, uint64_t* out_keys, uint64_t* out_counts) {
    if (!p) return set_fail(MVF_ERR_INVALID_ARGUMENT, "partition is NULL");
    if (count && (!out_keys || !out_counts)) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (first > p->n_keys || count > p->n_keys - first)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "[first, first + count) exceeds the partition's " + std::to_string(p->n_keys) + " keys");
    for (uint64_t i = 0; i < count; i++) {
        out_keys[i] = p->keys()[first + i];
        out_counts[i] = p->offsets()[first + i + 1] - p->offsets()[first + i];
    }
    return MVF_OK;
}

int mvfgpu_search_partitioned_device(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                     uint8_t query_dtype, uint32_t query_dim, uint32_t nq, const uint64_t* keys, uint32_t k,
                                     float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream) {
    const int rc = check_partitioned_args(c, part, metric, d_queries, query_dtype, query_dim, nq, keys, k, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        return partitioned_core(corpus_view(c), part, metric, d_queries, nq, keys, k, d_scores, d_indices, d_raw, s);
    });
}

int mvfgpu_search_partitioned(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries,
                              uint8_t query_dtype, uint32_t query_dim, uint32_t nq, const uint64_t* keys, uint32_t k,
                              float* out_scores, uint64_t* out_indices, int32_t* out_raw) {
    const int rc0 = check_partitioned_args(c, part, metric, queries, query_dtype, query_dim, nq, keys, k, out_scores, out_indices);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, query_row_bytes(v)}};
    const HostOut out[] = {{out_indices, (size_t)k * 8}, {out_scores, (size_t)k * 4}, {out_raw, (size_t)k * 4}};
    return stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t w0, uint32_t wn, void* const* d_in, void* const* d_out) {
        return partitioned_core(v, part, metric, d_in[0], wn, keys + w0, k, static_cast<float*>(d_out[1]), static_cast<uint64_t*>(d_out[0]),
                                static_cast<int32_t*>(d_out[2]), s);
    });
}

int mvfgpu_selftest_partition_plan(const uint64_t* counts, const uint64_t* keys, uint32_t nq, uint32_t k, uint32_t* out_tier,
                                   uint32_t* out_groups) {
    if (!counts || !keys || !out_tier || !out_groups) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (k == 0 || k > MVFGPU_MAX_K) return set_fail(MVF_ERR_INVALID_ARGUMENT, "k must be in 1..2^31");
    PartPlan plan;
    plan_partitioned(counts, nullptr, keys, nq, k, true, out_tier, &plan);
    *out_groups = (uint32_t)plan.groups.size();
    return MVF_OK;
}

}  // extern "C"
