// columns.hip — mvfgpu_column_* and mvfgpu_filter_create_where: per-row metadata values resident next to the rows, and filters
// built from predicates over them on the device (include/mvf_gpu.h; DESIGN.md §3 "Column filters", §5 "P0 — column predicates").
//
// A column is a plain copy of one UInt32 / UInt64 value per local row.  A where-call normalises its clauses on the host --
// every comparison becomes one range test, possibly negated; set values are sorted, de-duplicated and uploaded with the call --
// and P0 (scan_columns.hip) writes the allow words of the whole predicate, the base filter included, in one launch.  From there
// the filter is built by the bitmap filters' own code (filter.hip: F0 / F1), so it is the same object in every respect.

#include "../../include/mvf_gpu.h"

#include "internal.h"
#include "scan_columns.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace mvf;

struct mvfgpu_column {
    const mvfgpu_corpus* owner = nullptr;
    int device = 0;
    uint8_t dtype = 0;
    uint64_t rows = 0;
    void* values = nullptr;  // [rows] u32 or u64
    size_t device_bytes = 0;
};

namespace {

uint32_t column_elem_size(uint8_t data_type) { return data_type == MVF_DTYPE_UINT32 ? 4u : data_type == MVF_DTYPE_UINT64 ? 8u : 0u; }

mvfgpu_column* new_column(const mvfgpu_corpus* c, const CorpusView& v, uint8_t data_type) {
    mvfgpu_column* col = new mvfgpu_column();
    col->owner = c;
    col->device = v.device;
    col->dtype = data_type;
    col->rows = v.n;
    return col;
}

void free_column(mvfgpu_column* col) {
    if (col->values) (void)hipFree(col->values);
    delete col;
}

int alloc_column(mvfgpu_column* col) {
    col->device_bytes = (size_t)col->rows * column_elem_size(col->dtype);
    MVF_HIP_TRY(hipMalloc(&col->values, std::max<size_t>(col->device_bytes, 16)));
    MVF_HIP_TRY(poison_fill(col->values, std::max<size_t>(col->device_bytes, 16)));
    return MVF_OK;
}

struct Range {
    uint64_t lo = 1, hi = 0;  // empty
    uint32_t negate = 0;
};

// every operator but IN / NOT_IN as lo <= v <= hi over the values of `data_type`; false: not such an operator
bool predicate_range(uint8_t data_type, uint32_t op, uint64_t a, uint64_t b, Range* out) {
    const uint64_t top = UINT64_MAX, tmax = data_type == MVF_DTYPE_UINT32 ? 0xFFFFFFFFull : top;
    bool some = true;
    uint64_t lo = 0, hi = top;
    switch (op) {
    case MVFGPU_OP_EQ:
    case MVFGPU_OP_NE: lo = hi = a; break;
    case MVFGPU_OP_LT: some = a != 0, hi = a - 1; break;
    case MVFGPU_OP_LE: hi = a; break;
    case MVFGPU_OP_GT: some = a != top, lo = a + 1; break;
    case MVFGPU_OP_GE: lo = a; break;
    case MVFGPU_OP_BETWEEN: lo = a, hi = b; break;
    default: return false;
    }
    hi = std::min(hi, tmax);
    Range r;
    r.negate = op == MVFGPU_OP_NE ? 1u : 0u;
    if (some && lo <= hi) r.lo = lo, r.hi = hi;
    *out = r;
    return true;
}

// a where-call checked and normalised: what P0 takes but the device buffers
struct WherePlan {
    WhereParams p{};
    std::vector<uint64_t> sets;
};

// every refusal of mvfgpu_filter_create_where, none of which touches the device -- and, up to the columns' own checks, none of
// which reads the handle
int plan_where(const mvfgpu_corpus* c, const mvfgpu_predicate* clauses, uint32_t n_clauses, uint32_t combine, const mvfgpu_filter* base,
               WherePlan* plan) {
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (!clauses) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (n_clauses < 1 || n_clauses > MVFGPU_WHERE_MAX_CLAUSES)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "n_clauses must be in 1.." + std::to_string(MVFGPU_WHERE_MAX_CLAUSES) + ", got " + std::to_string(n_clauses));
    if (combine != MVFGPU_WHERE_ALL && combine != MVFGPU_WHERE_ANY)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "unknown combine code " + std::to_string(combine) + " (MVFGPU_WHERE_ALL or MVFGPU_WHERE_ANY)");
    WhereParams& p = plan->p;
    p.n_clauses = n_clauses;
    p.any = combine == MVFGPU_WHERE_ANY ? 1u : 0u;
    for (uint32_t i = 0; i < n_clauses; i++) {
        const mvfgpu_predicate& in = clauses[i];
        WhereClause& cl = p.clause[i];
        if (in.op > MVFGPU_OP_NOT_IN)
            return set_fail(MVF_ERR_INVALID_ARGUMENT, "clause " + std::to_string(i) + ": unknown predicate op " + std::to_string(in.op));
        if (in.op != MVFGPU_OP_IN && in.op != MVFGPU_OP_NOT_IN) continue;
        if (in.n_values && !in.values)
            return set_fail(MVF_ERR_INVALID_ARGUMENT, "clause " + std::to_string(i) + ": values is NULL with n_values > 0");
        std::vector<uint64_t> vals(in.values, in.values + in.n_values);
        std::sort(vals.begin(), vals.end());
        vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
        if (plan->sets.size() + vals.size() > MVFGPU_WHERE_MAX_SET_VALUES)
            return set_fail(MVF_ERR_INVALID_ARGUMENT,
                            "more than " + std::to_string(MVFGPU_WHERE_MAX_SET_VALUES) +
                                " distinct IN / NOT_IN values in one call: evaluate the predicate into a bitmap and use mvfgpu_filter_create");
        cl.is_set = 1;
        cl.negate = in.op == MVFGPU_OP_NOT_IN ? 1 : 0;
        cl.set_first = (uint32_t)plan->sets.size();
        cl.set_count = (uint32_t)vals.size();
        plan->sets.insert(plan->sets.end(), vals.begin(), vals.end());
    }
    p.n_sets = (uint32_t)plan->sets.size();
    for (uint32_t i = 0; i < n_clauses; i++) {
        const mvfgpu_predicate& in = clauses[i];
        WhereClause& cl = p.clause[i];
        if (!in.column) return set_fail(MVF_ERR_INVALID_ARGUMENT, "clause " + std::to_string(i) + ": column is NULL");
        if (in.column->owner != c)
            return set_fail(MVF_ERR_INVALID_ARGUMENT, "clause " + std::to_string(i) + ": the column was created for another corpus handle");
        cl.values = in.column->values;
        cl.is_u64 = in.column->dtype == MVF_DTYPE_UINT64 ? 1 : 0;
        if (!cl.is_set) {
            Range r;
            (void)predicate_range(in.column->dtype, in.op, in.a, in.b, &r);
            cl.lo = r.lo, cl.hi = r.hi, cl.negate = (uint8_t)r.negate;
        }
    }
    if (base) {
        const FilterOrigin o = filter_origin(base);
        if (o.owner != c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the filter was created for another corpus handle");
        if (o.tomb_gen != corpus_view(c).tomb_gen)
            return set_fail(MVF_ERR_INVALID_ARGUMENT,
                            "stale filter: mvfgpu_corpus_set_tombstones changed the handle's tombstones after the filter was created");
        p.base_deny = o.deny;
    }
    return MVF_OK;
}

// the call's set values and the allow words, on `s`
struct WhereBuffers {
    AsyncBuf sets, allow;
    int prepare(WherePlan& plan, const CorpusView& v, hipStream_t s) {
        WhereParams& p = plan.p;
        p.n = v.n;
        if (p.n_sets) {
            MVF_HIP_TRY(sets.alloc((size_t)p.n_sets * 8, s));
            MVF_HIP_TRY(hipMemcpyAsync(sets.p, plan.sets.data(), (size_t)p.n_sets * 8, hipMemcpyHostToDevice, s));
            p.sets = static_cast<const uint64_t*>(sets.p);
        }
        MVF_HIP_TRY(allow.alloc(std::max<size_t>((size_t)((v.n + 31) / 32), 1) * 4, s));
        p.allow = static_cast<uint32_t*>(allow.p);
        return MVF_OK;
    }
};

}  // namespace

namespace mvf {
ColumnOrigin column_origin(const mvfgpu_column* col) { return ColumnOrigin{col->owner, col->dtype, col->values}; }
}  // namespace mvf

extern "C" {

int mvfgpu_column_create(const mvfgpu_corpus* c, const void* values_le, uint8_t data_type, uint64_t first_value, uint64_t n_values,
                         mvfgpu_column** out) {
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (!values_le || !out) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    *out = nullptr;
    const uint32_t es = column_elem_size(data_type);
    if (!es) return set_fail(MVF_ERR_BUILD, "Unsupported metadata column data type");
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));  // the handle's own stream belongs to the host-buffer calls
    mvfgpu_column* col = nullptr;
    const int rc = [&]() -> int {
        const CorpusView v = corpus_view(c);
        if (first_value + v.n > n_values || first_value + v.n < first_value)
            return set_fail(MVF_ERR_INVALID_ARGUMENT, "column covers fewer rows than the shard holds");
        hipStream_t s = static_cast<hipStream_t>(v.stream);
        col = new_column(c, v, data_type);
        return corpus_device_call(c, s, [&]() -> int {
            if (const int arc = alloc_column(col)) return arc;
            const unsigned char* src = static_cast<const unsigned char*>(values_le) + (size_t)first_value * es;  // any alignment
            if (col->device_bytes) MVF_HIP_TRY(hipMemcpyAsync(col->values, src, col->device_bytes, hipMemcpyHostToDevice, s));
            MVF_HIP_TRY(hipStreamSynchronize(s));  // the caller's buffer is its own again
            return MVF_OK;
        });
    }();
    if (rc != MVF_OK) {
        if (col) free_column(col);
        return rc;
    }
    *out = col;
    return MVF_OK;
}

int mvfgpu_column_create_device(const mvfgpu_corpus* c, const void* d_values, uint8_t data_type, void* hip_stream, mvfgpu_column** out) {
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (!d_values || !out) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    *out = nullptr;
    const uint32_t es = column_elem_size(data_type);
    if (!es) return set_fail(MVF_ERR_BUILD, "Unsupported metadata column data type");
    if (reinterpret_cast<uintptr_t>(d_values) % es)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "d_values is not aligned to the column's element size");
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    mvfgpu_column* col = new_column(c, corpus_view(c), data_type);
    const int rc = corpus_device_call(c, s, [&]() -> int {
        if (const int arc = alloc_column(col)) return arc;
        if (col->device_bytes) MVF_HIP_TRY(hipMemcpyAsync(col->values, d_values, col->device_bytes, hipMemcpyDeviceToDevice, s));
        return MVF_OK;
    });
    if (rc != MVF_OK) {
        free_column(col);
        return rc;
    }
    *out = col;
    return MVF_OK;
}

void mvfgpu_column_destroy(mvfgpu_column* col) {
    if (!col) return;
    DevScope guard(col->device);
    (void)corpus_wait_newest(col->owner);  // a where-call or the copy enqueued on the handle may still touch the values
    free_column(col);
}

int mvfgpu_column_get_info(const mvfgpu_column* col, mvfgpu_column_info* out) {
    if (!col) return set_fail(MVF_ERR_INVALID_ARGUMENT, "column is NULL");
    if (!out) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    mvfgpu_column_info inf{};
    if (out->struct_size < 8u) return copy_out_struct(out, inf);  // refused before the column is read
    inf.data_type = col->dtype;
    inf.rows = col->rows;
    inf.device_bytes = col->device_bytes;
    return copy_out_struct(out, inf);
}

int mvfgpu_filter_create_where(const mvfgpu_corpus* c, const mvfgpu_predicate* clauses, uint32_t n_clauses, uint32_t combine,
                               const mvfgpu_filter* base, mvfgpu_filter** out) {
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (!out) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    *out = nullptr;
    WherePlan plan;
    if (const int rc = plan_where(c, clauses, n_clauses, combine, base, &plan)) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));  // the handle's own stream belongs to the host-buffer calls
    hipStream_t s = static_cast<hipStream_t>(corpus_view(c).stream);
    WhereBuffers buf;
    return corpus_device_call(c, s, [&]() -> int {
        const CorpusView v = corpus_view(c);
        if (const int rc = buf.prepare(plan, v, s)) return rc;
        MVF_HIP_TRY(where_launch(plan.p, v.num_cus, s));
        return filter_from_allow_words(c, v, plan.p.allow, s, out);  // waits for the admitted count: `plan.sets` is uploaded by then
    });
}

int mvfgpu_selftest_predicate_range(uint8_t data_type, uint32_t op, uint64_t a, uint64_t b, uint64_t* out_lo, uint64_t* out_hi,
                                    uint32_t* out_negate) {
    if (!out_lo || !out_hi || !out_negate) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (!column_elem_size(data_type)) return set_fail(MVF_ERR_BUILD, "Unsupported metadata column data type");
    Range r;
    if (!predicate_range(data_type, op, a, b, &r))
        return set_fail(MVF_ERR_INVALID_ARGUMENT, op == MVFGPU_OP_IN || op == MVFGPU_OP_NOT_IN ? "IN / NOT_IN are set tests, not ranges"
                                                                                                : "unknown predicate op " + std::to_string(op));
    *out_lo = r.lo, *out_hi = r.hi, *out_negate = r.negate;
    return MVF_OK;
}

int mvfgpu_selftest_where_kernel_ms(const mvfgpu_corpus* c, const mvfgpu_predicate* clauses, uint32_t n_clauses, uint32_t combine,
                                    const mvfgpu_filter* base, uint32_t repeats, float* out_ms) {
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (repeats < 1 || repeats > 64) return set_fail(MVF_ERR_INVALID_ARGUMENT, "repeats must be in 1..64");
    WherePlan plan;
    if (const int rc = plan_where(c, clauses, n_clauses, combine, base, &plan)) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    hipStream_t s = static_cast<hipStream_t>(corpus_view(c).stream);
    WhereBuffers buf;
    std::vector<hipEvent_t> ev(repeats + 1, nullptr);
    const int rc = corpus_device_call(c, s, [&]() -> int {
        const CorpusView v = corpus_view(c);
        if (const int prc = buf.prepare(plan, v, s)) return prc;
        for (auto& e : ev) MVF_HIP_TRY(hipEventCreate(&e));
        MVF_HIP_TRY(hipEventRecord(ev[0], s));
        for (uint32_t i = 0; i < repeats; i++) {
            MVF_HIP_TRY(where_launch(plan.p, v.num_cus, s));
            MVF_HIP_TRY(hipEventRecord(ev[i + 1], s));
        }
        MVF_HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t i = 0; i < repeats; i++) MVF_HIP_TRY(hipEventElapsedTime(&out_ms[i], ev[i], ev[i + 1]));
        return MVF_OK;
    });
    for (auto e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

}  // extern "C"
