// update.hip — mvfgpu_corpus_write_rows / mvfgpu_corpus_write_rows_device: new bytes into row positions of a resident corpus
// (include/mvf_gpu_update.h; DESIGN.md §3 "Row writes", §5 "W0 / W1").
//
// Both calls check everything on the host first (nothing below touches the device on a refusal), turn the positions into a list
// of distinct local rows, and then enqueue, under mvfgpu_search_device's stream discipline (corpus_device_call):
//   1. W0 (scan_update.hip): the rows into the resident array, pad bytes zero;
//   2. W1, one launch per derived array that is RESIDENT at that moment (corpus_write_targets): the norms, the scaled-f16
//      shadow, the int8 shadow (the rows a partial shadow covers), the 6-bit shadow -- the builders' own per-row bodies, the
//      corpus-wide maxima raised with their atomicMax;
//   3. the cached read-backs of a refreshed shadow's maxima are forgotten (corpus_rows_written).
// At most five launches whatever the count.  What has not been built stays unbuilt: its first use builds it from the new bytes.
// The host call packs list and rows into one blob at the row pitch (only the rows' own bytes are copied: the gaps of the
// caller's stride never leave the host), sends it with one copy -- through the handle's pinned mirror where it is small -- and
// waits for the stream.  The device call sends the list through the handle's pinned upload buffer (host_staging.h) and makes no
// host wait; W0 reads the caller's device rows at their stride.

#include "../../include/mvf_gpu_update.h"

#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_update.h"
#include "shadow_5p1.h"
#include "shadow_6b.h"

#include <algorithm>
#include <string>
#include <unordered_set>
#include <vector>

using namespace mvf;

namespace {

// Refusals 3 to 5 of the header, in its order; `pos` holds global positions (ids already mapped: `named` are the caller's own
// entries, for the messages).  out_local: the distinct local rows.
int check_write(const CorpusView& v, const uint64_t* named, const uint64_t* pos, uint64_t count, uint64_t stride_bytes, bool by_id,
                const mvfgpu_write_report* report, std::vector<uint32_t>* out_local) {
    const uint64_t row_bytes = (uint64_t)v.dim * elem_size(v.dtype);
    if (stride_bytes < row_bytes)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "stride_bytes " + std::to_string(stride_bytes) + " is smaller than a row (" +
                                                      std::to_string(row_bytes) + " bytes)");
    for (uint64_t i = 0; i < count; i++) {
        if (by_id && pos[i] == ~0ull)
            return set_fail(MVF_ERR_INDEX_OUT_OF_BOUNDS, "Index out of bounds: vector id " + std::to_string(named[i]) + " is not in this shard");
        if (pos[i] < v.index_base || pos[i] - v.index_base >= v.n)
            return set_fail(MVF_ERR_INDEX_OUT_OF_BOUNDS,
                            "Index out of bounds: " + std::to_string(pos[i]) + " >= " + std::to_string(v.index_base + v.n));
    }
    out_local->resize(count);
    std::unordered_set<uint32_t> seen;
    seen.reserve((size_t)count * 2);
    for (uint64_t i = 0; i < count; i++) {
        const uint32_t r = (uint32_t)(pos[i] - v.index_base);
        if (!seen.insert(r).second)
            return set_fail(MVF_ERR_INVALID_ARGUMENT, "row position " + std::to_string(pos[i]) + " is named twice in one write (entry " +
                                                          std::to_string(i) + "): a parallel scatter has no \"last wins\"");
        (*out_local)[i] = r;
    }
    if (report && report->struct_size < 8u)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "struct_size not set (MVFGPU_INIT the out-struct before the call)");
    return MVF_OK;
}

// W0 and W1 on `s` for `count` listed rows; src: device rows at `stride`.  Under corpus_device_call.
int enqueue_write(const mvfgpu_corpus* c, const unsigned char* d_src, uint64_t stride, const uint32_t* d_list, const uint32_t* h_list,
                  uint32_t count, hipStream_t s, mvfgpu_write_report* rep) {
    const WriteTargets t = corpus_write_targets(c);
    const uint32_t row_bytes = t.dim * elem_size(t.dtype);
    uint64_t per_row = t.pitch, bytes = 0;
    uint32_t launches = 0, refreshed = 0;
    MVF_HIP_TRY(launch_write_scatter(d_src, stride, row_bytes, d_list, count, t.rows, t.pitch, s));
    launches++;
    if (t.norms) {
        MVF_HIP_TRY(launch_refresh_norms(t.rows, t.dtype, t.pitch, t.dim, d_list, count, t.norms, t.xx2, t.xxmax, s));
        launches++, refreshed |= MVFGPU_WRITE_NORMS;
        per_row += t.dtype == MVF_DTYPE_INT8 ? 4 : 8;
    }
    if (t.shadow16) {
        MVF_HIP_TRY(launch_refresh_shadow_f16(t.rows, t.pitch, d_list, count, t.shadow16, t.pitch16, t.xscale, s));
        launches++, refreshed |= MVFGPU_WRITE_SHADOW_F16;
        per_row += t.pitch16 + 4;
    }
    if (t.shadow8) {
        MVF_HIP_TRY(launch_refresh_shadow_i8(t.rows, t.dtype, t.pitch, t.dim, d_list, count, (uint32_t)t.shadow8_rows, t.shadow8, t.pitch8,
                                             t.xscale8, t.qs_stats, s));
        launches++, refreshed |= MVFGPU_WRITE_SHADOW_I8;
        uint64_t covered = 0;  // a partial shadow holds the rows below shadow8_rows only
        for (uint32_t i = 0; i < count; i++) covered += h_list[i] < t.shadow8_rows ? 1 : 0;
        bytes += covered * (t.pitch8 + 4);
    }
    if (t.shadow6) {
        MVF_HIP_TRY(launch_refresh_shadow_6b(t.rows, t.pitch, t.dim, d_list, count, t.shadow6, t.xscale6, t.qs6_stats, t.shadow6_p51, s));
        launches++, refreshed |= MVFGPU_WRITE_SHADOW_6B;
        per_row += (t.shadow6_p51 ? s51_units(t.dim) * 96u : s6_units(t.dim) * 48u) + 4;
    }
    corpus_rows_written(c, refreshed);
    rep->launches = launches;
    rep->rows_written = count;
    rep->bytes_written = bytes + (uint64_t)count * per_row;
    rep->refreshed = refreshed;
    return MVF_OK;
}

int check_pointers(const mvfgpu_corpus* c, const void* indices, const void* rows, uint64_t count) {
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (count && (!indices || !rows)) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    return MVF_OK;
}

int report_out(mvfgpu_write_report* out, const mvfgpu_write_report& rep) { return out ? copy_out_struct(out, rep) : MVF_OK; }

}  // namespace

extern "C" {

int mvfgpu_corpus_write_rows(mvfgpu_corpus* c, const uint64_t* indices, uint64_t count, const void* rows, uint64_t stride_bytes,
                             mvfgpu_write_report* out_report) {
    if (const int rc = check_pointers(c, indices, rows, count)) return rc;
    mvfgpu_write_report rep{};
    if (count == 0) return out_report && out_report->struct_size >= 8u ? report_out(out_report, rep) : MVF_OK;
    const CorpusView v = corpus_view(c);
    std::vector<uint64_t> mapped;  // with vector ids attached the entries are ids, as a search reports them
    const uint64_t* pos = indices;
    bool by_id = false;
    if ((uint64_t)v.dim * elem_size(v.dtype) <= stride_bytes) {  // (a refusal by the stride comes first: check_write)
        mapped.resize(count);
        by_id = corpus_ids_to_positions(c, indices, count, mapped.data());
        if (by_id) pos = mapped.data();
    }
    std::vector<uint32_t> local;
    if (const int rc = check_write(v, indices, pos, count, stride_bytes, by_id, out_report, &local)) return rc;

    DevScope guard(v.device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    // the blob: the list, padded to 16 bytes, then the rows at the pitch (W0's aligned path)
    const uint32_t row_bytes = v.dim * elem_size(v.dtype);
    const size_t list_bytes = ((size_t)count * 4 + 15) & ~(size_t)15, blob_bytes = list_bytes + (size_t)count * v.pitch;
    std::vector<unsigned char> pageable;
    unsigned char* blob = nullptr;
    if (blob_bytes <= kPinnedBytes) {
        void *pi = nullptr, *po = nullptr;
        if (const int rc = corpus_pinned_mirrors(c, blob_bytes, 0, &pi, &po)) return rc;
        blob = static_cast<unsigned char*>(pi);
    } else {
        pageable.resize(blob_bytes);
        blob = pageable.data();
    }
    std::memcpy(blob, local.data(), (size_t)count * 4);
    for (uint64_t i = 0; i < count; i++)
        std::memcpy(blob + list_bytes + (size_t)i * v.pitch, static_cast<const unsigned char*>(rows) + (size_t)i * stride_bytes, row_bytes);
    AsyncBuf dblob;
    MVF_HIP_TRY(dblob.alloc(blob_bytes, s));
    const int rc = corpus_device_call(c, s, [&]() -> int {
        MVF_HIP_TRY(hipMemcpyAsync(dblob.p, blob, blob_bytes, hipMemcpyHostToDevice, s));
        const unsigned char* d = static_cast<const unsigned char*>(dblob.p);
        return enqueue_write(c, d + list_bytes, v.pitch, reinterpret_cast<const uint32_t*>(d), local.data(), (uint32_t)count, s, &rep);
    });
    // work may sit on the stream whatever rc is, and it reads the blob: wait before anything is released
    const hipError_t e = hipStreamSynchronize(s);
    if (rc != MVF_OK) return rc;
    MVF_HIP_TRY(e);
    return report_out(out_report, rep);
}

int mvfgpu_corpus_write_rows_device(mvfgpu_corpus* c, const uint64_t* positions, uint64_t count, const void* d_rows,
                                    uint64_t stride_bytes, void* hip_stream, mvfgpu_write_report* out_report) {
    if (const int rc = check_pointers(c, positions, d_rows, count)) return rc;
    mvfgpu_write_report rep{};
    if (count == 0) return out_report && out_report->struct_size >= 8u ? report_out(out_report, rep) : MVF_OK;
    const CorpusView v = corpus_view(c);
    std::vector<uint32_t> local;
    if (const int rc = check_write(v, positions, positions, count, stride_bytes, false, out_report, &local)) return rc;

    DevScope guard(v.device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    AsyncBuf dlist;  // released in stream order, behind the launches that read it
    const int rc = corpus_device_call(c, s, [&]() -> int {
        MVF_HIP_TRY(dlist.alloc((size_t)count * 4, s));
        PinnedUpload& up = corpus_write_upload(c);
        void* pin = nullptr;
        if (const int rc1 = up.reserve((size_t)count * 4, &pin)) return rc1;
        std::memcpy(pin, local.data(), (size_t)count * 4);
        if (const int rc1 = up.send(dlist.p, (size_t)count * 4, s)) return rc1;
        return enqueue_write(c, static_cast<const unsigned char*>(d_rows), stride_bytes, static_cast<const uint32_t*>(dlist.p),
                             local.data(), (uint32_t)count, s, &rep);
    });
    if (rc != MVF_OK) return rc;
    return report_out(out_report, rep);
}

}  // extern "C"
