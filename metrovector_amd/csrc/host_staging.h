// host_staging.h — the host-buffer loop of the list searches (candidates.hip, partition.hip, grouped.hip; DESIGN.md §5
// "Host staging"): a call's queries, lists and results travel between the caller's buffers and the device work in windows
// of queries, so that the device copies stay bounded whatever nq, m and k are.
//
// A window holds W = max(1, min(nq, kHostWindowBytes / bytes per query of all streams)) queries.  Per window: the inputs are
// copied in, the feature's core runs and the outputs are copied out, all on the handle's own stream under corpus_device_call
// (mvfgpu_search_device's stream discipline), then ONE host wait.  A window of up to kPinnedBytes travels through the handle's
// pinned mirrors (inputs and outputs back to back, in the order given), a larger one copies from and to the caller's buffers.
// The caller holds corpus_host_mutex and has set the device.
#pragma once

#include "internal.h"

#include <algorithm>
#include <cstring>

namespace mvf {

constexpr size_t kHostWindowBytes = 256ull << 20;  // the device copies of a window's inputs and outputs
constexpr size_t kPinnedBytes = 1ull << 20;        // windows up to this size travel through the handle's pinned mirrors

// One array of a call, `bytes` per query in the caller's buffer `host`.  An input of 0 bytes is empty.  An output the caller
// did not ask for (host NULL) still has its place in the window and in the mirror; it has a device copy -- the core receives
// NULL otherwise -- only where `device` says that the core always writes it.
struct HostIn {
    const void* host;
    size_t bytes;
};
struct HostOut {
    void* host;
    size_t bytes;
    bool device = false;
};

// prepare(w0, wn, src): may replace src[i], the host pointer the window's input i is staged from (queries [w0, w0 + wn)).
// core(w0, wn, d_in, d_out): the device work of the window on the window's device pointers; enqueues on `s`, does not wait.
template <size_t NI, size_t NO, class Prepare, class Core>
int stage_host_windows(const mvfgpu_corpus* c, hipStream_t s, uint32_t nq, const HostIn (&in)[NI], const HostOut (&out)[NO],
                       Prepare prepare, Core core) {
    size_t per_query = 0;
    for (const HostIn& i : in) per_query += i.bytes;
    for (const HostOut& o : out) per_query += o.bytes;
    const uint32_t W = (uint32_t)std::max<size_t>(1, std::min<size_t>(nq, kHostWindowBytes / per_query));
    AsyncBuf bin[NI], bout[NO];
    void *d_in[NI], *d_out[NO];
    for (size_t i = 0; i < NI; i++) {
        MVF_HIP_TRY(bin[i].alloc((size_t)W * in[i].bytes, s));
        d_in[i] = bin[i].p;
    }
    for (size_t i = 0; i < NO; i++) {
        if (out[i].host || out[i].device) MVF_HIP_TRY(bout[i].alloc((size_t)W * out[i].bytes, s));
        d_out[i] = bout[i].p;
    }
    for (uint32_t w0 = 0; w0 < nq; w0 += W) {
        const uint32_t wn = std::min(W, nq - w0);
        const void* src[NI];
        unsigned char* dst[NO];
        size_t in_bytes = 0, out_bytes = 0;
        for (size_t i = 0; i < NI; i++) {
            src[i] = in[i].host ? static_cast<const unsigned char*>(in[i].host) + (size_t)w0 * in[i].bytes : nullptr;
            in_bytes += (size_t)wn * in[i].bytes;
        }
        for (size_t i = 0; i < NO; i++) {
            dst[i] = out[i].host ? static_cast<unsigned char*>(out[i].host) + (size_t)w0 * out[i].bytes : nullptr;
            out_bytes += (size_t)wn * out[i].bytes;
        }
        prepare(w0, wn, src);
        const bool pinned = in_bytes + out_bytes <= kPinnedBytes;
        unsigned char* pin_out = nullptr;
        if (pinned) {
            void *pi = nullptr, *po = nullptr;
            const int rc = corpus_pinned_mirrors(c, in_bytes, out_bytes, &pi, &po);
            if (rc != MVF_OK) return rc;
            unsigned char* at = static_cast<unsigned char*>(pi);
            pin_out = static_cast<unsigned char*>(po);
            for (size_t i = 0; i < NI; i++) {
                const size_t n = (size_t)wn * in[i].bytes;
                if (n) std::memcpy(at, src[i], n);
                src[i] = at;
                at += n;
            }
        }
        const int rc = corpus_device_call(c, s, [&]() -> int {
            for (size_t i = 0; i < NI; i++)
                if (in[i].bytes) MVF_HIP_TRY(hipMemcpyAsync(d_in[i], src[i], (size_t)wn * in[i].bytes, hipMemcpyHostToDevice, s));
            const int rc1 = core(w0, wn, d_in, d_out);
            if (rc1 != MVF_OK) return rc1;
            size_t at = 0;  // in the output mirror
            for (size_t i = 0; i < NO; i++) {
                const size_t n = (size_t)wn * out[i].bytes;
                void* to = pinned ? pin_out + at : dst[i];
                if (d_out[i] && to) MVF_HIP_TRY(hipMemcpyAsync(to, d_out[i], n, hipMemcpyDeviceToHost, s));
                at += n;
            }
            return MVF_OK;
        });
        if (rc != MVF_OK) return rc;
        MVF_HIP_TRY(hipStreamSynchronize(s));
        if (pinned) {
            const unsigned char* at = pin_out;
            for (size_t i = 0; i < NO; i++) {
                const size_t n = (size_t)wn * out[i].bytes;
                if (dst[i]) std::memcpy(dst[i], at, n);
                at += n;
            }
        }
    }
    return MVF_OK;
}

inline void stage_as_given(uint32_t, uint32_t, const void**) {}  // the `prepare` of a call whose inputs are staged as they are

// A small host array of a DEVICE call (the positions of a row write) on its way to the device without a wait for it: through a
// pinned buffer the handle keeps, so that the caller's array is free again when the call returns.  upload() waits only for the
// previous upload to have left the buffer.  The caller holds the handle's lock (corpus_device_call) and has set the device.
struct PinnedUpload {
    void* pin = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;
    bool busy = false;
    // room for `need` bytes, the previous upload out of it: fill it, then send()
    int reserve(size_t need, void** out) {
        if (busy) {
            MVF_HIP_TRY(hipEventSynchronize(copied));
            busy = false;
        }
        if (!copied) MVF_HIP_TRY(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        if (bytes < need) {
            if (pin) (void)hipHostFree(pin);
            pin = nullptr, bytes = 0;
            const size_t want = std::max<size_t>(need, 16u << 10);
            MVF_HIP_TRY(hipHostMalloc(&pin, want, hipHostMallocDefault));
            poison_fill_host(pin, want);
            bytes = want;
        }
        *out = pin;
        return MVF_OK;
    }
    int send(void* dst, size_t n, hipStream_t s) {
        MVF_HIP_TRY(hipMemcpyAsync(dst, pin, n, hipMemcpyHostToDevice, s));
        MVF_HIP_TRY(hipEventRecord(copied, s));
        busy = true;
        return MVF_OK;
    }
    void release() {
        if (pin) (void)hipHostFree(pin);
        if (copied) (void)hipEventDestroy(copied);
        pin = nullptr, bytes = 0, copied = nullptr, busy = false;
    }
};

}  // namespace mvf
