// stage_marks.h — the events of the multi-vector searches' stage timers (maxsim.hip, hamming_maxsim.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "internal.h"

namespace mvf {

// the stage timer's events: one behind every stage of every chunk and window, with the stage it closes
struct StageMarks {
    std::vector<std::pair<int, hipEvent_t>> ev;
    hipError_t mark(int stage, hipStream_t s) {
        hipEvent_t e = nullptr;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.emplace_back(stage, e);
        return hipEventRecord(e, s);
    }
    ~StageMarks() {
        for (auto& m : ev) (void)hipEventDestroy(m.second);
    }
};

// the stage timer's sums: every stage's time from the event in front of it
inline int stage_sums(const StageMarks& marks, float* out_ms, int stages = 4) {
    for (int i = 0; i < stages; i++) out_ms[i] = 0.0f;
    for (size_t i = 1; i < marks.ev.size(); i++) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, marks.ev[i - 1].second, marks.ev[i].second) != hipSuccess) return set_fail(MVF_ERR_DEVICE, "hipEventElapsedTime failed");
        if (marks.ev[i].first >= 0 && marks.ev[i].first < stages) out_ms[marks.ev[i].first] += ms;
    }
    return MVF_OK;
}

}  // namespace mvf
