// Offline smoothing, host side: the sizes of a history, shared by the filter handle (ekf_log_api.hip records,
// ekf_smooth_api.hip reads) and the batch handle (ekf_batch_smooth_host.h).  Both lay their records out for the kernels of
// ekf_smooth.hip, so there is one formula.
#pragma once
#include "ekf_host.h"

namespace {

// one record: state [dims] and the packed lower triangle, f64, in a 256-byte aligned piece (ekf_history_record_bytes)
size_t history_record_bytes(int64_t dims) { return align256((size_t)(dims + dims * (dims + 1) / 2) * 8); }

// upper bound from the log alone: the header and one record per frame at the dims that frame ends with
void history_bound(int lmd, int n_lm, const LogCheck& lc, int64_t frames, size_t* bytes) {
    size_t total = 256;
    for (int64_t t = 0; t < frames; ++t) total += history_record_bytes(EKF_CAM + (int64_t)lmd * (n_lm + lc.new_at[t + 1]));
    *bytes = total;
}

}  // namespace
