// Batch smoothing, host side (include/ekf_slam_hip.h, "Batch smoothing"): where the records of a recorded batch call lie --
// from the logs alone -- and the tables of the backward pass -- from the per-frame words the device wrote.  No device call in
// here: ekf_batch_api.hip uses both, and ekf_batch_history_table exposes the second to callers without a handle.
#pragma once
#include "ekf_smooth_host.h"

namespace {

// The history buffer of a recorded batch call:
//   [member 0: 256 B header | slots] [member 1: ...] ... | head [B] i64 | slot [Ftot] i64 | flag [Ftot] i32 |
//   s_eff [Ftot] f64 | motion [Ftot][6] f64 (a call with motions)
// every piece 256-byte aligned.  head / slot count doubles from the start of the buffer (slot: -1 for a frame without one).
struct BatchHistoryPlan {
    std::vector<int64_t> head, slot;      // [B], [Ftot]
    std::vector<int32_t> dims;            // [Ftot]: the dims the frame ends with
    size_t head_at = 0, slot_at = 0, flag_at = 0, seff_at = 0, motion_at = 0, total = 0;
};

// Member m's region, appended to the plan: a slot for every frame of its log that can change it -- one with detections, and
// every frame when the call carries motions -- at the dims the frame ends with (n_lm landmarks before the log, lc from
// check_log over its `frames` frames whose detection offsets are `offsets`).
void batch_history_add_member(BatchHistoryPlan& p, const int64_t* offsets, int64_t frames, int lmd, int n_lm, const LogCheck& lc,
                              bool with_motion) {
    p.head.push_back((int64_t)(p.total / 8));
    p.total += 256;
    for (int64_t t = 0; t < frames; ++t) {
        const int64_t dims = EKF_CAM + (int64_t)lmd * (n_lm + lc.new_at[t + 1]);
        const bool has = with_motion || offsets[t + 1] > offsets[t];
        p.dims.push_back((int32_t)dims);
        p.slot.push_back(has ? (int64_t)(p.total / 8) : -1);
        if (has) p.total += history_record_bytes(dims);      // (one record, as the filter handle's: ekf_smooth_host.h)
    }
}

// the per-call words behind the last member's region
void batch_history_finish(BatchHistoryPlan& p, bool with_motion) {
    const size_t B = p.head.size(), F = p.slot.size();
    Carve w;
    w.end = p.total;
    p.head_at = w.take(B * 8);
    p.slot_at = w.take(F * 8);
    p.flag_at = w.take(F * 4);
    p.seff_at = w.take(F * 8);
    p.motion_at = w.take(with_motion ? F * 48 : 0);
    p.total = w.end;
}

// The tables of the batched backward pass.  rec_frame / rec_stepped: per table entry the frame (a row of the call) and whether
// it was stepped; nmax: the dims of the largest record.
struct BatchSmoothTables {
    std::vector<EkfSmoothRec> tables;
    std::vector<EkfBatchSmoothMember> members;
    std::vector<int32_t> rec_frame, rec_stepped;
    int32_t nmax = 0;
};

// flag [Ftot]: 0 no record, 1 stepped, 2 moved only, < 0 the member has failed (from that frame on: NaN rows, no record);
// s_eff [Ftot]; motion [Ftot][6] or null; noise [B][6] in ekf_config order (Q_eff = fl(s_eff q) per entry, the member's own q).
void batch_smooth_tables(int32_t B, const int64_t* member_frames, const int64_t* head, const int64_t* slot, const int32_t* dims,
                         const int32_t* flag, const double* s_eff, const double* motion, const double* noise,
                         BatchSmoothTables* out) {
    *out = BatchSmoothTables{};
    for (int32_t m = 0; m < B; ++m) {
        const int64_t f0 = member_frames[m], f1 = member_frames[m + 1];
        EkfBatchSmoothMember mem{};
        mem.table = (int64_t)out->tables.size();
        mem.head = head[m];
        mem.frame0 = (int32_t)f0;
        mem.frame1 = (int32_t)f1;
        mem.nan0 = (int32_t)f1;
        for (int64_t t = f0; t < f1; ++t) {
            if (flag[t] < 0) {
                mem.nan0 = (int32_t)t;
                break;
            }
            if (flag[t] == 0) continue;
            EkfSmoothRec e{};
            e.off = slot[t];
            e.dims = dims[t];
            for (int i = 0; i < 6; ++i) {
                e.u[i] = motion ? motion[6 * t + i] : 0.0;
                e.moved = e.moved || e.u[i] != 0.0;
            }
            const double s = flag[t] == 1 ? s_eff[t] : 0.0;
            for (int i = 0; i < 3; ++i) e.q[i] = s * noise[6 * (size_t)m + 3 + i];
            e.frame0 = (int32_t)t;
            if (mem.records > 0) out->tables.back().frame1 = (int32_t)t;
            else mem.lead1 = (int32_t)t;
            out->tables.push_back(e);
            out->rec_frame.push_back((int32_t)t);
            out->rec_stepped.push_back(flag[t] == 1);
            out->nmax = std::max(out->nmax, e.dims);
            ++mem.records;
        }
        if (mem.records > 0) out->tables.back().frame1 = mem.nan0;
        else mem.lead1 = mem.nan0;
        out->members.push_back(mem);
    }
}

}  // namespace
