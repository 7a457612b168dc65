// C ABI of the EKF-SLAM HIP library (see include/ekf_slam_hip.h), the filter handle (ekf_filter.h): the log replay
// (BaseFilter.process_detections over a whole log), ekf_observe_log* -- recording included (ekf_observe_log_recorded).  Host
// side only; the kernels are in ekf_log.hip, the frames go through the scheduler of ekf_frames.hip.
#include <cstring>

#include "ekf_filter.h"
#include "ekf_smooth_host.h"

namespace {

// log_ws: [z of every detection, rd doubles each | landmark indices [D] | first-sighting slots [<= D]]
struct LogLayout {
    size_t idx, slots, total;
};

LogLayout log_layout(int rd, int64_t D) {
    Carve w;
    w.take((size_t)D * rd * 8);
    const size_t idx = w.take((size_t)D * 4), slots = w.take((size_t)D * 4);
    return {idx, slots, std::max<size_t>(256, w.end)};
}

// One call of the log replay: the arguments of ekf_observe_log_recorded (record: false from every other entry point), then
// what each step of the call leaves for the next.
struct LogCall {
    const int32_t* lm_index;
    const int64_t* offsets;
    int32_t frames;
    const double *poses_dev, *rows_dev, *scale, *motion;
    void* log_ws;
    size_t log_ws_bytes;
    double *trajectory_dev, *mahal_dev;
    bool record;
    void* history_dev;
    size_t history_bytes;
    // log_validate: gated, frame by frame in serial order; the detections, where they go, the first sightings
    bool gated = false, by_frame = false;
    int64_t D = 0;
    LogLayout LL{};
    LogCheck lc;
    // log_stage: the pinned staging of this call, the frames for the scheduler, and how they may run
    std::vector<int32_t> lead, rest;
    size_t up_bytes = 0;
    int turn = 0;
    char* pin = nullptr;
    int32_t *pin_lead = nullptr, *pin_rest = nullptr;
    uint8_t* pin_exempt = nullptr;
    std::vector<RunFrame> fr;
    RunPlan plan;
    int mode = EKF_SEQ_SERIAL;
};

// ---- validation on the host: nothing is enqueued before the whole log has passed.  Then what the call counts starts from
// zero, and a recorded call begins its history.
int log_validate(ekf_filter* f, LogCall& c) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (c.record && (rc = smoothing_supported(f))) return rc;
    if (c.rows_dev && !f->lay.has_rows) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_ROW_NOISE");
    if (c.mahal_dev && !f->lay.has_gate) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_GATE");
    // a gate that is set, or distances asked for: frame by frame in serial order, each frame on its survivors
    c.gated = f->gate_on() || c.mahal_dev;
    // frame by frame in serial order: a gated call, and a call with motions (a motion between two frames of a pipelined run
    // would change rows of the P_{t+1} the next front kernel completes from P_t and W_t)
    // ... and a call on a frozen map
    c.by_frame = c.gated || c.motion || f->frozen || c.record;
    const int32_t frames = c.frames;
    if (frames < 0) return fail(EKF_ERR_INVALID, "negative frame count");
    if ((rc = check_scales(f, c.scale, frames))) return rc;
    if ((rc = check_motions(f, c.motion, frames))) return rc;
    if (frames > 0 && !c.offsets) return fail(EKF_ERR_INVALID, "offsets is NULL");
    if (frames > 0 && (rc = check_offsets(c.offsets, frames, "offsets"))) return rc;
    c.D = frames > 0 ? c.offsets[frames] : 0;
    c.LL = log_layout(f->lay.rd, c.D);
    if (c.D > 0 && (!c.lm_index || !c.poses_dev)) return fail(EKF_ERR_INVALID, "NULL detections");
    if (c.D > 0 && (rc = check_device_buffers({c.log_ws}, c.log_ws_bytes, c.LL.total, "ekf_log_workspace_bytes"))) return rc;
    if ((rc = check_log(c.lm_index, c.offsets, frames, f->n_lm, f->cfg, "the log", &c.lc))) return rc;
    if (f->frozen && !c.lc.slots.empty())
        return fail(EKF_ERR_STATE, "the map is frozen: a log with first sightings would add landmarks (ekf_set_map_frozen)");
    if (c.record) {
        size_t need = 0;
        history_bound(f->lay.lmd, f->n_lm, c.lc, frames, &need);
        if ((rc = check_device_buffers({c.history_dev}, c.history_bytes, need, "ekf_history_bytes"))) return rc;
        f->hist = ekf_filter::History{};
        f->hist.buf = c.history_dev;
        f->hist.bytes = c.history_bytes;
        f->hist.frames = frames;
        f->hist.frame_rec.assign((size_t)frames, -1);
        f->hist.valid = true;
    }
    for (int i = 0; i < 4; ++i) f->log_stats[i] = 0;
    f->reset_gate_stats();
    return EKF_OK;
}

// ---- host staging: [indices | slots | (row, source) pairs of empty frames: those before the first stepped frame of the
// call (source: the state now), the others (source: the row of the last stepped frame before them)]; then the frames as the
// scheduler takes them, their scales, and whether their runs may pipeline
int log_stage(ekf_filter* f, LogCall& c) {
    const int32_t frames = c.frames;
    const int64_t* offsets = c.offsets;
    const int rd = f->lay.rd;
    {
        int last = -1;
        for (int t = 0; t < frames; ++t) {
            if (offsets[t + 1] > offsets[t]) last = t;
            else if (c.trajectory_dev && !c.by_frame) {      // (gated: which frames are stepped is known frame by frame; motions:
                                                             // an empty frame's row is the moved pose)
                std::vector<int32_t>& v = last < 0 ? c.lead : c.rest;
                v.push_back(t);
                v.push_back(last);
            }
        }
    }
    c.up_bytes = c.LL.slots - c.LL.idx + c.lc.slots.size() * 4;
    Carve p;
    p.take(c.up_bytes);
    const size_t lead_at = p.take(c.lead.size() * 4), rest_at = p.take(c.rest.size() * 4);
    p.take(256);
    const size_t exempt_at = c.gated ? p.take((size_t)c.D) : 0;      // rule 4: the first occurrence of every first sighting
    const int turn = c.turn = f->log_pin_turn;
    if (!f->log_pin_done[turn]) HIP_TRY(hipEventCreateWithFlags(&f->log_pin_done[turn], hipEventDisableTiming));
    HIP_TRY(hipEventSynchronize(f->log_pin_done[turn]));      // (the staging of the call before the previous one is consumed)
    int rc = f->log_pin[turn].reserve(p.end);
    if (rc) return rc;
    c.pin = f->log_pin[turn].get();
    c.pin_lead = f->log_pin[turn].at<int32_t>(lead_at);
    c.pin_rest = f->log_pin[turn].at<int32_t>(rest_at);
    if (c.D > 0) {
        std::memcpy(c.pin, c.lm_index, (size_t)c.D * 4);
        if (!c.lc.slots.empty()) std::memcpy(c.pin + (c.LL.slots - c.LL.idx), c.lc.slots.data(), c.lc.slots.size() * 4);
    }
    if (!c.lead.empty()) std::memcpy(c.pin_lead, c.lead.data(), c.lead.size() * 4);
    if (!c.rest.empty()) std::memcpy(c.pin_rest, c.rest.data(), c.rest.size() * 4);
    c.pin_exempt = f->log_pin[turn].at<uint8_t>(exempt_at);
    if (c.gated && c.D > 0) {
        std::memset(c.pin_exempt, 0, (size_t)c.D);
        for (int32_t d : c.lc.slots) c.pin_exempt[d] = 1;
    }

    char* ws = static_cast<char*>(c.log_ws);
    const double* z_all = reinterpret_cast<const double*>(ws);
    const int32_t* idx_all = reinterpret_cast<const int32_t*>(ws + c.LL.idx);
    const int32_t* slots_all = reinterpret_cast<const int32_t*>(ws + c.LL.slots);
    c.fr.resize((size_t)frames);
    for (int t = 0; t < frames; ++t) {
        const int64_t d0 = offsets[t];
        c.fr[t] = RunFrame{idx_all + d0, z_all + (size_t)d0 * rd, (int)(offsets[t + 1] - d0),
                           c.trajectory_dev ? c.trajectory_dev + (size_t)t * 7 : nullptr,
                           c.rows_dev ? c.rows_dev + (size_t)d0 * rd : nullptr, 1.0,
                           (int)(c.lc.new_at[t + 1] - c.lc.new_at[t]), slots_all + c.lc.new_at[t], c.poses_dev};
        // Without a gate the host knows which frames are stepped: rules 3 and 4 run over the whole log here, an empty frame's
        // scale goes into the pending scale and the next stepped frame takes it.  (Gated: frame by frame, in serial_frame.)
        if (!c.gated) {
            c.fr[t].s_eff = frame_scale(f, c.scale ? c.scale + t : nullptr);
            frame_scale_done(f, c.scale ? c.scale + t : nullptr, c.fr[t].s_eff, c.fr[t].m > 0);
        }
    }
    if (c.by_frame) {
        f->seq_mode = EKF_SEQ_SERIAL;
        return EKF_OK;
    }
    return plan_frames(f, c.fr, &c.plan, &c.mode);
}

// ---- device work, all on the handle's stream (the pipelined runs use the internal one as ekf_observe_sequence_device).
// record: the by-frame serial loop, and behind every frame that changed the filter -- stepped, or moved by a non-zero motion
// -- one pack launch that copies state and the lower triangle of P into the next record of the history (recording only
// reads: every other launch is the one the plain call enqueues, in its order).
int log_enqueue(ekf_filter* f, LogCall& c) {
    const int32_t frames = c.frames;
    char* ws = static_cast<char*>(c.log_ws);
    if (c.D > 0) {
        HIP_TRY(hipMemcpyAsync(ws + c.LL.idx, c.pin, c.up_bytes, hipMemcpyHostToDevice, f->stream));
        ekf_launch_log_prepare(c.poses_dev, c.D, f->lay.rd, reinterpret_cast<double*>(ws), f->stream);
    }
    if (!c.lead.empty())
        ekf_launch_log_fill_rows(c.trajectory_dev, c.pin_lead, (int32_t)(c.lead.size() / 2), f->state, f->stream);
    // recording: the camera state at the call (the rows of the frames before the first record), then record after record
    size_t hist_at = 256;
    if (c.record) HIP_TRY(hipMemcpyAsync(c.history_dev, f->state, 7 * 8, hipMemcpyDeviceToDevice, f->stream));
    auto record_frame = [&](int t, bool moved, bool stepped, double s_eff) {
        if (c.record && (moved || stepped)) {
            ekf_filter::HistoryRec h{};
            h.frame = t;
            h.dims = f->dims();
            h.off = hist_at;
            h.s_eff = stepped ? s_eff : 0.0;
            for (int i = 0; i < 6; ++i) h.u[i] = (moved && c.motion) ? c.motion[(size_t)t * 6 + i] : 0.0;
            h.stepped = stepped;
            h.moved = moved;
            ekf_launch_history_pack(static_cast<const double*>(f->cov), f->ld, f->state, h.dims,
                                    reinterpret_cast<double*>(static_cast<char*>(c.history_dev) + h.off), f->stream);
            hist_at += history_record_bytes(h.dims);
            f->hist.recs.push_back(h);
        }
        if (c.record) f->hist.frame_rec[t] = (int32_t)f->hist.recs.size() - 1;
    };
    int rc = EKF_OK;
    if (c.by_frame) {
        // serial_frame: the motion, first sightings (placed from the moved camera), the gate on the prior they leave, the frame
        // on its survivors; a frame without detections or without a survivor is not stepped, and its row repeats the camera
        // state.  (Without a gate the scales were folded over the whole log in log_stage.)
        for (int t = 0; t < frames && rc == EKF_OK; ++t) {
            const int64_t d0 = c.offsets[t];
            SerialFrame x;
            x.motion = c.motion ? c.motion + (size_t)t * 6 : nullptr;
            x.scale = c.scale ? c.scale + t : nullptr;
            x.folded = !c.gated;
            x.gated = c.gated;
            x.exempt = c.gated ? c.pin_exempt + d0 : nullptr;
            x.mahal = c.mahal_dev ? c.mahal_dev + d0 : nullptr;
            if ((rc = serial_frame(f, c.fr[t], &x))) break;
            f->log_stats[3] += c.fr[t].nnew;
            if (x.survivors > 0) f->log_stats[0] += 1;
            record_frame(t, x.moved, x.survivors > 0, x.s_eff);
        }
    } else {
        rc = run_planned_frames(f, c.fr, c.plan, c.mode, f->log_stats);
    }
    if (rc == EKF_OK && !c.rest.empty())
        ekf_launch_log_fill_rows(c.trajectory_dev, c.pin_rest, (int32_t)(c.rest.size() / 2), f->state, f->stream);
    // A state getter after the call must wait for the whole call (the last frame's state may come from a pipelined run, whose
    // front kernels record no event): no shortcut through the event of an earlier serial frame of the call.
    f->shortcut.log();
    // (the staging may be reused once the stream is here -- also after an error: its copy may have been enqueued)
    f->log_pin_turn = c.turn ^ 1;
    if (rc) f->hist.valid = f->hist.valid && !c.record;      // (a recorded call that failed leaves no history)
    HIP_TRY(hipEventRecord(f->log_pin_done[c.turn], f->stream));
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return EKF_OK;
}

// The log replay: validate, stage, enqueue.
int observe_log_run(ekf_filter* f, LogCall c) {
    int rc = log_validate(f, c);
    if (rc || c.frames == 0) return rc;
    if ((rc = log_stage(f, c))) return rc;
    return log_enqueue(f, c);
}

}  // namespace

extern "C" {

int ekf_log_workspace_bytes(const ekf_filter* f, int64_t detections, size_t* bytes) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!bytes || detections < 0) return fail(EKF_ERR_INVALID, "bad log size request");
    *bytes = log_layout(f->lay.rd, detections).total;
    return EKF_OK;
}

int ekf_last_log_stats(const ekf_filter* f, int64_t out[4]) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    for (int i = 0; i < 4; ++i) out[i] = f->log_stats[i];
    return EKF_OK;
}

int ekf_observe_log(ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames, const double* poses_dev,
                    void* log_ws, size_t log_ws_bytes, double* trajectory_dev) {
    return ekf_observe_log_rows(f, lm_index, offsets, frames, poses_dev, nullptr, log_ws, log_ws_bytes, trajectory_dev, nullptr);
}

int ekf_observe_log_gated(ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames,
                          const double* poses_dev, void* log_ws, size_t log_ws_bytes, double* trajectory_dev,
                          double* mahal_dev) {
    return ekf_observe_log_rows(f, lm_index, offsets, frames, poses_dev, nullptr, log_ws, log_ws_bytes, trajectory_dev, mahal_dev);
}

int ekf_observe_log_rows(ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames,
                         const double* poses_dev, const double* rows_dev, void* log_ws, size_t log_ws_bytes,
                         double* trajectory_dev, double* mahal_dev) {
    return ekf_observe_log_scaled(f, lm_index, offsets, frames, poses_dev, rows_dev, nullptr, log_ws, log_ws_bytes,
                                  trajectory_dev, mahal_dev);
}

int ekf_observe_log_scaled(ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames,
                           const double* poses_dev, const double* rows_dev, const double* scale, void* log_ws,
                           size_t log_ws_bytes, double* trajectory_dev, double* mahal_dev) {
    return ekf_observe_log_moved(f, lm_index, offsets, frames, poses_dev, rows_dev, scale, nullptr, log_ws, log_ws_bytes,
                                 trajectory_dev, mahal_dev);
}

int ekf_observe_log_moved(ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames,
                          const double* poses_dev, const double* rows_dev, const double* scale, const double* motion,
                          void* log_ws, size_t log_ws_bytes, double* trajectory_dev, double* mahal_dev) {
    return observe_log_run(f, LogCall{lm_index, offsets, frames, poses_dev, rows_dev, scale, motion, log_ws, log_ws_bytes,
                                      trajectory_dev, mahal_dev, false, nullptr, 0});
}

int ekf_observe_log_recorded(ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames,
                             const double* poses_dev, const double* rows_dev, const double* scale, const double* motion,
                             void* log_ws, size_t log_ws_bytes, double* trajectory_dev, double* mahal_dev,
                             void* history_dev, size_t history_bytes) {
    return observe_log_run(f, LogCall{lm_index, offsets, frames, poses_dev, rows_dev, scale, motion, log_ws, log_ws_bytes,
                                      trajectory_dev, mahal_dev, true, history_dev, history_bytes});
}

}  // extern "C"
