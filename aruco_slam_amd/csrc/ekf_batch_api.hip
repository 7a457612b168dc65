// C ABI of the batch of independent filters (ekf_batch_*, see include/ekf_slam_hip.h; kernels: ekf_batch.hip (EKF) and
// ekf_batch_rot.hip (EKF_Rotations), with EKF_FLAG_BATCH_LARGE_MAPS or EKF_FLAG_BATCH_WIDE_FRAMES ekf_batch_wide.hip
// (both models); one workgroup per member; the noisy poses of replicas: ekf_batch_replicas.hip, or, from noisy corners,
// ekf_batch_corner_replicas.hip; with a frozen member the FROZEN instances of ekf_batch_frozen.hip and
// ekf_batch_wide_frozen.hip).  Host side only: argument
// checking, workspace carving, launch sequencing.
#include <cmath>
#include <cstring>

#include "ekf_host.h"
#include "ekf_kernels.h"
#include "ekf_remove.h"
#include "ekf_batch_smooth_host.h"

struct ekf_batch {
    ekf_config cfg{};
    int32_t members = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t ld = 0;
    double* cov = nullptr;
    double* state = nullptr;
    char* ws = nullptr;
    bool bound = false;
    std::vector<double> noise;      // [B][6] host copy (initial_camera_uncertainty is used on the host, by reset)
    std::vector<int32_t> nlm;       // [B] host copy, refreshed after every call
    std::vector<int32_t> status;    // [B]
    std::vector<double> gate;       // [B] chi^2 gate per member (+inf: off); empty: no gate set (ekf_batch_set_gate)
    std::vector<int32_t> frozen;    // [B] "map frozen" per member (ekf_batch_set_map_frozen); the device copy: BatchLayout::frozen
    PinnedBuffer pin;               // pinned staging of a call's indices and offsets
    // Batch smoothing (include/ekf_slam_hip.h, "Batch smoothing"): the plan of the last recorded call (host side, from the
    // logs alone) and, once something asks for them (`fetched`), the words the device wrote and the tables built from them.
    // ekf_batch_reset, ekf_batch_set_member and ekf_batch_remove_markers clear `valid`.
    struct History {
        bool valid = false, fetched = false, with_motion = false;
        const void* buf = nullptr;
        BatchHistoryPlan plan;
        std::vector<int64_t> member_frames;       // [B + 1]
        std::vector<int32_t> flag;                // [Ftot] as the device wrote them
        std::vector<double> s_eff, motion;        // [Ftot], [Ftot][6] (zeros without motions)
        BatchSmoothTables tab;
    } hist;
};

namespace {

constexpr int kBatchWindow = 64;   // frames per member and launch: every dispatch stays short

// landmark dims and measurement rows per detection of the batch's model
int batch_lmd(const ekf_config& c) { return c.model == EKF_MODEL_ROTATIONS ? 10 : EKF_LM; }
int batch_rd(const ekf_config& c) { return c.model == EKF_MODEL_ROTATIONS ? 7 : 3; }

int64_t batch_ld(const ekf_config& c) { return round_up(batch_lmd(c) * (int64_t)c.max_landmarks + EKF_CAM, 32); }

bool batch_large(const ekf_config& c) { return (c.flags & EKF_FLAG_BATCH_LARGE_MAPS) != 0; }
bool batch_wide(const ekf_config& c) { return (c.flags & EKF_FLAG_BATCH_WIDE_FRAMES) != 0; }
bool batch_scaled(const ekf_config& c) { return (c.flags & EKF_FLAG_FRAME_SCALE) != 0; }

// A / W of one member of a large-maps or wide-frames batch: [rd max_visible][ld] doubles
int64_t batch_w_stride(const ekf_config& c) { return (int64_t)batch_rd(c) * c.max_visible * batch_ld(c); }

// workspace: [noise [B][6] | status [B] | landmark counts [B] | large maps or wide frames only: A / W [B][w_stride] |
// EKF_FLAG_FRAME_SCALE only: pending scales [B]]; the "map frozen" flags [B] lie directly behind the status words, in their
// piece
struct BatchLayout {
    size_t status, nlm, w, total, pending, frozen;
};

BatchLayout batch_layout(const ekf_config& c, int32_t members) {
    Carve w;
    w.take((size_t)members * 6 * 8);
    const size_t status = w.take((size_t)members * 8), nlm = w.take((size_t)members * 4);      // (status | frozen)
    const size_t wm = w.take(batch_large(c) || batch_wide(c) ? (size_t)members * batch_w_stride(c) * 8 : 0);
    const size_t pending = w.take(batch_scaled(c) ? (size_t)members * 8 : 0);
    return {status, nlm, wm, w.end, pending, status + (size_t)members * 4};
}

// zero the pending scale of members [lo, hi) (the stream is idle); nothing without EKF_FLAG_FRAME_SCALE
int batch_zero_pending(ekf_batch* b, int32_t lo, int32_t hi) {
    if (!batch_scaled(b->cfg)) return EKF_OK;
    HIP_TRY(hipMemset(b->ws + batch_layout(b->cfg, b->members).pending + 8 * (size_t)lo, 0, (size_t)(hi - lo) * 8));
    return EKF_OK;
}

// log workspace: [landmark indices [D] | frame offsets [Ftot+1] | member frame offsets [B+1] | with a gate set: gates [B]]
struct BatchLogLayout {
    size_t frames, members, gate, total;
};

BatchLogLayout batch_log_layout(int64_t D, int64_t F, int32_t B, bool gated) {
    Carve w;
    w.take((size_t)D * 4);
    const size_t frames = w.take((size_t)(F + 1) * 8), members = w.take((size_t)(B + 1) * 8);
    const size_t gate = w.take(gated ? (size_t)B * 8 : 0);
    return {frames, members, gate, w.end};
}

bool batch_gated(const ekf_batch* b) { return !b->gate.empty(); }

bool batch_any_frozen(const ekf_batch* b) {
    for (int32_t f : b->frozen)
        if (f) return true;
    return false;
}

// host copies of the "map frozen" flags of members [lo, hi) -> device (the stream is idle)
int batch_put_frozen(ekf_batch* b, int32_t lo, int32_t hi) {
    const BatchLayout L = batch_layout(b->cfg, b->members);
    HIP_TRY(hipMemcpy(b->ws + L.frozen + 4 * (size_t)lo, b->frozen.data() + lo, (size_t)(hi - lo) * 4, hipMemcpyHostToDevice));
    return EKF_OK;
}

// A frozen member adds nothing through observation (include/ekf_slam_hip.h, "Localisation mode"): an index at or beyond its
// landmark count is refused, before check_log would read it as a first sighting.
int check_frozen_log(const int32_t* lm_index, const int64_t* offsets, int64_t frames, int n_lm, const std::string& log) {
    for (int64_t d = offsets[0]; d < offsets[frames]; ++d)
        if (lm_index[d] >= n_lm)
            return fail(EKF_ERR_STATE, log + " holds a first sighting, and the member's map is frozen");
    return EKF_OK;
}

int check_batch_config(const ekf_config* c, int32_t members) {
    if (!c) return fail(EKF_ERR_INVALID, "config is NULL");
    if (members < 1) return fail(EKF_ERR_INVALID, "a batch needs at least one member");
    const bool wide = batch_wide(*c), large = batch_large(*c) || wide;      // (wide frames take the large-map limits)
    if (c->model == EKF_MODEL_ROTATIONS) {
        if (c->cov_dtype != EKF_COV_F64)
            return fail(EKF_ERR_INVALID, "EKF_MODEL_ROTATIONS batches keep an f64 covariance (cov_dtype EKF_COV_F64)");
        if (large && (c->max_landmarks < 1 || c->max_landmarks > EKF_BATCH_ROT_LARGE_MAX_LANDMARKS))
            return fail(EKF_ERR_INVALID, wide ? "EKF_MODEL_ROTATIONS batch max_landmarks must be in 1..101 (EKF_FLAG_BATCH_WIDE_FRAMES)"
                                              : "EKF_MODEL_ROTATIONS batch max_landmarks must be in 1..101 (EKF_FLAG_BATCH_LARGE_MAPS)");
        if (!large && (c->max_landmarks < 1 || c->max_landmarks > EKF_BATCH_ROT_MAX_LANDMARKS))
            return fail(EKF_ERR_INVALID, "EKF_MODEL_ROTATIONS batch max_landmarks must be in 1..24");
        if (wide && (c->max_visible < 1 || c->max_visible > EKF_BATCH_ROT_WIDE_MAX_VISIBLE))
            return fail(EKF_ERR_INVALID, "EKF_MODEL_ROTATIONS batch max_visible must be in 1..50 (EKF_FLAG_BATCH_WIDE_FRAMES)");
        if (!wide && (c->max_visible < 1 || c->max_visible > EKF_BATCH_ROT_MAX_VISIBLE))
            return fail(EKF_ERR_INVALID, "EKF_MODEL_ROTATIONS batch max_visible must be in 1..8");
        if (c->quat_mode != EKF_QUAT_SCALAR_FIRST)
            return fail(EKF_ERR_INVALID, "EKF_MODEL_ROTATIONS batch quat_mode must be EKF_QUAT_SCALAR_FIRST");
        return EKF_OK;
    }
    if (c->model != EKF_MODEL_EKF) return fail(EKF_ERR_INVALID, "batches exist for EKF_MODEL_EKF and EKF_MODEL_ROTATIONS only");
    if (c->cov_dtype != EKF_COV_F64) return fail(EKF_ERR_INVALID, "batches keep an f64 covariance (EKF_COV_F64)");
    if (large && (c->max_landmarks < 1 || c->max_landmarks > EKF_BATCH_LARGE_MAX_LANDMARKS))
        return fail(EKF_ERR_INVALID, wide ? "batch max_landmarks must be in 1..338 (EKF_FLAG_BATCH_WIDE_FRAMES)"
                                          : "batch max_landmarks must be in 1..338 (EKF_FLAG_BATCH_LARGE_MAPS)");
    if (!large && (c->max_landmarks < 1 || c->max_landmarks > EKF_BATCH_MAX_LANDMARKS))
        return fail(EKF_ERR_INVALID, "batch max_landmarks must be in 1..82");
    if (wide && (c->max_visible < 1 || c->max_visible > EKF_BATCH_WIDE_MAX_VISIBLE))
        return fail(EKF_ERR_INVALID, "batch max_visible must be in 1..64 (EKF_FLAG_BATCH_WIDE_FRAMES)");
    if (!wide && (c->max_visible < 1 || c->max_visible > EKF_BATCH_MAX_VISIBLE))
        return fail(EKF_ERR_INVALID, "batch max_visible must be in 1..16");
    if (c->quat_mode != EKF_QUAT_AS_WRITTEN && c->quat_mode != EKF_QUAT_SCALAR_FIRST)
        return fail(EKF_ERR_INVALID, "unknown quat_mode");
    return EKF_OK;
}

int check_noise(const double* nz) {
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(nz[i]) || nz[i] < 0.0) return fail(EKF_ERR_INVALID, "noise constants must be finite and >= 0");
    if (!(nz[2] > 0.0)) return fail(EKF_ERR_INVALID, "r_uncertainty must be > 0");
    return EKF_OK;
}

int batch_ready(const ekf_batch* b) {
    if (!b) return fail(EKF_ERR_INVALID, "batch handle is NULL");
    if (!b->bound) return fail(EKF_ERR_STATE, "ekf_batch_bind_buffers has not been called");
    HIP_TRY(hipSetDevice(b->device));
    return EKF_OK;
}

int batch_member(const ekf_batch* b, int32_t member) {
    if (member < 0 || member >= b->members) return fail(EKF_ERR_INVALID, "member index out of range");
    return EKF_OK;
}

// status and landmark counts of every member back to the host (the stream is idle afterwards)
int batch_refresh(ekf_batch* b) {
    const BatchLayout L = batch_layout(b->cfg, b->members);
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->status.data(), b->ws + L.status, (size_t)b->members * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b->nlm.data(), b->ws + L.nlm, (size_t)b->members * 4, hipMemcpyDeviceToHost));
    return EKF_OK;
}

// host copies of status and landmark count of members [lo, hi) -> device
int batch_put_member_words(ekf_batch* b, int32_t lo, int32_t hi) {
    const BatchLayout L = batch_layout(b->cfg, b->members);
    HIP_TRY(hipMemcpy(b->ws + L.status + 4 * (size_t)lo, b->status.data() + lo, (size_t)(hi - lo) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->ws + L.nlm + 4 * (size_t)lo, b->nlm.data() + lo, (size_t)(hi - lo) * 4, hipMemcpyHostToDevice));
    return EKF_OK;
}

// what the logs of a call ask of the window kernels' layout
struct BatchShape {
    int32_t n_max = 0, widest = 0;
    int64_t frames_max = 0;
    void add(const LogCheck& lc, int64_t frames) {
        n_max = std::max(n_max, (int32_t)lc.n);
        widest = std::max(widest, (int32_t)lc.widest);
        frames_max = std::max(frames_max, frames);
    }
};

int check_sigma(const double* sigma, int64_t rows) {
    for (int64_t i = 0; i < 6 * rows; ++i)
        if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return fail(EKF_ERR_INVALID, "sigma must be finite and >= 0");
    return EKF_OK;
}

// replica workspace: [noisy poses [B D][6] | the log layout of B tiled copies of the log (B D detections, B F frames)]
struct BatchReplicaLayout {
    size_t poses;
    BatchLogLayout log;
    size_t total;
};

BatchReplicaLayout batch_replica_layout(int64_t D, int64_t F, int32_t B, bool gated) {
    const BatchLogLayout log = batch_log_layout((int64_t)B * D, (int64_t)B * F, B, gated);
    return {log.total, log, log.total + align256((size_t)B * D * 6 * 8)};
}

// One call of the log replay: the arguments of ekf_batch_observe_logs_recorded (record: false from every other entry point;
// ekf_batch_history_bytes gives the log alone), then what batch_log_validate leaves for the staging and the windows.  A
// replica call fills what the windows read: log_ws and LL of its tiled log, sh, its noisy poses and the outputs.
struct BatchLogCall {
    const int32_t* lm_index;
    const int64_t *frame_offsets, *member_frames;
    const double *poses_dev, *rows_dev, *scale_dev, *motion_dev;
    void* log_ws;
    size_t log_ws_bytes;
    double *trajectory_dev, *nis_dev, *cam_cov_dev, *mahal_dev;
    bool record;
    void* history_dev;
    size_t history_bytes;
    // batch_log_validate: frames and detections of the call, where they go, what the logs ask of the kernels' layout, and of
    // a recorded (or sized) call where its records go
    bool with_motion = false;
    int64_t F = 0, D = 0;
    BatchLogLayout LL{};
    BatchShape sh;
    BatchHistoryPlan plan;
};

// The windows of a call whose indices and offsets are on the device (c.log_ws, layout c.LL): every member's frames
// [w, w + window) of its log per launch, state carried in HBM.  LDS is sized for the widest frame and the largest map of
// the call (a layout choice only: the arithmetic is the same)
int batch_run_windows(ekf_batch* b, const BatchLogCall& c, const EkfBatchRecord* record = nullptr) {
    const int32_t B = b->members;
    const BatchLayout L = batch_layout(b->cfg, B);
    const char* ws = static_cast<const char*>(c.log_ws);
    EkfBatchWindow a{};
    a.P = b->cov;
    a.ld = b->ld;
    a.state = b->state;
    a.noise = reinterpret_cast<const double*>(b->ws);
    a.status = reinterpret_cast<int32_t*>(b->ws + L.status);
    a.nlm = reinterpret_cast<int32_t*>(b->ws + L.nlm);
    a.lm_index = reinterpret_cast<const int32_t*>(ws);
    a.frame_offsets = reinterpret_cast<const int64_t*>(ws + c.LL.frames);
    a.member_frames = reinterpret_cast<const int64_t*>(ws + c.LL.members);
    a.poses = c.poses_dev;
    a.traj = c.trajectory_dev;
    a.nis = c.nis_dev;
    a.cam_cov = c.cam_cov_dev;
    a.quat_mode = b->cfg.quat_mode;
    a.gate = batch_gated(b) ? reinterpret_cast<const double*>(ws + c.LL.gate) : nullptr;
    a.mahal = c.mahal_dev;
    a.row_noise = c.rows_dev;      // (per-detection noise: data of the call, no workspace of its own)
    a.pending = batch_scaled(b->cfg) ? reinterpret_cast<double*>(b->ws + L.pending) : nullptr;
    a.scale = c.scale_dev;        // (per-frame scales: data of the call; checked by the caller: the flag is set)
    a.motion = c.motion_dev;      // (per-frame camera motions: data of the call, likewise)
    // (no member frozen: null, and every launcher runs the instance it ran before the flag existed)
    a.frozen = batch_any_frozen(b) ? reinterpret_cast<const int32_t*>(b->ws + L.frozen) : nullptr;
    const int rd = batch_rd(b->cfg);
    a.kmax = std::max(rd, rd * c.sh.widest);
    a.lda = (int32_t)round_up(batch_lmd(b->cfg) * c.sh.n_max + EKF_CAM + 1, 4);
    const bool rot = b->cfg.model == EKF_MODEL_ROTATIONS;
    // a frame of m detections costs about ceil(m / block) sweeps of P in ekf_batch_wide.hip (block = 16 / 8 detections), so
    // the window shrinks with the call's widest frame and every launch stays about as long.  Without the wide flag no frame
    // is wider than one block: 64 frames
    const int block = rot ? EKF_BATCH_ROT_MAX_VISIBLE : EKF_BATCH_MAX_VISIBLE;
    const int window = std::max(1, kBatchWindow / ((std::max(c.sh.widest, 1) + block - 1) / block));
    a.window_frames = window;
    // large maps or wide frames: every call runs ekf_batch_wide.hip, whatever the map size and the frame widths (A / W in
    // the workspace)
    const bool hbm = batch_large(b->cfg) || batch_wide(b->cfg);
    EkfBatchLargeWindow g{a, reinterpret_cast<double*>(b->ws + L.w), batch_w_stride(b->cfg)};
    for (int64_t w = 0; w < c.sh.frames_max; w += window) {
        a.window_first = (int32_t)w;
        g.w.window_first = (int32_t)w;
        if (record)      // (a recorded call: EKF, the one-column kernel, no frozen member -- checked by the caller)
            ekf_launch_batch_recorded_window(a, *record, B, b->stream);
        else if (hbm)
            ekf_launch_batch_wide_window(rot ? 1 : 0, !batch_wide(b->cfg), g, B, b->stream);
        else if (rot)
            ekf_launch_batch_rot_window(a, B, b->stream);
        else
            ekf_launch_batch_window(a, B, b->stream);
        HIP_TRY(hipGetLastError());
    }
    return EKF_OK;
}

// sigma_px [rows] finite and >= 0, marker_size > 0, a valid camera (make_camera): the noise arguments of the corner replicas
int check_corner_noise(const double* sigma_px, int64_t rows, double marker_size, const double camera_matrix[9],
                       const double* dist_coeffs, int32_t n_dist, EkfCamera* cam) {
    if (!sigma_px) return fail(EKF_ERR_INVALID, "sigma_px is NULL");
    for (int64_t i = 0; i < rows; ++i)
        if (!std::isfinite(sigma_px[i]) || sigma_px[i] < 0.0) return fail(EKF_ERR_INVALID, "sigma_px must be finite and >= 0");
    if (!(marker_size > 0.0)) return fail(EKF_ERR_INVALID, "marker_size must be > 0");
    return make_camera(camera_matrix, dist_coeffs, n_dist, cam);
}

// The replica calls: the log is checked for every member, its indices and offsets are tiled B times into ws, `launch` writes
// the B D poses the members consume into ws, and the windows run on them.  `c`: the log (lm_index, frame_offsets), the
// workspace and the outputs; `input_dev`: the log's poses or corners; `check_noise_args`: the call's own noise arguments (host
// side, before anything is enqueued).
template <typename Check, typename Launch>
int batch_observe_replicas(ekf_batch* b, BatchLogCall c, int64_t frames, const void* input_dev, uint32_t first_replica,
                           Check check_noise_args, Launch launch) {
    int rc = batch_ready(b);
    if (rc) return rc;
    // ---- validation on the host: nothing is enqueued before the log has passed for every member
    const int32_t B = b->members;
    if (frames < 0) return fail(EKF_ERR_INVALID, "frames must be >= 0");
    if (!c.frame_offsets) return fail(EKF_ERR_INVALID, "offsets are NULL");
    if ((rc = check_offsets(c.frame_offsets, frames, "frame_offsets"))) return rc;
    const int64_t D = c.frame_offsets[frames];
    if (D > 0 && (!c.lm_index || !input_dev)) return fail(EKF_ERR_INVALID, "NULL detections");
    if ((rc = check_noise_args(B))) return rc;
    if ((uint64_t)first_replica + (uint64_t)B > (1ull << 32))
        return fail(EKF_ERR_INVALID, "first_replica + members must not exceed 2^32");
    const BatchReplicaLayout RL = batch_replica_layout(D, frames, B, batch_gated(b));
    if ((rc = check_device_buffers({c.log_ws}, c.log_ws_bytes, RL.total, "ekf_batch_replica_workspace_bytes"))) return rc;
    if ((rc = batch_refresh(b))) return rc;
    LogCheck lc;
    for (int32_t m = 0; m < B; ++m) {
        if (m > 0 && b->nlm[m] == b->nlm[m - 1] && b->frozen[m] == b->frozen[m - 1]) {      // (the same log on the same landmark count and flag: the same verdict)
            c.sh.add(lc, frames);
            continue;
        }
        if (b->frozen[m] && (rc = check_frozen_log(c.lm_index, c.frame_offsets, frames, b->nlm[m], "the log (member " + std::to_string(m) + ")")))
            return rc;
        rc = check_log(c.lm_index, c.frame_offsets, frames, b->nlm[m], b->cfg, "the log (member " + std::to_string(m) + ")", &lc);
        if (rc) return rc;
        c.sh.add(lc, frames);
    }
    if (frames == 0) return EKF_OK;

    // ---- staging: the log's indices and offsets tiled member after member (member b: detections b D .., frames b F ..)
    const int64_t Ft = (int64_t)B * frames, Dt = (int64_t)B * D;
    const BatchLogLayout& LL = c.LL = RL.log;
    if ((rc = b->pin.reserve(LL.total))) return rc;
    int32_t* idx = b->pin.at<int32_t>(0);
    int64_t* fo = b->pin.at<int64_t>(LL.frames);
    int64_t* mf = b->pin.at<int64_t>(LL.members);
    for (int32_t m = 0; m < B; ++m) {
        if (D > 0) std::memcpy(idx + (size_t)m * D, c.lm_index, (size_t)D * 4);
        for (int64_t t = 0; t < frames; ++t) fo[(size_t)m * frames + t] = (int64_t)m * D + c.frame_offsets[t];
        mf[m] = (int64_t)m * frames;
    }
    fo[Ft] = Dt;
    mf[B] = Ft;
    if (batch_gated(b)) std::memcpy(b->pin.get() + LL.gate, b->gate.data(), (size_t)B * 8);
    char* w = static_cast<char*>(c.log_ws);
    HIP_TRY(hipMemcpyAsync(w, b->pin.get(), LL.total, hipMemcpyHostToDevice, b->stream));
    double* noisy = reinterpret_cast<double*>(w + RL.poses);
    if (D > 0) {
        launch(D, noisy);
        HIP_TRY(hipGetLastError());
    }
    c.poses_dev = noisy;
    return batch_run_windows(b, c);
}

// ---- batch smoothing (include/ekf_slam_hip.h, "Batch smoothing": the refusals) ------------------------------------------
int batch_smoothing_supported(const ekf_batch* b) {
    if (b->cfg.model != EKF_MODEL_EKF) return fail(EKF_ERR_STATE, "batch smoothing: EKF_MODEL_ROTATIONS is not supported");
    if (b->cfg.quat_mode != EKF_QUAT_SCALAR_FIRST)
        return fail(EKF_ERR_STATE, "batch smoothing needs EKF_QUAT_SCALAR_FIRST (the as-written injection has no inverse)");
    if (batch_large(b->cfg) || batch_wide(b->cfg))
        return fail(EKF_ERR_STATE, "batch smoothing: the window kernels of EKF_FLAG_BATCH_LARGE_MAPS / EKF_FLAG_BATCH_WIDE_FRAMES do not record");
    return EKF_OK;
}

// member m with a log of `frames` frames that check_log has passed (lc)
int batch_recordable(const ekf_batch* b, int32_t m, int64_t frames, const LogCheck& lc) {
    if (frames > 0 && b->frozen[m])
        return fail(EKF_ERR_STATE, "batch smoothing: member " + std::to_string(m) + "'s map is frozen");
    if (EKF_CAM + EKF_LM * lc.n > EKF_SMOOTH_RESIDENT_DIMS)
        return fail(EKF_ERR_STATE, "batch smoothing: member " + std::to_string(m) + " would pass 50 landmarks (the resident tier)");
    return EKF_OK;
}

// the words the device wrote in the last recorded call, and the tables from them (waits for the stream; once per recording)
int batch_history_fetch(ekf_batch* b) {
    ekf_batch::History& h = b->hist;
    if (!h.valid)
        return fail(EKF_ERR_STATE, "no recorded call (ekf_batch_observe_logs_recorded), or a member has been reset, set or pruned since");
    if (h.fetched) return EKF_OK;
    const size_t F = h.plan.slot.size();
    const char* hist = static_cast<const char*>(h.buf);
    h.flag.assign(F, 0);
    h.s_eff.assign(F, 0.0);
    h.motion.assign(F * 6, 0.0);
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (F > 0) {
        HIP_TRY(hipMemcpy(h.flag.data(), hist + h.plan.flag_at, F * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h.s_eff.data(), hist + h.plan.seff_at, F * 8, hipMemcpyDeviceToHost));
        if (h.with_motion) HIP_TRY(hipMemcpy(h.motion.data(), hist + h.plan.motion_at, F * 48, hipMemcpyDeviceToHost));
    }
    batch_smooth_tables(b->members, h.member_frames.data(), h.plan.head.data(), h.plan.slot.data(), h.plan.dims.data(),
                        h.flag.data(), h.s_eff.data(), h.with_motion ? h.motion.data() : nullptr, b->noise.data(), &h.tab);
    h.fetched = true;
    return EKF_OK;
}

// ---- validation on the host: nothing is enqueued before every log has passed.  A recorded call also plans its history and
// begins it.  sizing (ekf_batch_history_bytes): the logs alone, as far as the plan -- no poses, no workspace, and what
// batch_recordable refuses is left to the recorded call.
int batch_log_validate(ekf_batch* b, BatchLogCall& c, bool sizing) {
    int rc;
    if (!sizing) {
        if (c.record && (rc = batch_smoothing_supported(b))) return rc;
        if (c.motion_dev && (b->cfg.flags & EKF_FLAG_MOTION) == 0)
            return fail(EKF_ERR_STATE, "the batch was created without EKF_FLAG_MOTION");
        if (c.scale_dev && !batch_scaled(b->cfg)) return fail(EKF_ERR_STATE, "the batch was created without EKF_FLAG_FRAME_SCALE");
        c.with_motion = c.motion_dev != nullptr;
    }
    const int32_t B = b->members;
    if (!c.member_frames || !c.frame_offsets) return fail(EKF_ERR_INVALID, "offsets are NULL");
    if ((rc = check_offsets(c.member_frames, B, "member_frames"))) return rc;
    c.F = c.member_frames[B];
    if ((rc = check_offsets(c.frame_offsets, c.F, "frame_offsets"))) return rc;
    c.D = c.frame_offsets[c.F];
    if (c.D > 0 && (!c.lm_index || (!sizing && !c.poses_dev))) return fail(EKF_ERR_INVALID, "NULL detections");
    c.LL = batch_log_layout(c.D, c.F, B, batch_gated(b));
    if (!sizing && (rc = check_device_buffers({c.log_ws}, c.log_ws_bytes, c.LL.total, "ekf_batch_log_workspace_bytes"))) return rc;
    if ((rc = batch_refresh(b))) return rc;      // (landmark counts as the previous call left them)
    const bool planned = sizing || c.record;
    LogCheck lc;
    for (int32_t m = 0; m < B; ++m) {
        const int64_t* offsets = c.frame_offsets + c.member_frames[m];
        const int64_t frames = c.member_frames[m + 1] - c.member_frames[m];
        const std::string log = "member " + std::to_string(m) + "'s log";
        if (b->frozen[m] && (rc = check_frozen_log(c.lm_index, offsets, frames, b->nlm[m], log))) return rc;
        if ((rc = check_log(c.lm_index, offsets, frames, b->nlm[m], b->cfg, log, &lc))) return rc;
        c.sh.add(lc, frames);
        if (c.record && (rc = batch_recordable(b, m, frames, lc))) return rc;
        if (planned) batch_history_add_member(c.plan, offsets, frames, batch_lmd(b->cfg), b->nlm[m], lc, c.with_motion);
    }
    if (planned) batch_history_finish(c.plan, c.with_motion);
    if (!c.record) return EKF_OK;
    if (c.history_dev && c.history_bytes < c.plan.total)
        return fail(EKF_ERR_CAPACITY, "history smaller than ekf_batch_history_bytes");
    if ((rc = check_device_buffers({c.history_dev}, c.history_bytes, c.plan.total, "ekf_batch_history_bytes"))) return rc;
    b->hist = ekf_batch::History{};
    b->hist.valid = true;
    b->hist.with_motion = c.with_motion;
    b->hist.buf = c.history_dev;
    b->hist.member_frames.assign(c.member_frames, c.member_frames + B + 1);
    b->hist.plan = std::move(c.plan);
    return EKF_OK;
}

// The log call.  record: the RECORDED window kernels, which pack the member into the frame's slot of the history behind every
// frame that changed it (recording only reads the members: every output has the bits of the plain call).
int batch_observe_logs(ekf_batch* b, BatchLogCall c) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if ((rc = batch_log_validate(b, c, false))) return rc;
    const int32_t B = b->members;
    const int64_t F = c.F, D = c.D;
    if (F == 0) return EKF_OK;

    // ---- staging: one copy of indices and offsets (the stream is idle: batch_refresh synchronised it); a recorded call: the
    // headers' and slots' offsets behind them, into the history's own pieces
    const BatchLogLayout& LL = c.LL;
    const BatchHistoryPlan& hp = b->hist.plan;
    const size_t pin_head = LL.total, pin_slot = pin_head + align256((size_t)B * 8);
    if ((rc = b->pin.reserve(c.record ? pin_slot + align256((size_t)F * 8) : LL.total))) return rc;
    if (D > 0) std::memcpy(b->pin.get(), c.lm_index, (size_t)D * 4);
    std::memcpy(b->pin.get() + LL.frames, c.frame_offsets, (size_t)(F + 1) * 8);
    std::memcpy(b->pin.get() + LL.members, c.member_frames, (size_t)(B + 1) * 8);
    if (batch_gated(b)) std::memcpy(b->pin.get() + LL.gate, b->gate.data(), (size_t)B * 8);
    HIP_TRY(hipMemcpyAsync(c.log_ws, b->pin.get(), LL.total, hipMemcpyHostToDevice, b->stream));
    if (!c.record) return batch_run_windows(b, c);
    char* hist = static_cast<char*>(c.history_dev);
    std::memcpy(b->pin.get() + pin_head, hp.head.data(), (size_t)B * 8);
    std::memcpy(b->pin.get() + pin_slot, hp.slot.data(), (size_t)F * 8);
    HIP_TRY(hipMemcpyAsync(hist + hp.head_at, b->pin.get() + pin_head, (size_t)B * 8, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(hist + hp.slot_at, b->pin.get() + pin_slot, (size_t)F * 8, hipMemcpyHostToDevice, b->stream));
    if (c.motion_dev)      // (the tables need the motions on the host: they come back with the flags, from the history)
        HIP_TRY(hipMemcpyAsync(hist + hp.motion_at, c.motion_dev, (size_t)F * 48, hipMemcpyDeviceToDevice, b->stream));
    const EkfBatchRecord r{reinterpret_cast<double*>(hist), reinterpret_cast<const int64_t*>(hist + hp.head_at),
                           reinterpret_cast<const int64_t*>(hist + hp.slot_at), reinterpret_cast<int32_t*>(hist + hp.flag_at),
                           reinterpret_cast<double*>(hist + hp.seff_at)};
    rc = batch_run_windows(b, c, &r);
    if (rc) b->hist.valid = false;      // (a recorded call that failed leaves no history)
    return rc;
}

// The front of both smoothing calls, the refusals in the header's order: the batch, the recording, the history given against
// the recorded one, `flags` (the reserved word of the covariance call; the plain call has none: 0), then the device's words.
int batch_smooth_open(ekf_batch* b, const void* history_dev, size_t history_bytes, int32_t flags) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if ((rc = batch_smoothing_supported(b))) return rc;
    if (!b->hist.valid)
        return fail(EKF_ERR_STATE, "no recorded call (ekf_batch_observe_logs_recorded), or a member has been reset, set or pruned since");
    if (history_dev != b->hist.buf || history_bytes < b->hist.plan.total)
        return fail(EKF_ERR_STATE, "not the history of this handle's last recorded call");
    if (flags != 0) return fail(EKF_ERR_INVALID, "flags is reserved (0)");
    return batch_history_fetch(b);
}

// smoothing workspace: [status [B] | tables | members]
struct BatchSmoothLayout {
    size_t tables, members, total;
};
BatchSmoothLayout batch_smooth_layout(size_t records, int32_t B) {
    Carve w;
    w.take((size_t)B * 4);
    const size_t tables = w.take(std::max<size_t>(records, 1) * sizeof(EkfSmoothRec));
    const size_t members = w.take((size_t)B * sizeof(EkfBatchSmoothMember));
    return {tables, members, w.end};
}

// the pieces of a smoothing workspace `w`, the tables of the fetched history enqueued into them
struct BatchSmoothDev {
    int32_t* status;
    EkfSmoothRec* tables;
    EkfBatchSmoothMember* members;
};
int batch_smooth_upload(ekf_batch* b, char* w, const BatchSmoothLayout& L, BatchSmoothDev* d) {
    const BatchSmoothTables& tab = b->hist.tab;
    *d = {reinterpret_cast<int32_t*>(w), reinterpret_cast<EkfSmoothRec*>(w + L.tables),
          reinterpret_cast<EkfBatchSmoothMember*>(w + L.members)};
    if (!tab.tables.empty())
        HIP_TRY(hipMemcpyAsync(d->tables, tab.tables.data(), tab.tables.size() * sizeof(EkfSmoothRec), hipMemcpyHostToDevice,
                               b->stream));
    HIP_TRY(hipMemcpyAsync(d->members, tab.members.data(), (size_t)b->members * sizeof(EkfBatchSmoothMember),
                           hipMemcpyHostToDevice, b->stream));
    return EKF_OK;
}

// covariance workspace: the smoothing workspace, then [cov members | member 0: W Z T P^s | member 1: ...], a member's four
// matrices [ld][ld] with ld = the dims of its largest record rounded up to the tile (nothing for a member without a record)
struct BatchSmoothCovLayout {
    BatchSmoothLayout base;
    size_t cov_members, regions, total;
    std::vector<EkfBatchSmoothCovMember> members;      // region: doubles from `regions`
};
BatchSmoothCovLayout batch_smooth_cov_layout(const BatchSmoothTables& tab, int32_t B) {
    BatchSmoothCovLayout L;
    L.base = batch_smooth_layout(tab.tables.size(), B);
    Carve w;
    w.end = L.base.total;
    L.cov_members = w.take((size_t)B * sizeof(EkfBatchSmoothCovMember));
    L.regions = w.end;
    for (int32_t m = 0; m < B; ++m) {
        const EkfBatchSmoothMember& mem = tab.members[m];
        int32_t nmax = 0;
        for (int32_t r = 0; r < mem.records; ++r) nmax = std::max(nmax, tab.tables[(size_t)mem.table + r].dims);
        EkfBatchSmoothCovMember cm{};
        cm.ld = (nmax + EKF_SMOOTH_COV_TILE - 1) / EKF_SMOOTH_COV_TILE * EKF_SMOOTH_COV_TILE;
        cm.region = (int64_t)((w.take((size_t)4 * cm.ld * cm.ld * 8) - L.regions) / 8);
        L.members.push_back(cm);
    }
    L.total = w.end;
    return L;
}

}  // namespace

extern "C" {

int ekf_batch_query_sizes(const ekf_config* cfg, int32_t members, int64_t* ld, size_t* cov_bytes, size_t* state_bytes,
                          size_t* workspace_bytes) {
    int rc = check_batch_config(cfg, members);
    if (rc) return rc;
    const int64_t l = batch_ld(*cfg);
    if (ld) *ld = l;
    if (cov_bytes) *cov_bytes = (size_t)members * l * l * 8;
    if (state_bytes) *state_bytes = (size_t)members * l * 8;
    if (workspace_bytes) *workspace_bytes = batch_layout(*cfg, members).total;
    return EKF_OK;
}

int ekf_batch_create(const ekf_config* cfg, int32_t members, ekf_batch** out) {
    int rc = check_batch_config(cfg, members);
    if (rc) return rc;
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    const double nz[6] = {cfg->initial_camera_uncertainty, cfg->initial_landmark_uncertainty, cfg->r_uncertainty,
                          cfg->q_cam, cfg->q_err, cfg->q_lm};
    rc = check_noise(nz);
    if (rc) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(EKF_ERR_HIP, "no HIP device visible");
    ekf_batch* b = new ekf_batch();
    if (hipGetDevice(&b->device) != hipSuccess) b->device = 0;   // the caller's current device
    b->cfg = *cfg;
    b->members = members;
    b->stream = static_cast<hipStream_t>(cfg->stream);
    b->ld = batch_ld(*cfg);
    b->noise.resize((size_t)members * 6);
    for (int32_t m = 0; m < members; ++m)
        for (int i = 0; i < 6; ++i) b->noise[(size_t)m * 6 + i] = nz[i];
    b->nlm.assign(members, 0);
    b->status.assign(members, 0);
    b->frozen.assign(members, 0);
    *out = b;
    return EKF_OK;
}

int ekf_batch_destroy(ekf_batch* b) {
    if (!b) return EKF_OK;
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    delete b;
    return EKF_OK;
}

// Borrow the caller's buffers and reset every member to the identity pose (ekf_batch_reset to set the initial poses).
int ekf_batch_bind_buffers(ekf_batch* b, double* cov_dev, int64_t ld, double* state_dev, void* ws_dev, size_t ws_bytes) {
    if (!b) return fail(EKF_ERR_INVALID, "batch handle is NULL");
    int rc = check_device_buffers({cov_dev, state_dev, ws_dev}, ws_bytes, batch_layout(b->cfg, b->members).total,
                                  "ekf_batch_query_sizes");
    if (rc) return rc;
    if (ld != b->ld) return fail(EKF_ERR_INVALID, "ld must equal the value from ekf_batch_query_sizes");
    HIP_TRY(hipSetDevice(b->device));
    b->cov = cov_dev;
    b->state = state_dev;
    b->ws = static_cast<char*>(ws_dev);
    b->bound = true;
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->ws, b->noise.data(), b->noise.size() * 8, hipMemcpyHostToDevice));
    std::vector<double> poses((size_t)b->members * 10, 0.0);
    for (int32_t m = 0; m < b->members; ++m) poses[(size_t)m * 10 + 3] = 1.0;
    return ekf_batch_reset(b, -1, poses.data());
}

// gate [B]: finite and > 0, or +inf (that member's gate is off); NULL: no gate.  Persistent; nothing changes on error.
int ekf_batch_set_gate(ekf_batch* b, const double* gate) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (gate)
        for (int32_t m = 0; m < b->members; ++m)
            if (!(gate[m] > 0.0)) return fail(EKF_ERR_INVALID, "a gate must be > 0 (+inf: off) and not NaN");
    // (host copy only: every observe call stages the gates with its indices, so nothing on the stream reads this)
    if (gate)
        b->gate.assign(gate, gate + b->members);
    else
        b->gate.clear();
    return EKF_OK;
}

int ekf_batch_set_noise(ekf_batch* b, const double* noise) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (!noise) return fail(EKF_ERR_INVALID, "noise is NULL");
    for (int32_t m = 0; m < b->members; ++m) {
        rc = check_noise(noise + 6 * (size_t)m);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    std::memcpy(b->noise.data(), noise, b->noise.size() * 8);
    HIP_TRY(hipMemcpy(b->ws, b->noise.data(), b->noise.size() * 8, hipMemcpyHostToDevice));
    return EKF_OK;
}

// state = initial pose, P = initial_camera_uncertainty I_10 (the member's own), no landmarks, status cleared.
// member = -1: every member, initial_poses [B,10]; otherwise initial_poses [10].
int ekf_batch_reset(ekf_batch* b, int32_t member, const double* initial_poses) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (!initial_poses) return fail(EKF_ERR_INVALID, "initial poses are NULL");
    if (member != -1 && (rc = batch_member(b, member))) return rc;
    const int32_t lo = member < 0 ? 0 : member, hi = member < 0 ? b->members : member + 1;
    const int64_t ld = b->ld;
    b->hist.valid = false;      // (batch smoothing: the recording no longer describes the batch)
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemset(b->cov + (size_t)lo * ld * ld, 0, (size_t)(hi - lo) * ld * ld * 8));
    HIP_TRY(hipMemset(b->state + (size_t)lo * ld, 0, (size_t)(hi - lo) * ld * 8));
    HIP_TRY(hipMemcpy2D(b->state + (size_t)lo * ld, (size_t)ld * 8, initial_poses, 10 * 8, 10 * 8, hi - lo,
                        hipMemcpyHostToDevice));
    std::vector<double> diag((size_t)(hi - lo) * EKF_CAM);
    for (int32_t m = lo; m < hi; ++m) {
        for (int i = 0; i < EKF_CAM; ++i) diag[(size_t)(m - lo) * EKF_CAM + i] = b->noise[(size_t)m * 6];
        b->nlm[m] = 0;
        b->status[m] = 0;
        b->frozen[m] = 0;      // (a reset member maps again)
    }
    // P = icu I_10: the diagonal of every member's matrix is a strided run of ld + 1 elements
    for (int32_t m = lo; m < hi; ++m)
        HIP_TRY(hipMemcpy2D(b->cov + (size_t)m * ld * ld, (size_t)(ld + 1) * 8, diag.data() + (size_t)(m - lo) * EKF_CAM, 8, 8,
                            EKF_CAM, hipMemcpyHostToDevice));
    if ((rc = batch_zero_pending(b, lo, hi))) return rc;
    if ((rc = batch_put_frozen(b, lo, hi))) return rc;
    return batch_put_member_words(b, lo, hi);
}

// frozen [B] on the host (non-zero: frozen), or NULL: no member.  Persistent; nothing changes on error.  Waits for the stream.
int ekf_batch_set_map_frozen(ekf_batch* b, const int32_t* frozen) {
    int rc = batch_ready(b);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (int32_t m = 0; m < b->members; ++m) b->frozen[m] = frozen && frozen[m] ? 1 : 0;
    return batch_put_frozen(b, 0, b->members);
}

int ekf_batch_get_map_frozen(const ekf_batch* b, int32_t* out) {
    if (!b) return fail(EKF_ERR_INVALID, "batch handle is NULL");
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    std::memcpy(out, b->frozen.data(), b->frozen.size() * 4);
    return EKF_OK;
}

// (state [lmd n + 10], P [lmd n + 10, lmd n + 10]) of one member (lmd = 3: EKF, 10: EKF_Rotations) from the host; P is symmetrised ((P + P^T) / 2) on upload.
// The member's status is cleared.
int ekf_batch_set_member(ekf_batch* b, int32_t member, const double* state, int32_t num_landmarks, const double* cov) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if ((rc = batch_member(b, member))) return rc;
    if (!state || !cov || num_landmarks < 0) return fail(EKF_ERR_INVALID, "bad member state");
    if (num_landmarks > b->cfg.max_landmarks) return fail(EKF_ERR_CAPACITY, "more landmarks than max_landmarks");
    const int64_t ld = b->ld;
    const int dims = batch_lmd(b->cfg) * num_landmarks + EKF_CAM;
    std::vector<double> st((size_t)ld, 0.0), p((size_t)ld * ld, 0.0);
    std::memcpy(st.data(), state, (size_t)dims * 8);
    for (int i = 0; i < dims; ++i)
        for (int j = 0; j < dims; ++j) p[(size_t)i * ld + j] = 0.5 * (cov[(size_t)i * dims + j] + cov[(size_t)j * dims + i]);
    b->hist.valid = false;      // (batch smoothing: the recording no longer describes the batch)
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->state + (size_t)member * ld, st.data(), st.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->cov + (size_t)member * ld * ld, p.data(), p.size() * 8, hipMemcpyHostToDevice));
    b->nlm[member] = num_landmarks;
    b->status[member] = 0;
    if ((rc = batch_zero_pending(b, member, member + 1))) return rc;
    return batch_put_member_words(b, member, member + 1);
}

// state[0:count] and, if cov is not NULL, P [dims, dims] with dims = lmd n + 10 of one member.  Synchronises.
int ekf_batch_get_member(ekf_batch* b, int32_t member, double* state, int32_t count, double* cov, int32_t dims) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if ((rc = batch_member(b, member))) return rc;
    if ((rc = batch_refresh(b))) return rc;
    const int n = batch_lmd(b->cfg) * b->nlm[member] + EKF_CAM;
    if (count < 0 || count > n || (count > 0 && !state)) return fail(EKF_ERR_INVALID, "bad state request");
    if (cov && dims != n) return fail(EKF_ERR_INVALID, "dims must equal the member's state dimension");
    const int64_t ld = b->ld;
    if (count > 0) HIP_TRY(hipMemcpy(state, b->state + (size_t)member * ld, (size_t)count * 8, hipMemcpyDeviceToHost));
    if (cov)
        HIP_TRY(hipMemcpy2D(cov, (size_t)dims * 8, b->cov + (size_t)member * ld * ld, (size_t)ld * 8, (size_t)dims * 8, dims,
                            hipMemcpyDeviceToHost));
    return EKF_OK;
}

int ekf_batch_num_landmarks(const ekf_batch* b, int32_t* out) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    if ((rc = batch_refresh(const_cast<ekf_batch*>(b)))) return rc;
    std::memcpy(out, b->nlm.data(), b->nlm.size() * 4);
    return EKF_OK;
}

int ekf_batch_status(ekf_batch* b, int32_t* out) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    if ((rc = batch_refresh(b))) return rc;
    std::memcpy(out, b->status.data(), b->status.size() * 4);
    return EKF_OK;
}

int ekf_batch_log_workspace_bytes(const ekf_batch* b, int64_t detections, int64_t frames, size_t* bytes) {
    if (!b) return fail(EKF_ERR_INVALID, "batch handle is NULL");
    if (!bytes || detections < 0 || frames < 0) return fail(EKF_ERR_INVALID, "bad log size request");
    *bytes = batch_log_layout(detections, frames, b->members, batch_gated(b)).total;
    return EKF_OK;
}

int ekf_batch_observe_logs(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets, const int64_t* member_frames,
                           const double* poses_dev, void* log_ws, size_t log_ws_bytes, double* trajectory_dev) {
    return ekf_batch_observe_logs_gated(b, lm_index, frame_offsets, member_frames, poses_dev, log_ws, log_ws_bytes,
                                        trajectory_dev, nullptr, nullptr, nullptr);
}

int ekf_batch_observe_logs_diag(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets,
                                const int64_t* member_frames, const double* poses_dev, void* log_ws, size_t log_ws_bytes,
                                double* trajectory_dev, double* nis_dev, double* cam_cov_dev) {
    return ekf_batch_observe_logs_gated(b, lm_index, frame_offsets, member_frames, poses_dev, log_ws, log_ws_bytes,
                                        trajectory_dev, nis_dev, cam_cov_dev, nullptr);
}

int ekf_batch_observe_logs_gated(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets,
                                 const int64_t* member_frames, const double* poses_dev, void* log_ws, size_t log_ws_bytes,
                                 double* trajectory_dev, double* nis_dev, double* cam_cov_dev, double* mahal_dev) {
    return ekf_batch_observe_logs_rows(b, lm_index, frame_offsets, member_frames, poses_dev, nullptr, log_ws, log_ws_bytes,
                                       trajectory_dev, nis_dev, cam_cov_dev, mahal_dev);
}

int ekf_batch_observe_logs_rows(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets,
                                const int64_t* member_frames, const double* poses_dev, const double* rows_dev, void* log_ws,
                                size_t log_ws_bytes, double* trajectory_dev, double* nis_dev, double* cam_cov_dev,
                                double* mahal_dev) {
    return ekf_batch_observe_logs_scaled(b, lm_index, frame_offsets, member_frames, poses_dev, rows_dev, nullptr, log_ws,
                                         log_ws_bytes, trajectory_dev, nis_dev, cam_cov_dev, mahal_dev);
}

int ekf_batch_observe_logs_scaled(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets,
                                  const int64_t* member_frames, const double* poses_dev, const double* rows_dev,
                                  const double* scale_dev, void* log_ws, size_t log_ws_bytes, double* trajectory_dev,
                                  double* nis_dev, double* cam_cov_dev, double* mahal_dev) {
    return ekf_batch_observe_logs_moved(b, lm_index, frame_offsets, member_frames, poses_dev, rows_dev, scale_dev, nullptr,
                                        log_ws, log_ws_bytes, trajectory_dev, nis_dev, cam_cov_dev, mahal_dev);
}

int ekf_batch_observe_logs_moved(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets,
                                 const int64_t* member_frames, const double* poses_dev, const double* rows_dev,
                                 const double* scale_dev, const double* motion_dev, void* log_ws, size_t log_ws_bytes,
                                 double* trajectory_dev, double* nis_dev, double* cam_cov_dev, double* mahal_dev) {
    return batch_observe_logs(b, BatchLogCall{lm_index, frame_offsets, member_frames, poses_dev, rows_dev, scale_dev, motion_dev,
                                              log_ws, log_ws_bytes, trajectory_dev, nis_dev, cam_cov_dev, mahal_dev, false,
                                              nullptr, 0});
}

int ekf_batch_observe_logs_recorded(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets,
                                    const int64_t* member_frames, const double* poses_dev, const double* rows_dev,
                                    const double* scale_dev, const double* motion_dev, void* log_ws, size_t log_ws_bytes,
                                    double* trajectory_dev, double* nis_dev, double* cam_cov_dev, double* mahal_dev,
                                    void* history_dev, size_t history_bytes) {
    return batch_observe_logs(b, BatchLogCall{lm_index, frame_offsets, member_frames, poses_dev, rows_dev, scale_dev, motion_dev,
                                              log_ws, log_ws_bytes, trajectory_dev, nis_dev, cam_cov_dev, mahal_dev, true,
                                              history_dev, history_bytes});
}

// member = -1: every member, [B]; member >= 0: that one, [1].  Both wait for the batch's stream.
int ekf_batch_get_pending_scale(ekf_batch* b, int32_t member, double* out) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    if (member != -1 && (rc = batch_member(b, member))) return rc;
    const int32_t lo = member < 0 ? 0 : member, hi = member < 0 ? b->members : member + 1;
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (!batch_scaled(b->cfg)) {
        for (int32_t m = lo; m < hi; ++m) out[m - lo] = 0.0;
        return EKF_OK;
    }
    HIP_TRY(hipMemcpy(out, b->ws + batch_layout(b->cfg, b->members).pending + 8 * (size_t)lo, (size_t)(hi - lo) * 8,
                      hipMemcpyDeviceToHost));
    return EKF_OK;
}

int ekf_batch_set_pending_scale(ekf_batch* b, int32_t member, const double* pending) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (!pending) return fail(EKF_ERR_INVALID, "pending is NULL");
    if (member != -1 && (rc = batch_member(b, member))) return rc;
    if (!batch_scaled(b->cfg)) return fail(EKF_ERR_STATE, "the batch was created without EKF_FLAG_FRAME_SCALE");
    const int32_t lo = member < 0 ? 0 : member, hi = member < 0 ? b->members : member + 1;
    for (int32_t m = lo; m < hi; ++m)
        if (!std::isfinite(pending[m - lo]) || pending[m - lo] < 0.0)
            return fail(EKF_ERR_INVALID, "a pending scale must be finite and >= 0");
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->ws + batch_layout(b->cfg, b->members).pending + 8 * (size_t)lo, pending, (size_t)(hi - lo) * 8,
                      hipMemcpyHostToDevice));
    return EKF_OK;
}

int ekf_batch_replica_poses(const double* poses_dev, int64_t detections, const double* sigma, int32_t replicas,
                            uint64_t seed, uint32_t first_replica, double* out_dev, void* stream) {
    if (detections < 0 || replicas < 0) return fail(EKF_ERR_INVALID, "bad replica request");
    if ((uint64_t)first_replica + (uint64_t)replicas > (1ull << 32))
        return fail(EKF_ERR_INVALID, "first_replica + replicas must not exceed 2^32");
    if (replicas == 0) return EKF_OK;
    if (!sigma) return fail(EKF_ERR_INVALID, "sigma is NULL");
    int rc = check_sigma(sigma, replicas);
    if (rc) return rc;
    if (detections == 0) return EKF_OK;
    if (!poses_dev || !out_dev) return fail(EKF_ERR_INVALID, "NULL poses or output");
    ekf_launch_replica_poses(poses_dev, detections, sigma, replicas, seed, first_replica, out_dev,
                             static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return EKF_OK;
}

int ekf_batch_replica_workspace_bytes(const ekf_batch* b, int64_t detections, int64_t frames, size_t* bytes) {
    if (!b) return fail(EKF_ERR_INVALID, "batch handle is NULL");
    if (!bytes || detections < 0 || frames < 0) return fail(EKF_ERR_INVALID, "bad log size request");
    *bytes = batch_replica_layout(detections, frames, b->members, batch_gated(b)).total;
    return EKF_OK;
}

int ekf_batch_observe_replicas(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets, int64_t frames,
                               const double* poses_dev, const double* sigma, uint64_t seed, uint32_t first_replica,
                               void* ws, size_t ws_bytes, double* trajectory_dev, double* nis_dev, double* cam_cov_dev) {
    return ekf_batch_observe_replicas_gated(b, lm_index, frame_offsets, frames, poses_dev, sigma, seed, first_replica, ws,
                                            ws_bytes, trajectory_dev, nis_dev, cam_cov_dev, nullptr);
}

int ekf_batch_observe_replicas_gated(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets, int64_t frames,
                                     const double* poses_dev, const double* sigma, uint64_t seed, uint32_t first_replica,
                                     void* ws, size_t ws_bytes, double* trajectory_dev, double* nis_dev,
                                     double* cam_cov_dev, double* mahal_dev) {
    return batch_observe_replicas(
        b, BatchLogCall{lm_index, frame_offsets, nullptr, nullptr, nullptr, nullptr, nullptr, ws, ws_bytes, trajectory_dev,
                        nis_dev, cam_cov_dev, mahal_dev},
        frames, poses_dev, first_replica,
        [&](int32_t B) {
            if (!sigma) return fail(EKF_ERR_INVALID, "sigma is NULL");
            return check_sigma(sigma, B);
        },
        [&](int64_t D, double* noisy) {
            ekf_launch_replica_poses(poses_dev, D, sigma, b->members, seed, first_replica, noisy, b->stream);
        });
}

int ekf_batch_replica_corners(const double* corners_dev, int64_t detections, const double* sigma_px, int32_t replicas,
                              uint64_t seed, uint32_t first_replica, double marker_size, const double camera_matrix[9],
                              const double* dist_coeffs, int32_t n_dist, double* poses_dev, uint8_t* flipped_dev,
                              double* noisy_corners_dev, void* stream) {
    if (detections < 0 || replicas < 0) return fail(EKF_ERR_INVALID, "bad replica request");
    if ((uint64_t)first_replica + (uint64_t)replicas > (1ull << 32))
        return fail(EKF_ERR_INVALID, "first_replica + replicas must not exceed 2^32");
    if (replicas == 0) return EKF_OK;
    EkfCamera cam;
    int rc = check_corner_noise(sigma_px, replicas, marker_size, camera_matrix, dist_coeffs, n_dist, &cam);
    if (rc) return rc;
    if (detections == 0) return EKF_OK;
    if (!corners_dev) return fail(EKF_ERR_INVALID, "NULL corners");
    ekf_launch_corner_replicas(corners_dev, detections, sigma_px, replicas, seed, first_replica, marker_size, cam, poses_dev,
                               flipped_dev, noisy_corners_dev, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return EKF_OK;
}

int ekf_batch_observe_corner_replicas(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets, int64_t frames,
                                      const double* corners_dev, const double* sigma_px, uint64_t seed,
                                      uint32_t first_replica, double marker_size, const double camera_matrix[9],
                                      const double* dist_coeffs, int32_t n_dist, void* ws, size_t ws_bytes,
                                      double* trajectory_dev, double* nis_dev, double* cam_cov_dev, double* mahal_dev,
                                      uint8_t* flipped_dev) {
    EkfCamera cam;
    return batch_observe_replicas(
        b, BatchLogCall{lm_index, frame_offsets, nullptr, nullptr, nullptr, nullptr, nullptr, ws, ws_bytes, trajectory_dev,
                        nis_dev, cam_cov_dev, mahal_dev},
        frames, corners_dev, first_replica,
        [&](int32_t B) { return check_corner_noise(sigma_px, B, marker_size, camera_matrix, dist_coeffs, n_dist, &cam); },
        [&](int64_t D, double* noisy) {
            ekf_launch_corner_replicas(corners_dev, D, sigma_px, b->members, seed, first_replica, marker_size, cam, noisy,
                                       flipped_dev, nullptr, b->stream);
        });
}

// removal workspace: [index maps [B][ld] | landmark counts after the call [B]]
static size_t batch_remove_counts_at(const ekf_batch* b) { return align256((size_t)b->members * b->ld * 4); }
static size_t batch_remove_bytes(const ekf_batch* b) { return batch_remove_counts_at(b) + align256((size_t)b->members * 4); }

int ekf_batch_remove_workspace_bytes(const ekf_batch* b, int64_t total, size_t* bytes) {
    if (!b) return fail(EKF_ERR_INVALID, "batch handle is NULL");
    if (!bytes || total < 0) return fail(EKF_ERR_INVALID, "bad removal size request");
    *bytes = batch_remove_bytes(b);      // every member's index map, whatever the counts
    return EKF_OK;
}

// Semantics: include/ekf_slam_hip.h (ekf_remove_markers, per member).  One launch of the single filter's kernel with the
// member on blockIdx.y; it also stores the new landmark counts on the device.
int ekf_batch_remove_markers(ekf_batch* b, const int32_t* lm_index, const int64_t* offsets, double* cov_dev_new, int64_t ld,
                             double* state_dev_new, void* remove_ws, size_t remove_ws_bytes) {
    int rc = batch_ready(b);
    if (rc) return rc;
    const int32_t B = b->members;
    if (!offsets) return fail(EKF_ERR_INVALID, "offsets are NULL");
    if ((rc = check_offsets(offsets, B, "offsets"))) return rc;
    const int64_t total = offsets[B];
    if (total > 0 && !lm_index) return fail(EKF_ERR_INVALID, "bad removal list");
    const size_t need = batch_remove_bytes(b), counts_at = batch_remove_counts_at(b);
    if ((rc = check_device_buffers({cov_dev_new, state_dev_new, remove_ws}, need, need, "ekf_batch_remove_workspace_bytes")))
        return rc;
    if (ld != b->ld) return fail(EKF_ERR_INVALID, "ld must equal the value from ekf_batch_query_sizes");
    if (cov_dev_new == b->cov || state_dev_new == b->state)
        return fail(EKF_ERR_INVALID, "ekf_batch_remove_markers needs NEW buffers (the old ones are read)");
    if (remove_ws_bytes < need) return fail(EKF_ERR_CAPACITY, "remove_ws smaller than ekf_batch_remove_workspace_bytes");
    if ((rc = batch_refresh(b))) return rc;      // (landmark counts as the previous call left them; the stream is idle)
    const int lmd = batch_lmd(b->cfg);
    std::vector<int32_t> sorted;
    for (int32_t m = 0; m < B; ++m) {
        const std::string bad = ekf_remove_build_map(lm_index + offsets[m], offsets[m + 1] - offsets[m], b->nlm[m], lmd, b->ld,
                                                     nullptr, sorted);
        if (!bad.empty()) return fail(EKF_ERR_INVALID, bad + " (member " + std::to_string(m) + ")");
    }
    if (total == 0) return EKF_OK;
    if ((rc = b->pin.reserve(need))) return rc;
    int32_t* counts = b->pin.at<int32_t>(counts_at);
    for (int32_t m = 0; m < B; ++m) {
        const int64_t cnt = offsets[m + 1] - offsets[m];
        (void)ekf_remove_build_map(lm_index + offsets[m], cnt, b->nlm[m], lmd, b->ld, b->pin.at<int32_t>(0) + (size_t)m * b->ld,
                                   sorted);
        counts[m] = b->nlm[m] - (int32_t)cnt;
    }
    char* ws = static_cast<char*>(remove_ws);
    HIP_TRY(hipMemcpyAsync(ws, b->pin.get(), counts_at + (size_t)B * 4, hipMemcpyHostToDevice, b->stream));
    EkfRemoveArgs a{};
    a.cov_src = b->cov;
    a.cov_dst = cov_dev_new;
    a.state_src = b->state;
    a.state_dst = state_dev_new;
    a.ld = b->ld;
    a.map = reinterpret_cast<const int32_t*>(ws);
    a.nlm = reinterpret_cast<int32_t*>(b->ws + batch_layout(b->cfg, B).nlm);
    a.nlm_new = reinterpret_cast<const int32_t*>(ws + counts_at);
    ekf_launch_remove<double>(a, B, b->stream);
    HIP_TRY(hipGetLastError());
    b->cov = cov_dev_new;
    b->state = state_dev_new;
    b->hist.valid = false;      // (batch smoothing: the recording no longer describes the batch)
    return EKF_OK;
}

// ---- batch smoothing (include/ekf_slam_hip.h, "Batch smoothing"; kernels: ekf_batch_recorded.hip, ekf_smooth.hip) ---------
int ekf_batch_history_bytes(ekf_batch* b, const int32_t* lm_index, const int64_t* frame_offsets, const int64_t* member_frames,
                            int32_t with_motion, size_t* bytes) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (!bytes) return fail(EKF_ERR_INVALID, "bytes is NULL");
    BatchLogCall c{lm_index, frame_offsets, member_frames};
    c.with_motion = with_motion != 0;
    if ((rc = batch_log_validate(b, c, true))) return rc;
    *bytes = c.plan.total;
    return EKF_OK;
}

int ekf_batch_history_info(ekf_batch* b, int32_t member, int32_t* records, int32_t capacity, int32_t* frame, int32_t* dims,
                           double* s_eff, double* motion, int32_t* stepped, int32_t* frame_record) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if ((rc = batch_member(b, member))) return rc;
    if (!records || capacity < 0) return fail(EKF_ERR_INVALID, "bad history info request");
    if ((rc = batch_history_fetch(b))) return rc;
    const ekf_batch::History& h = b->hist;
    const EkfBatchSmoothMember& mem = h.tab.members[member];
    const int32_t R = mem.records;
    *records = R;
    const bool arrays = frame || dims || s_eff || motion || stepped;
    if (arrays && capacity < R) return fail(EKF_ERR_CAPACITY, "fewer entries than records");
    for (int32_t r = 0; r < R && arrays; ++r) {
        const size_t e = (size_t)mem.table + r;
        const int32_t t = h.tab.rec_frame[e];
        if (frame) frame[r] = t - mem.frame0;
        if (dims) dims[r] = h.tab.tables[e].dims;
        if (s_eff) s_eff[r] = h.tab.rec_stepped[e] ? h.s_eff[t] : 0.0;
        if (motion)
            for (int i = 0; i < 6; ++i) motion[6 * (size_t)r + i] = h.tab.tables[e].u[i];
        if (stepped) stepped[r] = h.tab.rec_stepped[e];
    }
    if (frame_record) {
        int32_t r = -1;
        for (int32_t t = mem.frame0; t < mem.frame1; ++t) {
            if (r + 1 < R && h.tab.rec_frame[(size_t)mem.table + r + 1] == t) ++r;
            frame_record[t - mem.frame0] = r;
        }
    }
    return EKF_OK;
}

int ekf_batch_history_record(ekf_batch* b, const void* history_dev, int32_t member, int32_t r, double* state_out,
                             double* cov_out, int32_t dims) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if ((rc = batch_member(b, member))) return rc;
    if (!b->hist.valid || history_dev != b->hist.buf)
        return fail(EKF_ERR_STATE, "not the history of this handle's last recorded call");
    if ((rc = batch_history_fetch(b))) return rc;
    const EkfBatchSmoothMember& mem = b->hist.tab.members[member];
    if (r < 0 || r >= mem.records) return fail(EKF_ERR_INVALID, "no such record");
    const EkfSmoothRec& e = b->hist.tab.tables[(size_t)mem.table + r];
    if (dims != e.dims) return fail(EKF_ERR_INVALID, "dims must equal the record's (ekf_batch_history_info)");
    const size_t N = (size_t)e.dims;
    std::vector<double> packed(N + N * (N + 1) / 2);
    HIP_TRY(hipMemcpy(packed.data(), static_cast<const double*>(history_dev) + e.off, packed.size() * 8, hipMemcpyDeviceToHost));
    if (state_out) std::memcpy(state_out, packed.data(), N * 8);
    if (cov_out) {
        const double* tri = packed.data() + N;
        size_t at = 0;
        for (size_t j = 0; j < N; ++j)
            for (size_t i = j; i < N; ++i, ++at) cov_out[i * N + j] = cov_out[j * N + i] = tri[at];
    }
    return EKF_OK;
}

// The table builder of the pass without a handle and without a device (what ekf_batch_smooth_history uploads).
int ekf_batch_history_table(int32_t members, const int64_t* member_frames, const int64_t* slot, const int32_t* dims,
                            const int32_t* flag, const double* s_eff, const double* motion, const double* noise,
                            int32_t capacity, int32_t* total, int32_t* member_rows, int32_t* rec_member, int32_t* rec_rows,
                            double* rec_q, int32_t* rec_moved) {
    if (members < 1 || !member_frames || !slot || !dims || !flag || !s_eff || !noise || !total || !member_rows || capacity < 0)
        return fail(EKF_ERR_INVALID, "bad table request");
    std::vector<int64_t> head((size_t)members, 0);
    BatchSmoothTables tab;
    batch_smooth_tables(members, member_frames, head.data(), slot, dims, flag, s_eff, motion, noise, &tab);
    *total = (int32_t)tab.tables.size();
    for (int32_t m = 0; m < members; ++m) {
        const EkfBatchSmoothMember& mem = tab.members[m];
        const int32_t row[5] = {mem.records, mem.frame0, mem.lead1, mem.nan0, mem.frame1};
        std::memcpy(member_rows + 5 * (size_t)m, row, sizeof row);
    }
    if (!rec_member && !rec_rows && !rec_q && !rec_moved) return EKF_OK;
    if (capacity < *total) return fail(EKF_ERR_CAPACITY, "fewer entries than records");
    for (int32_t m = 0; m < members; ++m)
        for (int32_t r = 0; r < tab.members[m].records; ++r) {
            const size_t e = (size_t)tab.members[m].table + r;
            if (rec_member) rec_member[e] = m;
            if (rec_rows) rec_rows[2 * e] = tab.tables[e].frame0, rec_rows[2 * e + 1] = tab.tables[e].frame1;
            if (rec_q)
                for (int i = 0; i < 3; ++i) rec_q[3 * e + i] = tab.tables[e].q[i];
            if (rec_moved) rec_moved[e] = tab.tables[e].moved;
        }
    return EKF_OK;
}

int ekf_batch_smooth_workspace_bytes(ekf_batch* b, size_t* bytes) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (!bytes) return fail(EKF_ERR_INVALID, "bytes is NULL");
    if ((rc = batch_history_fetch(b))) return rc;
    *bytes = batch_smooth_layout(b->hist.tab.tables.size(), b->members).total;
    return EKF_OK;
}

int ekf_batch_smooth_history(ekf_batch* b, const void* history_dev, size_t history_bytes, void* ws, size_t ws_bytes,
                             double* smoothed_dev, int32_t* status_out) {
    int rc = batch_smooth_open(b, history_dev, history_bytes, 0);
    if (rc) return rc;
    const int32_t B = b->members;
    const BatchSmoothTables& tab = b->hist.tab;
    if (status_out) std::memset(status_out, 0, (size_t)B * 4);
    if (b->hist.member_frames[B] == 0) return EKF_OK;
    if (!smoothed_dev) return fail(EKF_ERR_INVALID, "smoothed_dev is NULL");
    const BatchSmoothLayout L = batch_smooth_layout(tab.tables.size(), B);
    if ((rc = check_device_buffers({ws}, ws_bytes, L.total, "ekf_batch_smooth_workspace_bytes"))) return rc;
    BatchSmoothDev d;
    if ((rc = batch_smooth_upload(b, static_cast<char*>(ws), L, &d))) return rc;
    HIP_TRY(ekf_launch_batch_smooth(static_cast<const double*>(history_dev), d.tables, d.members, B, tab.nmax, smoothed_dev,
                                    d.status, b->stream));
    HIP_TRY(hipGetLastError());
    // every member has its own status word: a P_p that is not positive definite is reported there and nowhere else
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (status_out) HIP_TRY(hipMemcpy(status_out, d.status, (size_t)B * 4, hipMemcpyDeviceToHost));
    return EKF_OK;
}

// ---- batch smoothing, covariances (include/ekf_slam_hip.h, "Batch smoothing, covariances"; ekf_batch_smooth_cov.hip) ------
int ekf_batch_smooth_cov_workspace_bytes(ekf_batch* b, size_t* bytes) {
    int rc = batch_ready(b);
    if (rc) return rc;
    if (!bytes) return fail(EKF_ERR_INVALID, "bytes is NULL");
    if ((rc = batch_history_fetch(b))) return rc;
    *bytes = batch_smooth_cov_layout(b->hist.tab, b->members).total;
    return EKF_OK;
}

int ekf_batch_smooth_history_cov(ekf_batch* b, const void* history_dev, size_t history_bytes, void* ws, size_t ws_bytes,
                                 int32_t flags, double* smoothed_dev, double* cam_cov_dev, double* filt_cam_cov_dev,
                                 double* first_cov_dev, int32_t first_ld, int32_t* status_out) {
    int rc = batch_smooth_open(b, history_dev, history_bytes, flags);
    if (rc) return rc;
    const int32_t B = b->members;
    const BatchSmoothTables& tab = b->hist.tab;
    if (first_cov_dev)
        for (int32_t m = 0; m < B; ++m)
            if (tab.members[m].records > 0 && first_ld < tab.tables[(size_t)tab.members[m].table].dims)
                return fail(EKF_ERR_INVALID, "first_ld is below member " + std::to_string(m) + "'s first record (N_0)");
    const BatchSmoothCovLayout L = batch_smooth_cov_layout(tab, B);
    if (ws_bytes < L.total) return fail(EKF_ERR_INVALID, "workspace smaller than ekf_batch_smooth_cov_workspace_bytes");
    if (status_out) std::memset(status_out, 0, (size_t)B * 4);
    if (b->hist.member_frames[B] == 0) return EKF_OK;
    if (!smoothed_dev || !cam_cov_dev) return fail(EKF_ERR_INVALID, "smoothed_dev or cam_cov_dev is NULL");
    if ((rc = check_device_buffers({ws}, ws_bytes, L.total, "ekf_batch_smooth_cov_workspace_bytes"))) return rc;
    char* w = static_cast<char*>(ws);
    BatchSmoothDev d;
    if ((rc = batch_smooth_upload(b, w, L.base, &d))) return rc;
    EkfBatchSmoothCov a{};
    a.history = static_cast<const double*>(history_dev);
    a.status = d.status;
    EkfBatchSmoothCovMember* cov_members_dev = reinterpret_cast<EkfBatchSmoothCovMember*>(w + L.cov_members);
    a.tables = d.tables;
    a.members = d.members;
    a.cov_members = cov_members_dev;
    a.regions = reinterpret_cast<double*>(w + L.regions);
    a.smoothed = smoothed_dev;
    a.cam_cov = cam_cov_dev;
    a.filt_cam_cov = filt_cam_cov_dev;
    a.first_cov = first_cov_dev;
    a.first_ld = first_ld;
    a.nmax = tab.nmax;
    HIP_TRY(hipMemcpyAsync(cov_members_dev, L.members.data(), (size_t)B * sizeof(EkfBatchSmoothCovMember), hipMemcpyHostToDevice,
                           b->stream));
    // (L outlives the copies: the call waits for the stream below)
    HIP_TRY(ekf_launch_batch_smooth_cov(a, B, b->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (status_out) HIP_TRY(hipMemcpy(status_out, a.status, (size_t)B * 4, hipMemcpyDeviceToHost));
    return EKF_OK;
}

}  // extern "C"
