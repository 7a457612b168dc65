// The filter handle of the C ABI (include/ekf_slam_hip.h), for the translation units that share it: ekf_api.hip (the handle's
// life, state and getters), ekf_frames.hip (the frame scheduler and every observe call), ekf_log_api.hip (the log replay),
// ekf_smooth_api.hip (offline smoothing).  Not part of the public interface: whatever has external linkage in here is hidden.
#pragma once

#include "ekf_host.h"

#pragma GCC visibility push(hidden)

constexpr int kStageSlots = 64;   // pinned host ring for ekf_observe
constexpr int kMacroSuper = 8;    // macro-tile covariance update: super-tiles of 8 x 8 macro tiles per XCD (ekf_cov_macro.hip)
constexpr int kMacroMinTiles = 3000;   // ... chosen from this many 128 x 128 tiles of the lower triangle (n >= 3300 or so; measured: n=2048 1225 tiles 98 vs 80 us for the wave-per-tile kernel, n=4096 4753 tiles 290 vs 323)
constexpr int kTimedKernels = 4;
// Detections per frame that the gather kernel and the fused front kernel take; with EKF_FLAG_WIDE_FRAMES (flags bit 3) a
// configuration may allow up to kWideVisible, and every frame beyond the cap runs through the wide-frame path
// (ekf_wide.hip).  The rule depends on the model and m only, so a filter that grows into the wide range continues bit
// for bit like one built large.
constexpr int kWideVisible = 1024;
inline int visible_cap(int model) { return model == EKF_MODEL_ROTATIONS ? 50 : 64; }
inline bool wide_frame(int model, int m) { return m > visible_cap(model); }
constexpr int kEventPool = 2048;  // frames of timing events kept before folding

struct Layout {
    int64_t cap;      // padded state dimension (multiple of 128)
    int rd, lmd;      // rows per detection, landmark dims (model)
    int kmax;         // rd * max_visible rounded up to 16
    size_t elem;      // sizeof(cov element)
    size_t off_jac, off_resid, off_y, off_lmcol, off_amat, off_sblk, off_lmat, off_dinv, off_lop, off_dop, off_wpanel, off_wpanel2, off_cov2, off_wdbg,
        off_idx, off_z, off_status, off_stamps, off_dx, off_diag, off_xyz, off_unc,
        off_xl, off_done, off_sync, off_wsup, total;
    size_t off_wwork, off_xinv;   // wide frames beyond the stage kernels' size: A -> W in f64 [kmax][cap], X = L_BB^-1 (0: none)
    int wsup_ld;      // row length of the compact support-column copy of W (pipelined sequence mode; two copies, by frame parity)
    bool has_cov2;
    size_t off_tiles; // launch order of the macro-tile covariance update (f32, large problems)
    int tiles_cap;    // entries
    size_t slot_bytes;   // one slot of the pinned staging ring (reserve_host_buffers)
    // EKF_FLAG_GATE: the survivors of a gated frame (indices, z) and its distances; in a slot of the staging ring the exempt
    // mask and the host copy of the distances behind the detections (0: no gate scratch)
    bool has_gate;
    size_t off_gidx, off_gz, off_gmahal, slot_exempt, slot_mahal;
    // EKF_FLAG_ROW_NOISE: with the gate, the survivors' rows [max_visible][rd]; in a slot of the staging ring the frame's rows
    // behind everything else, where the kernels read them as they read the indices and z (0: none)
    bool has_rows;
    size_t off_grow, slot_rows;
    // fused front kernel: one exchange buffer per fused-frame parity (offsets / length in doubles)
    size_t xl_len, xl_dop, xl_y, xl_jac, xl_tag, xl_xs, xl_xr, xl_stag;
};

// What a state getter may skip (sync_and_check).  Each entry point names what it did; the four flags follow from that alone.
//   front_pending  ev_front marks where the state became final, and nothing that changes the state was enqueued since
//   mirror_fresh   ... and the front kernel of that frame also wrote the state and the status word into the pinned mirror
//   mirror_trust   entries no frame writes (EKF_Rotations: landmark error states) agree between mirror and device
//   status_clean   the device status word was zero when it was last read
// Only frame(true, true) -- a per-frame observe through the fused front kernel with timing off -- allows the zero-copy
// getter (an event wait and no copy at all), while the mirror is trusted (a reset or a full read back since the last
// state_set or new_workspace) and the status was clean at the last read back and is still zero in the mirror.
struct GetterShortcut {
    bool front_pending = false, mirror_fresh = false, mirror_trust = false, status_clean = false;
    bool zero_copy() const { return mirror_fresh && mirror_trust && status_clean; }
    void frame(bool recorded, bool mirrored) { front_pending = recorded; mirror_fresh = mirrored; }
    void run() { front_pending = status_clean = false; }   // (no front kernel of a run records ev_front; gate kernels
                                                           // raise status bits without the host word)
    void log() { front_pending = mirror_fresh = false; }
    void markers_added() { front_pending = false; }
    void state_set() { front_pending = mirror_trust = false; }
    void reset() { *this = {false, false, true, true}; }   // (state and mirror are both zero beyond what frames write)
    void new_workspace() { *this = {}; }
    void removed() { front_pending = mirror_fresh = false; mirror_trust = true; }   // (the removal launch writes the whole new state into the mirror)
    void moved() { front_pending = mirror_fresh = false; }   // (the motion launch changes the camera state behind ev_front and leaves the mirror alone: the next getter copies)
    void read_back(bool clean, bool full_state) { status_clean = clean; mirror_trust = mirror_trust || full_state; }
};

struct ekf_filter {
    ekf_config cfg{};
    Layout lay{};
    hipStream_t stream = nullptr;
    hipStream_t big = nullptr;          // internal stream: big covariance update in sequence mode
    hipEvent_t ev_front = nullptr;      // recorded behind the front part of the last per-frame observe: the state is final there
    GetterShortcut shortcut;
    int device = 0;
    void* cov = nullptr;
    int64_t ld = 0;
    double* state = nullptr;
    char* ws = nullptr;
    bool bound = false, is_reset = false;
    int n_lm = 0;
    int last_m = 0;
    bool debug_w = false;
    bool debug_stamps = false;
    bool debug_stamps_light = false;
    uint64_t fseq = 0;         // FUSED frames enqueued since reset: parity of the exchange buffer, frame tag
    uint64_t done_total = 0;   // column chunks of fused frames enqueued since reset
    uint64_t la_base = 0;      // frames that went through the pipelined sequence mode since reset (device counters)
    int la_ok = -1;            // pipelined mode usable (-1: not probed yet; 0: the two streams share a hardware queue)
    int seq_mode = EKF_SEQ_NONE;   // what the last ekf_observe_sequence_device call did (ekf_last_sequence_mode)
    // macro-tile covariance update: launch-order table in the workspace, rebuilt when the tile count changes
    int tiles_T = -1, tiles_grid = 0;
    // pinned host buffers sized by the capacity (reserve_host_buffers): the staging ring of host-pointer observes and
    // markers (kStageSlots slots of lay.slot_bytes), the readback mirror [status words (256 B) | state (cap doubles)] (one
    // sync per getter), the staging copy of the macro-tile table
    PinnedBuffer ring, readback, tiles_host;
    int slot = 0;
    hipEvent_t slot_done[kStageSlots] = {};
    // kernel timing
    bool timing = false;
    bool timing_cov_only = false;
    std::vector<hipEvent_t> ev;   // (kTimedKernels + 1) per frame
    int ev_frames = 0;
    double t_sum_us[kTimedKernels] = {};
    int64_t t_cnt[kTimedKernels] = {};
    // log replay (ekf_observe_log): pinned staging of the landmark indices, first-sighting slots and empty-frame rows, two
    // buffers used by turns (a call waits only for the call before the previous one), each reused once the stream has passed
    // its `log_pin_done`; what the last call did
    PinnedBuffer log_pin[2];
    hipEvent_t log_pin_done[2] = {};
    int log_pin_turn = 0;
    int64_t log_stats[4] = {};
    // per-detection gate (EKF_FLAG_GATE): the threshold (+inf: off; persistent across ekf_reset), the pinned mirror the gate
    // kernel leaves [survivors, some pivot failed (not read here: diagnostic)] in, the event behind it, what the last observe call tested / rejected
    double gate = __builtin_inf();
    PinnedBuffer gate_pin;
    hipEvent_t ev_gate = nullptr;
    int64_t gate_stats[2] = {};
    // landmark removal (ekf_remove_markers): pinned staging of the index map, two buffers used by turns as for the log
    // replay: a call waits only for the upload of the call before the previous one
    PinnedBuffer remove_pin[2];
    hipEvent_t remove_done[2] = {};
    int remove_turn = 0;

    // per-frame process-noise scale (EKF_FLAG_FRAME_SCALE): the pending scale p of the ABI's rules, kept on the host -- the
    // host launches every frame and knows which ones are stepped (a gated frame: after its round trip).  0 without the flag.
    double pending = 0.0;

    // frozen map (ekf_set_map_frozen; include/ekf_slam_hip.h, "Localisation mode"): frames inject the camera only and run the
    // camera-strip update (ekf_cov_strip.hip) in place of the covariance update, in serial order; off after create and reset
    bool frozen = false;

    // offline smoothing (include/ekf_slam_hip.h, "Offline smoothing"): the host-side table of the last recorded replay
    // (ekf_observe_log_recorded): per record the frame, N_r, where it lies in the caller's history buffer, s_eff (0: the frame
    // was only moved) and the motion; per frame its record (-1: before the first).  ekf_smooth_history reads it; `valid`
    // falls with ekf_remove_markers and ekf_reset.
    struct HistoryRec {
        int32_t frame, dims;
        size_t off;            // bytes from the start of the history buffer
        double s_eff;
        double u[6];
        int32_t stepped, moved;
    };
    struct History {
        bool valid = false;
        const void* buf = nullptr;
        size_t bytes = 0;
        int32_t frames = 0;
        std::vector<HistoryRec> recs;
        std::vector<int32_t> frame_rec;
        std::vector<EkfSmoothRec> table;      // what the kernels read, uploaded by ekf_smooth_history
    } hist;

    bool has_scale() const { return (cfg.flags & EKF_FLAG_FRAME_SCALE) != 0; }
    bool has_motion() const { return (cfg.flags & EKF_FLAG_MOTION) != 0; }
    bool gate_on() const { return lay.has_gate && gate < __builtin_inf(); }
    void reset_gate_stats() { gate_stats[0] = gate_stats[1] = 0; }      // every observe call counts from zero
    int dims() const { return lay.lmd * n_lm + EKF_CAM; }
    template <typename P> P* at(size_t off) const { return reinterpret_cast<P*>(ws + off); }
};

// fn(float{}) or fn(double{}), by the covariance dtype: the one place that picks the element type of a launch
template <class F>
auto by_cov_type(const ekf_filter* f, F&& fn) {
    return f->lay.elem == 4 ? fn(float{}) : fn(double{});
}

namespace {
// what every call on a running filter starts with: the handle is bound and reset; its device becomes the current one
int check_ready(ekf_filter* f) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!f->bound) return fail(EKF_ERR_STATE, "ekf_bind_buffers has not been called");
    if (!f->is_reset) return fail(EKF_ERR_STATE, "ekf_reset has not been called");
    HIP_TRY(hipSetDevice(f->device));
    return EKF_OK;
}
}  // namespace

// ---- ekf_smooth_api.hip: what smoothing refuses (also a recorded replay) ---------------------------------------------------
int smoothing_supported(const ekf_filter* f);

// ---- ekf_frames.hip: what other files need of the frame scheduler, per call or per frame of a serial loop (the per-frame
// path from ekf_observe down to enqueue_frame is all inside that file) -------------------------------------------------------
void release_pipelining_token(ekf_filter* f);
int fold_timing(ekf_filter* f);
EkfNoise frame_noise(const ekf_filter* f, double s_eff);
int check_scales(const ekf_filter* f, const double* scale, int64_t count);
int check_motions(const ekf_filter* f, const double* motion, int64_t count);
double frame_scale(const ekf_filter* f, const double* scale);
void frame_scale_done(ekf_filter* f, const double* scale, double s_eff, bool stepped);

// One frame of a call: its detections (device), their number (0: the frame is not stepped), its trajectory row (or null).
struct RunFrame {
    const int32_t* idx;
    const double* z;
    int m;
    double* traj_row;
    const double* rows = nullptr;      // [m][rd] or null: per-detection noise
    double s_eff = 1.0;                // the frame's process-noise scale (pending part included)
    int nnew = 0;                      // first sightings among the detections (log replay); of them ...
    const int32_t* new_slots = nullptr;      // ... the detections' numbers in the log [nnew], and the log's poses
    const double* poses = nullptr;
};

// Which frames of a call may pipeline (plan_runs)
struct RunPlan {
    std::vector<char> candidate;   // frame t may be in a run
    std::vector<char> joins;       // ... and continues the run of the stepped frame before it
    bool want_runs = false;        // some frame joins a run
};

// What a frame in serial order takes beside its detections, and (moved, survivors, s_eff) what became of it (serial_frame).
struct SerialFrame {
    const double *motion = nullptr, *scale = nullptr;      // [6] or null; the frame's scale, or null: it carries none
    bool folded = false;                 // rules 3 and 4 of the scale ran over the whole call beforehand: r.s_eff is final
    bool gated = false;                  // through the gate, on its survivors
    const uint8_t* exempt = nullptr;     // [m] (device or pinned host) or null: set for the first sightings
    double* mahal = nullptr;             // [m] (device) or null
    bool moved = false;                  // the motion enqueued something
    int survivors = 0;                   // detections the frame was stepped on (0: not stepped)
    double s_eff = 1.0;                  // the scale it ran with, or would have
};
int serial_frame(ekf_filter* f, const RunFrame& r, SerialFrame* x);

// A call whose frames are listed once per call (the log replay): plan the runs and settle whether they may pipeline (*mode:
// EKF_SEQ_*) before anything of the call is enqueued; then step the frames (stats: ekf_last_log_stats).
int plan_frames(ekf_filter* f, const std::vector<RunFrame>& frames, RunPlan* plan, int* mode);
int run_planned_frames(ekf_filter* f, const std::vector<RunFrame>& frames, const RunPlan& plan, int mode, int64_t* stats);

#pragma GCC visibility pop
