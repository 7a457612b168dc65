// C ABI of the EKF-SLAM HIP library (see include/ekf_slam_hip.h): the filter handle.  The batch handle is in
// ekf_batch_api.hip.  Host side only: argument checking, workspace carving, launch sequencing.
#include <atomic>
#include <cmath>
#include <cstring>

#include "ekf_host.h"
#include "ekf_kernels.h"
#include "ekf_remove.h"

thread_local std::string g_err;

namespace {

// Pipelined sequence mode orders its two streams with device-side gates that spin.  HIP multiplexes streams onto a small
// pool of hardware queues: with two handles pipelining at once, handle X's gate can sit in the queue in front of the
// launch handle Y's gate waits for, and vice versa -- both poll budgets run out.  So at most ONE handle of the
// process has gates in flight; another handle that asks for the pipelined mode meanwhile runs its call in serial order
// (same results, bit for bit) and says so (ekf_last_sequence_mode).
std::atomic<ekf_filter*> g_pipelining{nullptr};

void release_pipelining_token(ekf_filter* f) { (void)g_pipelining.compare_exchange_strong(f, nullptr); }

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

Layout make_layout(const ekf_config& c) {
    Layout L{};
    L.rd = c.model == EKF_MODEL_ROTATIONS ? 7 : 3;
    L.lmd = c.model == EKF_MODEL_ROTATIONS ? 10 : 3;
    L.cap = round_up((int64_t)L.lmd * c.max_landmarks + EKF_CAM, 128);
    // (a configuration that admits wide frames pads the rows to whole block columns of the blocked factorisation)
    const bool wide = c.max_visible > visible_cap(c.model);
    L.kmax = (int)round_up(L.rd * c.max_visible, wide ? EKF_WIDE_BLOCK : EKF_RB);
    L.elem = c.cov_dtype == EKF_COV_F32 ? 4 : 8;
    Carve w;
    L.off_jac = w.take((size_t)L.kmax * EKF_JLD * 8);
    L.off_resid = w.take((size_t)L.kmax * 8);
    L.off_y = w.take((size_t)L.kmax * 8);
    L.off_lmcol = w.take((size_t)c.max_visible * 4);
    L.off_amat = w.take((size_t)L.kmax * L.cap * 8);
    L.off_sblk = w.take((size_t)(L.kmax / EKF_RB) * (L.kmax / EKF_RB + 1) / 2 * 256 * 8);
    L.off_lmat = w.take((size_t)L.kmax * L.kmax * 8);
    L.off_dinv = w.take((size_t)L.kmax * EKF_RB * 8);
    {
        const size_t nb = (size_t)L.kmax / EKF_RB;
        L.off_lop = w.take(nb * (nb - 1) / 2 * 256 * 8 + 256);
        L.off_dop = w.take(nb * 256 * 8);
    }
    L.off_wpanel = w.take((size_t)L.kmax * L.cap * L.elem);
    L.off_wpanel2 = w.take((size_t)L.kmax * L.cap * L.elem);
    // pipelined sequence mode (MFMA update, fused front kernel): the second covariance buffer
    // (P_t is read, P_{t+1} written elsewhere, so that the next front kernel can read P_t beside the update)
    L.has_cov2 = c.cov_kernel != EKF_COVK_VALU && (c.flags & 5) == 0;
    L.off_cov2 = L.has_cov2 ? w.take((size_t)L.cap * L.cap * L.elem) : 0;
    L.off_wdbg = w.take((size_t)L.kmax * L.cap * 8);
    L.off_idx = w.take((size_t)c.max_visible * 4);
    L.off_z = w.take((size_t)c.max_visible * 7 * 8);
    L.off_status = w.take(256);
    L.off_stamps = w.take(64 * 8);
    L.off_dx = w.take((size_t)L.cap * 8);
    L.off_diag = w.take((size_t)L.cap * 8);
    L.off_xyz = w.take((size_t)256 * 6 * 8);
    L.off_unc = w.take((size_t)256 * 10 * 8);
    {
        const size_t nb = (size_t)L.kmax / EKF_RB;
        L.xl_dop = nb * (nb - 1) / 2 * 256 + 64;
        L.xl_y = L.xl_dop + nb * 256;
        L.xl_jac = L.xl_y + L.kmax;
        L.xl_tag = L.xl_jac + (size_t)L.kmax * EKF_JLD;
        L.xl_xs = L.xl_tag + 32;                          // S blocks, layout of sblk (block (i, tc) at (i (i + 1) / 2 + tc) * 256)
        L.xl_xr = L.xl_xs + nb * (nb + 1) / 2 * 256;      // residual
        L.xl_stag = L.xl_xr + (size_t)round_up(L.kmax, 16);   // S-block tags [16 tc + i]
        L.xl_len = L.xl_stag + 256;
        L.off_xl = w.take(2 * L.xl_len * 8);
        L.off_done = w.take(256);
        L.off_sync = w.take(EKF_SYNC_WORDS * 8);      // [0], [1] the two cross-stream counters, [2..9] the queue probe, then the update's arrival counts
        L.wsup_ld = (int)round_up(EKF_CAM + (int64_t)L.lmd * c.max_visible, 32);
        L.off_wsup = w.take((size_t)2 * L.kmax * L.wsup_ld * L.elem);
    }
    {
        // (the grid is 8 x the longest per-XCD list: the tile count plus, at worst, one super-tile per XCD)
        const int tmax = (int)(L.cap / 128);
        L.tiles_cap = (L.elem == 4 && c.cov_kernel != EKF_COVK_VALU && c.cov_kernel != EKF_COVK_MFMA_TILE)
                          ? tmax * (tmax + 1) / 2 + 8 * kMacroSuper * kMacroSuper : 0;
        L.off_tiles = w.take((size_t)L.tiles_cap * 4);
    }
    // wide frames beyond the stage kernels' size (ekf_wide.hip); configurations within the caps keep their sizes
    L.off_wwork = wide ? w.take((size_t)L.kmax * L.cap * 8) : 0;
    L.off_xinv = wide ? w.take((size_t)EKF_WIDE_BLOCK * EKF_WIDE_BLOCK * 8) : 0;
    // the per-detection gate (ekf_gate.hip); configurations without the flag keep their sizes
    L.has_gate = (c.flags & EKF_FLAG_GATE) != 0;
    L.off_gidx = L.has_gate ? w.take((size_t)c.max_visible * 4) : 0;
    L.off_gz = L.has_gate ? w.take((size_t)c.max_visible * 7 * 8) : 0;
    L.off_gmahal = L.has_gate ? w.take((size_t)c.max_visible * 8) : 0;
    // per-detection measurement noise; configurations without the flag keep their sizes
    L.has_rows = (c.flags & EKF_FLAG_ROW_NOISE) != 0;
    L.off_grow = L.has_rows && L.has_gate ? w.take((size_t)c.max_visible * L.rd * 8) : 0;
    L.total = w.end;
    // one slot of the pinned staging ring: a frame's detections as ekf_observe stages them, or 256 markers of ekf_add_markers
    const size_t det_bytes = align256((size_t)c.max_visible * 4) + align256((size_t)c.max_visible * 56);
    L.slot_exempt = det_bytes;
    L.slot_mahal = det_bytes + align256((size_t)c.max_visible);
    L.slot_rows = L.has_gate ? L.slot_mahal + align256((size_t)c.max_visible * 8) : det_bytes;
    L.slot_bytes = std::max(L.has_rows ? L.slot_rows + align256((size_t)c.max_visible * L.rd * 8) : L.slot_rows,
                            align256(256 * 48) + align256(256 * 80));
    return L;
}

int check_config(const ekf_config* c) {
    if (!c) return fail(EKF_ERR_INVALID, "config is NULL");
    if (c->max_landmarks < 1) return fail(EKF_ERR_INVALID, "max_landmarks must be >= 1");
    if (c->model != EKF_MODEL_EKF && c->model != EKF_MODEL_ROTATIONS)
        return fail(EKF_ERR_INVALID, "unknown model");
    if (c->max_visible < 1 || c->max_visible > ((c->flags & EKF_FLAG_WIDE_FRAMES) ? kWideVisible : visible_cap(c->model)))
        return fail(EKF_ERR_INVALID, (c->flags & EKF_FLAG_WIDE_FRAMES)
                                         ? "max_visible must be in 1..1024 (EKF_FLAG_WIDE_FRAMES)"
                                         : "max_visible must be in 1..64 (1..50 for EKF_MODEL_ROTATIONS; up to 1024 with "
                                           "EKF_FLAG_WIDE_FRAMES)");
    if (c->cov_dtype != EKF_COV_F64 && c->cov_dtype != EKF_COV_F32)
        return fail(EKF_ERR_INVALID, "cov_dtype must be EKF_COV_F64 or EKF_COV_F32");
    if (c->quat_mode != EKF_QUAT_AS_WRITTEN && c->quat_mode != EKF_QUAT_SCALAR_FIRST)
        return fail(EKF_ERR_INVALID, "unknown quat_mode");
    if (c->cov_kernel < EKF_COVK_AUTO || c->cov_kernel > EKF_COVK_MFMA_MACRO)
        return fail(EKF_ERR_INVALID, "unknown cov_kernel");
    if (c->cov_kernel == EKF_COVK_MFMA_MACRO && c->cov_dtype != EKF_COV_F32)
        return fail(EKF_ERR_INVALID, "EKF_COVK_MFMA_MACRO exists for the f32 covariance only");
    if (!(c->r_uncertainty > 0.0)) return fail(EKF_ERR_INVALID, "r_uncertainty must be > 0");
    return EKF_OK;
}

}  // namespace

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

namespace {

// fn(float{}) or fn(double{}), by the covariance dtype: the one place that picks the element type of a launch
template <class F>
auto by_cov_type(const ekf_filter* f, F&& fn) {
    return f->lay.elem == 4 ? fn(float{}) : fn(double{});
}

int fold_timing(ekf_filter* f) {
    if (f->ev_frames == 0) return EKF_OK;
    HIP_TRY(hipStreamSynchronize(f->stream));
    for (int fr = 0; fr < f->ev_frames; ++fr) {
        for (int kq = f->timing_cov_only ? kTimedKernels - 1 : 0; kq < kTimedKernels; ++kq) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, f->ev[fr * (kTimedKernels + 1) + kq],
                                        f->ev[fr * (kTimedKernels + 1) + kq + 1]));
            f->t_sum_us[kq] += 1e3 * ms;
            f->t_cnt[kq] += 1;
        }
    }
    f->ev_frames = 0;
    return EKF_OK;
}

// The noise of a frame that runs with the scale s_eff: Q_eff = fl(s_eff q) per entry -- one f64 multiplication each, rounded
// here, before any kernel adds it to anything (a device-side v + s q would contract into an fma) -- and r_uncertainty.
// s_eff = 1 (every frame of a filter without EKF_FLAG_FRAME_SCALE) gives the constants themselves.
EkfNoise frame_noise(const ekf_filter* f, double s_eff) {
    return EkfNoise{s_eff * f->cfg.q_cam, s_eff * f->cfg.q_err, s_eff * f->cfg.q_lm, f->cfg.r_uncertainty};
}

// a scale of a frame: finite and >= 0
bool scale_ok(double s) { return std::isfinite(s) && s >= 0.0; }

EkfFrame make_frame(ekf_filter* f, const int32_t* idx_dev, const double* z_dev, const double* rows_dev, int m,
                    double* traj_row, double s_eff) {
    EkfFrame fr{};
    const Layout& L = f->lay;
    fr.cov = f->cov;
    fr.ld = f->ld;
    fr.state = f->state;
    fr.model = f->cfg.model;
    fr.dims = f->dims();
    fr.ncols = (int)round_up(fr.dims, 128);
    fr.m = m;
    fr.k = L.rd * m;
    fr.kpad = (int)round_up(fr.k, EKF_RB);
    fr.idx = idx_dev;
    fr.z = z_dev;
    fr.rrow = rows_dev;
    fr.jac = f->at<double>(L.off_jac);
    fr.resid = f->at<double>(L.off_resid);
    fr.lmcol = f->at<int32_t>(L.off_lmcol);
    fr.amat = f->at<double>(L.off_amat);
    fr.lda = L.cap;
    fr.sblk = f->at<double>(L.off_sblk);
    fr.lmat = f->at<double>(L.off_lmat);
    fr.ldl = L.kmax;
    fr.dinv = f->at<double>(L.off_dinv);
    fr.lop = f->at<double>(L.off_lop);
    fr.dop = f->at<double>(L.off_dop);
    fr.yvec = f->at<double>(L.off_y);
    fr.wpanel = f->at<void>(L.off_wpanel);
    fr.ldw = L.cap;
    fr.wdbg = f->debug_w ? f->at<double>(L.off_wdbg) : nullptr;
    fr.status = f->at<int32_t>(L.off_status);
    fr.traj_row = traj_row;
    fr.dxvec = f->at<double>(L.off_dx);
    fr.stamps = (f->debug_w || f->debug_stamps) ? f->at<long long>(L.off_stamps) : nullptr;
    fr.stamps_heavy = f->debug_stamps_light ? 0 : 1;
    // (role-level stamps only: the per-frame ring of the end gate borrows the W debug copy, which is idle in that mode)
    fr.gate_log = (fr.stamps && !fr.stamps_heavy && !f->debug_w && (size_t)L.kmax * L.cap >= 4 * EKF_GATE_LOG_FRAMES)
                      ? f->at<long long>(L.off_wdbg) : nullptr;
    fr.nz = frame_noise(f, s_eff);
    fr.qprev_cam = fr.nz.q_cam;
    fr.qprev_err = fr.nz.q_err;
    fr.qprev_lm = fr.nz.q_lm;
    fr.quat_mode = f->cfg.quat_mode;
    fr.n_lm = f->n_lm;
    fr.state_host = nullptr;
    fr.status_host = nullptr;
    fr.frozen = f->frozen ? 1 : 0;
    fr.cov_tiles = nullptr;
    fr.cov_grid = 0;
    if (f->tiles_T > 0 && f->tiles_T == (fr.dims + 127) / 128) {
        fr.cov_tiles = f->at<uint32_t>(L.off_tiles);
        fr.cov_grid = f->tiles_grid;
    }
    return fr;
}

// Fused front kernel or the three stage kernels?  Fused unless the caller opted out (flags bit 2).
// Beyond k = 192 rows (EKF_Rotations with more than 27 markers in view) the frame runs through the stage kernels: the fused
// kernel's chunk and S-block roles are laid out for at most twelve block columns.
bool use_front_kernel(const ekf_filter* f, const EkfFrame& fr) { return (f->cfg.flags & 4) == 0 && fr.kpad <= 192; }

// Exchange buffers of a FUSED frame.  Parity, frame tag and the chunk counter advance with the fused
// frames only: a stage-kernel frame neither uses nor re-arms the exchange, so a filter may alternate
// between the two paths (flags can differ per handle, not per frame, today -- but the bookkeeping does
// not depend on that).
void bind_exchange(ekf_filter* f, EkfFrame& fr) {
    const Layout& L = f->lay;
    double* base = f->at<double>(L.off_xl);
    fr.xl = base + (f->fseq & 1) * L.xl_len;
    fr.xl_next = base + ((f->fseq + 1) & 1) * L.xl_len;
    fr.xl_dop = (int32_t)L.xl_dop;
    fr.xl_y = (int32_t)L.xl_y;
    fr.xl_jac = (int32_t)L.xl_jac;
    fr.xl_tag = (int32_t)L.xl_tag;
    fr.xl_len = (int32_t)L.xl_len;
    fr.xs = fr.xl + L.xl_xs;
    fr.xr = fr.xl + L.xl_xr;
    fr.xs_tag = fr.xl + L.xl_stag;
    fr.seqno = (double)(f->fseq + 1);
    fr.done_ctr = f->at<unsigned long long>(L.off_done);
    f->done_total += (uint64_t)(fr.ncols / 64);
    fr.done_target = f->done_total;
    f->fseq++;
}

// Macro-tile covariance update (f32, large problems: ekf_cov_macro.hip): chosen from kMacroMinTiles tiles of 128 x 128
// (or forced); its launch-order table depends on the tile count only and is rebuilt -- synchronously: this happens when
// landmarks are added, a few dozen times in the life of a filter -- whenever that changes.
int ensure_tiles(ekf_filter* f) {
    const Layout& L = f->lay;
    const int T = (f->dims() + 127) / 128;
    const bool want = L.tiles_cap > 0 &&
                      (f->cfg.cov_kernel == EKF_COVK_MFMA_MACRO || T * (T + 1) / 2 >= kMacroMinTiles);
    if (!want) {
        f->tiles_T = -1;
        return EKF_OK;
    }
    if (f->tiles_T == T) return EKF_OK;
    HIP_TRY(hipStreamSynchronize(f->stream));
    HIP_TRY(hipStreamSynchronize(f->big));
    const int grid = ekf_cov_macro_table(T, kMacroSuper, f->tiles_host.at<uint32_t>(0), L.tiles_cap);
    if (grid <= 0) return fail(EKF_ERR_STATE, "macro-tile launch table does not fit the workspace");
    HIP_TRY(hipMemcpy(f->at<uint32_t>(L.off_tiles), f->tiles_host.get(), (size_t)grid * 4, hipMemcpyHostToDevice));
    f->tiles_T = T;
    f->tiles_grid = grid;
    return EKF_OK;
}

// predict + update for one frame: the front kernel (or gather / solve / panel) and the covariance update
// `mirror`: the frame also leaves its state in the pinned host mirror (per-frame entry points: a state getter usually follows;
// frames of a sequence call do not -- no getter can run between them, and the mirror is 8 N bytes over PCIe per frame)
// rows_dev [m][rd] (device, or pinned host) or null: per-detection noise
// s_eff: the frame's process-noise scale (1: the constants)
int enqueue_frame(ekf_filter* f, const int32_t* idx_dev, const double* z_dev, const double* rows_dev, int m,
                  double* traj_row, bool mirror, double s_eff) {
    if (!f->frozen) {      // (a frozen frame runs the camera strip: no macro-tile table)
        int trc = ensure_tiles(f);
        if (trc) return trc;
    }
    EkfFrame fr = make_frame(f, idx_dev, z_dev, rows_dev, m, traj_row, s_eff);
    const int variant = f->cfg.cov_kernel == EKF_COVK_VALU ? 1 : 2;
    hipEvent_t* ev = nullptr;
    if (f->timing) {
        if (f->ev_frames == kEventPool) {
            int rc = fold_timing(f);
            if (rc) return rc;
        }
        ev = &f->ev[f->ev_frames * (kTimedKernels + 1)];
        f->ev_frames++;
    }
    hipEvent_t* ev_all = (ev && !f->timing_cov_only) ? ev : nullptr;
    if (ev_all) HIP_TRY(hipEventRecord(ev[0], f->stream));
    // (a frozen frame writes the camera only, so it is not mirrored: the mirror's landmark entries come from mirrored mapping
    // frames, removals and full read backs alone, and add_markers, a log or a sequence call may have changed the device's
    // since -- which the next mirrored mapping frame repairs by writing every entry, and a frozen one would not.  The getter
    // behind a frozen frame copies the state from the device.)
    const bool mirrored = use_front_kernel(f, fr) && !f->timing && mirror && !f->frozen;
    if (use_front_kernel(f, fr)) {
        // one launch: timing slot 0 = the whole front kernel, slots 1 and 2 stay empty
        bind_exchange(f, fr);
        if (mirrored) {
            fr.state_host = f->readback.at<double>(256);
            fr.status_host = f->readback.at<int32_t>(128);
        }
        by_cov_type(f, [&](auto elem) { ekf_launch_front<decltype(elem)>(fr, f->stream); });
        if (ev_all) {
            HIP_TRY(hipEventRecord(ev[1], f->stream));
            HIP_TRY(hipEventRecord(ev[2], f->stream));
        }
    } else if (wide_frame(fr.model, m)) {
        // Wide frame (ekf_wide.hip).  Timing slots: 0 = measurement, A and S; 1 = factorisation; 2 = W, dx and injection.
        // Up to kpad = 384 the factorisation and W are the stage kernels; beyond, the blocked factorisation works on a
        // copy of A (rows padded to whole block columns), so that A stays in `amat` (ekf_debug_fetch item 4).
        const bool blocked = fr.kpad > EKF_WIDE_REUSE_ROWS;
        const int rp = blocked ? (int)round_up(fr.k, EKF_WIDE_BLOCK) : fr.kpad;
        double* aw = blocked ? f->at<double>(f->lay.off_wwork) : nullptr;
        if (blocked && !f->lay.off_wwork) return fail(EKF_ERR_STATE, "internal: no wide-frame workspace");
        by_cov_type(f, [&](auto elem) { ekf_launch_wide_front<decltype(elem)>(fr, aw, rp, f->stream); });
        if (ev_all) HIP_TRY(hipEventRecord(ev[1], f->stream));
        if (blocked) ekf_launch_wide_factor(fr, aw, f->at<double>(f->lay.off_xinv), rp, f->stream);
        else ekf_launch_solve(fr, f->stream);
        if (ev_all) HIP_TRY(hipEventRecord(ev[2], f->stream));
        by_cov_type(f, [&](auto elem) {
            if (blocked) ekf_launch_wide_finish<decltype(elem)>(fr, aw, f->stream);
            else ekf_launch_panel<decltype(elem)>(fr, f->stream);
        });
        if (fr.model == 1) ekf_launch_inject_rot(fr, f->frozen ? 0 : f->n_lm, f->stream);      // (frozen map: block 0 only)
    } else {
        by_cov_type(f, [&](auto elem) { ekf_launch_gather<decltype(elem)>(fr, f->stream); });
        if (ev_all) HIP_TRY(hipEventRecord(ev[1], f->stream));
        ekf_launch_solve(fr, f->stream);
        if (ev_all) HIP_TRY(hipEventRecord(ev[2], f->stream));
        by_cov_type(f, [&](auto elem) { ekf_launch_panel<decltype(elem)>(fr, f->stream); });
        if (fr.model == 1) ekf_launch_inject_rot(fr, f->frozen ? 0 : f->n_lm, f->stream);
    }
    // The state (and the status word) are final here: a state getter that follows waits for this event only and
    // reads back beside the covariance update (sync_and_check) -- what BaseFilter.process_frame does every frame.
    f->shortcut.frame(!f->timing && hipEventRecord(f->ev_front, f->stream) == hipSuccess, mirrored);
    // the covariance update is timed by its own start / stop time stamps (what rocprofv3 reports), not by
    // events recorded around the launch (those also hold ~4 us of dispatch gap)
    if (fr.kpad > EKF_WIDE_REUSE_ROWS) {
        // W has more rows than the covariance-update kernels take: P <- P + Q - sum_c W_c^T W_c over row chunks of at most
        // 384 rows, in order, Q with the first chunk only.  Every kernel variant computes each chunk with the same bits,
        // so the sequence does too.  Timed by events around the launches (dispatch gaps included).
        if (ev) HIP_TRY(hipEventRecord(ev[3], f->stream));
        for (int r0 = 0; r0 < fr.kpad; r0 += EKF_WIDE_REUSE_ROWS) {
            EkfFrame cf = fr;
            cf.wpanel = static_cast<char*>(fr.wpanel) + (size_t)r0 * fr.ldw * f->lay.elem;
            cf.kpad = std::min(EKF_WIDE_REUSE_ROWS, fr.kpad - r0);
            cf.k = std::min(cf.kpad, std::max(0, fr.k - r0));
            if (r0 > 0) cf.nz.q_cam = cf.nz.q_err = cf.nz.q_lm = 0.0;
            const bool ok = by_cov_type(f, [&](auto elem) {
                if (f->frozen) return ekf_launch_cov_strip<decltype(elem)>(cf, variant, f->stream);      // (the same chunks in the same order)
                ekf_launch_cov_update<decltype(elem)>(cf, variant, f->stream);
                return true;
            });
            if (!ok) return fail(EKF_ERR_STATE, "internal: a row chunk larger than the strip kernel takes");
        }
        if (ev) HIP_TRY(hipEventRecord(ev[4], f->stream));
    } else {
        // frozen map: the camera strip, in place, in the covariance update's timing slot
        const bool ok = by_cov_type(f, [&](auto elem) {
            if (f->frozen) return ekf_launch_cov_strip<decltype(elem)>(fr, variant, f->stream, ev ? ev[3] : nullptr, ev ? ev[4] : nullptr);
            ekf_launch_cov_update<decltype(elem)>(fr, variant, f->stream, ev ? ev[3] : nullptr, ev ? ev[4] : nullptr);
            return true;
        });
        if (!ok) return fail(EKF_ERR_STATE, "internal: more rows than the strip kernel takes in one launch");
    }
    HIP_TRY(hipGetLastError());
    f->last_m = m;
    return EKF_OK;
}

int check_ready(ekf_filter* f) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!f->bound) return fail(EKF_ERR_STATE, "ekf_bind_buffers has not been called");
    if (!f->is_reset) return fail(EKF_ERR_STATE, "ekf_reset has not been called");
    HIP_TRY(hipSetDevice(f->device));
    return EKF_OK;
}

// `state_count` > 0: the first state_count doubles of the state come back with the same synchronisation
// (f->readback + 256): one stream sync per getter instead of a sync and two blocking copies
int sync_and_check(ekf_filter* f, int state_count = 0) {
    if (state_count > 0 && f->shortcut.front_pending) {
        // State getter right after a per-frame observe: the state and the status word were final when the front part
        // of that frame ended; the covariance update behind it goes on while the host reads back (internal stream: idle
        // outside ekf_observe_sequence_device, ordered here by the host having seen the event) and prepares the next frame.
        HIP_TRY(hipEventSynchronize(f->ev_front));
        // ... and if the fused front kernel has written the state into the pinned mirror and nobody has raised a status
        // bit (their stores to host memory are complete with the kernel), there is nothing to copy at all
        if (f->shortcut.zero_copy() && *f->readback.at<volatile int32_t>(128) == 0)
            return EKF_OK;
        HIP_TRY(hipMemcpyAsync(f->readback.get(), f->at<int32_t>(f->lay.off_status), 32, hipMemcpyDeviceToHost, f->big));
        HIP_TRY(hipMemcpyAsync(f->readback.at<double>(256), f->state, (size_t)state_count * 8, hipMemcpyDeviceToHost, f->big));
        HIP_TRY(hipStreamSynchronize(f->big));
    } else {
        HIP_TRY(hipMemcpyAsync(f->readback.get(), f->at<int32_t>(f->lay.off_status), 32, hipMemcpyDeviceToHost, f->stream));
        if (state_count > 0)
            HIP_TRY(hipMemcpyAsync(f->readback.at<double>(256), f->state, (size_t)state_count * 8, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        release_pipelining_token(f);      // (everything this handle has enqueued is complete: its gates are gone)
    }
    const int32_t* info = f->readback.at<int32_t>(0);
    const int32_t st = info[0];
    f->shortcut.read_back(st == 0, state_count == f->dims());      // (a full copy has just refreshed the mirror)
    if (st != 0) {
        // (sticky until ekf_reset: after any of these the filter state is not trustworthy)
        if (st & EKF_ST_BAD_INDEX)
            return fail(EKF_ERR_INVALID, "landmark index out of range in a device-resident detection array "
                                         "(clamped on the device; the filter state is no longer meaningful, reset it)");
        if (st & (EKF_ST_STALE_JAC | EKF_ST_STALE_COL | EKF_ST_STALE_S))
            return fail(EKF_ERR_NUMERIC, "internal: exchange data of another frame accepted in the front kernel (status " +
                                             std::to_string(st) + ")");
        if (st & EKF_ST_GATE_TIMEOUT)
            return fail(EKF_ERR_NUMERIC, "internal: a device-side wait between the two streams of the pipelined sequence mode timed out");
        if (st & EKF_ST_TIMEOUT)   // a bounded wait inside the fused front kernel ran out (should never happen)
            return fail(EKF_ERR_NUMERIC, "internal: exchange wait timed out in the front kernel (status " +
                                             std::to_string(st) + ")");
        if (info[2] >= 200)      // (ekf_solve_cw.h: a bounded wait on one of the factorisation's LDS flag words ran out; should never happen)
            return fail(EKF_ERR_NUMERIC, "internal: a wait inside the factorisation workgroup timed out (flag word " +
                                             std::to_string(info[2] - 200) + ")");
        return fail(EKF_ERR_NUMERIC, "innovation covariance S was not positive definite (block column " +
                                         std::to_string(info[2] - 100) + ", wave mask " + std::to_string(info[1]) + ")");
    }
    return EKF_OK;
}

// Pipelined sequence mode for a frame of this size (ekf_observe_sequence_device; the log replay asks per frame), before the
// frame count, the hardware-queue probe and the one-handle token.  Flags bit 1 forces it, bit 0 forbids it, otherwise it is
// chosen where it was measured to win.  MFMA covariance update (f32 or f64) and the fused front kernel only.
// tools/mode_select.py (profiles/r03_mode_select.txt: 2000 frames per call after a warm-up call, start-to-start of the
// front kernels on the device clock, pipelined / serial in us per frame): n=32 m=3 11.1 / 16.1 - n=64 m=8 12.5 / 18.5 -
// n=128 m=16 15.5 / 21.7 - C2 (n=256 m=16 f64) 15.9 / 21.5 - n=512 m=32 22.8 / 31.6 - n=1024 m=32 24.2 / 39.3: it wins at
// every shape down to the smallest.  (Round 2's soak tool had it slower at C2: its timed region began with the handle's
// very first pipelined call, which holds the one-time queue self-test.)  tools/pipeline_sweep.py, larger shapes:
// n=1024 m=64 81.8 / 95.1 - n=2048 m=32 61.7 / 73.3 - n=2048 m=64 115.7 / 152.4 - n=4096 m=32 237 / 238 - n=4096 m=64
// 398 / 371: there the front kernel's 273 workgroups hold every CU while they wait for the factorisation, and the update
// cannot run beside them.
bool pipeline_wanted(const ekf_filter* f, int dims, int kpad, int m) {
    // (measured, profiles/r03_mode_select.txt.  EKF model: pipelined wins everywhere except N > 9000 with k > 96, where the front
    // kernel's workgroups and the macro-tile update cannot share CUs.  EKF_Rotations: its chunks complete 10 + 10 m support rows
    // per frame in the pipelined form; from k = 91 (m = 13) on the serial order is faster: 28.2k vs 24.3k updates/s at n=100
    // m=13, 25.5k vs 16.4k at m=16, 15.7k vs 12.7k at n=200 m=21, 9.3k vs 9.1k at n=400 m=27; below, pipelined: 41.0k vs
    // 32.5k at n=100 m=9)
    const bool auto_on = !(dims > 9000 && kpad > 96) && !(f->cfg.model == EKF_MODEL_ROTATIONS && kpad > 64);
    const bool want = (f->cfg.flags & 2) != 0 || ((f->cfg.flags & 1) == 0 && auto_on);
    return want && f->lay.has_cov2 && !f->timing && (f->cfg.flags & 4) == 0 && kpad <= 192 &&
           !wide_frame(f->cfg.model, m);      // (wide frames run in serial order)
}

// The device-side gates need the two streams on DIFFERENT hardware queues (HIP maps streams to a small pool
// of queues): a gate that shares its queue with the launch it waits for would wait for ever.  Probe once: a
// gate on the internal stream, the matching signal on the handle's stream, a short poll budget.
// HIP gives a new stream the hardware queue that carries the fewest streams, so when the probe fails a FRESH internal stream
// usually sits on another queue: up to sixteen are tried before the handle settles for the serial order.  The streams that
// failed stay alive until the probe is over: destroyed at once, each would leave the shared queue the emptiest again, and
// the next fresh stream would land on it again (seen when many streams of the process had come and gone before).
int probe_queues(ekf_filter* f) {
    if (f->la_ok >= 0) return EKF_OK;
    unsigned long long* probe = f->at<unsigned long long>(f->lay.off_sync) + 2;
    int32_t* pstat = f->at<int32_t>(f->lay.off_sync) + 8;
    std::vector<hipStream_t> failed;
    auto attempt = [&](bool fresh_stream) {
        if (fresh_stream) {
            hipStream_t fresh = nullptr;
            HIP_TRY(hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking));
            failed.push_back(f->big);
            f->big = fresh;
        }
        HIP_TRY(hipMemsetAsync(probe, 0, 64, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        ekf_launch_gate(probe, 1ull, pstat, f->big, 1 << 14);
        ekf_launch_signal(probe, 1ull, f->stream);
        HIP_TRY(hipStreamSynchronize(f->big));
        HIP_TRY(hipStreamSynchronize(f->stream));
        int32_t ps = 0;
        HIP_TRY(hipMemcpy(&ps, pstat, 4, hipMemcpyDeviceToHost));
        f->la_ok = (ps == 0) ? 1 : 0;
        return (int)EKF_OK;
    };
    f->la_ok = 0;
    int rc = EKF_OK;
    for (int i = 0; i < 16 && f->la_ok == 0 && rc == EKF_OK; ++i) rc = attempt(i > 0);
    for (hipStream_t s : failed) {      // (each was synchronised at the end of its own attempt)
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    return rc;
}

// one pipelining handle per process (see g_pipelining): take the token, or take it over from a handle whose streams
// have drained; false: run in serial order
bool take_pipelining_token(ekf_filter* f) {
    ekf_filter* owner = nullptr;
    if (!g_pipelining.compare_exchange_strong(owner, f) && owner != f) {
        bool idle = hipStreamQuery(owner->stream) == hipSuccess && hipStreamQuery(owner->big) == hipSuccess;
        (void)hipGetLastError();      // (hipErrorNotReady is not an error here)
        if (!(idle && g_pipelining.compare_exchange_strong(owner, f))) return false;
    }
    return true;
}

// Whether the runs of a call may pipeline (want_runs: the call has a run to pipeline): probe the queues, then take the token.
// *mode: the EKF_SEQ_* value that explains the outcome (ekf_last_sequence_mode), EKF_SEQ_PIPELINED if they may.
int choose_pipelining(ekf_filter* f, bool want_runs, int* mode) {
    *mode = EKF_SEQ_SERIAL;
    if (!want_runs || f->frozen) return EKF_OK;      // (a frozen map: frame by frame in serial order)
    int rc = probe_queues(f);
    if (rc) return rc;
    if (f->la_ok == 0) *mode = EKF_SEQ_SERIAL_ONE_QUEUE;
    else if (!take_pipelining_token(f)) *mode = EKF_SEQ_SERIAL_OTHER_HANDLE;
    else *mode = EKF_SEQ_PIPELINED;
    return EKF_OK;
}

// One frame of a pipelined run: its detections (device), their number, its trajectory row (or null).
struct RunFrame {
    const int32_t* idx;
    const double* z;
    int m;
    double* traj_row;
    const double* rows = nullptr;      // [m][rd] or null: per-detection noise
    double s_eff = 1.0;                // the frame's process-noise scale (pending part included)
};

// A run of `frames` >= 2 frames in the pipelined sequence mode; frame_at(t) describes frame t.  Every frame of a run has the
// same state dimension and the same kpad (rows rounded up to EKF_RB): a front kernel completes its support rows from the
// previous frame's W over ITS OWN kpad rows (ekf_front_impl.h: the S-block and chunk completions), and the support-column
// copy W_sup the previous frame leaves behind is [kpad][wsup_ld].  The number of detections may differ from frame to
// frame: next_m is separate from m, and the LDS claim and the grid are taken per frame.
// The covariance starts in f->cov and ping-pongs with `other`; f->cov is where it ends (`other` after an odd number of
// frames: run_frames copies it back at the end of the call).  Advances la_base by `frames`.
// One frame is a serial chain on one P, but the front kernel F(t+1) needs of P_{t+1}
// only its support rows (camera + the landmarks of frame t+1's detections), and those follow from P_t and W_t:
//     P_{t+1}[r][c] = (P_t[r][c] + Q[r == c]) + sum_k fma(-W_t[k][r], W_t[k][c])
// -- per element the instruction sequence of the covariance update, so the bits are the same.  The covariance
// therefore ping-pongs between two buffers: C(t) reads buf[t & 1] (P_t) and writes buf[(t + 1) & 1]; F(t+1) runs
// BESIDE C(t) on the other stream, reads P_t from buf[t & 1] and W_t, and completes the entries it needs itself
// (S-block workgroups: from the compact support columns W_sup the chunks of F(t) left behind; chunk workgroups:
// on the matrix cores).  Nothing on the critical path F(t) -> F(t+1) waits for a covariance update.
//   stream A (the handle's):  F(0) - F(1) - F(2) - ... - F(last) - C(last)
//   stream B (internal)    :  gate - C(0) - gate - C(1) - ...
// Edges between the streams are ordered on the device (an event pair costs ~13 us per edge):
//   F(t) complete   -> C(t) may start (it reads W_t and overwrites the buffer F(t) read, P_{t-1}): F(t+1) stores
//                      "t+1 started" when it starts (it follows F(t) on stream A); a one-wave gate kernel in front
//                      of C(t) polls that counter (the last update of a call follows its front kernel on stream A);
//   C(t-1) complete -> F(t+1) may read buf[t & 1] and overwrite W_{t-1}: C(t-1) stores a second counter ITSELF (no
//                      launch of its own, no kernel boundary in front of it: ekf_kernels.h, ekf_cov_arrive): every
//                      workgroup waits for the acknowledgement of its stores and counts itself, the last one stores
//                      the frame's value; F(t) does not finish before it has seen it (its measurement workgroup polls
//                      at its end), and F(t+1) follows F(t) on stream A.
// Memory ordering.  F(t) -> C(t): kernel boundaries (F(t) is over when F(t+1) starts, C(t) starts behind the gate).
// C(t-1) -> F(t+1): NOT a kernel boundary of stream B any more -- C(t-1) may still be a launch when the signal is out.
// The argument is: (1) every store to cov_out is a write-through (sc1) store (ekf_cov_store, cm_store16), and a wave
// counts as arrived only behind `s_waitcnt vmcnt(0)`, i.e. once its stores are acknowledged by the device's coherence
// point, so all of P_t is in memory before the signal is stored; (2) the consumer of the signal is the OPEN launch F(t),
// which reads nothing of P_t: the data is read only by LATER launches (F(t+1) on stream A, C(t) on stream B), whose
// kernel-start acquire drops whatever stale lines their L2s hold.  The W panel F(t+1) overwrites was read by C(t-1)
// before the stores that depend on it.  The counters only carry "those stores are complete".
// Every wait is bounded.  The front kernel claims (almost) all LDS of its CUs while its grid is small, so the
// covariance update's workgroups run on the other CUs instead of next to the pivot chain.
template <class FrameAt>
int run_pipelined(ekf_filter* f, int frames, FrameAt frame_at, void* other) {
    const Layout& L = f->lay;
    int rc = ensure_tiles(f);
    if (rc) return rc;
    void* wbuf[2] = {f->at<void>(L.off_wpanel), f->at<void>(L.off_wpanel2)};
    void* cbuf[2] = {f->cov, other};
    char* wsup0 = f->at<char>(L.off_wsup);
    void* wsup[2] = {wsup0, wsup0 + (size_t)L.kmax * L.wsup_ld * L.elem};
    unsigned long long* sync = f->at<unsigned long long>(L.off_sync);
    int32_t* status = f->at<int32_t>(L.off_status);
    const uint64_t base = f->la_base;
    f->shortcut.run();
    // (stream B needs no edge from stream A at the start: its first launch is the gate in front of C(0), which waits
    // for "F(1) has started", i.e. for everything that is on stream A now and F(0); the previous run ended with
    // stream A waiting for stream B)
    RunFrame nx = frame_at(0);
    EkfNoise nz_before{};      // the noise frame t - 1 ran with: what its covariance update adds to the diagonal
    for (int t = 0; t < frames; ++t) {
        const int par = t & 1;
        const RunFrame cf_t = nx;
        EkfFrame fr = make_frame(f, cf_t.idx, cf_t.z, cf_t.rows, cf_t.m, cf_t.traj_row, cf_t.s_eff);
        fr.cov = cbuf[0];
        fr.wpanel = wbuf[par];
        if (t > 0) {                                           // P_{t-1} + the completion from W_{t-1}, with Q_{t-1}
            fr.qprev_cam = nz_before.q_cam;
            fr.qprev_err = nz_before.q_err;
            fr.qprev_lm = nz_before.q_lm;
            fr.cov = cbuf[par ^ 1];
            fr.wprev = wbuf[par ^ 1];
            fr.wsup_prev = wsup[par ^ 1];
        }
        const int nb = fr.kpad / EKF_RB;
        const int grid = nb * (nb + 1) / 2 + 2 + fr.ncols / 64;
        fr.wsup_ld = L.wsup_ld;
        fr.la_sync = sync;
        fr.la_signal = (t > 0) ? base + (uint64_t)t : 0;       // "F(t) has started": F(t-1) is complete
        fr.la_gate = (t > 0) ? base + (uint64_t)t : 0;         // C(t-1) complete before F(t) ends
        fr.lds_min = grid <= 100 ? 148 * 1024 : 0;
        if (t + 1 < frames) {                                  // the next frame's detections: its support columns of W_t
            nx = frame_at(t + 1);
            fr.next_idx = nx.idx;
            fr.next_m = nx.m;
            fr.wsup = wsup[par];
        }
        bind_exchange(f, fr);
        by_cov_type(f, [&](auto elem) { ekf_launch_front<decltype(elem)>(fr, f->stream); });
        EkfFrame cu = fr;
        cu.cov = cbuf[par];
        cu.cov_out = cbuf[par ^ 1];
        if (t + 1 < frames) {
            ekf_launch_gate(sync, base + (uint64_t)t + 1, status, f->big);
            cu.cov_signal = base + (uint64_t)t + 1;            // "C(t) complete", stored by the update's last workgroup
            by_cov_type(f, [&](auto elem) { ekf_launch_cov_update<decltype(elem)>(cu, 2, f->big); });
        } else {
            // The LAST update of the run goes on the handle's stream, straight behind its front kernel: stream order says
            // that F(t) is over, and F(t) did not finish before it had seen C(t-1) complete (its end gate) -- no gate, no
            // signal (cov_signal stays 0: no atomic), and nothing to join afterwards (4 device-side hops of ~1.2 us per
            // call).  The counters keep the values of frame t - 1; the next run's waits are for values beyond
            // base + frames, which its own launches set.
            by_cov_type(f, [&](auto elem) { ekf_launch_cov_update<decltype(elem)>(cu, 2, f->stream); });
        }
        HIP_TRY(hipGetLastError());
        f->last_m = cf_t.m;
        nz_before = fr.nz;
    }
    f->cov = cbuf[frames & 1];
    f->la_base = base + (uint64_t)frames;
    return EKF_OK;
}

// Which frames of a call (ekf_observe_sequence_device, ekf_observe_log) may pipeline, in one pass: a run is >= 2 consecutive
// stepped frames that pipeline_wanted admits, of one kpad, none but the first with a first sighting (the front kernel clamps
// next-frame indices >= n_lm, and the new rows exist in neither covariance buffer).  m_of(t): the detections of frame t
// (0: not stepped); nnew_of(t): how many of them are first sightings.
struct RunPlan {
    std::vector<char> candidate;   // frame t may be in a run
    std::vector<char> joins;       // ... and continues the run of the stepped frame before it
    bool want_runs = false;        // some frame joins a run
};

template <class MOf, class NNewOf>
RunPlan plan_runs(const ekf_filter* f, int frames, MOf m_of, NNewOf nnew_of) {
    RunPlan p;
    p.candidate.assign((size_t)frames, 0);
    p.joins.assign((size_t)frames, 0);
    int prev_kpad = -1;          // kpad of the previous stepped frame if it was a candidate, else -1
    int nn = f->n_lm;
    for (int t = 0; t < frames; ++t) {
        const int m = m_of(t);
        if (m == 0) continue;
        const int nnew = nnew_of(t);
        nn += nnew;
        const int kpad = (int)round_up(f->lay.rd * m, EKF_RB);
        p.candidate[t] = pipeline_wanted(f, f->lay.lmd * nn + EKF_CAM, kpad, m);
        p.joins[t] = p.candidate[t] && nnew == 0 && prev_kpad == kpad;
        p.want_runs = p.want_runs || p.joins[t];
        prev_kpad = p.candidate[t] ? kpad : -1;
    }
    return p;
}

// Steps the frames of a call in order: the runs of `plan` in the pipelined mode if pipe_ok (choose_pipelining), every other
// stepped frame in serial order.  frame_of(t): frame t (m == 0: not stepped).  first_sightings(t): enqueues the add-marker
// launch of frame t's first sightings and returns their number; the run before the frame ends first, so that the new
// landmarks see the camera the previous frame left on the device.  stats (ekf_last_log_stats, or null): stepped frames,
// pipelined frames, runs, new landmarks.
// The covariance ping-pongs between the caller's buffer and the second one across runs: a run with an odd number of frames
// leaves it in the other buffer, and everything after it (serial frames, first sightings, the next run) works there; one
// copy at the end brings it back.
template <class FrameOf, class FirstSightings>
int run_frames(ekf_filter* f, int frames, FrameOf frame_of, FirstSightings first_sightings, const RunPlan& plan, bool pipe_ok,
               int64_t* stats) {
    void* const home = f->cov;
    void* const spare = f->lay.has_cov2 ? f->at<void>(f->lay.off_cov2) : nullptr;
    std::vector<int> run;
    auto serial = [&](int t) {
        const RunFrame r = frame_of(t);
        if (stats) stats[0] += 1;
        return enqueue_frame(f, r.idx, r.z, r.rows, r.m, r.traj_row, false, r.s_eff);
    };
    auto flush = [&]() -> int {
        int rc = EKF_OK;
        if (run.size() == 1) {
            rc = serial(run[0]);
        } else if (run.size() >= 2) {
            rc = run_pipelined(f, (int)run.size(), [&](int i) { return frame_of(run[i]); }, f->cov == home ? spare : home);
            if (stats) {
                stats[0] += (int64_t)run.size();
                stats[1] += (int64_t)run.size();
                stats[2] += 1;
            }
        }
        run.clear();
        return rc;
    };
    int rc = EKF_OK;
    for (int t = 0; t < frames && rc == EKF_OK; ++t) {
        if (frame_of(t).m == 0) continue;
        const bool in_run = pipe_ok && plan.candidate[t];
        if (!(in_run && plan.joins[t])) {
            rc = flush();
            if (rc) break;
        }
        const int nnew = first_sightings(t);
        f->n_lm += nnew;
        if (stats) stats[3] += nnew;
        if (in_run) run.push_back(t);
        else rc = serial(t);
    }
    if (rc == EKF_OK) rc = flush();
    if (f->cov != home) {
        // (also on an error: the caller's buffer is the filter's covariance again)
        hipError_t e = hipMemcpyAsync(home, f->cov, (size_t)f->lay.cap * f->lay.cap * f->lay.elem, hipMemcpyDeviceToDevice,
                                      f->stream);
        f->cov = home;
        if (e != hipSuccess && rc == EKF_OK) rc = fail(EKF_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
    }
    return rc;
}

// The pinned host buffers of a capacity (ekf_create, ekf_grow).  The readback mirror comes last: a failed allocation leaves
// every buffer large enough for the old capacity, and the mirror -- what a state getter may return without a copy -- as it was.
int reserve_host_buffers(ekf_filter* f, const Layout& L) {
    int rc = f->ring.reserve(L.slot_bytes * kStageSlots);
    if (rc == EKF_OK) rc = f->tiles_host.reserve((size_t)L.tiles_cap * 4);
    if (rc == EKF_OK) rc = f->readback.reserve(256 + (size_t)L.cap * 8);
    return rc;
}

// pinned host buffers, internal stream and events of a new handle
int open_handle(ekf_filter* f) {
    int rc = reserve_host_buffers(f, f->lay);
    if (rc) return rc;
    HIP_TRY(hipStreamCreateWithFlags(&f->big, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&f->ev_front, hipEventDisableTiming));
    for (hipEvent_t& e : f->slot_done) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (f->lay.has_gate) {
        if ((rc = f->gate_pin.reserve(256))) return rc;
        std::memset(f->gate_pin.get(), 0, 256);
        HIP_TRY(hipEventCreateWithFlags(&f->ev_gate, hipEventDisableTiming));
    }
    return EKF_OK;
}

// ---- the per-detection gate (include/ekf_slam_hip.h: ekf_set_gate) ---------------------------------------------------------
// One gated frame: the gate kernel on the frame's detections (device or pinned host pointers), a wait for the survivor count
// in the pinned mirror -- the one host round trip a gated frame costs --, then the ordinary frame on the compacted arrays:
// the same launches as the same call on the frame with the rejected detections deleted.  No survivor: nothing is stepped.
// exempt [m] (pinned host or device) or null; n_exempt: how many of them are set (statistics); mahal_dev / mahal_host [m] or
// null.  *survivors: how many detections stayed.
// rows [m][rd] or null: per-detection noise; the gate tests with them and compacts them with the survivors.
// s_eff: the frame's process-noise scale; the gate's S_d and the frame on the survivors use the same Q_eff.
int gated_frame(ekf_filter* f, const int32_t* idx, const double* z, const double* rows, int m, const uint8_t* exempt,
                int n_exempt, double* mahal_dev, double* mahal_host, double* traj_row, bool mirror, int* survivors,
                double s_eff) {
    const Layout& L = f->lay;
    EkfGateArgs g{};
    g.cov = f->cov;
    g.ld = f->ld;
    g.state = f->state;
    g.n_lm = f->n_lm;
    g.dims = f->dims();
    g.m = m;
    g.idx = idx;
    g.z = z;
    g.exempt = exempt;
    g.nz = frame_noise(f, s_eff);
    g.gate = f->gate;
    g.mahal = mahal_dev ? mahal_dev : f->at<double>(L.off_gmahal);
    g.mahal_host = mahal_host;
    g.out_idx = f->at<int32_t>(L.off_gidx);
    g.out_z = f->at<double>(L.off_gz);
    g.rows = rows;
    g.out_rows = rows ? f->at<double>(L.off_grow) : nullptr;
    g.status = f->at<int32_t>(L.off_status);
    g.status_host = f->readback.at<int32_t>(128);
    g.result_host = f->gate_pin.at<int32_t>(0);
    by_cov_type(f, [&](auto elem) { ekf_launch_frame_gate<decltype(elem)>(f->cfg.model, g, f->stream); });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(f->ev_gate, f->stream));
    HIP_TRY(hipEventSynchronize(f->ev_gate));
    const int s = *f->gate_pin.at<volatile int32_t>(0);
    if (s < 0 || s > m) return fail(EKF_ERR_STATE, "internal: survivor count of the gate kernel out of range");
    f->gate_stats[0] += m - n_exempt;
    f->gate_stats[1] += m - s;
    if (survivors) *survivors = s;
    if (s == 0) return EKF_OK;
    return enqueue_frame(f, g.out_idx, g.out_z, g.out_rows, s, traj_row, mirror, s_eff);
}

// Rules 3 and 4 of the per-frame scale (include/ekf_slam_hip.h), kept on the host.  `scale`: the frame's scale, or null: the
// frame carries none -- stepped, it runs with p + 1 (p = 0: the constants, the call as it ever was); not stepped, it leaves
// p alone.  A filter without EKF_FLAG_FRAME_SCALE has p = 0 and every frame runs with the constants.
double frame_scale(const ekf_filter* f, const double* scale) {
    return f->has_scale() ? f->pending + (scale ? *scale : 1.0) : 1.0;
}
void frame_scale_done(ekf_filter* f, const double* scale, double s_eff, bool stepped) {
    if (!f->has_scale()) return;
    if (stepped) f->pending = 0.0;
    else if (scale) f->pending = s_eff;
}
// scale [count] of a call (host, or null): the flag and the values, before anything is enqueued
int check_scales(const ekf_filter* f, const double* scale, int64_t count) {
    if (!scale) return EKF_OK;
    if (!f->has_scale()) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_FRAME_SCALE");
    for (int64_t i = 0; i < count; ++i)
        if (!scale_ok(scale[i])) return fail(EKF_ERR_INVALID, "a frame's scale must be finite and >= 0");
    return EKF_OK;
}

// motion [count][6] of a call (host, or null): the flag and the values, before anything is enqueued
int check_motions(const ekf_filter* f, const double* motion, int64_t count) {
    if (!motion) return EKF_OK;
    if (!f->has_motion()) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_MOTION");
    for (int64_t i = 0; i < 6 * count; ++i)
        if (!std::isfinite(motion[i])) return fail(EKF_ERR_INVALID, "a motion must be finite");
    return EKF_OK;
}

// The motion of one frame (include/ekf_slam_hip.h, the motion rules): null, or six exact zeros: nothing is enqueued (bit
// rule 6(a)).  Otherwise the launch of ekf_motion.hip on the handle's stream, behind everything the frame before left there
// (a frame that is not stepped takes its trajectory row from the state afterwards: repeat_row).  Returns whether something
// was enqueued in *moved (or null).
int enqueue_motion(ekf_filter* f, const double* u, bool* moved = nullptr) {
    if (moved) *moved = false;
    if (!u) return EKF_OK;
    bool zero = true;
    for (int i = 0; i < 6; ++i) zero = zero && u[i] == 0.0;
    if (zero) return EKF_OK;
    EkfMotionArgs a{};
    a.cov = f->cov;
    a.ld = f->ld;
    a.state = f->state;
    a.dims = f->dims();
    for (int i = 0; i < 6; ++i) a.u[i] = u[i];
    a.status = f->at<int32_t>(f->lay.off_status);
    by_cov_type(f, [&](auto elem) { ekf_launch_motion<decltype(elem)>(a, f->stream); });
    HIP_TRY(hipGetLastError());
    f->shortcut.moved();
    if (moved) *moved = true;
    return EKF_OK;
}

// trajectory row of a frame that is not stepped: the camera state as it is on the device
int repeat_row(ekf_filter* f, double* traj_row) {
    if (traj_row) HIP_TRY(hipMemcpyAsync(traj_row, f->state, 7 * 8, hipMemcpyDeviceToDevice, f->stream));
    return EKF_OK;
}

// A gated frame of a sequence or of a log (device arrays, no host mirror): the frame on its survivors, or, with none left,
// its trajectory row alone
int gated_frame_or_row(ekf_filter* f, const int32_t* idx, const double* z, const double* rows, int m, const uint8_t* exempt,
                       int n_exempt, double* mahal_dev, double* traj_row, int* survivors, double s_eff) {
    const int rc = gated_frame(f, idx, z, rows, m, exempt, n_exempt, mahal_dev, nullptr, traj_row, false, survivors, s_eff);
    return rc == EKF_OK && *survivors == 0 ? repeat_row(f, traj_row) : rc;
}

// ekf_observe / ekf_observe_gated: the frame's detections (host) through a slot of the pinned staging ring
// rows [m][rd] (host) or null: per-detection noise, staged behind everything else of the slot
// scale: the frame's process-noise scale, or null (checked by the caller: check_scales)
// motion: the frame's camera motion [6], or null (checked by the caller: check_motions); applied once the frame has passed
// every check, in front of the gate
int observe_host(ekf_filter* f, const int32_t* lm_index, const double* z, const double* rows, int32_t m, bool gated,
                 const uint8_t* exempt, double* mahal, int32_t* survivors, const double* scale = nullptr,
                 const double* motion = nullptr) {
    if (m < 1) return fail(EKF_ERR_INVALID, "observe needs at least one detection");
    if (m > f->cfg.max_visible) return fail(EKF_ERR_CAPACITY, "more detections than max_visible");
    if (!lm_index || !z) return fail(EKF_ERR_INVALID, "NULL detections");
    for (int i = 0; i < m; ++i)
        if (lm_index[i] < 0 || lm_index[i] >= f->n_lm)
            return fail(EKF_ERR_INVALID, "landmark index out of range");
    const Layout& L = f->lay;
    if (rows) {
        if (!L.has_rows) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_ROW_NOISE");
        for (size_t i = 0; i < (size_t)m * L.rd; ++i)
            if (!(rows[i] > 0.0) || !std::isfinite(rows[i]))
                return fail(EKF_ERR_INVALID, "a row variance must be finite and > 0");
    }
    char* slot = f->ring.get() + (size_t)f->slot * L.slot_bytes;
    HIP_TRY(hipEventSynchronize(f->slot_done[f->slot]));
    int32_t* hidx = reinterpret_cast<int32_t*>(slot);
    double* hz = reinterpret_cast<double*>(slot + align256((size_t)f->cfg.max_visible * 4));
    const size_t zb = (size_t)m * L.rd * 8;
    std::memcpy(hidx, lm_index, (size_t)m * 4);
    std::memcpy(hz, z, zb);
    double* hrows = nullptr;
    if (rows) {
        hrows = reinterpret_cast<double*>(slot + L.slot_rows);
        std::memcpy(hrows, rows, zb);
    }
    // one copy: the pinned slot mirrors the device staging layout [indices, padded to 256 B | z]
    static_assert(sizeof(int32_t) == 4, "layout");
    if (L.off_z - L.off_idx != align256((size_t)f->cfg.max_visible * 4)) return fail(EKF_ERR_STATE, "staging layout");
    // The kernels read the frame's detections (128 + 768 bytes at m = 32) straight from the pinned slot: a host-to-device
    // copy in front of them costs more (API call + DMA start, ~8 us before the front kernel begins) than the PCIe reads
    // cost the kernel's first round trip.  The slot is not reused before this frame's event (64-slot ring).
    int rc = enqueue_motion(f, motion);
    if (rc) return rc;
    const double s_eff = frame_scale(f, scale);
    if (gated) {
        uint8_t* hex = nullptr;
        int n_exempt = 0;
        if (exempt) {
            hex = reinterpret_cast<uint8_t*>(slot + L.slot_exempt);
            std::memcpy(hex, exempt, (size_t)m);
            for (int i = 0; i < m; ++i) n_exempt += exempt[i] != 0;
        }
        double* hm = mahal ? reinterpret_cast<double*>(slot + L.slot_mahal) : nullptr;
        int s = 0;
        rc = gated_frame(f, hidx, hz, hrows, m, hex, n_exempt, nullptr, hm, nullptr, true, &s, s_eff);
        if (rc) return rc;
        if (mahal) std::memcpy(mahal, hm, (size_t)m * 8);      // (complete: the gate kernel's event has been waited for)
        if (survivors) *survivors = s;
        frame_scale_done(f, scale, s_eff, s > 0);      // (no survivor: the frame is not stepped, its scale stays pending)
    } else {
        rc = enqueue_frame(f, hidx, hz, hrows, m, nullptr, true, s_eff);
        if (rc) return rc;
        frame_scale_done(f, scale, s_eff, true);
    }
    HIP_TRY(hipEventRecord(f->slot_done[f->slot], f->stream));
    f->slot = (f->slot + 1) % kStageSlots;
    return EKF_OK;
}

// A fresh workspace, in two steps.  clear_buffers enqueues it on the handle's stream: covariance, state and workspace zero
// (capacity padding stays exactly zero), the exchange buffers of the fused front kernel armed (ekf_solve_device.h:
// EKF_SENT_BITS) -- ekf_reset on the handle's buffers, ekf_grow on the new ones before it copies the old contents in.
// restart_workspace follows once the workspace is the handle's and the stream is idle: everything that counts frames in
// it starts again (the macro-tile table with it), and the pinned mirror is zero.
int clear_buffers(const ekf_filter* f, void* cov, double* state, char* ws, const Layout& L) {
    HIP_TRY(hipMemsetAsync(cov, 0, (size_t)L.cap * L.cap * L.elem, f->stream));
    HIP_TRY(hipMemsetAsync(state, 0, (size_t)L.cap * 8, f->stream));
    HIP_TRY(hipMemsetAsync(ws, 0, L.total, f->stream));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws + L.off_xl), (int)0xFFFBADC0u, L.xl_len * 4, f->stream));
    return EKF_OK;
}

void restart_workspace(ekf_filter* f) {
    f->fseq = 0;
    f->done_total = 0;
    f->la_base = 0;
    f->tiles_T = -1;
    std::memset(f->readback.get(), 0, 256 + (size_t)f->lay.cap * 8);
}

}  // namespace

extern "C" {

const char* ekf_last_error_string(void) { return g_err.c_str(); }

int ekf_default_config(ekf_config* cfg) {
    if (!cfg) return fail(EKF_ERR_INVALID, "config is NULL");
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->max_landmarks = 50;   // DICT_5X5_50, base_filter.py:81-82
    cfg->max_visible = 50;
    cfg->cov_dtype = EKF_COV_F64;
    cfg->quat_mode = EKF_QUAT_AS_WRITTEN;
    cfg->cov_kernel = EKF_COVK_AUTO;
    cfg->model = EKF_MODEL_EKF;
    cfg->initial_camera_uncertainty = 0.1;
    cfg->initial_landmark_uncertainty = 0.7;
    cfg->r_uncertainty = 0.9;
    cfg->q_cam = 0.3;
    cfg->q_err = 0.5;
    cfg->q_lm = 0.01;
    cfg->stream = nullptr;
    return EKF_OK;
}

int ekf_query_sizes(const ekf_config* cfg, int64_t* ld, size_t* cov_bytes, size_t* state_bytes,
                    size_t* workspace_bytes) {
    int rc = check_config(cfg);
    if (rc) return rc;
    Layout L = make_layout(*cfg);
    if (ld) *ld = L.cap;
    if (cov_bytes) *cov_bytes = (size_t)L.cap * L.cap * L.elem;
    if (state_bytes) *state_bytes = (size_t)L.cap * 8;
    if (workspace_bytes) *workspace_bytes = L.total;
    return EKF_OK;
}

int ekf_create(const ekf_config* cfg, ekf_filter** out) {
    int rc = check_config(cfg);
    if (rc) return rc;
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(EKF_ERR_HIP, "no HIP device visible");
    ekf_filter* f = new ekf_filter();
    if (hipGetDevice(&f->device) != hipSuccess) f->device = 0;   // the caller's current device
    f->cfg = *cfg;
    f->lay = make_layout(*cfg);
    f->stream = static_cast<hipStream_t>(cfg->stream);
    rc = open_handle(f);
    if (rc) {
        ekf_destroy(f);
        return rc;
    }
    *out = f;
    return EKF_OK;
}

int ekf_destroy(ekf_filter* f) {
    if (!f) return EKF_OK;
    (void)hipStreamSynchronize(f->stream);
    if (f->big) {
        (void)hipStreamSynchronize(f->big);
        (void)hipStreamDestroy(f->big);
    }
    release_pipelining_token(f);
    if (f->ev_front) (void)hipEventDestroy(f->ev_front);
    if (f->ev_gate) (void)hipEventDestroy(f->ev_gate);
    for (auto& e : f->remove_done)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : f->ev) (void)hipEventDestroy(e);
    for (int i = 0; i < kStageSlots; ++i)
        if (f->slot_done[i]) (void)hipEventDestroy(f->slot_done[i]);
    for (auto& e : f->log_pin_done)
        if (e) (void)hipEventDestroy(e);
    delete f;      // (the pinned buffers with it)
    return EKF_OK;
}

int ekf_bind_buffers(ekf_filter* f, void* cov_dev, int64_t ld, double* state_dev, void* workspace_dev,
                     size_t workspace_bytes) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    int rc = check_device_buffers({cov_dev, state_dev, workspace_dev}, workspace_bytes, f->lay.total, "ekf_query_sizes");
    if (rc) return rc;
    if (ld != f->lay.cap) return fail(EKF_ERR_INVALID, "ld must equal the value from ekf_query_sizes");
    f->cov = cov_dev;
    f->ld = ld;
    f->state = state_dev;
    f->ws = static_cast<char*>(workspace_dev);
    f->bound = true;
    f->is_reset = false;
    f->tiles_T = -1;
    return EKF_OK;
}

int ekf_grow(ekf_filter* f, int32_t new_max_landmarks, int32_t new_max_visible, void* cov_dev, int64_t ld, double* state_dev,
             void* workspace_dev, size_t workspace_bytes) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!f->bound || !f->is_reset) return fail(EKF_ERR_STATE, "ekf_grow needs a bound, reset filter");
    if (new_max_landmarks < f->cfg.max_landmarks || new_max_visible < f->cfg.max_visible)
        return fail(EKF_ERR_INVALID, "ekf_grow cannot shrink the capacity");
    ekf_config ncfg = f->cfg;
    ncfg.max_landmarks = new_max_landmarks;
    ncfg.max_visible = new_max_visible;
    int rc = check_config(&ncfg);
    if (rc) return rc;
    const Layout nl = make_layout(ncfg);
    rc = check_device_buffers({cov_dev, state_dev, workspace_dev}, workspace_bytes, nl.total,
                              "ekf_query_sizes for the new capacity");
    if (rc) return rc;
    if (ld != nl.cap) return fail(EKF_ERR_INVALID, "ld must equal the value from ekf_query_sizes for the new capacity");
    if (cov_dev == f->cov || state_dev == f->state || workspace_dev == static_cast<void*>(f->ws))
        return fail(EKF_ERR_INVALID, "ekf_grow needs NEW buffers (the old ones are read)");
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipStreamSynchronize(f->stream));
    HIP_TRY(hipStreamSynchronize(f->big));
    release_pipelining_token(f);
    const Layout& ol = f->lay;
    char* nws = static_cast<char*>(workspace_dev);
    // new buffers: zero (capacity padding stays exactly zero), exchange buffers armed, then the old contents
    rc = clear_buffers(f, cov_dev, state_dev, nws, nl);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(state_dev, f->state, (size_t)ol.cap * 8, hipMemcpyDeviceToDevice, f->stream));
    HIP_TRY(hipMemcpy2DAsync(cov_dev, (size_t)nl.cap * nl.elem, f->cov, (size_t)ol.cap * ol.elem, (size_t)ol.cap * ol.elem,
                             (size_t)ol.cap, hipMemcpyDeviceToDevice, f->stream));
    HIP_TRY(hipMemcpyAsync(nws + nl.off_status, f->ws + ol.off_status, 32, hipMemcpyDeviceToDevice, f->stream));   // (sticky bits stay)
    HIP_TRY(hipStreamSynchronize(f->stream));
    // (every slot's event is complete: the stream has just been synchronised.  On failure the filter goes on at the old
    // capacity: nothing of it has changed but the size of some pinned buffers.)
    rc = reserve_host_buffers(f, nl);
    if (rc) return rc;
    f->cfg = ncfg;
    f->lay = nl;
    f->cov = cov_dev;
    f->ld = ld;
    f->state = state_dev;
    f->ws = nws;
    restart_workspace(f);
    f->shortcut.new_workspace();
    return EKF_OK;
}

int ekf_remove_workspace_bytes(const ekf_filter* f, int32_t count, size_t* bytes) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!bytes || count < 0) return fail(EKF_ERR_INVALID, "bad removal size request");
    *bytes = align256((size_t)f->lay.cap * 4);      // the index map [cap], whatever the count
    return EKF_OK;
}

// Semantics: include/ekf_slam_hip.h.  Everything is checked before anything is enqueued or rebound; then, on the handle's
// stream: the index map (pinned staging -> remove_ws) and ONE launch: the gather into the new buffers, the fringe of the
// second covariance buffer, the pinned mirror of the state.
int ekf_remove_markers(ekf_filter* f, const int32_t* lm_index, int32_t count, void* cov_dev_new, int64_t ld,
                       double* state_dev_new, void* remove_ws, size_t remove_ws_bytes) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (count < 0 || (count > 0 && !lm_index)) return fail(EKF_ERR_INVALID, "bad removal list");
    const Layout& L = f->lay;
    const size_t need = align256((size_t)L.cap * 4);
    rc = check_device_buffers({cov_dev_new, state_dev_new, remove_ws}, need, need, "ekf_remove_workspace_bytes");
    if (rc) return rc;
    if (ld != L.cap) return fail(EKF_ERR_INVALID, "ld must equal the value from ekf_query_sizes");
    if (cov_dev_new == f->cov || state_dev_new == f->state)
        return fail(EKF_ERR_INVALID, "ekf_remove_markers needs NEW buffers (the old ones are read)");
    if (remove_ws_bytes < need) return fail(EKF_ERR_CAPACITY, "remove_ws smaller than ekf_remove_workspace_bytes");
    std::vector<int32_t> sorted;
    const std::string bad = ekf_remove_build_map(lm_index, count, f->n_lm, L.lmd, L.cap, nullptr, sorted);
    if (!bad.empty()) return fail(EKF_ERR_INVALID, bad);
    if (count == 0) return EKF_OK;
    const int turn = f->remove_turn;
    PinnedBuffer& pin = f->remove_pin[turn];
    hipEvent_t& done = f->remove_done[turn];
    if ((rc = pin.reserve(need))) return rc;
    if (!done) HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    HIP_TRY(hipEventSynchronize(done));      // (the upload of the call before the previous one: long complete in practice)
    (void)ekf_remove_build_map(lm_index, count, f->n_lm, L.lmd, L.cap, pin.at<int32_t>(0), sorted);
    HIP_TRY(hipMemcpyAsync(remove_ws, pin.get(), (size_t)L.cap * 4, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipEventRecord(done, f->stream));
    f->remove_turn = turn ^ 1;
    const int64_t n_old = f->dims(), n_new = n_old - (int64_t)L.lmd * count;
    EkfRemoveArgs a{};
    a.cov_src = f->cov;
    a.cov_dst = cov_dev_new;
    a.state_src = f->state;
    a.state_dst = state_dev_new;
    a.ld = L.cap;
    a.map = static_cast<const int32_t*>(remove_ws);
    // the whole new state also goes into the pinned mirror (what the front kernel does every frame), and the second
    // covariance buffer of the pipelined mode, zero beyond the (rounded) state dimension and rewritten inside it by every
    // pipelined run (ekf_set_cov), gets the rows and columns the map has just lost back to zero
    a.state_host = f->readback.at<double>(256);
    a.n_new = (int32_t)n_new;
    if (L.has_cov2) {
        a.cov2 = f->at<void>(L.off_cov2);
        a.fringe_hi = (int32_t)std::min<int64_t>(round_up(n_old, 128), L.cap);
    }
    by_cov_type(f, [&](auto elem) { ekf_launch_remove<decltype(elem)>(a, 1, f->stream); });
    HIP_TRY(hipGetLastError());
    f->shortcut.removed();
    f->hist.valid = false;      // (the records no longer describe this filter's map)
    f->cov = cov_dev_new;
    f->state = state_dev_new;
    f->n_lm -= count;
    return EKF_OK;
}

int ekf_reset(ekf_filter* f, const double initial_camera_pose[10]) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!f->bound) return fail(EKF_ERR_STATE, "ekf_bind_buffers has not been called");
    if (!initial_camera_pose) return fail(EKF_ERR_INVALID, "initial pose is NULL");
    HIP_TRY(hipSetDevice(f->device));
    const Layout& L = f->lay;
    HIP_TRY(hipStreamSynchronize(f->stream));
    int rc = clear_buffers(f, f->cov, f->state, f->ws, L);
    if (rc) return rc;
    restart_workspace(f);          // (the stream is idle: synchronised above)
    f->shortcut.reset();
    HIP_TRY(hipMemcpyAsync(f->state, initial_camera_pose, 10 * sizeof(double), hipMemcpyHostToDevice,
                           f->stream));
    // P = 0.1 I_10  (extended_kalman_filter.py:48)
    char diag[8 * EKF_CAM];
    by_cov_type(f, [&](auto elem) {
        for (int i = 0; i < EKF_CAM; ++i)
            reinterpret_cast<decltype(elem)*>(diag)[i] = (decltype(elem))f->cfg.initial_camera_uncertainty;
    });
    HIP_TRY(hipMemcpy2DAsync(f->cov, (size_t)(L.cap + 1) * L.elem, diag, L.elem, L.elem, EKF_CAM,
                             hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    f->n_lm = 0;
    f->last_m = 0;
    f->pending = 0.0;
    f->frozen = false;      // (a reset filter has no map)
    f->hist.valid = false;
    f->is_reset = true;
    return EKF_OK;
}

int ekf_add_markers(ekf_filter* f, const double* cam_frame_xyz, const double* diag_uncertainty,
                    int32_t count) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (count < 0 || (count > 0 && !cam_frame_xyz)) return fail(EKF_ERR_INVALID, "bad marker list");
    if (f->n_lm + count > f->cfg.max_landmarks)
        return fail(EKF_ERR_CAPACITY, "more landmarks than max_landmarks");
    const Layout& L = f->lay;
    f->shortcut.markers_added();
    int done = 0;
    while (done < count) {
        const int chunk = std::min(256, count - done);
        char* slot = f->ring.get() + (size_t)f->slot * L.slot_bytes;
        HIP_TRY(hipEventSynchronize(f->slot_done[f->slot]));
        double* hx = reinterpret_cast<double*>(slot);
        double* hu = reinterpret_cast<double*>(slot + align256(256 * 48));
        const bool rot = f->cfg.model == EKF_MODEL_ROTATIONS;
        const size_t pb = rot ? 48 : 24, ub = rot ? 80 : 24;      // bytes per marker: pose / variances
        std::memcpy(hx, cam_frame_xyz + (pb / 8) * done, (size_t)chunk * pb);
        if (diag_uncertainty) std::memcpy(hu, diag_uncertainty + (ub / 8) * done, (size_t)chunk * ub);
        HIP_TRY(hipMemcpyAsync(f->at<double>(L.off_xyz), hx, (size_t)chunk * pb, hipMemcpyHostToDevice,
                               f->stream));
        if (diag_uncertainty)
            HIP_TRY(hipMemcpyAsync(f->at<double>(L.off_unc), hu, (size_t)chunk * ub,
                                   hipMemcpyHostToDevice, f->stream));
        const double* unc_dev = diag_uncertainty ? f->at<double>(L.off_unc) : nullptr;
        by_cov_type(f, [&](auto elem) {
            auto* launch = rot ? ekf_launch_add_markers_rot<decltype(elem)> : ekf_launch_add_markers<decltype(elem)>;
            launch(f->cov, f->ld, f->state, f->dims(), f->at<double>(L.off_xyz), unc_dev, f->cfg.initial_landmark_uncertainty,
                   chunk, f->stream);
        });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(f->slot_done[f->slot], f->stream));
        f->slot = (f->slot + 1) % kStageSlots;
        f->n_lm += chunk;
        done += chunk;
    }
    return EKF_OK;
}

int ekf_observe(ekf_filter* f, const int32_t* lm_index, const double* z, int32_t m) {
    int rc = check_ready(f);
    if (rc) return rc;
    f->reset_gate_stats();
    return observe_host(f, lm_index, z, nullptr, m, f->gate_on(), nullptr, nullptr, nullptr);
}

int ekf_observe_gated(ekf_filter* f, const int32_t* lm_index, const double* z, int32_t m, const uint8_t* exempt, double* mahal,
                      int32_t* survivors) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (!f->lay.has_gate) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_GATE");
    f->reset_gate_stats();
    const bool gated = f->gate_on() || mahal;
    rc = observe_host(f, lm_index, z, nullptr, m, gated, exempt, mahal, survivors);
    if (rc == EKF_OK && !gated && survivors) *survivors = m;
    return rc;
}

namespace {
int observe_rows_scaled(ekf_filter* f, const int32_t* lm_index, const double* z, const double* rows, int32_t m,
                        const uint8_t* exempt, double* mahal, int32_t* survivors, const double* scale,
                        const double* motion = nullptr) {
    int rc = check_ready(f);
    if (rc) return rc;
    if ((exempt || mahal) && !f->lay.has_gate) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_GATE");
    if ((rc = check_scales(f, scale, 1))) return rc;
    if ((rc = check_motions(f, motion, 1))) return rc;
    f->reset_gate_stats();
    const bool gated = f->gate_on() || mahal;
    rc = observe_host(f, lm_index, z, rows, m, gated, exempt, mahal, survivors, scale, motion);
    if (rc == EKF_OK && !gated && survivors) *survivors = m;
    return rc;
}
}  // namespace

int ekf_observe_rows(ekf_filter* f, const int32_t* lm_index, const double* z, const double* rows, int32_t m,
                     const uint8_t* exempt, double* mahal, int32_t* survivors) {
    return observe_rows_scaled(f, lm_index, z, rows, m, exempt, mahal, survivors, nullptr);
}

int ekf_observe_scaled(ekf_filter* f, const int32_t* lm_index, const double* z, const double* rows, int32_t m,
                       const uint8_t* exempt, double* mahal, int32_t* survivors, double scale) {
    return observe_rows_scaled(f, lm_index, z, rows, m, exempt, mahal, survivors, &scale);
}

int ekf_observe_moved(ekf_filter* f, const int32_t* lm_index, const double* z, const double* rows, int32_t m,
                      const uint8_t* exempt, double* mahal, int32_t* survivors, double scale, const double* motion) {
    return observe_rows_scaled(f, lm_index, z, rows, m, exempt, mahal, survivors, &scale, motion);
}

int ekf_move(ekf_filter* f, const double motion[6]) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (!motion) return fail(EKF_ERR_INVALID, "motion is NULL");
    if ((rc = check_motions(f, motion, 1))) return rc;
    return enqueue_motion(f, motion);
}

int ekf_advance(ekf_filter* f, double scale) {
    int rc = check_ready(f);
    if (rc) return rc;
    if ((rc = check_scales(f, &scale, 1))) return rc;
    f->pending = f->pending + scale;
    return EKF_OK;
}

int ekf_get_pending_scale(const ekf_filter* f, double* out) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    *out = f->pending;
    return EKF_OK;
}

int ekf_set_pending_scale(ekf_filter* f, double pending) {
    int rc = check_ready(f);
    if (rc) return rc;
    if ((rc = check_scales(f, &pending, 1))) return rc;
    f->pending = pending;
    return EKF_OK;
}

int ekf_set_gate(ekf_filter* f, double gate) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!f->lay.has_gate) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_GATE");
    if (!(gate > 0.0)) return fail(EKF_ERR_INVALID, "the gate must be > 0 (+inf: off) and not NaN");
    f->gate = gate;
    return EKF_OK;
}

int ekf_last_gate_stats(const ekf_filter* f, int64_t out[2]) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    out[0] = f->gate_stats[0];
    out[1] = f->gate_stats[1];
    return EKF_OK;
}

int ekf_observe_device(ekf_filter* f, const int32_t* lm_index_dev, const double* z_dev, int32_t m) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (m < 1) return fail(EKF_ERR_INVALID, "observe needs at least one detection");
    if (m > f->cfg.max_visible) return fail(EKF_ERR_CAPACITY, "more detections than max_visible");
    if (!lm_index_dev || !z_dev) return fail(EKF_ERR_INVALID, "NULL detections");
    if (f->n_lm < 1) return fail(EKF_ERR_STATE, "observe before any landmark was added");
    // the indices are device-resident: range-checked by the kernels (EKF_ERR_INVALID at the next sync)
    f->reset_gate_stats();
    const double s_eff = frame_scale(f, nullptr);
    int s = m;
    rc = f->gate_on() ? gated_frame(f, lm_index_dev, z_dev, nullptr, m, nullptr, 0, nullptr, nullptr, nullptr, true, &s, s_eff)
                      : enqueue_frame(f, lm_index_dev, z_dev, nullptr, m, nullptr, true, s_eff);
    if (rc == EKF_OK) frame_scale_done(f, nullptr, s_eff, s > 0);
    return rc;
}

int ekf_observe_sequence_device(ekf_filter* f, const int32_t* lm_index_dev, const double* z_dev,
                                int32_t m, int32_t frames, double* trajectory_dev) {
    return ekf_observe_sequence_device_rows(f, lm_index_dev, z_dev, nullptr, m, frames, trajectory_dev);
}

int ekf_observe_sequence_device_rows(ekf_filter* f, const int32_t* lm_index_dev, const double* z_dev, const double* rows_dev,
                                     int32_t m, int32_t frames, double* trajectory_dev) {
    return ekf_observe_sequence_device_scaled(f, lm_index_dev, z_dev, rows_dev, nullptr, m, frames, trajectory_dev);
}

int ekf_observe_sequence_device_scaled(ekf_filter* f, const int32_t* lm_index_dev, const double* z_dev, const double* rows_dev,
                                       const double* scale, int32_t m, int32_t frames, double* trajectory_dev) {
    return ekf_observe_sequence_device_moved(f, lm_index_dev, z_dev, rows_dev, scale, nullptr, m, frames, trajectory_dev);
}

int ekf_observe_sequence_device_moved(ekf_filter* f, const int32_t* lm_index_dev, const double* z_dev, const double* rows_dev,
                                      const double* scale, const double* motion, int32_t m, int32_t frames,
                                      double* trajectory_dev) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (rows_dev && !f->lay.has_rows) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_ROW_NOISE");
    if (m < 1 || frames < 0) return fail(EKF_ERR_INVALID, "bad sequence shape");
    if ((rc = check_scales(f, scale, frames))) return rc;
    if ((rc = check_motions(f, motion, frames))) return rc;
    if (m > f->cfg.max_visible) return fail(EKF_ERR_CAPACITY, "more detections than max_visible");
    if (!lm_index_dev || !z_dev) return fail(EKF_ERR_INVALID, "NULL detections");
    if (f->n_lm < 1) return fail(EKF_ERR_STATE, "observe before any landmark was added");
    const int rd = f->lay.rd;
    f->reset_gate_stats();
    if (f->gate_on() || motion || f->frozen) {
        // a frozen map: frame by frame in serial order, the camera strip behind every front part.
        // a gate is set: frame by frame in serial order, each frame on its survivors (gating inside a pipelined run would
        // need the mask inside the front kernel).  Motions: serial order as well -- a front kernel of a run completes
        // P_{t+1} from P_t and W_t, and a motion between the two frames changes rows of it
        f->seq_mode = EKF_SEQ_SERIAL;
        f->shortcut.log();      // (a getter after the call waits for all of it)
        for (int t = 0; t < frames; ++t) {
            int s = m;
            const double* sc = scale ? scale + t : nullptr;
            if ((rc = enqueue_motion(f, motion ? motion + (size_t)t * 6 : nullptr))) return rc;
            const double s_eff = frame_scale(f, sc);
            const int32_t* idx_t = lm_index_dev + (size_t)t * m;
            const double* z_t = z_dev + (size_t)t * m * rd;
            const double* rows_t = rows_dev ? rows_dev + (size_t)t * m * rd : nullptr;
            double* row_t = trajectory_dev ? trajectory_dev + (size_t)t * 7 : nullptr;
            rc = f->gate_on() ? gated_frame_or_row(f, idx_t, z_t, rows_t, m, nullptr, 0, nullptr, row_t, &s, s_eff)
                              : enqueue_frame(f, idx_t, z_t, rows_t, m, row_t, false, s_eff);
            if (rc) return rc;
            frame_scale_done(f, sc, s_eff, s > 0);
        }
        f->shortcut.log();
        return EKF_OK;
    }
    // every frame is stepped: the pending scale goes into the first one (rule 3), and none is left
    std::vector<double> s_effs((size_t)frames, 1.0);
    for (int t = 0; t < frames; ++t) {
        s_effs[t] = frame_scale(f, scale ? scale + t : nullptr);
        frame_scale_done(f, scale ? scale + t : nullptr, s_effs[t], true);
    }
    // Pipelined mode (F(t+1) beside C(t), see run_pipelined) for the whole call if pipeline_wanted admits the frame shape
    const RunPlan plan = plan_runs(f, frames, [&](int) { return m; }, [](int) { return 0; });
    int mode = EKF_SEQ_SERIAL;
    rc = choose_pipelining(f, plan.want_runs, &mode);
    if (rc) return rc;
    f->seq_mode = mode == EKF_SEQ_PIPELINED ? EKF_SEQ_SERIAL : mode;     // (PIPELINED once the run is enqueued)
    rc = run_frames(
        f, frames,
        [&](int t) {
            return RunFrame{lm_index_dev + (size_t)t * m, z_dev + (size_t)t * m * rd, m,
                            trajectory_dev ? trajectory_dev + (size_t)t * 7 : nullptr,
                            rows_dev ? rows_dev + (size_t)t * m * rd : nullptr, s_effs[t]};
        },
        [](int) { return 0; }, plan, mode == EKF_SEQ_PIPELINED, nullptr);
    if (rc) return rc;
    f->seq_mode = mode;
    return EKF_OK;
}

// ---- log replay (BaseFilter.process_detections over a whole log): ekf_observe_log ---------------------------------------
}  // extern "C"

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

// ---- offline smoothing: what is supported, and the sizes of a history ----------------------------------------------------
// (include/ekf_slam_hip.h, "Offline smoothing": the refusals)
int smoothing_supported(const ekf_filter* f) {
    if (f->cfg.model != EKF_MODEL_EKF) return fail(EKF_ERR_STATE, "smoothing: EKF_MODEL_ROTATIONS is not supported");
    if (f->cfg.cov_dtype != EKF_COV_F64) return fail(EKF_ERR_STATE, "smoothing needs the f64 covariance");
    if (f->cfg.quat_mode != EKF_QUAT_SCALAR_FIRST)
        return fail(EKF_ERR_STATE, "smoothing needs EKF_QUAT_SCALAR_FIRST (the as-written injection has no inverse)");
    if (f->frozen) return fail(EKF_ERR_STATE, "smoothing: the map is frozen");
    return EKF_OK;
}

// one record: state [dims] and the packed lower triangle, f64, in a 256-byte aligned piece
size_t history_record_bytes(int64_t dims) { return align256((size_t)(dims + dims * (dims + 1) / 2) * 8); }

// upper bound from the log alone: the header and one record per frame at the dims that frame ends with
void history_bound(int lmd, int n_lm, const LogCheck& lc, int64_t frames, size_t* bytes) {
    size_t total = 256;
    for (int64_t t = 0; t < frames; ++t) total += history_record_bytes(EKF_CAM + (int64_t)lmd * (n_lm + lc.new_at[t + 1]));
    *bytes = total;
}

// smoothing workspace: [status 256 | table | xs | xp | yv | wv | cv | xinv | M], the vectors and M sized by the largest record
// rounded up to whole block columns (the resident tier uses the first two pieces only)
struct SmoothLayout {
    size_t table, xs, xp, yv, wv, cv, xinv, M, total;
};
SmoothLayout smooth_layout(size_t records, int64_t nmax) {
    const size_t npad = (size_t)round_up(std::max<int64_t>(nmax, 1), EKF_WIDE_BLOCK);
    Carve w;
    w.take(256);
    SmoothLayout L{};
    L.table = w.take(std::max<size_t>(records, 1) * sizeof(EkfSmoothRec));
    L.xs = w.take(npad * 8);
    L.xp = w.take(npad * 8);
    L.yv = w.take(npad * 8);
    L.wv = w.take(npad * 8);
    L.cv = w.take(npad * 8);
    L.xinv = w.take((size_t)EKF_WIDE_BLOCK * EKF_WIDE_BLOCK * 8);
    L.M = w.take(npad * npad * 8);
    L.total = w.end;
    return L;
}

int64_t history_nmax(const ekf_filter* f) {
    int64_t nmax = 0;
    for (const auto& h : f->hist.recs) nmax = std::max<int64_t>(nmax, h.dims);
    return nmax;
}

// the table the smoothing kernels read, from the records of the last recorded replay (F: the frames of that call)
void smooth_table(ekf_filter* f, int32_t F) {
    const int32_t R = (int32_t)f->hist.recs.size();
    std::vector<EkfSmoothRec>& table = f->hist.table;
    table.assign((size_t)R, EkfSmoothRec{});
    for (int32_t r = 0; r < R; ++r) {
        const auto& h = f->hist.recs[r];
        EkfSmoothRec& e = table[r];
        e.off = (int64_t)(h.off / 8);
        e.dims = h.dims;
        e.moved = h.moved;
        for (int i = 0; i < 6; ++i) e.u[i] = h.u[i];
        const EkfNoise nz = frame_noise(f, h.s_eff);
        e.q[0] = nz.q_cam;
        e.q[1] = nz.q_err;
        e.q[2] = nz.q_lm;
        e.frame0 = h.frame;
        e.frame1 = r + 1 < R ? f->hist.recs[r + 1].frame : F;
    }
}

// the covariance pass: the blocked step's pieces with one xinv per block column, then A, Z, T and P^s, all [npad][npad]
struct SmoothCovLayout {
    SmoothLayout s;
    size_t A, Z, T, Ps, total;
    int64_t npad;
};
SmoothCovLayout smooth_cov_layout(size_t records, int64_t nmax) {
    const size_t npad = (size_t)round_up(std::max<int64_t>(nmax, 1), EKF_WIDE_BLOCK);
    Carve w;
    w.take(256);
    SmoothCovLayout L{};
    L.npad = (int64_t)npad;
    L.s.table = w.take(std::max<size_t>(records, 1) * sizeof(EkfSmoothRec));
    L.s.xs = w.take(npad * 8);
    L.s.xp = w.take(npad * 8);
    L.s.yv = w.take(npad * 8);
    L.s.wv = w.take(npad * 8);
    L.s.cv = w.take(npad * 8);
    L.s.xinv = w.take(npad / EKF_WIDE_BLOCK * EKF_WIDE_BLOCK * EKF_WIDE_BLOCK * 8);
    L.s.M = w.take(npad * npad * 8);
    L.A = w.take(npad * npad * 8);
    L.Z = w.take(npad * npad * 8);
    L.T = w.take(npad * npad * 8);
    L.Ps = w.take(npad * npad * 8);
    L.s.total = L.total = w.end;
    return L;
}

}  // namespace

extern "C" {

static int observe_log_run(ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames,
                           const double* poses_dev, const double* rows_dev, const double* scale, const double* motion,
                           void* log_ws, size_t log_ws_bytes, double* trajectory_dev, double* mahal_dev, bool record,
                           void* history_dev, size_t history_bytes);

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
    return observe_log_run(f, lm_index, offsets, frames, poses_dev, rows_dev, scale, motion, log_ws, log_ws_bytes,
                           trajectory_dev, mahal_dev, false, nullptr, 0);
}

int ekf_observe_log_recorded(ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames,
                             const double* poses_dev, const double* rows_dev, const double* scale, const double* motion,
                             void* log_ws, size_t log_ws_bytes, double* trajectory_dev, double* mahal_dev,
                             void* history_dev, size_t history_bytes) {
    return observe_log_run(f, lm_index, offsets, frames, poses_dev, rows_dev, scale, motion, log_ws, log_ws_bytes,
                           trajectory_dev, mahal_dev, true, history_dev, history_bytes);
}

// The log replay.  record: the by-frame serial loop, and behind every frame that changed the filter -- stepped, or moved by a
// non-zero motion -- one pack launch that copies state and the lower triangle of P into the next record of the history
// (recording only reads: every other launch is the one the plain call enqueues, in its order).
static int observe_log_run(ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames,
                           const double* poses_dev, const double* rows_dev, const double* scale, const double* motion,
                           void* log_ws, size_t log_ws_bytes, double* trajectory_dev, double* mahal_dev, bool record,
                           void* history_dev, size_t history_bytes) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (record && (rc = smoothing_supported(f))) return rc;
    if (rows_dev && !f->lay.has_rows) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_ROW_NOISE");
    if (mahal_dev && !f->lay.has_gate) return fail(EKF_ERR_STATE, "the filter was created without EKF_FLAG_GATE");
    // a gate that is set, or distances asked for: frame by frame in serial order, each frame on its survivors
    const bool gated = f->gate_on() || mahal_dev;
    // frame by frame in serial order: a gated call, and a call with motions (a motion between two frames of a pipelined run
    // would change rows of the P_{t+1} the next front kernel completes from P_t and W_t)
    // ... and a call on a frozen map
    const bool by_frame = gated || motion || f->frozen || record;
    // ---- validation on the host: nothing is enqueued before the whole log has passed
    if (frames < 0) return fail(EKF_ERR_INVALID, "negative frame count");
    if ((rc = check_scales(f, scale, frames))) return rc;
    if ((rc = check_motions(f, motion, frames))) return rc;
    if (frames > 0 && !offsets) return fail(EKF_ERR_INVALID, "offsets is NULL");
    if (frames > 0 && (rc = check_offsets(offsets, frames, "offsets"))) return rc;
    const int64_t D = frames > 0 ? offsets[frames] : 0;
    const int rd = f->lay.rd;
    const LogLayout LL = log_layout(rd, D);
    if (D > 0 && (!lm_index || !poses_dev)) return fail(EKF_ERR_INVALID, "NULL detections");
    if (D > 0 && (rc = check_device_buffers({log_ws}, log_ws_bytes, LL.total, "ekf_log_workspace_bytes"))) return rc;
    LogCheck lc;
    if ((rc = check_log(lm_index, offsets, frames, f->n_lm, f->cfg, "the log", &lc))) return rc;
    if (f->frozen && !lc.slots.empty())
        return fail(EKF_ERR_STATE, "the map is frozen: a log with first sightings would add landmarks (ekf_set_map_frozen)");
    if (record) {
        size_t need = 0;
        history_bound(f->lay.lmd, f->n_lm, lc, frames, &need);
        if ((rc = check_device_buffers({history_dev}, history_bytes, need, "ekf_history_bytes"))) return rc;
        f->hist = ekf_filter::History{};
        f->hist.buf = history_dev;
        f->hist.bytes = history_bytes;
        f->hist.frames = frames;
        f->hist.frame_rec.assign((size_t)frames, -1);
        f->hist.valid = true;
    }
    for (int i = 0; i < 4; ++i) f->log_stats[i] = 0;
    f->reset_gate_stats();
    if (frames == 0) return EKF_OK;

    // ---- host staging: [indices | slots | (row, source) pairs of empty frames: those before the first stepped frame of the
    // call (source: the state now), the others (source: the row of the last stepped frame before them)]
    std::vector<int32_t> lead, rest;
    {
        int last = -1;
        for (int t = 0; t < frames; ++t) {
            if (offsets[t + 1] > offsets[t]) last = t;
            else if (trajectory_dev && !by_frame) {      // (gated: which frames are stepped is known frame by frame; motions:
                                                         // an empty frame's row is the moved pose)
                std::vector<int32_t>& v = last < 0 ? lead : rest;
                v.push_back(t);
                v.push_back(last);
            }
        }
    }
    const size_t up_bytes = LL.slots - LL.idx + lc.slots.size() * 4;
    Carve p;
    p.take(up_bytes);
    const size_t lead_at = p.take(lead.size() * 4), rest_at = p.take(rest.size() * 4);
    p.take(256);
    const size_t exempt_at = gated ? p.take((size_t)D) : 0;      // rule 4: the first occurrence of every first sighting
    const int turn = f->log_pin_turn;
    if (!f->log_pin_done[turn]) HIP_TRY(hipEventCreateWithFlags(&f->log_pin_done[turn], hipEventDisableTiming));
    HIP_TRY(hipEventSynchronize(f->log_pin_done[turn]));      // (the staging of the call before the previous one is consumed)
    if ((rc = f->log_pin[turn].reserve(p.end))) return rc;
    char* pin = f->log_pin[turn].get();
    int32_t* pin_lead = f->log_pin[turn].at<int32_t>(lead_at);
    int32_t* pin_rest = f->log_pin[turn].at<int32_t>(rest_at);
    char* ws = static_cast<char*>(log_ws);
    double* z_all = reinterpret_cast<double*>(ws);
    const int32_t* idx_all = reinterpret_cast<const int32_t*>(ws + LL.idx);
    const int32_t* slots_all = reinterpret_cast<const int32_t*>(ws + LL.slots);
    if (D > 0) {
        std::memcpy(pin, lm_index, (size_t)D * 4);
        if (!lc.slots.empty()) std::memcpy(pin + (LL.slots - LL.idx), lc.slots.data(), lc.slots.size() * 4);
    }
    if (!lead.empty()) std::memcpy(pin_lead, lead.data(), lead.size() * 4);
    if (!rest.empty()) std::memcpy(pin_rest, rest.data(), rest.size() * 4);
    uint8_t* pin_exempt = f->log_pin[turn].at<uint8_t>(exempt_at);
    if (gated && D > 0) {
        std::memset(pin_exempt, 0, (size_t)D);
        for (int32_t d : lc.slots) pin_exempt[d] = 1;
    }

    auto m_of = [&](int t) { return (int)(offsets[t + 1] - offsets[t]); };
    auto nnew_of = [&](int t) { return (int)(lc.new_at[t + 1] - lc.new_at[t]); };
    // Without a gate the host knows which frames are stepped: rules 3 and 4 run over the whole log here, an empty frame's
    // scale goes into the pending scale and the next stepped frame takes it.  (Gated: frame by frame below.)
    std::vector<double> s_effs((size_t)frames, 1.0);
    if (!gated)
        for (int t = 0; t < frames; ++t) {
            s_effs[t] = frame_scale(f, scale ? scale + t : nullptr);
            frame_scale_done(f, scale ? scale + t : nullptr, s_effs[t], m_of(t) > 0);
        }
    const RunPlan plan = by_frame ? RunPlan{} : plan_runs(f, frames, m_of, nnew_of);
    int mode = EKF_SEQ_SERIAL;
    rc = choose_pipelining(f, plan.want_runs, &mode);
    if (rc) return rc;
    if (by_frame) f->seq_mode = EKF_SEQ_SERIAL;

    // ---- device work, all on the handle's stream (the pipelined runs use the internal one as ekf_observe_sequence_device)
    if (D > 0) {
        HIP_TRY(hipMemcpyAsync(ws + LL.idx, pin, up_bytes, hipMemcpyHostToDevice, f->stream));
        ekf_launch_log_prepare(poses_dev, D, rd, z_all, f->stream);
    }
    if (!lead.empty()) ekf_launch_log_fill_rows(trajectory_dev, pin_lead, (int32_t)(lead.size() / 2), f->state, f->stream);
    // recording: the camera state at the call (the rows of the frames before the first record), then record after record
    size_t hist_at = 256;
    if (record) HIP_TRY(hipMemcpyAsync(history_dev, f->state, 7 * 8, hipMemcpyDeviceToDevice, f->stream));
    auto record_frame = [&](int t, bool moved, bool stepped, double s_eff) {
        if (record && (moved || stepped)) {
            ekf_filter::HistoryRec h{};
            h.frame = t;
            h.dims = f->dims();
            h.off = hist_at;
            h.s_eff = stepped ? s_eff : 0.0;
            for (int i = 0; i < 6; ++i) h.u[i] = (moved && motion) ? motion[(size_t)t * 6 + i] : 0.0;
            h.stepped = stepped;
            h.moved = moved;
            ekf_launch_history_pack(static_cast<const double*>(f->cov), f->ld, f->state, h.dims,
                                    reinterpret_cast<double*>(static_cast<char*>(history_dev) + h.off), f->stream);
            hist_at += history_record_bytes(h.dims);
            f->hist.recs.push_back(h);
        }
        if (record) f->hist.frame_rec[t] = (int32_t)f->hist.recs.size() - 1;
    };
    auto frame_of = [&](int t) {
        const int64_t d0 = offsets[t];
        return RunFrame{idx_all + d0, z_all + (size_t)d0 * rd, m_of(t), trajectory_dev ? trajectory_dev + (size_t)t * 7 : nullptr,
                        rows_dev ? rows_dev + (size_t)d0 * rd : nullptr, s_effs[t]};
    };
    auto first_sightings = [&](int t) {
        const int nnew = nnew_of(t);
        if (nnew > 0)
            by_cov_type(f, [&](auto elem) {
                ekf_launch_log_add_markers<decltype(elem)>(f->cfg.model, f->cov, f->ld, f->state, f->dims(), poses_dev,
                                                           slots_all + lc.new_at[t], f->cfg.initial_landmark_uncertainty, nnew,
                                                           f->stream);
            });
        return nnew;
    };
    if (by_frame) {
        // the motion, first sightings (placed from the moved camera), the gate on the prior they leave, the frame on its
        // survivors; a frame without detections or without a survivor is not stepped, and its row repeats the camera state
        // (Without a gate the scales were folded over the whole log above: s_effs.)
        for (int t = 0; t < frames && rc == EKF_OK; ++t) {
            const RunFrame r = frame_of(t);
            const double* sc = scale ? scale + t : nullptr;
            bool moved = false;
            if ((rc = enqueue_motion(f, motion ? motion + (size_t)t * 6 : nullptr, &moved))) break;
            const double s_eff = gated ? frame_scale(f, sc) : s_effs[t];
            if (r.m == 0) {
                rc = repeat_row(f, r.traj_row);
                if (gated) frame_scale_done(f, sc, s_eff, false);
                if (rc == EKF_OK) record_frame(t, moved, false, s_eff);
                continue;
            }
            const int nnew = first_sightings(t);
            f->n_lm += nnew;
            f->log_stats[3] += nnew;
            const int64_t d0 = offsets[t];
            int s = r.m;
            rc = gated ? gated_frame_or_row(f, r.idx, r.z, r.rows, r.m, pin_exempt + d0, nnew,
                                            mahal_dev ? mahal_dev + d0 : nullptr, r.traj_row, &s, s_eff)
                       : enqueue_frame(f, r.idx, r.z, r.rows, r.m, r.traj_row, false, s_eff);
            if (rc == EKF_OK && s > 0) f->log_stats[0] += 1;
            if (rc == EKF_OK && gated) frame_scale_done(f, sc, s_eff, s > 0);
            if (rc == EKF_OK) record_frame(t, moved, s > 0, s_eff);
        }
    } else {
        rc = run_frames(f, frames, frame_of, first_sightings, plan, mode == EKF_SEQ_PIPELINED, f->log_stats);
    }
    if (rc == EKF_OK && !rest.empty())
        ekf_launch_log_fill_rows(trajectory_dev, pin_rest, (int32_t)(rest.size() / 2), f->state, f->stream);
    // A state getter after the call must wait for the whole call (the last frame's state may come from a pipelined run, whose
    // front kernels record no event): no shortcut through the event of an earlier serial frame of the call.
    f->shortcut.log();
    // (the staging may be reused once the stream is here -- also after an error: its copy may have been enqueued)
    f->log_pin_turn = turn ^ 1;
    if (rc) f->hist.valid = f->hist.valid && !record;      // (a recorded call that failed leaves no history)
    HIP_TRY(hipEventRecord(f->log_pin_done[turn], f->stream));
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return EKF_OK;
}

// ---- offline smoothing (include/ekf_slam_hip.h, "Offline smoothing"; kernels: ekf_smooth.hip) ---------------------------
int ekf_history_record_bytes(int32_t dims, size_t* bytes) {
    if (!bytes || dims < EKF_CAM) return fail(EKF_ERR_INVALID, "bad record size request");
    *bytes = history_record_bytes(dims);
    return EKF_OK;
}

int ekf_history_bytes(const ekf_filter* f, const int32_t* lm_index, const int64_t* offsets, int32_t frames, size_t* bytes) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!bytes || frames < 0) return fail(EKF_ERR_INVALID, "bad history size request");
    int rc;
    if (frames > 0 && !offsets) return fail(EKF_ERR_INVALID, "offsets is NULL");
    if (frames > 0 && (rc = check_offsets(offsets, frames, "offsets"))) return rc;
    if (frames > 0 && offsets[frames] > 0 && !lm_index) return fail(EKF_ERR_INVALID, "NULL detections");
    LogCheck lc;
    if ((rc = check_log(lm_index, offsets, frames, f->n_lm, f->cfg, "the log", &lc))) return rc;
    history_bound(f->lay.lmd, f->n_lm, lc, frames, bytes);
    return EKF_OK;
}

int ekf_history_info(const ekf_filter* f, int32_t* records, int32_t capacity, int32_t* frame, int32_t* dims, double* s_eff,
                     double* motion, int32_t* stepped, int32_t* frame_record) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!records || capacity < 0) return fail(EKF_ERR_INVALID, "bad history info request");
    if (!f->hist.valid) return fail(EKF_ERR_STATE, "no recorded replay (ekf_observe_log_recorded), or the filter has changed since");
    const int32_t R = (int32_t)f->hist.recs.size();
    *records = R;
    const bool arrays = frame || dims || s_eff || motion || stepped;
    if (arrays && capacity < R) return fail(EKF_ERR_CAPACITY, "fewer entries than records");
    for (int32_t r = 0; r < R && arrays; ++r) {
        const auto& h = f->hist.recs[r];
        if (frame) frame[r] = h.frame;
        if (dims) dims[r] = h.dims;
        if (s_eff) s_eff[r] = h.s_eff;
        if (motion)
            for (int i = 0; i < 6; ++i) motion[6 * (size_t)r + i] = h.u[i];
        if (stepped) stepped[r] = h.stepped;
    }
    if (frame_record)
        for (int32_t t = 0; t < f->hist.frames; ++t) frame_record[t] = f->hist.frame_rec[t];
    return EKF_OK;
}

int ekf_history_record(ekf_filter* f, const void* history_dev, int32_t r, double* state_out, double* cov_out, int32_t dims) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (!f->hist.valid || history_dev != f->hist.buf)
        return fail(EKF_ERR_STATE, "not the history of this handle's last recorded replay");
    if (r < 0 || r >= (int32_t)f->hist.recs.size()) return fail(EKF_ERR_INVALID, "no such record");
    const auto& h = f->hist.recs[r];
    if (dims != h.dims) return fail(EKF_ERR_INVALID, "dims must equal the record's (ekf_history_info)");
    HIP_TRY(hipStreamSynchronize(f->stream));
    const size_t N = (size_t)h.dims;
    std::vector<double> packed(N + N * (N + 1) / 2);
    HIP_TRY(hipMemcpy(packed.data(), static_cast<const char*>(history_dev) + h.off, packed.size() * 8, hipMemcpyDeviceToHost));
    if (state_out) std::memcpy(state_out, packed.data(), N * 8);
    if (cov_out) {
        const double* tri = packed.data() + N;
        size_t e = 0;
        for (size_t j = 0; j < N; ++j)
            for (size_t i = j; i < N; ++i, ++e) cov_out[i * N + j] = cov_out[j * N + i] = tri[e];
    }
    return EKF_OK;
}

int ekf_smooth_workspace_bytes(const ekf_filter* f, size_t* bytes) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!bytes) return fail(EKF_ERR_INVALID, "bytes is NULL");
    if (!f->hist.valid) return fail(EKF_ERR_STATE, "no recorded replay (ekf_observe_log_recorded), or the filter has changed since");
    *bytes = smooth_layout(f->hist.recs.size(), history_nmax(f)).total;
    return EKF_OK;
}

int ekf_smooth_history(ekf_filter* f, const void* history_dev, size_t history_bytes, void* ws, size_t ws_bytes, int32_t flags,
                       double* smoothed_dev) {
    int rc = check_ready(f);
    if (rc) return rc;
    if ((rc = smoothing_supported(f))) return rc;
    if (!f->hist.valid) return fail(EKF_ERR_STATE, "no recorded replay (ekf_observe_log_recorded), or the filter has changed since");
    if (history_dev != f->hist.buf || history_bytes < f->hist.bytes)
        return fail(EKF_ERR_STATE, "not the history of this handle's last recorded replay");
    const int32_t F = f->hist.frames, R = (int32_t)f->hist.recs.size();
    if (F == 0) return EKF_OK;
    if (!smoothed_dev) return fail(EKF_ERR_INVALID, "smoothed_dev is NULL");
    const int64_t nmax = history_nmax(f);
    const SmoothLayout L = smooth_layout((size_t)R, nmax);
    if ((rc = check_device_buffers({ws}, ws_bytes, L.total, "ekf_smooth_workspace_bytes"))) return rc;
    const bool resident = nmax <= EKF_SMOOTH_RESIDENT_DIMS && !(flags & 1);
    // (the backward substitution keeps y in LDS: 64 KiB without an attribute, less its static kilobyte)
    if (!resident && round_up(nmax, EKF_WIDE_BLOCK) > 8064)
        return fail(EKF_ERR_CAPACITY, "the blocked smoothing tier takes records of up to 8064 dims");
    const double* hist = static_cast<const double*>(history_dev);
    if (R == 0) {      // nothing changed the filter: every row is the camera state at the call
        ekf_launch_smooth_rows(hist, smoothed_dev, 0, F, f->stream);
        HIP_TRY(hipGetLastError());
        return EKF_OK;
    }
    smooth_table(f, F);
    const std::vector<EkfSmoothRec>& table = f->hist.table;
    char* w = static_cast<char*>(ws);
    int32_t* status = reinterpret_cast<int32_t*>(w);
    EkfSmoothRec* table_dev = reinterpret_cast<EkfSmoothRec*>(w + L.table);
    HIP_TRY(hipMemsetAsync(w, 0, 256, f->stream));
    HIP_TRY(hipMemcpyAsync(table_dev, table.data(), (size_t)R * sizeof(EkfSmoothRec), hipMemcpyHostToDevice, f->stream));
    const int32_t lead = table[0].frame0;
    if (resident) {
        HIP_TRY(ekf_launch_smooth_resident(hist, table_dev, R, (int32_t)nmax, lead, smoothed_dev, status, f->stream));
    } else {
        EkfSmoothBlocked a{};
        a.history = hist;
        a.M = reinterpret_cast<double*>(w + L.M);
        a.xs = reinterpret_cast<double*>(w + L.xs);
        a.xp = reinterpret_cast<double*>(w + L.xp);
        a.yv = reinterpret_cast<double*>(w + L.yv);
        a.wv = reinterpret_cast<double*>(w + L.wv);
        a.cv = reinterpret_cast<double*>(w + L.cv);
        a.xinv = reinterpret_cast<double*>(w + L.xinv);
        a.smoothed = smoothed_dev;
        a.status = status;
        const EkfSmoothRec& last = table[R - 1];
        HIP_TRY(hipMemcpyAsync(a.xs, hist + last.off, (size_t)last.dims * 8, hipMemcpyDeviceToDevice, f->stream));
        ekf_launch_smooth_rows(hist + last.off, smoothed_dev, last.frame0, last.frame1, f->stream);
        ekf_launch_smooth_rows(hist, smoothed_dev, 0, lead, f->stream);
        for (int32_t r = R - 2; r >= 0; --r) {
            a.rec = table[r];
            a.next = table[r + 1];
            ekf_launch_smooth_blocked_step(a, f->stream);
        }
    }
    HIP_TRY(hipGetLastError());
    // the pass has its own status word: a P_p that is not positive definite is reported here and leaves nothing on the filter
    HIP_TRY(hipStreamSynchronize(f->stream));
    int32_t st = 0;
    HIP_TRY(hipMemcpy(&st, status, 4, hipMemcpyDeviceToHost));
    if (st != 0) return fail(EKF_ERR_NUMERIC, "smoothing: a predicted covariance P_p is not positive definite");
    return EKF_OK;
}

// ---- smoothed covariances (include/ekf_slam_hip.h, "Smoothed covariances"; kernels: ekf_smooth_cov.hip) -------------------
int ekf_smooth_cov_workspace_bytes(const ekf_filter* f, size_t* bytes) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!bytes) return fail(EKF_ERR_INVALID, "bytes is NULL");
    if (!f->hist.valid) return fail(EKF_ERR_STATE, "no recorded replay (ekf_observe_log_recorded), or the filter has changed since");
    *bytes = smooth_cov_layout(f->hist.recs.size(), history_nmax(f)).total;
    return EKF_OK;
}

int ekf_smooth_history_cov(ekf_filter* f, const void* history_dev, size_t history_bytes, void* ws, size_t ws_bytes, int32_t flags,
                           double* smoothed_dev, double* cam_cov_dev, double* filt_cam_cov_dev, double* first_cov_dev) {
    (void)flags;      // (the covariance pass has one tier)
    int rc = check_ready(f);
    if (rc) return rc;
    if ((rc = smoothing_supported(f))) return rc;
    if (!f->hist.valid) return fail(EKF_ERR_STATE, "no recorded replay (ekf_observe_log_recorded), or the filter has changed since");
    if (history_dev != f->hist.buf || history_bytes < f->hist.bytes)
        return fail(EKF_ERR_STATE, "not the history of this handle's last recorded replay");
    const int32_t F = f->hist.frames, R = (int32_t)f->hist.recs.size();
    if (F == 0) return EKF_OK;
    if (!smoothed_dev || !cam_cov_dev) return fail(EKF_ERR_INVALID, "smoothed_dev or cam_cov_dev is NULL");
    const int64_t nmax = history_nmax(f);
    const SmoothCovLayout L = smooth_cov_layout((size_t)R, nmax);
    if ((rc = check_device_buffers({ws}, ws_bytes, L.total, "ekf_smooth_cov_workspace_bytes"))) return rc;
    if (L.npad > 8064) return fail(EKF_ERR_CAPACITY, "the covariance pass takes records of up to 8064 dims");
    const double* hist = static_cast<const double*>(history_dev);
    if (R == 0) {      // nothing changed the filter: the start pose on every row, and no covariance was ever recorded
        ekf_launch_smooth_rows(hist, smoothed_dev, 0, F, f->stream);
        ekf_launch_smooth_cov_nan(cam_cov_dev, filt_cam_cov_dev, 0, F, f->stream);
        HIP_TRY(hipGetLastError());
        return EKF_OK;
    }
    smooth_table(f, F);
    const std::vector<EkfSmoothRec>& table = f->hist.table;
    char* w = static_cast<char*>(ws);
    int32_t* status = reinterpret_cast<int32_t*>(w);
    EkfSmoothRec* table_dev = reinterpret_cast<EkfSmoothRec*>(w + L.s.table);
    HIP_TRY(hipMemsetAsync(w, 0, 256, f->stream));
    HIP_TRY(hipMemcpyAsync(table_dev, table.data(), (size_t)R * sizeof(EkfSmoothRec), hipMemcpyHostToDevice, f->stream));
    EkfSmoothCov a{};
    a.b.history = hist;
    a.b.M = reinterpret_cast<double*>(w + L.s.M);
    a.b.xs = reinterpret_cast<double*>(w + L.s.xs);
    a.b.xp = reinterpret_cast<double*>(w + L.s.xp);
    a.b.yv = reinterpret_cast<double*>(w + L.s.yv);
    a.b.wv = reinterpret_cast<double*>(w + L.s.wv);
    a.b.cv = reinterpret_cast<double*>(w + L.s.cv);
    a.b.xinv = reinterpret_cast<double*>(w + L.s.xinv);
    a.b.smoothed = smoothed_dev;
    a.b.status = status;
    a.A = reinterpret_cast<double*>(w + L.A);
    a.Z = reinterpret_cast<double*>(w + L.Z);
    a.T = reinterpret_cast<double*>(w + L.T);
    a.Ps = reinterpret_cast<double*>(w + L.Ps);
    a.ldp = L.npad;
    a.cam_cov = cam_cov_dev;
    a.filt_cam_cov = filt_cam_cov_dev;
    a.first_cov = first_cov_dev;
    const EkfSmoothRec& last = table[R - 1];
    const int32_t lead = table[0].frame0;
    // (P^s keeps its leading dimension over the pass; zero first, so that what a smaller record leaves unwritten is finite)
    HIP_TRY(hipMemsetAsync(a.Ps, 0, (size_t)L.npad * L.npad * 8, f->stream));
    HIP_TRY(hipMemcpyAsync(a.b.xs, hist + last.off, (size_t)last.dims * 8, hipMemcpyDeviceToDevice, f->stream));
    ekf_launch_smooth_rows(hist + last.off, smoothed_dev, last.frame0, last.frame1, f->stream);
    ekf_launch_smooth_rows(hist, smoothed_dev, 0, lead, f->stream);
    ekf_launch_smooth_cov_nan(cam_cov_dev, filt_cam_cov_dev, 0, lead, f->stream);
    a.b.rec = last;
    a.first = R == 1;
    ekf_launch_smooth_cov_last(a, f->stream);
    for (int32_t r = R - 2; r >= 0; --r) {
        a.b.rec = table[r];
        a.b.next = table[r + 1];
        a.first = r == 0;
        ekf_launch_smooth_cov_step(a, f->stream);
    }
    HIP_TRY(hipGetLastError());
    // the pass has its own status word, as ekf_smooth_history: nothing sticky is left on the filter
    HIP_TRY(hipStreamSynchronize(f->stream));
    int32_t st = 0;
    HIP_TRY(hipMemcpy(&st, status, 4, hipMemcpyDeviceToHost));
    if (st != 0) return fail(EKF_ERR_NUMERIC, "smoothing: a predicted covariance P_p is not positive definite");
    return EKF_OK;
}

// ---- detection -> pose front end (base_filter.py:92-171): stateless, no filter handle -------------------------
int ekf_estimate_poses_device(const double* corners_dev, int32_t count, double marker_size, const double camera_matrix[9],
                              const double* dist_coeffs, int32_t n_dist, double* poses_dev, void* stream) {
    if (count < 0) return fail(EKF_ERR_INVALID, "negative marker count");
    if (count == 0) return EKF_OK;
    if (!corners_dev || !poses_dev) return fail(EKF_ERR_INVALID, "NULL device buffer");
    if (!(marker_size > 0.0)) return fail(EKF_ERR_INVALID, "marker_size must be > 0");
    EkfCamera cam;
    int rc = make_camera(camera_matrix, dist_coeffs, n_dist, &cam);
    if (rc) return rc;
    ekf_launch_ippe_square(corners_dev, count, marker_size, cam, poses_dev, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return EKF_OK;
}

int ekf_estimate_poses(const double* corners, int32_t count, double marker_size, const double camera_matrix[9],
                       const double* dist_coeffs, int32_t n_dist, double* poses, void* stream) {
    if (count < 0) return fail(EKF_ERR_INVALID, "negative marker count");
    if (count == 0) return EKF_OK;
    if (!corners || !poses) return fail(EKF_ERR_INVALID, "NULL host buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* dev = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&dev), (size_t)count * 14 * 8, s));
    hipError_t e = hipMemcpyAsync(dev, corners, (size_t)count * 8 * 8, hipMemcpyHostToDevice, s);
    int rc = EKF_OK;
    if (e == hipSuccess) {
        rc = ekf_estimate_poses_device(dev, count, marker_size, camera_matrix, dist_coeffs, n_dist, dev + (size_t)count * 8, s);
        if (rc == EKF_OK) e = hipMemcpyAsync(poses, dev + (size_t)count * 8, (size_t)count * 6 * 8, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFreeAsync(dev, s);
    if (rc) return rc;
    if (e != hipSuccess) return fail(EKF_ERR_HIP, std::string("ekf_estimate_poses: ") + hipGetErrorString(e));
    return EKF_OK;
}

int ekf_sync(ekf_filter* f) {
    int rc = check_ready(f);
    if (rc) return rc;
    return sync_and_check(f);
}

int ekf_num_landmarks(const ekf_filter* f) { return f ? f->n_lm : EKF_ERR_INVALID; }

int ekf_get_state(ekf_filter* f, double* out, int32_t count) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (!out || count < 0 || count > f->dims()) return fail(EKF_ERR_INVALID, "bad state request");
    rc = sync_and_check(f, count);
    if (rc) return rc;
    std::memcpy(out, f->readback.at<double>(256), (size_t)count * 8);
    return EKF_OK;
}

int ekf_get_camera(ekf_filter* f, double out[10]) { return ekf_get_state(f, out, EKF_CAM); }

int ekf_get_cov_diag(ekf_filter* f, double* out, int32_t count) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (!out || count < 0 || count > f->dims()) return fail(EKF_ERR_INVALID, "bad diag request");
    double* scratch = f->at<double>(f->lay.off_diag);
    by_cov_type(f, [&](auto elem) { ekf_launch_cov_diag<decltype(elem)>(f->cov, f->ld, scratch, count, f->stream); });
    HIP_TRY(hipGetLastError());
    rc = sync_and_check(f);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, scratch, (size_t)count * 8, hipMemcpyDeviceToHost));
    return EKF_OK;
}

int ekf_get_cov(ekf_filter* f, double* out, int32_t dims) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (!out || dims != f->dims()) return fail(EKF_ERR_INVALID, "dims must equal the state dimension");
    rc = sync_and_check(f);
    if (rc) return rc;
    const size_t el = f->lay.elem;
    if (el == 8) {
        HIP_TRY(hipMemcpy2D(out, (size_t)dims * 8, f->cov, (size_t)f->ld * 8, (size_t)dims * 8, dims,
                            hipMemcpyDeviceToHost));
    } else {
        std::vector<float> tmp((size_t)dims * dims);
        HIP_TRY(hipMemcpy2D(tmp.data(), (size_t)dims * 4, f->cov, (size_t)f->ld * 4, (size_t)dims * 4,
                            dims, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tmp.size(); ++i) out[i] = (double)tmp[i];
    }
    return EKF_OK;
}

int ekf_set_state(ekf_filter* f, const double* state, int32_t num_landmarks) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (!state || num_landmarks < 0) return fail(EKF_ERR_INVALID, "bad state");
    if (num_landmarks > f->cfg.max_landmarks)
        return fail(EKF_ERR_CAPACITY, "more landmarks than max_landmarks");
    f->shortcut.state_set();
    HIP_TRY(hipStreamSynchronize(f->stream));
    HIP_TRY(hipMemset(f->state, 0, (size_t)f->lay.cap * 8));
    HIP_TRY(hipMemcpy(f->state, state, (size_t)(f->lay.lmd * num_landmarks + EKF_CAM) * 8,
                      hipMemcpyHostToDevice));
    f->n_lm = num_landmarks;
    f->pending = 0.0;
    return EKF_OK;
}

int ekf_set_cov(ekf_filter* f, const double* cov, int32_t dims) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (!cov || dims != f->dims())
        return fail(EKF_ERR_INVALID, "dims must equal the state dimension (call ekf_set_state first)");
    const Layout& L = f->lay;
    HIP_TRY(hipStreamSynchronize(f->stream));
    HIP_TRY(hipMemset(f->cov, 0, (size_t)L.cap * L.cap * L.elem));
    // ... and the second covariance buffer of the pipelined mode: it may hold entries of a larger map from earlier frames,
    // and what lies beyond the state dimension must be zero in both buffers (an odd pipelined run copies or leaves the
    // whole second buffer as the covariance; new landmarks only write their diagonal)
    if (L.has_cov2) {
        HIP_TRY(hipStreamSynchronize(f->big));
        HIP_TRY(hipMemset(f->at<void>(L.off_cov2), 0, (size_t)L.cap * L.cap * L.elem));
    }
    // symmetrise on upload: the kernels keep P bitwise symmetric from then on
    return by_cov_type(f, [&](auto elem) -> int {
        using T = decltype(elem);
        std::vector<T> tmp((size_t)dims * dims);
        for (int i = 0; i < dims; ++i)
            for (int j = 0; j < dims; ++j)
                tmp[(size_t)i * dims + j] = (T)(0.5 * (cov[(size_t)i * dims + j] + cov[(size_t)j * dims + i]));
        HIP_TRY(hipMemcpy2D(f->cov, (size_t)f->ld * sizeof(T), tmp.data(), (size_t)dims * sizeof(T), (size_t)dims * sizeof(T),
                            dims, hipMemcpyHostToDevice));
        return EKF_OK;
    });
}

int ekf_last_sequence_mode(const ekf_filter* f) { return f ? f->seq_mode : EKF_ERR_INVALID; }

int ekf_set_map_frozen(ekf_filter* f, int32_t frozen) {
    int rc = check_ready(f);
    if (rc) return rc;
    f->frozen = frozen != 0;
    return EKF_OK;
}

int ekf_get_map_frozen(const ekf_filter* f) { return f ? (f->frozen ? 1 : 0) : EKF_ERR_INVALID; }

int ekf_set_fused(ekf_filter* f, int32_t enable) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (enable) f->cfg.flags &= ~4; else f->cfg.flags |= 4;
    return EKF_OK;
}

int ekf_set_kernel_timing(ekf_filter* f, int32_t enable) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    HIP_TRY(hipStreamSynchronize(f->stream));
    if (enable && f->ev.empty()) {
        f->ev.resize((size_t)kEventPool * (kTimedKernels + 1));
        for (auto& e : f->ev) HIP_TRY(hipEventCreate(&e));
    }
    f->timing = enable != 0;
    f->timing_cov_only = enable == 2;
    f->ev_frames = 0;
    for (int i = 0; i < kTimedKernels; ++i) {
        f->t_sum_us[i] = 0.0;
        f->t_cnt[i] = 0;
    }
    return EKF_OK;
}

int ekf_get_kernel_timing(ekf_filter* f, int32_t which, double* mean_us, int64_t* launches) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (which < 0 || which >= kTimedKernels) return fail(EKF_ERR_INVALID, "which must be 0..3");
    int rc = fold_timing(f);
    if (rc) return rc;
    if (mean_us) *mean_us = f->t_cnt[which] ? f->t_sum_us[which] / (double)f->t_cnt[which] : 0.0;
    if (launches) *launches = f->t_cnt[which];
    return EKF_OK;
}

// Items 0 - 4: include/ekf_slam_hip.h.  Diagnostics beyond the public list: 5 = the 64 in-kernel time stamps (after
// what = -2: all of them, -3: role level only), 6 = the end-gate ring of the pipelined mode, [EKF_GATE_LOG_FRAMES][4]
// (EkfFrame::gate_log; role-level stamps only: it borrows the W debug copy; hip_backend.GATE_LOG_FRAMES is the same number).
int ekf_debug_fetch(ekf_filter* f, int32_t what, double* out, size_t count) {
    int rc = check_ready(f);
    if (rc) return rc;
    if (!out) return fail(EKF_ERR_INVALID, "out is NULL");
    if (what == -1) {           // enable the f64 copy of W in subsequent frames
        f->debug_w = true;
        return EKF_OK;
    }
    if (what == -2 || what == -3) {   // in-kernel time stamps only (no debug copies: the production code path); -3: role level only
        f->debug_stamps = true;
        f->debug_stamps_light = what == -3;
        return EKF_OK;
    }
    const Layout& L = f->lay;
    const int k = L.rd * f->last_m, kp = (int)round_up(k, EKF_RB), dims = f->dims();
    const int jc = f->cfg.model == EKF_MODEL_ROTATIONS ? 20 : EKF_JCOLS;
    HIP_TRY(hipStreamSynchronize(f->stream));
    switch (what) {
        case 0:
            if (count < (size_t)k * jc) return fail(EKF_ERR_INVALID, "out too small");
            HIP_TRY(hipMemcpy2D(out, (size_t)jc * 8, f->at<double>(L.off_jac), EKF_JLD * 8, (size_t)jc * 8,
                                k, hipMemcpyDeviceToHost));
            return EKF_OK;
        case 1:
            if (count < (size_t)k) return fail(EKF_ERR_INVALID, "out too small");
            HIP_TRY(hipMemcpy(out, f->at<double>(L.off_resid), (size_t)k * 8, hipMemcpyDeviceToHost));
            return EKF_OK;
        case 2:
            if (count < (size_t)kp * kp) return fail(EKF_ERR_INVALID, "out too small");
            HIP_TRY(hipMemcpy2D(out, (size_t)kp * 8, f->at<double>(L.off_lmat), (size_t)L.kmax * 8,
                                (size_t)kp * 8, kp, hipMemcpyDeviceToHost));
            return EKF_OK;
        case 3:
            if (!f->debug_w) return fail(EKF_ERR_STATE, "call ekf_debug_fetch(f,-1,..) first");
            if (count < (size_t)kp * dims) return fail(EKF_ERR_INVALID, "out too small");
            HIP_TRY(hipMemcpy2D(out, (size_t)dims * 8, f->at<double>(L.off_wdbg), (size_t)L.cap * 8,
                                (size_t)dims * 8, kp, hipMemcpyDeviceToHost));
            return EKF_OK;
        case 4:
            if (count < (size_t)k * dims) return fail(EKF_ERR_INVALID, "out too small");
            HIP_TRY(hipMemcpy2D(out, (size_t)dims * 8, f->at<double>(L.off_amat), (size_t)L.cap * 8,
                                (size_t)dims * 8, k, hipMemcpyDeviceToHost));
            return EKF_OK;
        case 5:
            if (count < 64) return fail(EKF_ERR_INVALID, "out too small");
            {
                long long st[64];
                HIP_TRY(hipMemcpy(st, f->at<long long>(L.off_stamps), sizeof(st), hipMemcpyDeviceToHost));
                for (int i = 0; i < 64; ++i) out[i] = (double)st[i];
            }
            return EKF_OK;
        case 6:      // the end-gate ring of the pipelined mode (EkfFrame::gate_log), [EKF_GATE_LOG_FRAMES][4]
            if (count < 4 * EKF_GATE_LOG_FRAMES) return fail(EKF_ERR_INVALID, "out too small");
            if (!(f->debug_stamps && f->debug_stamps_light) || f->debug_w || (size_t)L.kmax * L.cap < 4 * EKF_GATE_LOG_FRAMES)
                return fail(EKF_ERR_STATE, "the gate log needs role-level stamps (ekf_debug_fetch(f,-3,..)) and kmax * cap >= 8192");
            {
                std::vector<long long> st(4 * EKF_GATE_LOG_FRAMES);
                HIP_TRY(hipMemcpy(st.data(), f->at<long long>(L.off_wdbg), st.size() * 8, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < st.size(); ++i) out[i] = (double)st[i];
            }
            return EKF_OK;
        default:
            return fail(EKF_ERR_INVALID, "unknown debug item");
    }
}

}  // extern "C"
