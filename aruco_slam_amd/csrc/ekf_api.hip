// C ABI of the EKF-SLAM HIP library (see include/ekf_slam_hip.h): the filter handle (ekf_filter.h) -- its workspace layout
// and its life (create, bind, grow, reset, destroy), markers, state and covariance in and out, the getters and their
// synchronisation, settings, timing and debug fetch -- and the pose front end.  Frames: ekf_frames.hip; the log replay:
// ekf_log_api.hip; offline smoothing: ekf_smooth_api.hip; the batch handle: ekf_batch_api.hip.  Host side only: argument
// checking, workspace carving, launch sequencing.
#include <cmath>
#include <cstring>

#include "ekf_filter.h"
#include "ekf_remove.h"

thread_local std::string g_err;

namespace {

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
