// C ABI of the EKF-SLAM HIP library (see include/ekf_slam_hip.h), the filter handle (ekf_filter.h): offline smoothing --
// the queries of a recorded history (ekf_history_*) and the two backward passes over it (ekf_smooth_history,
// ekf_smooth_history_cov).  Host side only; the kernels are in ekf_smooth.hip and ekf_smooth_cov.hip, the recording is part
// of the log replay (ekf_log_api.hip).
#include <cstring>

#include "ekf_filter.h"
#include "ekf_smooth_host.h"

// ---- offline smoothing: what is supported ---------------------------------------------------------------------------------
// (include/ekf_slam_hip.h, "Offline smoothing": the refusals)
int smoothing_supported(const ekf_filter* f) {
    if (f->cfg.model != EKF_MODEL_EKF) return fail(EKF_ERR_STATE, "smoothing: EKF_MODEL_ROTATIONS is not supported");
    if (f->cfg.cov_dtype != EKF_COV_F64) return fail(EKF_ERR_STATE, "smoothing needs the f64 covariance");
    if (f->cfg.quat_mode != EKF_QUAT_SCALAR_FIRST)
        return fail(EKF_ERR_STATE, "smoothing needs EKF_QUAT_SCALAR_FIRST (the as-written injection has no inverse)");
    if (f->frozen) return fail(EKF_ERR_STATE, "smoothing: the map is frozen");
    return EKF_OK;
}

namespace {

// Is there a history -- the last recorded replay, and nothing has changed the filter's map since --, and is `history_dev`,
// with history_bytes behind it, that history?  (A call without a buffer of its own passes f->hist.buf and f->hist.bytes.)
// buffer_only: the call tells a missing history like a wrong buffer.
int history_ready(const ekf_filter* f, const void* history_dev, size_t history_bytes, bool buffer_only = false) {
    if (!f->hist.valid && !buffer_only)
        return fail(EKF_ERR_STATE, "no recorded replay (ekf_observe_log_recorded), or the filter has changed since");
    if (!f->hist.valid || history_dev != f->hist.buf || history_bytes < f->hist.bytes)
        return fail(EKF_ERR_STATE, "not the history of this handle's last recorded replay");
    return EKF_OK;
}

// Smoothing workspace: [status 256 | table | xs | xp | yv | wv | cv | xinv | M] and, for the covariance pass, [A | Z | T |
// P^s] behind them; the vectors sized by the largest record rounded up to whole block columns (npad), the matrices
// [npad][npad].  xinv_blocks: the blocked step keeps one xinv, the covariance pass one per block column.  (The resident
// tier uses the first two pieces only.)
struct SmoothLayout {
    size_t table, xs, xp, yv, wv, cv, xinv, M, A, Z, T, Ps, total;
    int64_t npad;
};
int64_t smooth_npad(int64_t nmax) { return round_up(std::max<int64_t>(nmax, 1), EKF_WIDE_BLOCK); }
SmoothLayout smooth_layout(size_t records, int64_t nmax, size_t xinv_blocks, bool cov_pieces) {
    const size_t npad = (size_t)smooth_npad(nmax);
    Carve w;
    w.take(256);
    SmoothLayout L{};
    L.npad = (int64_t)npad;
    L.table = w.take(std::max<size_t>(records, 1) * sizeof(EkfSmoothRec));
    L.xs = w.take(npad * 8);
    L.xp = w.take(npad * 8);
    L.yv = w.take(npad * 8);
    L.wv = w.take(npad * 8);
    L.cv = w.take(npad * 8);
    L.xinv = w.take(xinv_blocks * EKF_WIDE_BLOCK * EKF_WIDE_BLOCK * 8);
    L.M = w.take(npad * npad * 8);
    if (cov_pieces) {
        L.A = w.take(npad * npad * 8);
        L.Z = w.take(npad * npad * 8);
        L.T = w.take(npad * npad * 8);
        L.Ps = w.take(npad * npad * 8);
    }
    L.total = w.end;
    return L;
}

int64_t history_nmax(const ekf_filter* f) {
    int64_t nmax = 0;
    for (const auto& h : f->hist.recs) nmax = std::max<int64_t>(nmax, h.dims);
    return nmax;
}

// the workspace of a pass over this handle's history (cov: the covariance pass)
SmoothLayout smooth_layout(const ekf_filter* f, bool cov) {
    const int64_t nmax = history_nmax(f);
    return smooth_layout(f->hist.recs.size(), nmax, cov ? (size_t)(smooth_npad(nmax) / EKF_WIDE_BLOCK) : 1, cov);
}

int smooth_workspace_bytes(const ekf_filter* f, size_t* bytes, bool cov) {
    if (!f) return fail(EKF_ERR_INVALID, "filter handle is NULL");
    if (!bytes) return fail(EKF_ERR_INVALID, "bytes is NULL");
    int rc = history_ready(f, f->hist.buf, f->hist.bytes);
    if (rc) return rc;
    *bytes = smooth_layout(f, cov).total;
    return EKF_OK;
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

// One backward pass over the history, as smooth_begin leaves it for the launches of ekf_smooth_history and
// ekf_smooth_history_cov.
struct SmoothPass {
    int32_t F = 0, R = 0;          // frames of the recorded call, records (the table: f->hist.table)
    int64_t nmax = 0;              // dims of the largest record
    bool resident = false;         // the resident tier (never for the covariance pass)
    SmoothLayout L{};
    const double* hist = nullptr;
    EkfSmoothRec* table_dev = nullptr;
    EkfSmoothBlocked a{};          // the blocked step's arguments, all but rec and next
};

// What both passes begin with, in this order: the handle, what smoothing supports, the history; F == 0: nothing to do
// (p->F); `missing` (null, or what to say about an output the caller left NULL); the workspace and the size the pass takes;
// R == 0: nothing changed the filter, the caller fills its rows (p->R) and nothing is uploaded.  Otherwise the table is
// built and uploaded behind the cleared status word, and the blocked step's arguments are filled.
int smooth_begin(ekf_filter* f, const void* history_dev, size_t history_bytes, void* ws, size_t ws_bytes, int32_t flags,
                 bool cov, const char* missing, double* smoothed_dev, SmoothPass* p) {
    int rc = check_ready(f);
    if (rc) return rc;
    if ((rc = smoothing_supported(f))) return rc;
    if ((rc = history_ready(f, history_dev, history_bytes))) return rc;
    p->F = f->hist.frames;
    p->R = (int32_t)f->hist.recs.size();
    if (p->F == 0) return EKF_OK;
    if (missing) return fail(EKF_ERR_INVALID, missing);
    p->nmax = history_nmax(f);
    const SmoothLayout& L = p->L = smooth_layout(f, cov);
    if ((rc = check_device_buffers({ws}, ws_bytes, L.total, cov ? "ekf_smooth_cov_workspace_bytes" : "ekf_smooth_workspace_bytes")))
        return rc;
    p->resident = !cov && p->nmax <= EKF_SMOOTH_RESIDENT_DIMS && !(flags & 1);
    // (the backward substitution keeps y in LDS: 64 KiB without an attribute, less its static kilobyte)
    if (!p->resident && L.npad > 8064)
        return fail(EKF_ERR_CAPACITY, cov ? "the covariance pass takes records of up to 8064 dims"
                                          : "the blocked smoothing tier takes records of up to 8064 dims");
    p->hist = static_cast<const double*>(history_dev);
    if (p->R == 0) return EKF_OK;
    smooth_table(f, p->F);
    char* w = static_cast<char*>(ws);
    p->table_dev = reinterpret_cast<EkfSmoothRec*>(w + L.table);
    HIP_TRY(hipMemsetAsync(w, 0, 256, f->stream));
    HIP_TRY(hipMemcpyAsync(p->table_dev, f->hist.table.data(), (size_t)p->R * sizeof(EkfSmoothRec), hipMemcpyHostToDevice,
                           f->stream));
    EkfSmoothBlocked& a = p->a;
    a.history = p->hist;
    a.M = reinterpret_cast<double*>(w + L.M);
    a.xs = reinterpret_cast<double*>(w + L.xs);
    a.xp = reinterpret_cast<double*>(w + L.xp);
    a.yv = reinterpret_cast<double*>(w + L.yv);
    a.wv = reinterpret_cast<double*>(w + L.wv);
    a.cv = reinterpret_cast<double*>(w + L.cv);
    a.xinv = reinterpret_cast<double*>(w + L.xinv);
    a.smoothed = smoothed_dev;
    a.status = reinterpret_cast<int32_t*>(w);
    return EKF_OK;
}

// The last record is its own smoothed estimate: into xs, and onto the rows of its frames; the frames before the first record
// keep the camera state at the call.
int smooth_last_record(ekf_filter* f, const SmoothPass& p) {
    const EkfSmoothRec& last = f->hist.table[p.R - 1];
    HIP_TRY(hipMemcpyAsync(p.a.xs, p.hist + last.off, (size_t)last.dims * 8, hipMemcpyDeviceToDevice, f->stream));
    ekf_launch_smooth_rows(p.hist + last.off, p.a.smoothed, last.frame0, last.frame1, f->stream);
    ekf_launch_smooth_rows(p.hist, p.a.smoothed, 0, f->hist.table[0].frame0, f->stream);
    return EKF_OK;
}

// The pass has its own status word: a P_p that is not positive definite is reported here and leaves nothing sticky on the
// filter.
int smooth_end(ekf_filter* f, const SmoothPass& p) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(f->stream));
    int32_t st = 0;
    HIP_TRY(hipMemcpy(&st, p.a.status, 4, hipMemcpyDeviceToHost));
    if (st != 0) return fail(EKF_ERR_NUMERIC, "smoothing: a predicted covariance P_p is not positive definite");
    return EKF_OK;
}

}  // namespace

extern "C" {

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
    int rc = history_ready(f, f->hist.buf, f->hist.bytes);
    if (rc) return rc;
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
    if ((rc = history_ready(f, history_dev, f->hist.bytes, true))) return rc;
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

int ekf_smooth_workspace_bytes(const ekf_filter* f, size_t* bytes) { return smooth_workspace_bytes(f, bytes, false); }

int ekf_smooth_history(ekf_filter* f, const void* history_dev, size_t history_bytes, void* ws, size_t ws_bytes, int32_t flags,
                       double* smoothed_dev) {
    SmoothPass p;
    int rc = smooth_begin(f, history_dev, history_bytes, ws, ws_bytes, flags, false,
                          smoothed_dev ? nullptr : "smoothed_dev is NULL", smoothed_dev, &p);
    if (rc || p.F == 0) return rc;
    if (p.R == 0) {      // nothing changed the filter: every row is the camera state at the call
        ekf_launch_smooth_rows(p.hist, smoothed_dev, 0, p.F, f->stream);
        HIP_TRY(hipGetLastError());
        return EKF_OK;
    }
    const std::vector<EkfSmoothRec>& table = f->hist.table;
    if (p.resident) {
        HIP_TRY(ekf_launch_smooth_resident(p.hist, p.table_dev, p.R, (int32_t)p.nmax, table[0].frame0, smoothed_dev, p.a.status,
                                           f->stream));
    } else {
        EkfSmoothBlocked a = p.a;
        if ((rc = smooth_last_record(f, p))) return rc;
        for (int32_t r = p.R - 2; r >= 0; --r) {
            a.rec = table[r];
            a.next = table[r + 1];
            ekf_launch_smooth_blocked_step(a, f->stream);
        }
    }
    return smooth_end(f, p);
}

// ---- smoothed covariances (include/ekf_slam_hip.h, "Smoothed covariances"; kernels: ekf_smooth_cov.hip) -------------------
int ekf_smooth_cov_workspace_bytes(const ekf_filter* f, size_t* bytes) { return smooth_workspace_bytes(f, bytes, true); }

int ekf_smooth_history_cov(ekf_filter* f, const void* history_dev, size_t history_bytes, void* ws, size_t ws_bytes, int32_t flags,
                           double* smoothed_dev, double* cam_cov_dev, double* filt_cam_cov_dev, double* first_cov_dev) {
    SmoothPass p;      // (the covariance pass has one tier: no flag is read)
    int rc = smooth_begin(f, history_dev, history_bytes, ws, ws_bytes, flags, true,
                          smoothed_dev && cam_cov_dev ? nullptr : "smoothed_dev or cam_cov_dev is NULL", smoothed_dev, &p);
    if (rc || p.F == 0) return rc;
    if (p.R == 0) {      // nothing changed the filter: the start pose on every row, and no covariance was ever recorded
        ekf_launch_smooth_rows(p.hist, smoothed_dev, 0, p.F, f->stream);
        ekf_launch_smooth_cov_nan(cam_cov_dev, filt_cam_cov_dev, 0, p.F, f->stream);
        HIP_TRY(hipGetLastError());
        return EKF_OK;
    }
    const std::vector<EkfSmoothRec>& table = f->hist.table;
    const SmoothLayout& L = p.L;
    char* w = static_cast<char*>(ws);
    EkfSmoothCov a{};
    a.b = p.a;
    a.A = reinterpret_cast<double*>(w + L.A);
    a.Z = reinterpret_cast<double*>(w + L.Z);
    a.T = reinterpret_cast<double*>(w + L.T);
    a.Ps = reinterpret_cast<double*>(w + L.Ps);
    a.ldp = L.npad;
    a.cam_cov = cam_cov_dev;
    a.filt_cam_cov = filt_cam_cov_dev;
    a.first_cov = first_cov_dev;
    // (P^s keeps its leading dimension over the pass; zero first, so that what a smaller record leaves unwritten is finite)
    HIP_TRY(hipMemsetAsync(a.Ps, 0, (size_t)L.npad * L.npad * 8, f->stream));
    if ((rc = smooth_last_record(f, p))) return rc;
    ekf_launch_smooth_cov_nan(cam_cov_dev, filt_cam_cov_dev, 0, table[0].frame0, f->stream);
    a.b.rec = table[p.R - 1];
    a.first = p.R == 1;
    ekf_launch_smooth_cov_last(a, f->stream);
    for (int32_t r = p.R - 2; r >= 0; --r) {
        a.b.rec = table[r];
        a.b.next = table[r + 1];
        a.first = r == 0;
        ekf_launch_smooth_cov_step(a, f->stream);
    }
    return smooth_end(f, p);
}

}  // extern "C"
