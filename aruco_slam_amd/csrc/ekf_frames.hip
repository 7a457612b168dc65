// C ABI of the EKF-SLAM HIP library (see include/ekf_slam_hip.h), the filter handle (ekf_filter.h): the frame scheduler and
// every call that steps frames from the caller's arrays -- ekf_observe*, ekf_move, ekf_advance, ekf_observe_device,
// ekf_observe_sequence_device*.  The per-frame host path, from those entry points down to enqueue_frame, is all in this file;
// the log replay (ekf_log_api.hip) comes in through the per-call functions at the end of ekf_filter.h.
#include <atomic>
#include <cmath>
#include <cstring>

#include "ekf_filter.h"

// Pipelined sequence mode orders its two streams with device-side gates that spin.  HIP multiplexes streams onto a small
// pool of hardware queues: with two handles pipelining at once, handle X's gate can sit in the queue in front of the
// launch handle Y's gate waits for, and vice versa -- both poll budgets run out.  So at most ONE handle of the
// process has gates in flight; another handle that asks for the pipelined mode meanwhile runs its call in serial order
// (same results, bit for bit) and says so (ekf_last_sequence_mode).
static std::atomic<ekf_filter*> g_pipelining{nullptr};

void release_pipelining_token(ekf_filter* f) { (void)g_pipelining.compare_exchange_strong(f, nullptr); }

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

namespace {

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

// The first sightings of a frame (log replay): the add-marker launch that places them from the camera as it is on the
// device; the map grows by them.  Returns their number.
int first_sightings(ekf_filter* f, const RunFrame& r) {
    if (r.nnew > 0)
        by_cov_type(f, [&](auto elem) {
            ekf_launch_log_add_markers<decltype(elem)>(f->cfg.model, f->cov, f->ld, f->state, f->dims(), r.poses, r.new_slots,
                                                       f->cfg.initial_landmark_uncertainty, r.nnew, f->stream);
        });
    f->n_lm += r.nnew;
    return r.nnew;
}

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
// next-frame indices >= n_lm, and the new rows exist in neither covariance buffer).  frame_of(t): frame t; of it, m (0: not
// stepped) and nnew, how many of its detections are first sightings.
template <class FrameOf>
RunPlan plan_runs(const ekf_filter* f, int frames, FrameOf frame_of) {
    RunPlan p;
    p.candidate.assign((size_t)frames, 0);
    p.joins.assign((size_t)frames, 0);
    int prev_kpad = -1;          // kpad of the previous stepped frame if it was a candidate, else -1
    int nn = f->n_lm;
    for (int t = 0; t < frames; ++t) {
        const int m = frame_of(t).m;
        if (m == 0) continue;
        const int nnew = frame_of(t).nnew;
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
// stepped frame in serial order.  frame_of(t): frame t (m == 0: not stepped).  The run before a frame with first sightings
// ends first, so that the new landmarks see the camera the previous frame left on the device (first_sightings).  stats
// (ekf_last_log_stats, or null): stepped frames, pipelined frames, runs, new landmarks.
// The covariance ping-pongs between the caller's buffer and the second one across runs: a run with an odd number of frames
// leaves it in the other buffer, and everything after it (serial frames, first sightings, the next run) works there; one
// copy at the end brings it back.
template <class FrameOf>
int run_frames(ekf_filter* f, int frames, FrameOf frame_of, const RunPlan& plan, bool pipe_ok, int64_t* stats) {
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
        const int nnew = first_sightings(f, frame_of(t));
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

}  // namespace

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

namespace {

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

}  // namespace

// One frame in serial order (a sequence call's loop, the log replay's frame-by-frame loop; device arrays, no host mirror): its
// motion, its first sightings (placed from the moved camera), the gate on the prior they leave and the frame on its survivors,
// or the plain frame; rules 3 and 4 of the scale around it unless the caller ran them over the whole call (x->folded).  A
// frame without detections or without a survivor is not stepped: its scale stays pending, its row repeats the camera state.
int serial_frame(ekf_filter* f, const RunFrame& r, SerialFrame* x) {
    int rc = enqueue_motion(f, x->motion, &x->moved);
    if (rc) return rc;
    x->s_eff = x->folded ? r.s_eff : frame_scale(f, x->scale);
    x->survivors = r.m;
    if (r.m > 0) {
        const int nnew = first_sightings(f, r);      // (rule 4 of the gate: they are the exempt detections)
        rc = x->gated ? gated_frame(f, r.idx, r.z, r.rows, r.m, x->exempt, nnew, x->mahal, nullptr, r.traj_row, false,
                                    &x->survivors, x->s_eff)
                      : enqueue_frame(f, r.idx, r.z, r.rows, r.m, r.traj_row, false, x->s_eff);
        if (rc) return rc;
    }
    if (!x->folded) frame_scale_done(f, x->scale, x->s_eff, x->survivors > 0);
    return x->survivors == 0 ? repeat_row(f, r.traj_row) : EKF_OK;
}

int plan_frames(ekf_filter* f, const std::vector<RunFrame>& frames, RunPlan* plan, int* mode) {
    *plan = plan_runs(f, (int)frames.size(), [&](int t) -> const RunFrame& { return frames[t]; });
    return choose_pipelining(f, plan->want_runs, mode);
}

int run_planned_frames(ekf_filter* f, const std::vector<RunFrame>& frames, const RunPlan& plan, int mode, int64_t* stats) {
    return run_frames(f, (int)frames.size(), [&](int t) -> const RunFrame& { return frames[t]; }, plan,
                      mode == EKF_SEQ_PIPELINED, stats);
}

namespace {

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

}  // namespace

extern "C" {

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
    std::vector<double> s_effs;      // per frame, once rules 3 and 4 have run over the call (the serial loop: frame by frame)
    auto frame_of = [&](int t) {
        return RunFrame{lm_index_dev + (size_t)t * m, z_dev + (size_t)t * m * rd, m,
                        trajectory_dev ? trajectory_dev + (size_t)t * 7 : nullptr,
                        rows_dev ? rows_dev + (size_t)t * m * rd : nullptr, s_effs.empty() ? 1.0 : s_effs[t]};
    };
    if (f->gate_on() || motion || f->frozen) {
        // a frozen map: frame by frame in serial order, the camera strip behind every front part.
        // a gate is set: frame by frame in serial order, each frame on its survivors (gating inside a pipelined run would
        // need the mask inside the front kernel).  Motions: serial order as well -- a front kernel of a run completes
        // P_{t+1} from P_t and W_t, and a motion between the two frames changes rows of it
        f->seq_mode = EKF_SEQ_SERIAL;
        f->shortcut.log();      // (a getter after the call waits for all of it)
        for (int t = 0; t < frames; ++t) {
            SerialFrame x;
            x.motion = motion ? motion + (size_t)t * 6 : nullptr;
            x.scale = scale ? scale + t : nullptr;
            x.gated = f->gate_on();
            if ((rc = serial_frame(f, frame_of(t), &x))) return rc;
        }
        f->shortcut.log();
        return EKF_OK;
    }
    // every frame is stepped: the pending scale goes into the first one (rule 3), and none is left
    s_effs.assign((size_t)frames, 1.0);
    for (int t = 0; t < frames; ++t) {
        s_effs[t] = frame_scale(f, scale ? scale + t : nullptr);
        frame_scale_done(f, scale ? scale + t : nullptr, s_effs[t], true);
    }
    // Pipelined mode (F(t+1) beside C(t), see run_pipelined) for the whole call if pipeline_wanted admits the frame shape
    const RunPlan plan = plan_runs(f, frames, frame_of);
    int mode = EKF_SEQ_SERIAL;
    rc = choose_pipelining(f, plan.want_runs, &mode);
    if (rc) return rc;
    f->seq_mode = mode == EKF_SEQ_PIPELINED ? EKF_SEQ_SERIAL : mode;     // (PIPELINED once the run is enqueued)
    rc = run_frames(f, frames, frame_of, plan, mode == EKF_SEQ_PIPELINED, nullptr);
    if (rc) return rc;
    f->seq_mode = mode;
    return EKF_OK;
}

}  // extern "C"
