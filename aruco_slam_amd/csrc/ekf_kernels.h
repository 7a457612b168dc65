// Host-visible launch interface of the EKF kernels (internal to the library).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ekf_device.h"

// status word bits (sticky until ekf_reset; decoded by sync_and_check in ekf_api.hip)
#define EKF_ST_NOT_SPD 1          // a pivot of the innovation covariance was not positive
#define EKF_ST_TIMEOUT 4          // a bounded exchange wait inside the fused front kernel ran out
#define EKF_ST_STALE_JAC 16       // a chunk accepted Jacobian rows that carry another frame's tag
#define EKF_ST_STALE_COL 32       // a chunk accepted a factor block column that carries another frame's tag
#define EKF_ST_STALE_S 64         // the factorisation accepted an S block / residual that carries another frame's tag
#define EKF_ST_BAD_INDEX 128      // a landmark index outside [0, n_lm) reached a kernel (clamped to 0 there)
#define EKF_ST_GATE_TIMEOUT 256   // pipelined sequence mode: a device-side wait for the other stream ran out

// Everything one frame's kernels need; passed by value.
struct EkfFrame {
    void* cov;             // P, f32 or f64, row-major, leading dim ld
    int64_t ld;
    double* state;         // [cap]
    int32_t model;         // 0 = EKF, 1 = EKF_Rotations (see EkfModel in ekf_device.h)
    int32_t dims;          // N = lmd n + 10
    int32_t ncols;         // N rounded up to 128 (<= ld): columns the panel covers
    int32_t m;             // detections this frame
    int32_t k;             // 3 m
    int32_t kpad;          // k rounded up to EKF_RB
    const int32_t* idx;    // [m] landmark indices (device)
    const double* z;       // [m,3] measured positions, camera frame (device)
    double* jac;           // [kmax, EKF_JLD] Jacobian rows (13 used)
    double* resid;         // [kmax] z - h
    int32_t* lmcol;        // [mmax] first state column of each detection
    double* amat;          // A = H (P+Q), [kmax, lda] f64
    int64_t lda;
    double* sblk;          // S = Hs (P+Q)[supp,supp] Hs^T + R in 16x16 blocks (lower block triangle), block (i, tc) at
                           // (i (i + 1) / 2 + tc) * 256 in OP memory order (ekf_solve_device.h); diagonal blocks symmetric
    // Per-detection measurement noise (EKF_FLAG_ROW_NOISE; include/ekf_slam_hip.h): the variance of every measurement row of
    // the frame, [k] in the order of z (device, or pinned host), S = H (P+Q) H^T + diag(rrow); null: the constant nz.r_unc.
    // (It takes the eight bytes of a retired int32 and the padding behind it: every other argument is where it was, and
    // the kernel arguments keep their size.)
    const double* rrow;
    double* lmat;          // Cholesky factor L of S, [kmax, ldl] f64 (lower)
    int32_t ldl;
    double* dinv;          // inverse of the 16x16 diagonal blocks of L, [kmax/16,16,16]
    // the same factor pre-arranged as v_mfma_f64_16x16x4 A operands (one
    // coalesced 512-byte read per MFMA in the panel kernel):
    //   lop[((b(b-1)/2 + q) 4 + r) 64 + lane] = -L[16b + (lane&15)][16q + (lane>>4) + 4r], q < b
    //   dop[(4 b + r) 64 + lane]             = Dinv_b[lane&15][(lane>>4) + 4r]
    double* lop;
    double* dop;
    double* yvec;          // L^-1 (z - h), [kmax]
    void* wpanel;          // W = L^-1 A, [kmax, ldw], cov dtype, k-major
    int64_t ldw;
    double* wdbg;          // optional f64 copy of W for tests (may be null)
    int32_t* status;       // [0] sticky error bits (EKF_ST_*), [1..2] diagnostics of the first non-SPD block column
    double* traj_row;      // optional: state[0:7] after the update
    double* dxvec;         // model 1: dx = W^T y for every state dimension (input of the injection kernel)
    long long* stamps;     // optional: s_memtime stamps of the solve kernel's phases (diagnostics)
    int32_t stamps_heavy;  // 0: only the stamps at the start / end of the roles (a stamp is a global store: the wave that takes it
                           // later waits for its acknowledgement), 1: also inside the factorisation and the chunk prologue
    // Pipelined sequence mode (ekf_frames.hip: ekf_observe_sequence_device).  The covariance lives in TWO buffers: the
    // update of frame t reads `cov` (P_t) and writes `cov_out` (P_{t+1}); the front kernel of frame t+1 runs beside it
    // and takes the entries of P_{t+1} it needs -- support rows only -- from P_t and W_t on the fly:
    //     P_{t+1}[r][c] = (P_t[r][c] + Q[r == c]) + sum_k fma(-W_t[k][r], W_t[k][c])     (k ascending, from zero)
    // which is, instruction for instruction, what the covariance update computes for that element (bitwise equal).
    // For such a front kernel `cov` is P_t (the PREVIOUS frame's input), `wprev` the previous frame's W panel and
    // `wsup_prev` the compact copy of its support columns, W_t[:, row(slot)], slot = 10 + lmd j + d for detection
    // j of THIS frame (written by the previous front kernel's chunks, which know this frame's indices: next_idx).
    const int32_t* next_idx;   // [next_m] landmark indices of the next frame (device); null: none
    int32_t next_m;
    void* cov_out;             // covariance update: destination (null = in place)
    const void* wprev;         // front kernel: W panel of the previous frame [kpad][ldw] (null = `cov` is current)
    const void* wsup_prev;     // front kernel: [kpad][wsup_ld], see above
    // device-side cross-stream ordering of the pipelined sequence mode (ekf_frames.hip: run_pipelined):
    // la_sync[0] = "front kernel of frame n has started" counter, la_sync[1] = "covariance update of frame n is
    // complete" counter.  A front kernel stores la_signal into [0] when it starts (0 = no) and does not
    // finish before [1] >= la_gate (0 = no gate).  A covariance update stores cov_signal into [1] itself once all its
    // workgroups' stores are complete (ekf_cov_arrive; 0 = no: serial order and the last update of a run execute no atomic);
    // la_sync[EKF_SYNC_SHARD(..)] count its workgroups and are zero again when the launch ends.
    unsigned long long* la_sync;
    unsigned long long la_signal, la_gate;
    unsigned long long cov_signal;
    long long* gate_log;       // optional (diagnostics, role-level stamps): per-frame ring of the front kernel's end gate,
                               // [EKF_GATE_LOG_FRAMES][4] = {launch started, gate entered, gate left, polls} by frame number
    int32_t lds_min;           // front kernel: claim at least this much LDS (keeps other kernels' workgroups off its CUs)
    void* wsup;                // pipelined mode, written by the chunks: W[:, support rows of the NEXT frame], [kpad][wsup_ld] in cov dtype (null: none)
    int32_t wsup_ld;
    EkfNoise nz;               // this frame's noise: Q_eff = fl(s_eff q) per entry (formed on the host), and r_unc
    int32_t quat_mode;
    // fused front kernel (ekf_front_impl.h): exchange buffers between its workgroups.  ONE buffer per
    // fused-frame parity holds everything that travels between workgroups inside a launch:
    //   [-L operands | Dinv operands | y | Jacobian rows [k][JC] | tags | S blocks | residual | S-block tags]
    // Every word is sentinel-armed (EKF_SENT_BITS) until its producer overwrites it; the buffer of
    // parity p is re-armed during the NEXT fused frame (parity p^1) by that frame's S-block
    // workgroups, i.e. at least one kernel boundary after its last reader and one before its next
    // writer.  No role ever re-arms what it has just read.
    double* xl;                // this frame's exchange buffer
    double* xl_next;           // the other buffer, re-armed during this frame for the next fused frame
    int32_t xl_dop, xl_y, xl_jac;   // offsets (doubles) of the Dinv operands, y and the Jacobian rows inside xl
    int32_t xl_len;            // doubles per buffer
    double* xs;                // = xl + offset: S blocks, layout of sblk (OP memory order)
    double* xr;                // = xl + offset: [kmax] z - h (0 for rows k..kpad-1)
    double* xs_tag;            // = xl + offset: frame tag of S block (row block i, block column tc) at [16 tc + i]
    int32_t n_lm;              // landmarks in the state (index validation; model 1 injection)
    unsigned long long* done_ctr;      // chunks finished since reset (device)
    unsigned long long done_target;    // value of done_ctr once this frame's last chunk is done
    int32_t xl_tag;                    // frame tags inside xl ([0] Jacobian, [1 + q] block column q, [16] residual): integrity check
    double seqno;                      // this frame's tag (fused frames since reset, from 1)
    // Per-frame host boundary (ekf_observe + a state getter every frame): the injection code of the fused front kernel
    // also writes the new state into pinned HOST memory, and whoever raises a status bit also sets a word there, so
    // that the getter is a wait for the front kernel's event and a memcpy -- no device-to-host copies (null: off).
    double* state_host;
    int32_t* status_host;
    // Large problems (f32 covariance): launch order of the 128 x 128 macro-tile covariance update (ekf_cov_macro.hip):
    // tile (I << 16 | J) of block b, 0xFFFFFFFF = none; null: the wave-per-tile kernel (ekf_cov_update.hip)
    const uint32_t* cov_tiles;
    int32_t cov_grid;
    // Pipelined sequence mode with per-frame process-noise scales (EKF_FLAG_FRAME_SCALE): the front kernel completes rows of
    // P_{t+1} with the PREVIOUS frame's Q (the covariance update it stands in for ran with that frame's nz) and predicts
    // with its own.  q_cam / q_err / q_lm of the previous frame of the run; equal to nz's without scales, and read only by
    // the front-kernel instances a frame with another Q than its predecessor's runs (ekf_front_impl.h: QPREV).  At the end:
    // every other argument is where it was (the kernel arguments grow from 504 to 528 bytes).
    double qprev_cam, qprev_err, qprev_lm;
    // Frozen map (include/ekf_slam_hip.h, "Localisation mode"): non-zero = the injection writes the camera only -- dx[0:3], the
    // quaternion rule on dx[7:10], state[7:10] = 0; EKF_Rotations: block 0 -- and every landmark entry of the state and of
    // the pinned mirror keeps its bits.  Everything up to W and dx is the mapping frame's.  At the end, as the qprev fields
    // before it: every other argument is where it was (the kernel arguments grow from 528 to 536 bytes).
    int32_t frozen;
};

// process-noise diagonal of state dimension i as the PREVIOUS frame of a pipelined run added it (ekf_qdiag on its Q_eff)
__device__ __forceinline__ double ekf_qdiag_prev(const EkfFrame& fr, int i) {
    return ekf_qdiag(i, fr.dims, EkfNoise{fr.qprev_cam, fr.qprev_err, fr.qprev_lm, 0.0});
}

// variance of measurement row r: the one thing of a frame the rows change (the diagonal of S)
__device__ __forceinline__ double ekf_row_noise(const EkfFrame& fr, int r) { return fr.rrow ? fr.rrow[r] : fr.nz.r_unc; }

// raise sticky status bits (and tell the host mirror, if there is one, that the status word is no longer zero)
__device__ __forceinline__ void ekf_raise(const EkfFrame& fr, int bits) {
    atomicOr(fr.status, bits);
    if (fr.status_host) __hip_atomic_store(fr.status_host, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Pipelined sequence mode: "this covariance update is complete", stored by the update itself (fr.cov_signal != 0; every
// wave of every workgroup of the launch calls ekf_cov_arrive exactly once, waves and workgroups without a tile included).
// A wave waits for the acknowledgement of its own write-through stores to cov_out, the workgroup barrier collects the
// waves, and ONE thread per workgroup counts the workgroup (a count per wave would put ~4.8k atomics on one address at
// the tail of the n=1024 launch, whose waves finish in phase).  The count is sharded: workgroup b counts on shard b & 7,
// the workgroup that completes a shard counts the shard on a second level, and the one that completes that stores the
// signal at system scope.  ONE counter for all 1204 workgroups of the headline launch cost 2.6 us per pipelined frame
// (measured, n=1024 m=32 f32, us per frame of 2000-frame calls: signal kernel 23.5 - 23.7, one counter 26.1 - 26.5, the
// same without the wait for the stores 25.7 - 26.0, 8 shards 23.2 - 23.3, 32 / 64 shards 23.3 - 23.5; counting the waves
// in LDS instead of the barrier: 27.0 - 27.3 with one counter, 23.5 - 23.8 with 8 shards).
// Whoever completes a count re-arms it -- the next launch that counts follows on the same stream -- so the counters need
// no host state: whatever runs to its end leaves them zero (a call that ends in a sticky error included), ekf_reset and
// ekf_grow zero the workspace, and every handle has its own.  Every store of the launch was acknowledged before the
// atomic of its workgroup was issued, so it is at the device's coherence point before the signal.
#define EKF_COV_SHARDS 8
#define EKF_SYNC_SHARD(s) (32 + 32 * (s))     // word of la_sync: shard s < EKF_COV_SHARDS, second level s = EKF_COV_SHARDS (256 B apart)
#define EKF_SYNC_WORDS EKF_SYNC_SHARD(EKF_COV_SHARDS + 1)
#define EKF_GATE_LOG_FRAMES 2048              // frames in the gate_log ring
__device__ __forceinline__ bool ekf_cov_count(unsigned long long* ctr, unsigned long long full) {
    if (__hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 != full) return false;
    __hip_atomic_store(ctr, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}
__device__ __forceinline__ void ekf_cov_arrive(const EkfFrame& fr) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (threadIdx.x == 0) {
        const unsigned grid = gridDim.x, sh = blockIdx.x % EKF_COV_SHARDS;
        const unsigned in_shard = (grid + EKF_COV_SHARDS - 1 - sh) / EKF_COV_SHARDS;      // workgroups b with b % 8 == sh
        const unsigned shards = grid < EKF_COV_SHARDS ? grid : EKF_COV_SHARDS;            // shards with a workgroup
        if (ekf_cov_count(fr.la_sync + EKF_SYNC_SHARD(sh), in_shard) &&
            ekf_cov_count(fr.la_sync + EKF_SYNC_SHARD(EKF_COV_SHARDS), shards))
            __hip_atomic_store(fr.la_sync + 1, fr.cov_signal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// First state column of detection j.  Indices that arrive through the device-pointer entry points
// cannot be checked on the host: an index outside [0, n_lm) is clamped to 0 (so that nothing is read
// or written out of bounds) and, where `flag` is set, recorded in the status word -> EKF_ERR_INVALID
// at the next synchronising call.
__device__ __forceinline__ int ekf_lm_column(const EkfFrame& fr, int lmd, int j, bool flag) {
    int i = fr.idx[j];
    if ((unsigned)i >= (unsigned)fr.n_lm) {
        if (flag) ekf_raise(fr, EKF_ST_BAD_INDEX);
        i = 0;
    }
    return EKF_CAM + lmd * i;
}

// EKF model: the camera part of the state injection (extended_kalman_filter.py:138-152) once the additive part is done:
// err = dx[7:10], x = the new camera position state[0:3].  Shared by the panel kernel and the wide-frame finish kernel.
__device__ inline void ekf_inject_camera(const EkfFrame& fr, const double err[3], const double x[3]) {
    double q[4] = {fr.state[3], fr.state[4], fr.state[5], fr.state[6]};
    ekf_quat_inject(q, err, fr.quat_mode);
    for (int i = 0; i < 4; ++i) fr.state[3 + i] = q[i];
    for (int i = 0; i < 3; ++i) fr.state[7 + i] = 0.0;   // :152
    if (fr.traj_row) {
        fr.traj_row[0] = x[0]; fr.traj_row[1] = x[1]; fr.traj_row[2] = x[2];
        for (int i = 0; i < 4; ++i) fr.traj_row[3 + i] = q[i];
    }
}

// fused gather + solve + panel (+ injection); see ekf_front_impl.h
template <typename T> void ekf_launch_front(const EkfFrame& fr, hipStream_t s);
template <typename T> void ekf_launch_gather(const EkfFrame& fr, hipStream_t s);
void ekf_launch_solve(const EkfFrame& fr, hipStream_t s);
template <typename T> void ekf_launch_panel(const EkfFrame& fr, hipStream_t s);
// P <- P + Q - W^T W.  variant: 1 = VALU reference kernel, 2 = MFMA kernel.
// e0 / e1 (optional): events that receive the kernel's own start / stop time stamps (hipExtLaunchKernelGGL)
template <typename T> void ekf_launch_cov_update(const EkfFrame& fr, int variant, hipStream_t s,
                                                 hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// Frozen map (ekf_cov_strip.hip): the camera strip of the same update, in place: rows and columns 0 .. 9 of P get the value
// the full update gives them (the same fma chain per element), P[10:N, 10:N] is neither read nor written.  e0 / e1 as above.
// variant: the covariance update the handle runs (1 = VALU reference kernel, 2 = MFMA): the strip takes its chain step, which
// differs between the two for the f32 covariance.  false: nothing was launched, fr.kpad exceeds EKF_WIDE_REUSE_ROWS (the
// caller chunks such a frame).
#define EKF_STRIP_THREADS 256
template <typename T> bool ekf_launch_cov_strip(const EkfFrame& fr, int variant, hipStream_t s, hipEvent_t e0 = nullptr,
                                                hipEvent_t e1 = nullptr);
// f32, large problems: one workgroup per 128 x 128 macro tile, launch order fr.cov_tiles / fr.cov_grid (ekf_cov_macro.hip)
void ekf_launch_cov_update_macro(const EkfFrame& fr, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// launch order for T x T macro tiles (lower triangle), super-tiles of S x S dealt to the 8 XCDs: returns the grid size
// (out == nullptr: only that), -1 if it exceeds `capacity` entries
int ekf_cov_macro_table(int T, int S, uint32_t* out, int capacity);
// pipelined sequence mode: one-wave kernels that order the two streams on the device
void ekf_launch_gate(unsigned long long* counter, unsigned long long target, int32_t* status, hipStream_t s,
                     int max_polls = 1 << 22);
void ekf_launch_signal(unsigned long long* counter, unsigned long long value, hipStream_t s);

// Wide frames (ekf_wide.hip): more detections than the gather kernel takes (EKF m > 64, EKF_Rotations m > 50).
// kpad <= EKF_WIDE_REUSE_ROWS: measurement, A and S (into `sblk`), then the stage solve / panel kernels.  Beyond: S into
// `lmat`, blocked Cholesky over block columns of EKF_WIDE_BLOCK rows (rows padded to rp = k rounded up to that), with A
// copied to `aw` [rp][lda] f64 and turned into W there; `xinv`: EKF_WIDE_BLOCK^2 doubles (per block column, xinv_stride
// doubles apart, when xinv_stride != 0: the covariance smoother reads every L_BB^-1 again).
#define EKF_WIDE_REUSE_ROWS 384
#define EKF_WIDE_BLOCK 64
template <typename T> void ekf_launch_wide_front(const EkfFrame& fr, double* aw, int rp, hipStream_t s);
void ekf_launch_wide_factor(const EkfFrame& fr, double* aw, double* xinv, int rp, hipStream_t s, int64_t xinv_stride = 0);
template <typename T> void ekf_launch_wide_finish(const EkfFrame& fr, const double* aw, hipStream_t s);

template <typename T>
void ekf_launch_add_markers(void* cov, int64_t ld, double* state, int32_t dims,
                            const double* xyz_dev, const double* unc_dev, double default_unc,
                            int32_t count, hipStream_t s);
void ekf_launch_inject_rot(const EkfFrame& fr, int n_lm, hipStream_t s);
template <typename T>
void ekf_launch_add_markers_rot(void* cov, int64_t ld, double* state, int32_t dims, const double* pose6_dev,
                                const double* unc_dev, double default_unc, int32_t count, hipStream_t s);
// Log replay (ekf_log.hip, ekf_observe_log): z of every detection of the log from its pose [count][6] (rd = 3: pose[0:3];
// rd = 7: [pose[0:3] | quaternion of the xyz Euler angles pose[3:6], scalar first]); first sightings gathered from the
// logged poses by slot (default uncertainty); trajectory rows of empty frames from pinned (row, source) pairs.
void ekf_launch_log_prepare(const double* poses_dev, int64_t count, int rd, double* z_dev, hipStream_t s);
template <typename T>
void ekf_launch_log_add_markers(int model, void* cov, int64_t ld, double* state, int32_t dims, const double* poses_dev,
                                const int32_t* slots_dev, double default_unc, int32_t count, hipStream_t s);
void ekf_launch_log_fill_rows(double* traj_dev, const int32_t* pairs, int32_t count, const double* state, hipStream_t s);
// Per-detection chi-square gate of one frame (ekf_gate.hip; EKF_FLAG_GATE): d^2 of every detection on the prior, and the
// survivors compacted in log order.  One workgroup of EKF_GATE_THREADS threads, whatever m.
#define EKF_GATE_THREADS 256
struct EkfGateArgs {
    const void* cov;            // P, f32 or f64 (widened on load), leading dimension ld
    int64_t ld;
    const double* state;
    int32_t n_lm, dims, m;
    const int32_t* idx;         // [m] landmark indices (device, or pinned host)
    const double* z;            // [m, rd]
    const uint8_t* exempt;      // [m] or null: non-zero = d^2 = 0 is reported and the detection is never rejected
    EkfNoise nz;
    double gate;                // +inf: nothing is rejected
    double* mahal;              // [m] or null
    double* mahal_host;         // [m] pinned host or null: the same values for a host caller
    int32_t* out_idx;           // [<= m] indices of the survivors, in log order
    double* out_z;              // [<= m, rd]
    const double* rows;         // [m, rd] or null: per-detection noise, the variances of every detection's rows
    double* out_rows;           // [<= m, rd]: the survivors' rows (rows != null)
    int32_t* status;            // the filter's status words ([0] != 0: nothing is tested any more, everything stays)
    int32_t* status_host;       // pinned mirror of "the status word is no longer zero", or null
    int32_t* result_host;       // pinned: [0] survivors (what the host waits for), [1] some pivot failed (diagnostic only: the
                                // frame's own factorisation reports the failure, as it does without a gate)
};
template <typename T> void ekf_launch_frame_gate(int model, const EkfGateArgs& a, hipStream_t s);
// Camera motion between frames (ekf_motion.hip; EKF_FLAG_MOTION; arithmetic: ekf_motion_device.h): the camera moves by
// u = (d, w) in its own frame, P <- F~ P F~^T on rows and columns 0 .. 9.  One thread per column of the strip P[0:10, 10:N]
// (EKF_MOTION_THREADS per workgroup); workgroup 0 also owns the 10 x 10 block.  Every workgroup forms F from the OLD camera
// state, so the new one is stored only once all of them are over: by the one workgroup itself when the grid is one
// workgroup, by a second one-thread launch behind the first otherwise.
#define EKF_MOTION_THREADS 256
struct EkfMotionArgs {
    void* cov;                  // P, f32 or f64 (widened on load, rounded once on store), leading dimension ld
    int64_t ld;
    double* state;
    int32_t dims;               // N: nothing at or beyond it is read or written
    double u[6];                // the motion (d, w)
    const int32_t* status;      // the filter's status words ([0] != 0: a failed filter ignores motions)
};
template <typename T> void ekf_launch_motion(const EkfMotionArgs& a, hipStream_t s);
template <typename T>
void ekf_launch_cov_diag(const void* cov, int64_t ld, double* out_dev, int32_t count, hipStream_t s);

// Offline smoothing (ekf_smooth.hip; include/ekf_slam_hip.h: the smoothing rules; arithmetic: ekf_smooth_device.h).
// A history is [256 B: state[0:7] at the start of the recorded call | records]; record r at `off` doubles from the start of
// the history: state[0:dims], then the lower triangle of P packed column by column (ekf_smooth_tri), all f64.
#define EKF_SMOOTH_RESIDENT_DIMS 160      // resident tier: every record has at most this many dims (n <= 50)
#define EKF_SMOOTH_THREADS 512
struct EkfSmoothRec {
    int64_t off;                // doubles from the start of the history
    int32_t dims;               // N_r
    int32_t moved;              // the transition INTO this record starts with the motion u (0: u is zero)
    double u[6];
    double q[3];                // Q_eff of the transition into this record: fl(s_eff q_cam), fl(s_eff q_err), fl(s_eff q_lm)
    int32_t frame0, frame1;     // output rows [frame0, frame1) take this record's smoothed pose
};
// the pack launch of a recorded replay: state[0:dims] and the lower triangle of P (f64, leading dimension ld) into a record
void ekf_launch_history_pack(const double* cov, int64_t ld, const double* state, int32_t dims, double* record, hipStream_t s);
// trajectory rows [f0, f1) <- src[0:7]
void ekf_launch_smooth_rows(const double* src, double* smoothed, int32_t f0, int32_t f1, hipStream_t s);
// Resident tier: ONE launch of ONE workgroup runs the whole backward pass; P_p as a packed triangle of nmax dims in dynamic
// LDS.  status[0] |= EKF_ST_NOT_SPD when a pivot of a P_p is not positive.  Returns the error of the attribute call.
hipError_t ekf_launch_smooth_resident(const double* history, const EkfSmoothRec* table_dev, int32_t records, int32_t nmax,
                                      int32_t lead_frames, double* smoothed, int32_t* status, hipStream_t s);
// Blocked tier: one backward step, r+1 -> r, as a short launch sequence.  Workspace pieces (all device): M [npad][npad] with
// npad = dims of `rec` rounded up to EKF_WIDE_BLOCK, xs (x^s, in and out), xp, yv [npad], wv, cv, xinv [64 * 64].
struct EkfSmoothBlocked {
    const double* history;
    EkfSmoothRec rec, next;     // record r and record r + 1
    double *M, *xs, *xp, *yv, *wv, *cv, *xinv;
    double* smoothed;
    int32_t* status;            // [0] sticky EKF_ST_NOT_SPD, [1..2] diagnostics of the factorisation kernels
};
void ekf_launch_smooth_blocked_step(const EkfSmoothBlocked& a, hipStream_t s);
// The step's two halves around the factorisation, for whoever factors with right-hand sides of its own (ekf_smooth_cov.hip):
// prepare = expand / move / Q_eff and delta (M = P_p, xp, yv), solve = backward substitution and finish (xs, the rows).
void ekf_launch_smooth_blocked_prepare(const EkfSmoothBlocked& a, hipStream_t s);
void ekf_launch_smooth_blocked_solve(const EkfSmoothBlocked& a, hipStream_t s);

// Smoothed covariances (ekf_smooth_cov.hip; include/ekf_slam_hip.h: the covariance rule): the blocked step with A = F~ P_r
// riding along the factorisation, then Z = L^-T W, T = P^s_{r+1} Z, D = -W^T W + Z^T T (lower tiles) and
// P^s_r = P_r + D mirrored over P^s_{r+1}.  Workspace pieces beyond the blocked step's (all device, npad = dims of `rec`
// rounded up to EKF_WIDE_BLOCK): xinv [npad / 64][64 * 64] (b.xinv), A, Z, T [npad][npad], Ps [ldp][ldp] with ldp fixed
// over the pass (zero at the start, so that its padding is finite).
struct EkfSmoothCov {
    EkfSmoothBlocked b;
    double *A, *Z, *T, *Ps;
    int64_t ldp;
    double* cam_cov;            // [frames][10][10]
    double* filt_cam_cov;       // [frames][10][10] or NULL
    double* first_cov;          // [N_0][N_0] or NULL; written at the step whose `rec` is record 0 (first != 0)
    int32_t first;
};
// P^s_{R-1} = P_{R-1}: b.rec is the LAST record (b.next unused); Ps and the record's output rows
void ekf_launch_smooth_cov_last(const EkfSmoothCov& a, hipStream_t s);
void ekf_launch_smooth_cov_step(const EkfSmoothCov& a, hipStream_t s);
// covariance rows [f0, f1) of cam_cov (and filt_cam_cov) <- NaN: frames before the first record
void ekf_launch_smooth_cov_nan(double* cam_cov, double* filt_cam_cov, int32_t f0, int32_t f1, hipStream_t s);
// Batch smoothing (include/ekf_slam_hip.h, "Batch smoothing"): workgroup b of ekf_batch_smooth_kernel runs the resident pass
// over member b's records.  Offsets of the table entries count doubles from the start of the WHOLE history buffer, their
// frame0 / frame1 are rows of smoothed [Ftot][7].
struct EkfBatchSmoothMember {
    int64_t table;              // the member's first entry in the tables
    int64_t head;               // doubles from the start of the history: the member's camera state at the start of the call
    int32_t records;            // R_b (0: only the lead rows are written)
    int32_t frame0, frame1;     // the member's rows of smoothed
    int32_t lead1;              // rows [frame0, lead1) repeat the start camera (before the first record)
    int32_t nan0;               // rows [nan0, frame1) are NaN: the member failed in the replay at that frame
    int32_t pad;
};
// status [B] (device) <- 0, or EKF_BATCH_ST_NUMERIC where a P_p of the member is not positive definite (all its rows: NaN).
// nmax: the dims of the call's largest record (<= EKF_SMOOTH_RESIDENT_DIMS).  Returns the error of the attribute call.
hipError_t ekf_launch_batch_smooth(const double* history, const EkfSmoothRec* tables_dev, const EkfBatchSmoothMember* members_dev,
                                   int32_t members, int32_t nmax, double* smoothed, int32_t* status, hipStream_t s);
// Batch smoothing, covariances (ekf_batch_smooth_cov.hip; include/ekf_slam_hip.h, "Batch smoothing, covariances"): workgroup
// b of ekf_batch_smooth_cov_kernel runs the resident pass over member b's records and, inside every backward step, the
// covariance rule on the factor the state step has just formed in LDS.  A member's region of the workspace holds W, Z, T
// and P^s, four [ld][ld] matrices of f64 with ld = the dims of its largest record rounded up to 16.
#define EKF_SMOOTH_COV_TILE 16
struct EkfBatchSmoothCovMember {
    int64_t region;             // doubles from `regions`: W | Z | T | P^s, ld * ld each
    int32_t ld;                 // 0 for a member without a record
    int32_t pad;
};
struct EkfBatchSmoothCov {
    const double* history;
    const EkfSmoothRec* tables;
    const EkfBatchSmoothMember* members;
    const EkfBatchSmoothCovMember* cov_members;
    double* regions;
    double* smoothed;           // [Ftot][7]
    double* cam_cov;            // [Ftot][10][10]
    double* filt_cam_cov;       // [Ftot][10][10] or NULL
    double* first_cov;          // [B][first_ld][first_ld] or NULL
    int32_t first_ld;
    int32_t nmax;               // the dims of the call's largest record (<= EKF_SMOOTH_RESIDENT_DIMS)
    int32_t* status;            // [B]
};
// dynamic LDS of the kernel for a call whose largest record has nmax dims: the triangle, the inverses of the diagonal
// blocks of L and ten rows of F P_r
size_t ekf_batch_smooth_cov_lds(int32_t nmax);
hipError_t ekf_launch_batch_smooth_cov(const EkfBatchSmoothCov& a, int32_t members, hipStream_t s);

// Batch of independent filters (ekf_batch.hip: EKF, ekf_batch_rot.hip: EKF_Rotations; frame body ekf_batch_impl.h): one
// workgroup per member, frames [member_frames[b] + window_first, + window_frames) of its log.  Everything is validated on
// the host (indices, first-sighting order, widths, capacity).
#define EKF_BATCH_MAX_LANDMARKS 82   // EKF: N = 3 n + 10 <= 256: one column per thread of the 256-thread workgroup
#define EKF_BATCH_MAX_VISIBLE 16     // EKF: k = 3 m <= 48 rows
#define EKF_BATCH_ROT_MAX_LANDMARKS 24   // EKF_Rotations: N = 10 n + 10 <= 256
#define EKF_BATCH_ROT_MAX_VISIBLE 8      // EKF_Rotations: k = 7 m <= 56 rows
#define EKF_BATCH_ST_NUMERIC (-5)    // per-member status after a failed pivot (= EKF_ERR_NUMERIC)
struct EkfBatchWindow {
    double* P;                      // [B][ld][ld] f64
    int64_t ld;
    double* state;                  // [B][ld]
    const double* noise;            // [B][6] in ekf_config order
    int32_t* status;                // [B] 0 or EKF_BATCH_ST_NUMERIC (sticky)
    int32_t* nlm;                   // [B] landmarks
    const int32_t* lm_index;        // [D]
    const int64_t* frame_offsets;   // [Ftot + 1] detection offsets, frame after frame, member after member
    const int64_t* member_frames;   // [B + 1] frame offsets per member
    const double* poses;            // [D][6] [tvec | rvec]; z = pose[0:3] (EKF), ekf_pose_z (EKF_Rotations)
    double* traj;                   // [Ftot][7] or null
    double* nis;                    // [Ftot] or null: y^T y = (z-h)^T S^-1 (z-h) of every stepped frame (0: empty frame)
    double* cam_cov;                // [Ftot][10][10] or null: P[0:10, 0:10] after every frame
    int32_t quat_mode;              // (EKF; EKF_Rotations is scalar-first)
    int32_t window_first, window_frames;
    int32_t kmax, lda;              // LDS layout: rows of A / W, row length of A / W (> N; column N holds the residual)
    const double* gate;             // [B] or null: chi^2 gate on every detection's own d^2 (+inf: off); ekf_batch_gate
    double* mahal;                  // [D] or null: d^2 per detection (0: exempt first sighting, NaN: not tested)
    const double* row_noise;        // [D][RD] or null: per-detection noise, indexed like lm_index (null: the member's r_uncertainty)
    // Per-frame process-noise scale (EKF_FLAG_FRAME_SCALE; include/ekf_slam_hip.h): pending [B] is every member's pending
    // scale, loaded at the start of a window and stored at its end (null: a batch without the flag, the constants as they
    // are); scale [Ftot] is every frame's scale, indexed like frame_offsets (null: 1 for every frame)
    double* pending;
    const double* scale;
    // Camera motion per frame (EKF_FLAG_MOTION; include/ekf_slam_hip.h, "Odometry input"): motion [Ftot][6], every frame's
    // (d, w), indexed like frame_offsets; null: no motion stage (a batch without the flag, or a call without motions)
    const double* motion;
    // Frozen maps (include/ekf_slam_hip.h, "Localisation mode"; ekf_batch_set_map_frozen): frozen [B], non-zero = that
    // member's frames update the camera strip of P and inject the camera only; null: no member of the batch is frozen, and
    // the launchers run the instances without the branch (the FROZEN instances live in ekf_batch_frozen.hip and
    // ekf_batch_wide_frozen.hip)
    const int32_t* frozen;
};
// dynamic LDS of one launch (C linkage: the tests read them)
extern "C" size_t ekf_batch_lds_bytes(int kmax, int lda);
extern "C" size_t ekf_batch_rot_lds_bytes(int kmax, int lda);
void ekf_launch_batch_window(const EkfBatchWindow& a, int members, hipStream_t s);
void ekf_launch_batch_rot_window(const EkfBatchWindow& a, int members, hipStream_t s);
// Recording (include/ekf_slam_hip.h, "Batch smoothing"; ekf_batch_recorded.hip): a second kernel argument of the RECORDED
// instances only, so the other instances keep their arguments.  All offsets count doubles from `history`.
struct EkfBatchRecord {
    double* history;                // the caller's history buffer
    const int64_t* head;            // [B] the member's header: state[0:7] at the start of the call (written by window 0)
    const int64_t* slot;            // [Ftot] the frame's record slot, -1: the frame has none (it cannot change the member)
    int32_t* flag;                  // [Ftot] 0: no record, 1: stepped, 2: moved only, -1: the member has failed
    double* s_eff;                  // [Ftot] the scale the frame was stepped with (1 without frame scales; 0: not stepped)
};
void ekf_launch_batch_recorded_window(const EkfBatchWindow& a, const EkfBatchRecord& r, int members, hipStream_t s);
// Dictionary-sized maps (EKF_FLAG_BATCH_LARGE_MAPS) and wide frames (EKF_FLAG_BATCH_WIDE_FRAMES), one kernel per model in
// ekf_batch_wide.hip: N <= 1024, ld <= 1024; A / W of a member in the batch workspace, [k][ld] at w_stride = rd max_visible ld
// doubles per member (kmax and window fields of `w` as above, w.lda unused)
#define EKF_BATCH_LARGE_MAX_LANDMARKS 338       // EKF: N = 3 n + 10 <= 1024
#define EKF_BATCH_ROT_LARGE_MAX_LANDMARKS 101   // EKF_Rotations: N = 10 n + 10 <= 1020
struct EkfBatchLargeWindow {
    EkfBatchWindow w;
    double* W;                      // [B][w_stride]
    int64_t w_stride;
};
// wide frames: up to 64 / 50 detections per frame, in blocks of EKF_BATCH_MAX_VISIBLE / EKF_BATCH_ROT_MAX_VISIBLE (a frame of
// a large-map batch is one block)
#define EKF_BATCH_WIDE_MAX_VISIBLE 64       // EKF: k = 3 m <= 192 rows
#define EKF_BATCH_ROT_WIDE_MAX_VISIBLE 50   // EKF_Rotations: k = 7 m <= 350 rows
extern "C" size_t ekf_batch_wide_lds_bytes(int model, int kmax);
// one_block: no frame is wider than one block (a batch without the wide flag): the instance without the loops over blocks
void ekf_launch_batch_wide_window(int model, bool one_block, const EkfBatchLargeWindow& g, int members, hipStream_t s);
// Replicas of one log (ekf_batch_replicas.hip): out[r][d][c] = poses[d][c] + sigma[r][c] g_c(seed, r0 + r, d), c < 6, for
// `count` <= EKF_REPLICA_CHUNK replicas per launch (sigma travels in the kernel arguments); g: Philox4x32-10 + Box-Muller,
// the definition in include/ekf_slam_hip.h (ekf_batch_replica_poses)
#define EKF_REPLICA_CHUNK 64
void ekf_launch_replica_poses(const double* poses_dev, int64_t D, const double* sigma, int32_t count, uint64_t seed,
                              uint32_t r0, double* out_dev, hipStream_t s);

// Detection -> pose front end (ekf_pose_ippe.hip): pinhole camera + Brown-Conrady distortion k1 k2 p1 p2 k3 k4 k5 k6
struct EkfCamera {
    double fx, fy, cx, cy;
    double k[8];
};
// one [tvec | rvec] per marker from its four pixel corners [count][4][2] (IPPE for a square of side marker_size)
void ekf_launch_ippe_square(const double* corners_dev, int count, double marker_size, const EkfCamera& cam,
                            double* poses_dev, hipStream_t s);
// Replicas with pixel noise on the marker corners (ekf_batch_corner_replicas.hip): for `count` replicas from r0 on, the noisy
// corners [count][D][4][2], their IPPE poses [count][D][6] and the flip labels [count][D] (each output may be null);
// sigma_px [count] on the host, chunked by EKF_REPLICA_CHUNK; the definition in include/ekf_slam_hip.h
// (ekf_batch_replica_corners)
void ekf_launch_corner_replicas(const double* corners_dev, int64_t D, const double* sigma_px, int32_t count, uint64_t seed,
                                uint32_t r0, double marker_size, const EkfCamera& cam, double* poses_dev,
                                uint8_t* flipped_dev, double* noisy_dev, hipStream_t s);
