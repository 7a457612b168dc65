// Window kernel body of the batch of independent filters (ekf_batch_observe_logs, ekf_batch_api.hip), for both models:
// ONE workgroup owns ONE member for a window of its log's frames.  Per stepped frame, the algebra of DESIGN section 2 with
// everything but P in LDS:
//   first sightings (the frame's pre-update camera), h and dh of every detection,
//   A = H (P+Q) [k, N], S = A[:,supp] H^T + R I (or + diag(row_noise)) (lower triangle), S = L L^T (left-looking, in LDS),
//   W = L^-1 A and y = L^-1 (z - h) (y is column N of A), dx = W^T y and the injection,
//   P <- (P+Q) - W^T W in global memory.
// MODEL 0 (EKF): RD = 3 rows per detection, LMD = 3 landmark dims, JC = 13 Jacobian columns (ekf_batch.hip).
// MODEL 1 (EKF_Rotations): RD = 7, LMD = 10, JC = 20 (ekf_batch_rot.hip).  Each model is instantiated in its own file.
// P of a member is read and written by its own workgroup only: workgroup barriers are the only ordering.
#pragma once
#include "ekf_gate_device.h"
#include "ekf_markers.h"
#include "ekf_motion_device.h"
#include "ekf_smooth_device.h"

template <int MODEL> struct EkfBatchCaps;
template <> struct EkfBatchCaps<0> { static constexpr int MAX_VISIBLE = EKF_BATCH_MAX_VISIBLE; };
template <> struct EkfBatchCaps<1> { static constexpr int MAX_VISIBLE = EKF_BATCH_ROT_MAX_VISIBLE; };

// dynamic LDS, doubles: A/W [kmax][lda] | L [kmax][kmax] (strictly lower part used) | dinv [kmax] | J [kmax][JC] | dx [lda],
// then ints: first state column per detection [MAX_VISIBLE] | failure flag
template <int MODEL> inline size_t ekf_batch_lds_bytes_of(int kmax, int lda) {
    return 8 * ((size_t)kmax * lda + (size_t)kmax * kmax + kmax + (size_t)kmax * EkfModel<MODEL>::JC + lda) +
           4 * (EkfBatchCaps<MODEL>::MAX_VISIBLE + 4);
}

// Per-frame outputs of every window kernel (traj, nis, cam_cov; each may be null).  A frame that is not stepped repeats the
// state and P[0:10, 0:10] with nis = 0; once the member has failed (its failing frame included) all three are NaN.
__device__ __forceinline__ void ekf_batch_rows_unstepped(const EkfBatchWindow& a, int64_t t, int tid, const double* st,
                                                         const double* P, bool failed) {
    const double nan = __builtin_nan("");
    if (a.traj && tid < 7) a.traj[7 * t + tid] = failed ? nan : st[tid];
    if (a.nis && tid == 0) a.nis[t] = failed ? nan : 0.0;
    if (a.cam_cov && tid < EKF_CAM * EKF_CAM)
        a.cam_cov[EKF_CAM * EKF_CAM * t + tid] = failed ? nan : P[(int64_t)(tid / EKF_CAM) * a.ld + tid % EKF_CAM];
}

// After a stepped frame, behind the barrier that ends the covariance update: y [k] (stride ys) is the whitened residual
// L^-1 (z - h) of the frame; nis is one thread's i-ascending fma chain over it (the same bits wherever y has the same bits).
__device__ __forceinline__ void ekf_batch_rows_stepped(const EkfBatchWindow& a, int64_t t, int tid, const double* st,
                                                       const double* P, const double* y, int ys, int k) {
    if (a.traj && tid < 7) a.traj[7 * t + tid] = st[tid];
    if (a.nis && tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < k; ++i) acc = fma(y[i * ys], y[i * ys], acc);
        a.nis[t] = acc;
    }
    if (a.cam_cov && tid < EKF_CAM * EKF_CAM)
        a.cam_cov[EKF_CAM * EKF_CAM * t + tid] = P[(int64_t)(tid / EKF_CAM) * a.ld + tid % EKF_CAM];
}

// Once the member has failed, the detections of its later frames are not tested: their mahal is NaN.
__device__ __forceinline__ void ekf_batch_mahal_untested(const EkfBatchWindow& a, int64_t d0, int m, int tid, int nt) {
    if (a.mahal)
        for (int d = tid; d < m; d += nt) a.mahal[d0 + d] = __builtin_nan("");
}

// Individual-compatibility gate of one frame (include/ekf_slam_hip.h, ekf_batch_set_gate), the ONE place every window kernel
// takes its per-detection distances from.  Called by the whole workgroup behind the barrier that follows the frame's first
// sightings, before anything else of the frame; n0 is the landmark count the previous frame left, N the state dimension
// with the first sightings.  Detection d (thread d, m <= 64: wave 0) gets the d^2 of ekf_gate_device.h on the prior P: the
// three stages the single filter's gate kernel (ekf_gate.hip) runs as well.
// The first occurrence of a landmark first sighted in this frame is exempt (d^2 = 0, kept); a failed pivot keeps the
// detection and reports NaN; otherwise the detection is rejected iff d^2 > gate[b].  Returns the 64-bit mask of the
// detections that stay (bit d), shared through `words` (two spare ints of LDS).
// `scr` is LDS nothing else uses yet: G = EkfGateScratch<MODEL>::DOUBLES (90 EKF / 336 EKF_Rotations) doubles per detection
// from the base of the dynamic LDS.  G w fits every launch the host makes for a widest frame of w detections
// (kmax >= RD w, lda >= 10 + LMD + 1, so A | L | dinv | J hold at least RD w (11 + LMD) + (RD w)^2 + RD w + RD w JC):
//   one-column: EKF 90 w <= 42 w + 9 w^2 + 3 w + 39 w, rotations 336 w <= 147 w + 49 w^2 + 7 w + 140 w;
//   large maps (R alone): G w <= 256 RD w;  wide frames: the same up to a full block, beyond it the static_assert
//   of ekf_batch_wide.hip on the widest frame the kernel admits.
template <int MODEL>
__device__ __forceinline__ uint64_t ekf_batch_gate(const EkfBatchWindow& a, int b, int64_t d0, int m, int n0, int N, int tid,
                                                   int nt, const double* st, const double* P, int64_t ld,
                                                   const EkfNoise& nz, double* scr, int* words) {
    constexpr int RD = EkfModel<MODEL>::RD, LMD = EkfModel<MODEL>::LMD, JC = EkfModel<MODEL>::JC;
    constexpr int SCR = EkfGateScratch<MODEL>::DOUBLES;
    const int32_t* idx = a.lm_index + d0;
    const double* pose = a.poses + 6 * d0;
    // h, dh and r = z - h of every detection (the exempt ones included: the wave does not diverge)
    if (tid < m) {
        double z[RD];
        if constexpr (MODEL == 0)
            for (int r = 0; r < 3; ++r) z[r] = pose[6 * tid + r];
        else
            ekf_pose_z(pose + 6 * tid, RD, z);
        ekf_gate_measure<MODEL>(st, EKF_CAM + LMD * idx[tid], z, scr + (size_t)tid * SCR);
    }
    __syncthreads();
    for (int task = tid; task < m * JC; task += nt) {
        const int d = task / JC;
        ekf_gate_project<MODEL>(P, ld, EKF_CAM + LMD * idx[d], task - d * JC, N, nz, scr + (size_t)d * SCR);
    }
    __syncthreads();
    bool keep = false;
    if (tid < m) {
        double d2;
        const bool ok = ekf_gate_distance<MODEL>(nz.r_unc, a.row_noise ? a.row_noise + (size_t)(d0 + tid) * RD : nullptr,
                                                    scr + (size_t)tid * SCR, d2);
        bool exempt = idx[tid] >= n0;
        for (int e = 0; e < tid; ++e) exempt = exempt && idx[e] != idx[tid];
        const double out = exempt ? 0.0 : ok ? d2 : __builtin_nan("");
        keep = !(a.gate && out > a.gate[b]);      // (NaN and 0 compare false: kept)
        if (a.mahal) a.mahal[d0 + tid] = out;
    }
    if (tid < 64) {
        const uint64_t mask = __ballot(keep);
        if (tid == 0) {
            words[0] = (int)(uint32_t)mask;
            words[1] = (int)(uint32_t)(mask >> 32);
        }
    }
    __syncthreads();
    return (uint64_t)(uint32_t)words[0] | ((uint64_t)(uint32_t)words[1] << 32);
}

// detection (position in the frame) of survivor `slot` of a gated frame: the slot-th set bit of the mask
__device__ __forceinline__ int ekf_batch_survivor(uint64_t mask, int slot) {
    for (int i = 0; i < slot; ++i) mask &= mask - 1;
    return __builtin_ctzll(mask);
}

// Variance of measurement row r of a frame's stacked survivors (detections from d0 on): the member's constant, or, with
// per-detection noise, the row of the survivor's detection in the log -- rows are indexed like lm_index, gate or no gate.
template <int RD>
__device__ __forceinline__ double ekf_batch_row_noise(const EkfBatchWindow& a, int64_t d0, bool gated, uint64_t mask, int r,
                                                      double r_unc) {
    if (!a.row_noise) return r_unc;
    const int slot = r / RD;
    const int src = gated ? ekf_batch_survivor(mask, slot) : slot;
    return a.row_noise[(size_t)(d0 + src) * RD + (r - slot * RD)];
}

// Per-frame process-noise scale (include/ekf_slam_hip.h, "Per-frame process-noise scale"): the scale a stepped frame runs
// with, s_eff = p + s (a frame without a scale: s = 1), and its noise Q_eff = fl(s_eff q) per entry -- an explicitly rounded
// multiply, once per frame, before any add sees it (the compiler would contract v + s q into an fma, which is not the bits
// of a filter configured with the products).  A batch without EKF_FLAG_FRAME_SCALE keeps the member's constants as they are.
__device__ __forceinline__ double ekf_batch_frame_scale(const EkfBatchWindow& a, int64_t t, bool scaled, double pend) {
    return scaled ? pend + (a.scale ? a.scale[t] : 1.0) : 1.0;
}
// (__dmul_rn is a plain product once it is inlined, open to contraction with the add that consumes it: the empty asm makes
// the rounded product opaque to the optimiser)
__device__ __forceinline__ double ekf_mul_rounded(double x, double y) {
    double v = __dmul_rn(x, y);
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ EkfNoise ekf_batch_frame_noise(const EkfNoise& nz0, bool scaled, double s_eff) {
    if (!scaled) return nz0;
    return EkfNoise{ekf_mul_rounded(s_eff, nz0.q_cam), ekf_mul_rounded(s_eff, nz0.q_err), ekf_mul_rounded(s_eff, nz0.q_lm),
                    nz0.r_unc};
}

// Camera motion of one member at the top of a frame (EkfBatchWindow::motion; the stage functions of ekf_motion_device.h, the
// ones the single filter's launch runs): the member's P and state are in HBM in every window kernel.  u = motion[t]; six
// exact zeros: nothing happens, no arithmetic.  All nt threads of the workgroup call it (u is uniform).  scr: 45 doubles of
// LDS nobody uses between frames (the start of the dynamic LDS).  Thread 0 forms F from the OLD camera state into scr; behind
// a barrier thread c moves the strip columns c, c + nt, ... (a column and its mirror row are its own), and thread i < 10
// forms row i of B = F P_cc -- entry (i, j) is entry i of ekf_motion_column(P_cc[:, j]), the value the single filter's
// launch leaves in its LDS copy of B -- keeps it in registers and, once every thread has read P_cc and the old state
// (barrier), applies F to it and stores the lower triangle and its mirror; thread 0 stores c' and q'.
__device__ __forceinline__ void ekf_batch_motion(const double* __restrict__ u, double* st, double* P, int64_t ld, int N,
                                                 int tid, int nt, void* scr) {
    bool moves = false;
    for (int i = 0; i < 6; ++i) moves = moves || u[i] != 0.0;
    if (!moves) return;
    EkfMotionF& f = *reinterpret_cast<EkfMotionF*>(scr);
    __syncthreads();      // (the frame before is over: its LDS is free, its state and P are in place)
    if (tid == 0) ekf_motion_form(st, u, f);
    __syncthreads();
    double in[EKF_CAM], out[EKF_CAM], brow[EKF_CAM];
    for (int j = EKF_CAM + tid; j < N; j += nt) {
#pragma unroll
        for (int k = 0; k < EKF_CAM; ++k) in[k] = P[(int64_t)k * ld + j];
        ekf_motion_column(f, in, out);
#pragma unroll
        for (int k = 0; k < EKF_CAM; ++k) {
            P[(int64_t)k * ld + j] = out[k];
            P[(int64_t)j * ld + k] = out[k];
        }
    }
    if (tid < EKF_CAM) {
#pragma unroll
        for (int j = 0; j < EKF_CAM; ++j) {
#pragma unroll
            for (int k = 0; k < EKF_CAM; ++k) in[k] = P[(int64_t)k * ld + j];
            ekf_motion_column(f, in, out);
            double v = out[0];
#pragma unroll
            for (int k = 1; k < EKF_CAM; ++k) v = k == tid ? out[k] : v;
            brow[j] = v;
        }
    }
    __syncthreads();      // (P_cc and the old state have been read by everyone who needs them)
    if (tid < EKF_CAM) {
        ekf_motion_column(f, brow, out);
#pragma unroll
        for (int k = 0; k < EKF_CAM; ++k)
            if (k <= tid) {
                P[(int64_t)tid * ld + k] = out[k];
                P[(int64_t)k * ld + tid] = out[k];
            }
    }
    if (tid == 0) {
        for (int i = 0; i < 3; ++i) st[i] = f.c1[i];
        for (int i = 0; i < 4; ++i) st[3 + i] = f.q1[i];
    }
    __syncthreads();
}

// MOVED: the instance with the motion stage at the top of the frame (a.motion != null).  A call without motions runs the
// instance without it, which is the kernel as it was: the stage's registers would cost every batch an occupancy step
// (one-column EKF kernel: 167 -> 256 VGPRs; measured -11 % / -19 % frames per second with the stage compiled in and off).
void ekf_launch_batch_moved_window(int model, const EkfBatchWindow& a, int members, hipStream_t s);            // ekf_batch_moved.hip
void ekf_launch_batch_moved_wide_window(int model, bool one_block, const EkfBatchLargeWindow& g, int members,
                                        hipStream_t s);                                                      // ekf_batch_wide_moved.hip
// FROZEN: the instance a batch with at least one frozen member runs (a.frozen != null; include/ekf_slam_hip.h, "Localisation
// mode").  The member's flag is a workgroup-uniform run-time branch: a frozen member forms dx[0:10] only, injects the camera
// only and updates the camera strip of P (ekf_batch_strip below); a member that is not frozen runs the statements of the
// instance without the branch, so it has that instance's bits.  Instances of their own for the reason MOVED has them, with
// and without the motion stage.
void ekf_launch_batch_frozen_window(int model, const EkfBatchWindow& a, int members, hipStream_t s);           // ekf_batch_frozen.hip
void ekf_launch_batch_frozen_wide_window(int model, bool one_block, const EkfBatchLargeWindow& g, int members,
                                         hipStream_t s);                                                     // ekf_batch_wide_frozen.hip

// The camera strip of P <- (P+Q) - W^T W for a frozen member of the one-column kernel, W [k][lda] in LDS: thread c owns
// column c and keeps the ten entries P[0:10][c] in registers; entry (i, c) runs the l-ascending chain fma(W[l][i], W[l][c],
// acc) from zero and is stored as (P[i][c] + q(i == c)) - acc, the operations the full sweep runs on that entry (and, with
// the factors swapped, on its mirror).  Column c >= 10 also stores the mirror P[c][0:10] (80 contiguous bytes per thread);
// the 10 x 10 block is written by the row stores of threads 0 .. 9 alone, so no address has two writers.  W[l][0:10] is one
// address for the whole wave (LDS broadcast); P[10:N, 10:N] is neither read nor written.
__device__ __forceinline__ void ekf_batch_strip(double* P, int64_t ld, const double* W, int lda, int k, int N,
                                                const EkfNoise& nz, int tid, int nt) {
    for (int c = tid; c < N; c += nt) {
        double pv[EKF_CAM], acc[EKF_CAM];
#pragma unroll
        for (int i = 0; i < EKF_CAM; ++i) {
            pv[i] = P[(int64_t)i * ld + c];
            acc[i] = 0.0;
        }
        for (int l = 0; l < k; ++l) {
            const double* Wl = W + l * lda;
            const double w = Wl[c];
#pragma unroll
            for (int i = 0; i < EKF_CAM; ++i) acc[i] = fma(Wl[i], w, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < EKF_CAM; ++i) {
            const double v = (pv[i] + (i == c ? ekf_qdiag(c, N, nz) : 0.0)) - acc[i];
            P[(int64_t)i * ld + c] = v;
            if (c >= EKF_CAM) P[(int64_t)c * ld + i] = v;
        }
    }
}

// RECORDED: the instances of a recorded call (ekf_batch_observe_logs_recorded; ekf_batch_recorded.hip), instances of their
// own for the reason MOVED has them.  The end of a frame that changed the member -- it was stepped, or moved by a non-zero
// motion -- packs st[0:N] and the lower triangle of P into the frame's slot (the record layout of ekf_smooth.hip: column j of
// the triangle is row j of the bitwise-symmetric P from its diagonal on, contiguous).  Wave w of the workgroup copies columns
// w, w + nt / 64, ...; its lanes walk down the column, so consecutive lanes read and write consecutive doubles.  Every frame
// of the call gets its flag and s_eff.  Called by the whole workgroup behind the barrier that ends the frame's writes to st
// and P; the stage only reads the member, and its own barrier keeps the next frame's writes behind its reads.
__device__ __forceinline__ void ekf_batch_record(const EkfBatchRecord& r, int64_t t, int tid, int nt, const double* st,
                                                 const double* P, int64_t ld, int N, int flag, double s_eff) {
    if (tid == 0) {
        r.flag[t] = flag;
        r.s_eff[t] = s_eff;
    }
    if (flag <= 0 || r.slot[t] < 0) return;      // (uniform: flag and slot are the same for every thread)
    double* rec = r.history + r.slot[t];
    for (int i = tid; i < N; i += nt) rec[i] = st[i];
    double* tri = rec + N;
    const int wave = tid >> 6, lane = tid & 63;
    for (int j = wave; j < N; j += nt >> 6) {
        double* col = tri + ekf_smooth_col(N, j) - j;
        const double* row = P + (int64_t)j * ld;
        for (int i = j + lane; i < N; i += 64) col[i] = row[i];
    }
    __syncthreads();
}

template <int MODEL, bool MOVED = false, bool FROZEN = false, bool RECORDED = false>
__device__ __forceinline__ void ekf_batch_window(const EkfBatchWindow& a, const EkfBatchRecord* rec = nullptr) {
    constexpr int RD = EkfModel<MODEL>::RD, LMD = EkfModel<MODEL>::LMD, JC = EkfModel<MODEL>::JC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int64_t t_end = a.member_frames[b + 1];
    const int64_t t0 = a.member_frames[b] + a.window_first;
    const int64_t t1 = t0 + a.window_frames < t_end ? t0 + a.window_frames : t_end;
    if (t0 >= t1) return;
    const int kmax = a.kmax, lda = a.lda;
    double* A = reinterpret_cast<double*>(smem);
    double* L = A + (size_t)kmax * lda;
    double* dinv = L + (size_t)kmax * kmax;
    double* J = dinv + kmax;
    double* dx = J + (size_t)kmax * JC;
    int* col0 = reinterpret_cast<int*>(dx + lda);
    int* flag = col0 + EkfBatchCaps<MODEL>::MAX_VISIBLE;

    const int64_t ld = a.ld;
    double* P = a.P + (size_t)b * ld * ld;
    double* st = a.state + (size_t)b * ld;
    const double* nzb = a.noise + 6 * b;      // ekf_config order: icu, ilu, r, q_cam, q_err, q_lm
    const EkfNoise nz0{nzb[3], nzb[4], nzb[5], nzb[2]};
    const double lm_unc = nzb[1];
    // per-frame process-noise scale: the member's pending scale travels through the window in `pend`
    const bool scaled = a.pending != nullptr;
    double pend = scaled ? a.pending[b] : 0.0;
    int n = a.nlm[b];
    bool failed = a.status[b] != 0;
    const bool gated = a.mahal || (a.gate && a.gate[b] < __builtin_inf());
    // a frozen member (the host admits no first sighting in its log): camera-only injection, camera strip of P
    bool frozen = false;
    if constexpr (FROZEN) frozen = a.frozen[b] != 0;
    if (tid == 0) *flag = 0;
    if constexpr (RECORDED)      // the member's camera at the start of the call: the rows before its first record
        if (a.window_first == 0 && tid < 7) rec->history[rec->head[b] + tid] = st[tid];

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t d0 = a.frame_offsets[t];
        const int mf = (int)(a.frame_offsets[t + 1] - d0);
        // recording: was the member moved by this frame (a failed member ignores motions)
        bool moved = false;
        if constexpr (RECORDED && MOVED)
            if (!failed)
                for (int i = 0; i < 6; ++i) moved = moved || a.motion[6 * t + i] != 0.0;
        // the camera's motion first: first sightings, gate, predict and update see the moved prior, and a frame that is not
        // stepped is still moved (a failed member ignores motions)
        if constexpr (MOVED)
            if (!failed) ekf_batch_motion(a.motion + 6 * t, st, P, ld, LMD * n + EKF_CAM, tid, nt, smem);
        if (failed || mf == 0) {      // not stepped: the rows repeat the state (NaN once the member has failed)
            if (scaled && !failed && a.scale) pend = pend + a.scale[t];      // (rule 4: the frame's scale stays pending)
            ekf_batch_rows_unstepped(a, t, tid, st, P, failed);
            ekf_batch_mahal_untested(a, d0, mf, tid, nt);
            if constexpr (RECORDED) ekf_batch_record(*rec, t, tid, nt, st, P, ld, LMD * n + EKF_CAM, failed ? -1 : moved ? 2 : 0, 0.0);
            continue;
        }
        const int32_t* idx = a.lm_index + d0;
        const double* pose = a.poses + 6 * d0;
        // first sightings (validated on the host: numbered n0, n0+1, ... in order of first occurrence), all with the
        // camera state the previous frame left, before predict
        const int n0 = n;
        for (int j = 0; j < mf; ++j) n = max(n, idx[j] + 1);
        if (tid < mf && idx[tid] >= n0) {
            bool first = true;
            for (int e = 0; e < tid; ++e) first = first && idx[e] != idx[tid];
            if (first) {
                if constexpr (MODEL == 0)
                    ekf_add_marker_xyz(P, ld, st, EKF_LM * n0 + EKF_CAM, idx[tid] - n0, pose + 6 * tid, nullptr, lm_unc);
                else
                    ekf_add_marker_pose(P, ld, st, LMD * n0 + EKF_CAM, idx[tid] - n0, pose + 6 * tid, nullptr, lm_unc);
            }
        }
        const int N = LMD * n + EKF_CAM;
        __syncthreads();
        const double s_eff = ekf_batch_frame_scale(a, t, scaled, pend);
        const EkfNoise nz = ekf_batch_frame_noise(nz0, scaled, s_eff);
        // the gate: the frame runs on the m detections that stay, in log order (mask: which ones)
        int m = mf;
        uint64_t mask = ~0ull;
        if (gated) {
            mask = ekf_batch_gate<MODEL>(a, b, d0, mf, n0, N, tid, nt, st, P, ld, nz, A, flag + 1);
            m = __popcll(mask);
            if (m == 0) {      // no survivor: an empty frame
                if (scaled && a.scale) pend = s_eff;      // (rule 4: p = p + s, the addition s_eff has made)
                ekf_batch_rows_unstepped(a, t, tid, st, P, false);
                if constexpr (RECORDED) ekf_batch_record(*rec, t, tid, nt, st, P, ld, N, moved ? 2 : 0, 0.0);
                continue;
            }
        }
        pend = 0.0;      // (rule 3: the frame is stepped)
        const int k = RD * m;
        // h, dh and z - h (column N of A)
        if (tid < m) {
            const int src = gated ? ekf_batch_survivor(mask, tid) : tid;
            const int c0 = EKF_CAM + LMD * idx[src];
            col0[tid] = c0;
            double cam[EKF_CAM], lm[LMD], h[RD], z[RD];
            for (int q = 0; q < EKF_CAM; ++q) cam[q] = st[q];
            for (int q = 0; q < LMD; ++q) lm[q] = st[c0 + q];
            if constexpr (MODEL == 0) {
                double Jt[3][EKF_JCOLS];
                ekf_measure(cam, lm, h, Jt);
                for (int r = 0; r < 3; ++r)
                    for (int s = 0; s < EKF_JCOLS; ++s) J[(3 * tid + r) * EKF_JCOLS + s] = Jt[r][s];
                for (int r = 0; r < 3; ++r) z[r] = pose[6 * src + r];
            } else {
                // the 7 x 20 rows go to LDS as ekf_measure_rot produces them (a register copy of them would spill)
                ekf_measure_rot(cam, lm, h, reinterpret_cast<double(*)[JC]>(J + (size_t)RD * tid * JC));
                ekf_pose_z(pose + 6 * src, RD, z);
            }
            for (int r = 0; r < RD; ++r) A[(RD * tid + r) * lda + N] = z[r] - h[r];
        }
        __syncthreads();
        // A = H (P+Q): thread c owns column c; the support rows of P (the camera's and the detection's landmark's) are read
        // once per detection
        for (int c = tid; c < N; c += nt) {
            double pc[EKF_CAM];
            for (int s = 0; s < EKF_CAM; ++s) pc[s] = P[(int64_t)s * ld + c] + (s == c ? ekf_qdiag(s, N, nz) : 0.0);
            for (int j = 0; j < m; ++j) {
                const int c0 = col0[j];
                double pl[LMD];
                for (int q = 0; q < LMD; ++q) pl[q] = P[(int64_t)(c0 + q) * ld + c] + (c0 + q == c ? ekf_qdiag(c, N, nz) : 0.0);
                for (int r = 0; r < RD; ++r) {
                    const double* Jr = J + (RD * j + r) * JC;
                    double acc = 0.0;
                    for (int s = 0; s < EKF_CAM; ++s) acc = fma(Jr[s], pc[s], acc);
                    for (int q = 0; q < LMD; ++q) acc = fma(Jr[EKF_CAM + q], pl[q], acc);
                    A[(RD * j + r) * lda + c] = acc;
                }
            }
        }
        __syncthreads();
        // S = A[:,supp] H^T + R I, lower triangle, into L
        for (int e = tid; e < k * k; e += nt) {
            const int r = e / k, rr = e - r * k;
            if (rr > r) continue;
            const double* Ar = A + r * lda;
            const double* Jr = J + rr * JC;
            const int c0 = col0[rr / RD];
            double acc = 0.0;
            for (int s = 0; s < EKF_CAM; ++s) acc = fma(Ar[s], Jr[s], acc);
            for (int q = 0; q < LMD; ++q) acc = fma(Ar[c0 + q], Jr[EKF_CAM + q], acc);
            L[r * kmax + rr] = acc + (r == rr ? ekf_batch_row_noise<RD>(a, d0, gated, mask, r, nz.r_unc) : 0.0);
        }
        __syncthreads();
        // S = L L^T, left-looking, one column per step: every thread of the column recomputes the pivot with the same
        // operations (same bits), so the pivot needs no extra barrier; S_jj stays in place, 1 / L_jj goes to dinv
        for (int j = 0; j < k; ++j) {
            if (tid >= j && tid < k) {
                const double* Lj = L + j * kmax;
                const double* Li = L + tid * kmax;
                double djj = Lj[j], v = Li[j];
                for (int l = 0; l < j; ++l) {
                    djj = fma(-Lj[l], Lj[l], djj);
                    v = fma(-Li[l], Lj[l], v);
                }
                if (!(djj > 0.0) || !isfinite(djj)) {
                    if (tid == j) *flag = 1;
                } else if (tid == j) {
                    dinv[j] = 1.0 / sqrt(djj);
                } else {
                    L[tid * kmax + j] = v / sqrt(djj);
                }
            }
            __syncthreads();
            if (*flag) break;
        }
        if (*flag) {      // the member stops here: the update of this frame changes neither state nor P
            failed = true;
            if (tid == 0) a.status[b] = EKF_BATCH_ST_NUMERIC;
            ekf_batch_rows_unstepped(a, t, tid, st, P, true);
            if constexpr (RECORDED) ekf_batch_record(*rec, t, tid, nt, st, P, ld, N, -1, 0.0);      // (the failing frame never records)
            continue;
        }
        // W = L^-1 A and y = L^-1 (z - h): thread c substitutes column c (c = N: the residual) in place
        for (int c = tid; c <= N; c += nt) {
            for (int i = 0; i < k; ++i) {
                const double* Li = L + i * kmax;
                double v = A[i * lda + c];
                for (int l = 0; l < i; ++l) v = fma(-Li[l], A[l * lda + c], v);
                A[i * lda + c] = v * dinv[i];
            }
        }
        __syncthreads();
        // dx = W^T y (a frozen member: the camera's ten entries, all that is injected)
        const int nx = frozen ? EKF_CAM : N;
        for (int c = tid; c < nx; c += nt) {
            double acc = 0.0;
            for (int i = 0; i < k; ++i) acc = fma(A[i * lda + c], A[i * lda + N], acc);
            dx[c] = acc;
        }
        __syncthreads();
        if constexpr (MODEL == 0) {
            // injection (extended_kalman_filter.py:133-152): dx[3:7] dropped, every landmark moves, error state reset
            if (tid == 0) {
                double q[4] = {st[3], st[4], st[5], st[6]};
                const double err[3] = {dx[7], dx[8], dx[9]};
                ekf_quat_inject(q, err, a.quat_mode);
                for (int r = 0; r < 4; ++r) st[3 + r] = q[r];
                for (int r = 7; r < 10; ++r) st[r] = 0.0;
            }
            for (int c = tid; c < nx; c += nt)
                if (c < 3 || c >= EKF_CAM) st[c] += dx[c];
        } else {
            // injection (ekf_with_rotations.py:146-177): thread 0 the camera block, thread i landmark i - 1 (n <= 24 < nt)
            if (tid <= (frozen ? 0 : n)) {
                const int c0 = tid == 0 ? 0 : EKF_CAM + LMD * (tid - 1);
                ekf_inject_rot_block(st + c0, dx + c0, tid == 0);
            }
        }
        // P <- (P+Q) - W^T W: thread c owns column c; entry (i,c) and (c,i) run the same l-ascending fma chain (the two
        // factors of each fma swap places, which does not change its result), so P stays bitwise symmetric.  The next row
        // block of the column is loaded before the fma chain of this one: its loads overlap the chain instead of each
        // block's read-modify-write of P waiting for its own load
        // (a frozen member: the camera strip instead, and no column of the full sweep)
        if (frozen) ekf_batch_strip(P, ld, A, lda, k, N, nz, tid, nt);
        for (int c = tid; c < (frozen ? 0 : N); c += nt) {
            double pv[4], pn[4];
            for (int u = 0; u < 4; ++u) pv[u] = u < N ? P[(int64_t)u * ld + c] : 0.0;
            for (int i0 = 0; i0 < N; i0 += 4) {
                for (int u = 0; u < 4; ++u) pn[u] = i0 + 4 + u < N ? P[(int64_t)(i0 + 4 + u) * ld + c] : 0.0;
                double acc[4] = {0.0, 0.0, 0.0, 0.0};
                for (int l = 0; l < k; ++l) {
                    const double* Wl = A + l * lda;
                    const double w = Wl[c];
                    for (int u = 0; u < 4; ++u) acc[u] = fma(Wl[i0 + u], w, acc[u]);
                }
                for (int u = 0; u < 4 && i0 + u < N; ++u) {
                    const int i = i0 + u;
                    P[(int64_t)i * ld + c] = (pv[u] + (i == c ? ekf_qdiag(c, N, nz) : 0.0)) - acc[u];
                }
                for (int u = 0; u < 4; ++u) pv[u] = pn[u];
            }
        }
        __syncthreads();
        ekf_batch_rows_stepped(a, t, tid, st, P, A + N, lda, k);      // (y is column N of A)
        if constexpr (RECORDED) ekf_batch_record(*rec, t, tid, nt, st, P, ld, N, 1, s_eff);
    }
    if (tid == 0) a.nlm[b] = n;
    if (tid == 0 && scaled) a.pending[b] = pend;
}

// one launch of `kernel` per window (> 64 KB of dynamic LDS needs the opt-in, once per kernel: `once`)
template <int MODEL>
void ekf_batch_launch(void (*kernel)(EkfBatchWindow), bool& once, const EkfBatchWindow& a, int members, hipStream_t s) {
    if (!once) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        once = true;
    }
    hipLaunchKernelGGL(kernel, dim3(members), dim3(256), ekf_batch_lds_bytes_of<MODEL>(a.kmax, a.lda), s, a);
}
