// Batch of independent filters, HBM-resident window kernel (ekf_batch_observe_logs with EKF_FLAG_BATCH_LARGE_MAPS or
// EKF_FLAG_BATCH_WIDE_FRAMES, ekf_batch_api.hip): the window kernels of both models on maps up to N = lmd n + 10 = 1024 (EKF
// n <= 338, EKF_Rotations n <= 101) and frames of up to 64 (EKF, k = 3 m <= 192) or 50 (EKF_Rotations, k = 7 m <= 350)
// detections.  ONE workgroup of 256 threads owns ONE member for a window of its log's frames, as in ekf_batch_impl.h, and a
// frame runs the algebra of that kernel with the same operation order per entry (so where both run, the bits are the same).
// What moves is the data: A, then W, [k][ld] lives in the member's slice of the batch workspace (HBM), y [k] in LDS.
// A frame's detections are split, in log order, into blocks of MB = 16 (EKF) / 8 (EKF_Rotations) detections, kb <= KW =
// 48 / 56 rows each; a frame of a batch without the wide flag is one block, and such a batch runs the ONE_BLOCK instances
// of the same body (ekf_batch_one_block_window_kernel / _rot_).  After the first sightings, for block j (rows
// r0 .. r0 + kb):
//   h and dh of its detections (J of the block and y_j = z_j - h_j),
//   A_j = H_j (P+Q), thread c owning column c,
//   for every earlier block i: the off-diagonal factor block L_ji = H_j W_i^T (only the support columns of the stored W_i
//     rows are read: W H^T = L^T - L^-1 R with L^-1 R lower triangular), then A_j <- A_j - L_ji W_i and y_j <- y_j - L_ji y_i,
//     one l-ascending fma chain per entry over all earlier rows,
//   S_jj = A_j[:,supp] H_j^T + R I (lower triangle), S_jj = L_jj L_jj^T (left-looking, in LDS),
//   W_j = L_jj^-1 A_j and y_j <- L_jj^-1 y_j; W_j stays in the workspace.
// Only then: dx = W^T y over all k rows, the injection, and P <- (P+Q) - W^T W as one read-modify-write sweep of P per block
// (Q added by the first).  Entry (i,c) and (c,i) run the same operations in every sweep, so P stays bitwise symmetric and
// its padding zero.  Nothing touches P or the state before the last pivot of the frame has passed, so a failing pivot in
// any block leaves them as the frame found them (its first sightings stay added, as everywhere).
// LDS holds the block's L_jj (and, in turn, each L_ji), 1 / L_jj, J of the block, y [kmax] and one region R of
// 256 x round_up(kb, 4) doubles that serves three phases in turn: each thread's private copy of the column it substitutes,
// then dx, then a panel of 256 rows of W_j^T for the covariance sweep.  LDS thus depends on kmax only: 122,768 / 149,848
// bytes with one block (kmax = 48 / 56), 123,920 at the EKF's kmax = 192, 152,200 at EKF_Rotations' kmax = 350.  The
// off-diagonal factor rows are not stored: each L_ji is formed from W rows in HBM when it is used.
// Covariance sweep: thread t owns column c = c0 + t for column blocks c0 = 0, 256, ...; it keeps W_j[:,c] in registers and
// streams its column of P in blocks of 8 rows with two blocks loaded ahead (24 doubles in flight per thread), against the
// panel of W_j^T rows in LDS (broadcast reads).  Entry (i,c) runs the l-ascending fma chain of ekf_batch_impl.h.
// P of a member is read and written by its own workgroup only: workgroup barriers are the only ordering.
#include "ekf_batch_impl.h"

namespace {

constexpr int kWideThreads = 256;
constexpr int kRowBlock = 8;        // rows of P per fma block

template <int MODEL> struct WideCaps;
template <> struct WideCaps<0> { static constexpr int MAX_VISIBLE = EKF_BATCH_WIDE_MAX_VISIBLE; };
template <> struct WideCaps<1> { static constexpr int MAX_VISIBLE = EKF_BATCH_ROT_WIDE_MAX_VISIBLE; };

// detections per block (the one-column kernels' max_visible) and rows of a full block (48 / 56, a multiple of 4)
template <int MODEL> constexpr int wide_mb() { return EkfBatchCaps<MODEL>::MAX_VISIBLE; }
template <int MODEL> constexpr int wide_kw() { return EkfModel<MODEL>::RD * wide_mb<MODEL>(); }
static_assert(wide_kw<0>() % 4 == 0 && wide_kw<1>() % 4 == 0, "a full block pads to no extra rows");

// dynamic LDS, doubles: R [256][round_up(kb, 4)] | L [kb][kb] | dinv [kb] | J [kb][JC] | y [kmax] with kb = min(kmax, KW),
// then ints: first state column per detection [MAX_VISIBLE] | failure flag
template <int MODEL> size_t wide_lds_bytes_of(int kmax) {
    const size_t kb = (size_t)(kmax < wide_kw<MODEL>() ? kmax : wide_kw<MODEL>());
    const size_t kbp = (kb + 3) / 4 * 4;
    return 8 * ((size_t)kWideThreads * kbp + kb * kb + kb + kb * EkfModel<MODEL>::JC + (size_t)kmax) +
           4 * (WideCaps<MODEL>::MAX_VISIBLE + 4);
}

// the gate's scratch (ekf_batch_gate) of the widest admitted frame lies in the doubles of a launch with full blocks:
// R | L | dinv | J of a KW-row block and y of at least KW rows
template <int MODEL> constexpr bool wide_gate_fits() {
    constexpr int KW = wide_kw<MODEL>();
    return EkfGateScratch<MODEL>::DOUBLES * WideCaps<MODEL>::MAX_VISIBLE <=
           kWideThreads * KW + KW * KW + KW + KW * EkfModel<MODEL>::JC + KW;
}
static_assert(wide_gate_fits<0>() && wide_gate_fits<1>(), "the gate's scratch must fit the wide kernels' LDS");

typedef double ekf_d2 __attribute__((ext_vector_type(2)));

// ONE_BLOCK: no frame of the launch is wider than one block (a batch without the wide flag: the host admits no wider frame),
// so the loops over blocks run once, with j0 = 0, and the loop over earlier blocks is gone: the same operations on the same
// data, with less control around them (the large-map shapes run 3 to 4 % faster than in the general instance)
// MOVED: the instance with the motion stage (ekf_batch_impl.h: why it is an instance of its own)
// FROZEN: the instance of a batch with frozen members (ekf_batch_impl.h; ekf_batch_wide_frozen.hip).  A frozen member forms
// dx[0:10] only, injects the camera only, and in place of every block's sweep of P runs one strip pass over W_j, in the block
// order of the sweep and with Q in the first pass: the ten camera columns of W_j (rows padded with zeros to kbp, as the
// sweep's panel is) are staged into R as [kbp][10], thread t owns column c = c0 + t, keeps W_j[:, c] in registers (read
// coalesced along c) and P[0:10][c] with them, runs the sweep's chain fma(W_j[l][i], W_j[l][c], acc) per entry against the
// staged rows (one LDS address per wave: broadcast), and stores the column entries and, for c >= 10, the mirror
// P[c][0:10].  P[0:10][c] is read and written by its own thread in every pass; the mirror entries are only written.
template <int MODEL, bool ONE_BLOCK, bool MOVED = false, bool FROZEN = false>
__device__ __forceinline__ void ekf_batch_wide_window(const EkfBatchLargeWindow& g) {
    constexpr int RD = EkfModel<MODEL>::RD, LMD = EkfModel<MODEL>::LMD, JC = EkfModel<MODEL>::JC;
    constexpr int MB = wide_mb<MODEL>(), KW = wide_kw<MODEL>();
    const EkfBatchWindow& a = g.w;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = kWideThreads;
    const int64_t t_end = a.member_frames[b + 1];
    const int64_t t0 = a.member_frames[b] + a.window_first;
    const int64_t t1 = t0 + a.window_frames < t_end ? t0 + a.window_frames : t_end;
    if (t0 >= t1) return;
    const int kmax = a.kmax, kbmax = kmax < KW ? kmax : KW, kbpmax = (kbmax + 3) & ~3;
    double* R = reinterpret_cast<double*>(smem);
    double* L = R + (size_t)nt * kbpmax;
    double* dinv = L + (size_t)kbmax * kbmax;
    double* J = dinv + kbmax;
    double* y = J + (size_t)kbmax * JC;
    int* col0 = reinterpret_cast<int*>(y + kmax);
    int* flag = col0 + WideCaps<MODEL>::MAX_VISIBLE;

    const int64_t ld = a.ld;
    double* P = a.P + (size_t)b * ld * ld;
    double* st = a.state + (size_t)b * ld;
    double* A = g.W + (size_t)b * g.w_stride;      // A, then W: [k][ld]
    const double* nzb = a.noise + 6 * b;      // ekf_config order: icu, ilu, r, q_cam, q_err, q_lm
    const EkfNoise nz0{nzb[3], nzb[4], nzb[5], nzb[2]};
    const double lm_unc = nzb[1];
    // per-frame process-noise scale: the member's pending scale travels through the window in `pend`
    const bool scaled = a.pending != nullptr;
    double pend = scaled ? a.pending[b] : 0.0;
    int n = a.nlm[b];
    bool failed = a.status[b] != 0;
    const bool gated = a.mahal || (a.gate && a.gate[b] < __builtin_inf());
    bool frozen = false;
    if constexpr (FROZEN) frozen = a.frozen[b] != 0;
    if (tid == 0) *flag = 0;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t d0 = a.frame_offsets[t];
        const int mf = (int)(a.frame_offsets[t + 1] - d0);
        // the camera's motion first (ekf_batch_impl.h: ekf_batch_motion), as in the one-column kernel
        if constexpr (MOVED)
            if (!failed) ekf_batch_motion(a.motion + 6 * t, st, P, ld, LMD * n + EKF_CAM, tid, nt, smem);
        if (failed || mf == 0) {      // not stepped: the rows repeat the state (NaN once the member has failed)
            if (scaled && !failed && a.scale) pend = pend + a.scale[t];      // (rule 4: the frame's scale stays pending)
            ekf_batch_rows_unstepped(a, t, tid, st, P, failed);
            ekf_batch_mahal_untested(a, d0, mf, tid, nt);
            continue;
        }
        const int32_t* idx = a.lm_index + d0;
        const double* pose = a.poses + 6 * d0;
        // first sightings, all with the camera state the previous frame left, before predict
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
        const double s_eff = ekf_batch_frame_scale(a, t, scaled, pend);
        const EkfNoise nz = ekf_batch_frame_noise(nz0, scaled, s_eff);
        // the gate, before the blocking: the blocks are formed from the m detections that stay, in log order
        int m = mf;
        uint64_t mask = ~0ull;
        if (gated) {
            __syncthreads();      // (first sightings are in place)
            mask = ekf_batch_gate<MODEL>(a, b, d0, mf, n0, N, tid, nt, st, P, ld, nz, R, flag + 1);
            m = __popcll(mask);
            if (m == 0) {      // no survivor: an empty frame
                if (scaled && a.scale) pend = s_eff;      // (rule 4: p = p + s, the addition s_eff has made)
                ekf_batch_rows_unstepped(a, t, tid, st, P, false);
                continue;
            }
        }
        pend = 0.0;      // (rule 3: the frame is stepped)
        const int k = RD * m, blocks_end = ONE_BLOCK ? 1 : m;
        // ---- the factorisation, block after block of detections; W_j and y_j of every block that passed stay behind
        for (int j0 = 0; j0 < blocks_end; j0 += MB) {
            const int mb = ONE_BLOCK ? m : min(MB, m - j0), kb = RD * mb, r0 = RD * j0;
            double* Aj = A + (int64_t)r0 * ld;
            __syncthreads();      // (first sightings, or the previous block's W_j and y_j, are in place)
            // h, dh and y = z - h of the block's detections
            if (tid < mb) {
                const int d = j0 + tid;
                const int src = gated ? ekf_batch_survivor(mask, d) : d;
                const int c0 = EKF_CAM + LMD * idx[src];
                col0[d] = c0;
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
                    ekf_measure_rot(cam, lm, h, reinterpret_cast<double(*)[JC]>(J + (size_t)RD * tid * JC));
                    ekf_pose_z(pose + 6 * src, RD, z);
                }
                for (int r = 0; r < RD; ++r) y[r0 + RD * tid + r] = z[r] - h[r];
            }
            __syncthreads();
            // A_j = H_j (P+Q): thread c owns column c
            for (int c = tid; c < N; c += nt) {
                double pc[EKF_CAM];
                for (int s = 0; s < EKF_CAM; ++s) pc[s] = P[(int64_t)s * ld + c] + (s == c ? ekf_qdiag(s, N, nz) : 0.0);
                for (int jj = 0; jj < mb; ++jj) {
                    const int c0 = col0[j0 + jj];
                    double pl[LMD];
                    for (int q = 0; q < LMD; ++q)
                        pl[q] = P[(int64_t)(c0 + q) * ld + c] + (c0 + q == c ? ekf_qdiag(c, N, nz) : 0.0);
                    for (int r = 0; r < RD; ++r) {
                        const double* Jr = J + (RD * jj + r) * JC;
                        double acc = 0.0;
                        for (int s = 0; s < EKF_CAM; ++s) acc = fma(Jr[s], pc[s], acc);
                        for (int q = 0; q < LMD; ++q) acc = fma(Jr[EKF_CAM + q], pl[q], acc);
                        Aj[(int64_t)(RD * jj + r) * ld + c] = acc;
                    }
                }
            }
            // earlier blocks i (always full: KW rows at q0): L_ji = H_j W_i^T into L, then A_j -= L_ji W_i, y_j -= L_ji y_i
            for (int q0 = 0; q0 < r0; q0 += KW) {
                __syncthreads();      // (A_j, or the previous L_ji's use of L, is done)
                for (int e = tid; e < kb * KW; e += nt) {
                    const int r = e / KW, l = e - r * KW;
                    const double* Wl = A + (int64_t)(q0 + l) * ld;
                    const double* Jr = J + r * JC;
                    const int c0 = col0[j0 + r / RD];
                    double acc = 0.0;
                    for (int s = 0; s < EKF_CAM; ++s) acc = fma(Wl[s], Jr[s], acc);
                    for (int q = 0; q < LMD; ++q) acc = fma(Wl[c0 + q], Jr[EKF_CAM + q], acc);
                    L[r * kbmax + l] = acc;
                }
                __syncthreads();
                for (int c = tid; c <= N; c += nt) {
                    double w[KW];
#pragma unroll
                    for (int l = 0; l < KW; ++l) w[l] = c == N ? y[q0 + l] : A[(int64_t)(q0 + l) * ld + c];
                    for (int r = 0; r < kb; ++r) {
                        const double* Lr = L + r * kbmax;
                        double v = c == N ? y[r0 + r] : Aj[(int64_t)r * ld + c];
#pragma unroll
                        for (int l = 0; l < KW; ++l) v = fma(-Lr[l], w[l], v);
                        if (c == N)
                            y[r0 + r] = v;
                        else
                            Aj[(int64_t)r * ld + c] = v;
                    }
                }
            }
            __syncthreads();
            // S_jj = A_j[:,supp] H_j^T + R I, lower triangle, into L
            for (int e = tid; e < kb * kb; e += nt) {
                const int r = e / kb, rr = e - r * kb;
                if (rr > r) continue;
                const double* Ar = Aj + (int64_t)r * ld;
                const double* Jr = J + rr * JC;
                const int c0 = col0[j0 + rr / RD];
                double acc = 0.0;
                for (int s = 0; s < EKF_CAM; ++s) acc = fma(Ar[s], Jr[s], acc);
                for (int q = 0; q < LMD; ++q) acc = fma(Ar[c0 + q], Jr[EKF_CAM + q], acc);
                L[r * kbmax + rr] = acc + (r == rr ? ekf_batch_row_noise<RD>(a, d0, gated, mask, r0 + r, nz.r_unc) : 0.0);
            }
            __syncthreads();
            // S_jj = L_jj L_jj^T, left-looking, as ekf_batch_impl.h (pivots recomputed by every thread of the column)
            for (int j = 0; j < kb; ++j) {
                if (tid >= j && tid < kb) {
                    const double* Lj = L + j * kbmax;
                    const double* Li = L + tid * kbmax;
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
                        L[tid * kbmax + j] = v / sqrt(djj);
                    }
                }
                __syncthreads();
                if (*flag) break;
            }
            if (*flag) break;
            // W_j = L_jj^-1 A_j and y_j <- L_jj^-1 y_j: thread c substitutes column c (c = N: y_j).  A column of A_j is
            // copied to the thread's own slice of R ([i][thread]: the lanes of a wave read consecutive doubles),
            // substituted there and written back once
            for (int c = tid; c <= N; c += nt) {
                double* v = c == N ? y + r0 : R + tid;
                const int vs = c == N ? 1 : nt;
                if (c < N)
                    for (int i = 0; i < kb; ++i) v[i * vs] = Aj[(int64_t)i * ld + c];
                for (int i = 0; i < kb; ++i) {
                    const double* Li = L + i * kbmax;
                    double s = v[i * vs];
                    for (int l = 0; l < i; ++l) s = fma(-Li[l], v[l * vs], s);
                    v[i * vs] = s * dinv[i];
                }
                if (c < N)
                    for (int i = 0; i < kb; ++i) Aj[(int64_t)i * ld + c] = v[i * vs];
            }
        }
        if (*flag) {      // the member stops here: the update of this frame changes neither state nor P
            failed = true;
            if (tid == 0) a.status[b] = EKF_BATCH_ST_NUMERIC;
            ekf_batch_rows_unstepped(a, t, tid, st, P, true);
            continue;
        }
        __syncthreads();
        // dx = W^T y over all k rows (into R: every thread's slice is done); a frozen member: the camera's ten entries
        double* dx = R;
        const int nx = frozen ? EKF_CAM : N;
        for (int c = tid; c < nx; c += nt) {
            double acc = 0.0;
            for (int i = 0; i < k; ++i) acc = fma(A[(int64_t)i * ld + c], y[i], acc);
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
            // injection (ekf_with_rotations.py:146-177): thread 0 the camera block, thread i landmark i - 1 (n <= 101 < nt)
            if (tid <= (frozen ? 0 : n)) {
                const int c0 = tid == 0 ? 0 : EKF_CAM + LMD * (tid - 1);
                ekf_inject_rot_block(st + c0, dx + c0, tid == 0);
            }
        }
        // P <- (P+Q) - W^T W, one sweep per block of rows W_j (Q with the first).  Rows l in [kb, kbp) of the panel and of
        // w are zero: fma(0, 0, acc) = acc (acc is never -0), so padding the chain to a multiple of 4 leaves every
        // entry's bits as they are.
        // A frozen member: the strip passes instead (FROZEN above), and no block of the full sweep.
        if (frozen) {
            double* WC = R;      // [kbp][10]: the camera columns of W_j
            for (int j0 = 0; j0 < blocks_end; j0 += MB) {
                const int kb = ONE_BLOCK ? k : RD * min(MB, m - j0), kbp = (kb + 3) & ~3;
                const double* Wj = A + (int64_t)RD * j0 * ld;
                __syncthreads();      // (dx, or the previous block's camera columns, are no longer read)
                for (int e = tid; e < kbp * EKF_CAM; e += nt) {
                    const int l = e / EKF_CAM, i = e - l * EKF_CAM;
                    WC[e] = l < kb ? Wj[(int64_t)l * ld + i] : 0.0;
                }
                __syncthreads();
                for (int c = tid; c < N; c += nt) {
                    const double qc = ekf_qdiag(c, N, nz);
                    double w[KW], p[EKF_CAM], acc[EKF_CAM];
#pragma unroll
                    for (int l = 0; l < KW; ++l) {
                        const double v = Wj[(int64_t)min(l, kb - 1) * ld + c];
                        w[l] = l < kb ? v : 0.0;
                    }
#pragma unroll
                    for (int i = 0; i < EKF_CAM; ++i) {
                        p[i] = P[(int64_t)i * ld + c];
                        acc[i] = 0.0;
                    }
#pragma unroll
                    for (int l0 = 0; l0 < KW; l0 += 4) {
                        if (l0 < kbp) {
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const double* Wr = WC + (l0 + u) * EKF_CAM;
#pragma unroll
                                for (int i = 0; i < EKF_CAM; ++i) acc[i] = fma(Wr[i], w[l0 + u], acc[i]);
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < EKF_CAM; ++i) {
                        const double pq = j0 == 0 ? p[i] + (i == c ? qc : 0.0) : p[i];
                        const double v = pq - acc[i];
                        P[(int64_t)i * ld + c] = v;
                        if (c >= EKF_CAM) P[(int64_t)c * ld + i] = v;
                    }
                }
            }
        }
        double* WT = R;      // [256 rows of the panel][kbp]
        for (int j0 = 0; j0 < (frozen ? 0 : blocks_end); j0 += MB) {
            const int kb = ONE_BLOCK ? k : RD * min(MB, m - j0), kbp = (kb + 3) & ~3;
            const double* Wj = A + (int64_t)RD * j0 * ld;
            for (int cb = 0; cb < N; cb += nt) {
                const int c = cb + tid;
                const bool own = c < N;
                const int cc = own ? c : N - 1;      // (loads stay inside the member's matrix)
                const double qc = ekf_qdiag(cc, N, nz);
                double w[KW];
#pragma unroll
                for (int l = 0; l < KW; ++l) {
                    const double v = Wj[(int64_t)min(l, kb - 1) * ld + cc];
                    w[l] = l < kb ? v : 0.0;
                }
                for (int i0 = 0; i0 < N; i0 += nt) {
                    const int rows = min(nt, N - i0);
                    __syncthreads();      // (the previous panel, or dx, is no longer read)
                    for (int l = 0; l < kbp; ++l)
                        WT[tid * kbp + l] = l < kb && tid < rows ? Wj[(int64_t)l * ld + i0 + tid] : 0.0;
                    __syncthreads();
                    double* Pc = P + (int64_t)i0 * ld + cc;
                    auto load = [&](double (&p)[kRowBlock], int ib) {
#pragma unroll
                        for (int u = 0; u < kRowBlock; ++u) p[u] = ib + u < rows ? Pc[(int64_t)(ib + u) * ld] : 0.0;
                    };
                    auto step = [&](const double (&p)[kRowBlock], int ib) {
                        if (ib >= rows) return;
                        double acc[kRowBlock];
#pragma unroll
                        for (int u = 0; u < kRowBlock; ++u) acc[u] = 0.0;
#pragma unroll
                        for (int l0 = 0; l0 < KW; l0 += 4) {
                            if (l0 < kbp) {
#pragma unroll
                                for (int u = 0; u < kRowBlock; ++u) {
                                    const ekf_d2* Wr = reinterpret_cast<const ekf_d2*>(WT + (ib + u) * kbp + l0);
                                    const ekf_d2 lo = Wr[0], hi = Wr[1];
                                    acc[u] = fma(lo.x, w[l0], acc[u]);
                                    acc[u] = fma(lo.y, w[l0 + 1], acc[u]);
                                    acc[u] = fma(hi.x, w[l0 + 2], acc[u]);
                                    acc[u] = fma(hi.y, w[l0 + 3], acc[u]);
                                }
                            }
                        }
                        if (!own) return;
#pragma unroll
                        for (int u = 0; u < kRowBlock; ++u) {
                            const int i = i0 + ib + u;
                            const double pq = j0 == 0 ? p[u] + (i == c ? qc : 0.0) : p[u];
                            if (ib + u < rows) Pc[(int64_t)(ib + u) * ld] = pq - acc[u];
                        }
                    };
                    // three blocks rotate through pa, pb, pc: two are in flight while the third is consumed
                    double pa[kRowBlock], pb[kRowBlock], pc[kRowBlock];
                    load(pa, 0);
                    load(pb, kRowBlock);
                    for (int ib = 0; ib < rows; ib += 3 * kRowBlock) {
                        load(pc, ib + 2 * kRowBlock);
                        step(pa, ib);
                        load(pa, ib + 3 * kRowBlock);
                        step(pb, ib + kRowBlock);
                        load(pb, ib + 4 * kRowBlock);
                        step(pc, ib + 2 * kRowBlock);
                    }
                }
            }
        }
        __syncthreads();
        ekf_batch_rows_stepped(a, t, tid, st, P, y, 1, k);
    }
    if (tid == 0) a.nlm[b] = n;
    if (tid == 0 && scaled) a.pending[b] = pend;
}

template <int MODEL>
void wide_launch(void (*kernel)(EkfBatchLargeWindow), bool& once, const EkfBatchLargeWindow& g, int members,
                 hipStream_t s) {
    if (!once) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        once = true;
    }
    hipLaunchKernelGGL(kernel, dim3(members), dim3(kWideThreads), wide_lds_bytes_of<MODEL>(g.w.kmax), s, g);
}

}  // namespace

#if defined(EKF_BATCH_WIDE_FROZEN)      // ekf_batch_wide_frozen.hip: the instances of a batch with frozen members
#define EKF_WIDE_FROZEN_KERNEL(name, model, one_block, moved)                                   \
    __global__ __launch_bounds__(256) void name(EkfBatchLargeWindow g) {                        \
        ekf_batch_wide_window<model, one_block, moved, true>(g);                                \
    }
EKF_WIDE_FROZEN_KERNEL(ekf_batch_frozen_wide_window_kernel, 0, false, false)
EKF_WIDE_FROZEN_KERNEL(ekf_batch_frozen_wide_rot_window_kernel, 1, false, false)
EKF_WIDE_FROZEN_KERNEL(ekf_batch_frozen_one_block_window_kernel, 0, true, false)
EKF_WIDE_FROZEN_KERNEL(ekf_batch_frozen_one_block_rot_window_kernel, 1, true, false)
EKF_WIDE_FROZEN_KERNEL(ekf_batch_frozen_moved_wide_window_kernel, 0, false, true)
EKF_WIDE_FROZEN_KERNEL(ekf_batch_frozen_moved_wide_rot_window_kernel, 1, false, true)
EKF_WIDE_FROZEN_KERNEL(ekf_batch_frozen_moved_one_block_window_kernel, 0, true, true)
EKF_WIDE_FROZEN_KERNEL(ekf_batch_frozen_moved_one_block_rot_window_kernel, 1, true, true)
#undef EKF_WIDE_FROZEN_KERNEL

void ekf_launch_batch_frozen_wide_window(int model, bool one_block, const EkfBatchLargeWindow& g, int members,
                                         hipStream_t s) {
    static bool once[2][2][2] = {};
    // [model][one_block][moved]
    static void (*const kernels[2][2][2])(EkfBatchLargeWindow) = {
        {{ekf_batch_frozen_wide_window_kernel, ekf_batch_frozen_moved_wide_window_kernel},
         {ekf_batch_frozen_one_block_window_kernel, ekf_batch_frozen_moved_one_block_window_kernel}},
        {{ekf_batch_frozen_wide_rot_window_kernel, ekf_batch_frozen_moved_wide_rot_window_kernel},
         {ekf_batch_frozen_one_block_rot_window_kernel, ekf_batch_frozen_moved_one_block_rot_window_kernel}}};
    const int mi = model == 1 ? 1 : 0, moved = g.w.motion != nullptr;
    if (mi == 1)
        wide_launch<1>(kernels[1][one_block][moved], once[1][one_block][moved], g, members, s);
    else
        wide_launch<0>(kernels[0][one_block][moved], once[0][one_block][moved], g, members, s);
}
#elif !defined(EKF_BATCH_WIDE_MOVED)
extern "C" size_t ekf_batch_wide_lds_bytes(int model, int kmax) {
    return model == 1 ? wide_lds_bytes_of<1>(kmax) : wide_lds_bytes_of<0>(kmax);
}

__global__ __launch_bounds__(256) void ekf_batch_wide_window_kernel(EkfBatchLargeWindow g) {
    ekf_batch_wide_window<0, false>(g);
}
__global__ __launch_bounds__(256) void ekf_batch_wide_rot_window_kernel(EkfBatchLargeWindow g) {
    ekf_batch_wide_window<1, false>(g);
}
__global__ __launch_bounds__(256) void ekf_batch_one_block_window_kernel(EkfBatchLargeWindow g) {
    ekf_batch_wide_window<0, true>(g);
}
__global__ __launch_bounds__(256) void ekf_batch_one_block_rot_window_kernel(EkfBatchLargeWindow g) {
    ekf_batch_wide_window<1, true>(g);
}

void ekf_launch_batch_wide_window(int model, bool one_block, const EkfBatchLargeWindow& g, int members, hipStream_t s) {
    if (g.w.frozen) return ekf_launch_batch_frozen_wide_window(model, one_block, g, members, s);     // (ekf_batch_wide_frozen.hip)
    if (g.w.motion) return ekf_launch_batch_moved_wide_window(model, one_block, g, members, s);      // (ekf_batch_wide_moved.hip)
    static bool once[2][2] = {{false, false}, {false, false}};
    if (model == 1)
        wide_launch<1>(one_block ? ekf_batch_one_block_rot_window_kernel : ekf_batch_wide_rot_window_kernel,
                       once[1][one_block], g, members, s);
    else
        wide_launch<0>(one_block ? ekf_batch_one_block_window_kernel : ekf_batch_wide_window_kernel, once[0][one_block], g,
                       members, s);
}
#else      // ekf_batch_wide_moved.hip: the instances with the motion stage
__global__ __launch_bounds__(256) void ekf_batch_moved_wide_window_kernel(EkfBatchLargeWindow g) {
    ekf_batch_wide_window<0, false, true>(g);
}
__global__ __launch_bounds__(256) void ekf_batch_moved_wide_rot_window_kernel(EkfBatchLargeWindow g) {
    ekf_batch_wide_window<1, false, true>(g);
}
__global__ __launch_bounds__(256) void ekf_batch_moved_one_block_window_kernel(EkfBatchLargeWindow g) {
    ekf_batch_wide_window<0, true, true>(g);
}
__global__ __launch_bounds__(256) void ekf_batch_moved_one_block_rot_window_kernel(EkfBatchLargeWindow g) {
    ekf_batch_wide_window<1, true, true>(g);
}

void ekf_launch_batch_moved_wide_window(int model, bool one_block, const EkfBatchLargeWindow& g, int members, hipStream_t s) {
    static bool once[2][2] = {{false, false}, {false, false}};
    if (model == 1)
        wide_launch<1>(one_block ? ekf_batch_moved_one_block_rot_window_kernel : ekf_batch_moved_wide_rot_window_kernel,
                       once[1][one_block], g, members, s);
    else
        wide_launch<0>(one_block ? ekf_batch_moved_one_block_window_kernel : ekf_batch_moved_wide_window_kernel,
                       once[0][one_block], g, members, s);
}
#endif
