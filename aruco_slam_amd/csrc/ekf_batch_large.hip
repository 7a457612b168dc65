// Batch of independent filters with dictionary-sized maps (ekf_batch_observe_logs with EKF_FLAG_BATCH_LARGE_MAPS,
// ekf_batch_api.hip): the window kernels of both models, for N = lmd n + 10 up to 1024 (EKF n <= 338, EKF_Rotations
// n <= 101).  ONE workgroup of 256 threads owns ONE member for a window of its log's frames, as in ekf_batch_impl.h, and
// every frame runs the algebra of that kernel in the same operation order (so where both run, the bits are the same):
//   first sightings, h and dh of every detection,
//   A = H (P+Q) [k, N], S = A[:,supp] H^T + R I (lower triangle), S = L L^T (left-looking, in LDS),
//   W = L^-1 A and y = L^-1 (z - h), dx = W^T y and the injection,
//   P <- (P+Q) - W^T W.
// What moves is the data: A / W [k][ld] lives in the member's slice of the batch workspace (HBM), y [k] in LDS.  LDS holds
// L, 1 / L_jj, J, y and one region R of 256 x round_up(kmax, 4) doubles that serves three phases in turn: each thread's
// private copy of the column it substitutes, then dx, then a panel of 256 rows of W^T for the covariance update.  LDS thus
// depends on kmax only (149,680 bytes at the rotations model's kmax = 56).
// Covariance update: thread t owns column c = c0 + t for column blocks c0 = 0, 256, ...; it keeps W[:,c] in registers and
// streams its column of P in blocks of 8 rows with two blocks loaded ahead (24 doubles in flight per thread), against the
// panel of W^T rows in LDS (broadcast reads).  Entry (i,c) runs the l-ascending fma chain of ekf_batch_impl.h.
// P of a member is read and written by its own workgroup only: workgroup barriers are the only ordering.
#include "ekf_batch_impl.h"

namespace {

constexpr int kLargeThreads = 256;
constexpr int kRowBlock = 8;        // rows of P per fma block

template <int MODEL> constexpr int large_kw() { return (EkfModel<MODEL>::RD * EkfBatchCaps<MODEL>::MAX_VISIBLE + 3) / 4 * 4; }

// dynamic LDS, doubles: R [256][round_up(kmax, 4)] | L [kmax][kmax] | dinv [kmax] | J [kmax][JC] | y [kmax],
// then ints: first state column per detection [MAX_VISIBLE] | failure flag
template <int MODEL> size_t large_lds_bytes_of(int kmax) {
    const size_t kp = (size_t)(kmax + 3) / 4 * 4;
    return 8 * ((size_t)kLargeThreads * kp + (size_t)kmax * kmax + kmax + (size_t)kmax * EkfModel<MODEL>::JC + kmax) +
           4 * (EkfBatchCaps<MODEL>::MAX_VISIBLE + 4);
}

typedef double ekf_d2 __attribute__((ext_vector_type(2)));

template <int MODEL> __device__ __forceinline__ void ekf_batch_large_window(const EkfBatchLargeWindow& g) {
    constexpr int RD = EkfModel<MODEL>::RD, LMD = EkfModel<MODEL>::LMD, JC = EkfModel<MODEL>::JC;
    constexpr int KW = large_kw<MODEL>();
    const EkfBatchWindow& a = g.w;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = kLargeThreads;
    const int64_t t_end = a.member_frames[b + 1];
    const int64_t t0 = a.member_frames[b] + a.window_first;
    const int64_t t1 = t0 + a.window_frames < t_end ? t0 + a.window_frames : t_end;
    if (t0 >= t1) return;
    const int kmax = a.kmax, kpmax = (kmax + 3) & ~3;
    double* R = reinterpret_cast<double*>(smem);
    double* L = R + (size_t)nt * kpmax;
    double* dinv = L + (size_t)kmax * kmax;
    double* J = dinv + kmax;
    double* y = J + (size_t)kmax * JC;
    int* col0 = reinterpret_cast<int*>(y + kmax);
    int* flag = col0 + EkfBatchCaps<MODEL>::MAX_VISIBLE;

    const int64_t ld = a.ld;
    double* P = a.P + (size_t)b * ld * ld;
    double* st = a.state + (size_t)b * ld;
    double* A = g.W + (size_t)b * g.w_stride;      // A, then W: [k][ld]
    const double* nzb = a.noise + 6 * b;      // ekf_config order: icu, ilu, r, q_cam, q_err, q_lm
    const EkfNoise nz{nzb[3], nzb[4], nzb[5], nzb[2]};
    const double lm_unc = nzb[1];
    int n = a.nlm[b];
    bool failed = a.status[b] != 0;
    const bool gated = a.mahal || (a.gate && a.gate[b] < __builtin_inf());
    if (tid == 0) *flag = 0;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t d0 = a.frame_offsets[t];
        const int mf = (int)(a.frame_offsets[t + 1] - d0);
        if (failed || mf == 0) {      // not stepped: the rows repeat the state (NaN once the member has failed)
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
        __syncthreads();
        // the gate: the frame runs on the m detections that stay, in log order (mask: which ones)
        int m = mf;
        uint64_t mask = ~0ull;
        if (gated) {
            mask = ekf_batch_gate<MODEL>(a, b, d0, mf, n0, N, tid, nt, st, P, ld, nz, R, flag + 1);
            m = __popcll(mask);
            if (m == 0) {      // no survivor: an empty frame
                ekf_batch_rows_unstepped(a, t, tid, st, P, false);
                continue;
            }
        }
        const int k = RD * m, kp = (k + 3) & ~3;
        // h, dh and y = z - h
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
                ekf_measure_rot(cam, lm, h, reinterpret_cast<double(*)[JC]>(J + (size_t)RD * tid * JC));
                ekf_pose_z(pose + 6 * src, RD, z);
            }
            for (int r = 0; r < RD; ++r) y[RD * tid + r] = z[r] - h[r];
        }
        __syncthreads();
        // A = H (P+Q): thread c owns column c
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
                    A[(int64_t)(RD * j + r) * ld + c] = acc;
                }
            }
        }
        __syncthreads();
        // S = A[:,supp] H^T + R I, lower triangle, into L
        for (int e = tid; e < k * k; e += nt) {
            const int r = e / k, rr = e - r * k;
            if (rr > r) continue;
            const double* Ar = A + (int64_t)r * ld;
            const double* Jr = J + rr * JC;
            const int c0 = col0[rr / RD];
            double acc = 0.0;
            for (int s = 0; s < EKF_CAM; ++s) acc = fma(Ar[s], Jr[s], acc);
            for (int q = 0; q < LMD; ++q) acc = fma(Ar[c0 + q], Jr[EKF_CAM + q], acc);
            L[r * kmax + rr] = acc + (r == rr ? nz.r_unc : 0.0);
        }
        __syncthreads();
        // S = L L^T, left-looking, as ekf_batch_impl.h (pivots recomputed by every thread of the column)
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
            continue;
        }
        // W = L^-1 A and y = L^-1 (z - h): thread c substitutes column c (c = N: y) in place; a column of A is copied to
        // the thread's own slice of R ([i][thread]: the lanes of a wave read consecutive doubles), substituted there and
        // written back once
        for (int c = tid; c <= N; c += nt) {
            double* v = c == N ? y : R + tid;
            const int vs = c == N ? 1 : nt;
            if (c < N)
                for (int i = 0; i < k; ++i) v[i * vs] = A[(int64_t)i * ld + c];
            for (int i = 0; i < k; ++i) {
                const double* Li = L + i * kmax;
                double s = v[i * vs];
                for (int l = 0; l < i; ++l) s = fma(-Li[l], v[l * vs], s);
                v[i * vs] = s * dinv[i];
            }
            if (c < N)
                for (int i = 0; i < k; ++i) A[(int64_t)i * ld + c] = v[i * vs];
        }
        __syncthreads();
        // dx = W^T y (into R: every thread's slice is done)
        double* dx = R;
        for (int c = tid; c < N; c += nt) {
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
            for (int c = tid; c < N; c += nt)
                if (c < 3 || c >= EKF_CAM) st[c] += dx[c];
        } else {
            // injection (ekf_with_rotations.py:146-177): thread 0 the camera block, thread i landmark i - 1 (n <= 101 < nt)
            if (tid <= n) {
                const int c0 = tid == 0 ? 0 : EKF_CAM + LMD * (tid - 1);
                ekf_inject_rot_block(st + c0, dx + c0, tid == 0);
            }
        }
        // P <- (P+Q) - W^T W.  Rows l in [k, kp) of the panel and of w are zero: fma(0, 0, acc) = acc (acc is never -0),
        // so padding the chain to a multiple of 4 leaves every entry's bits as they are.
        double* WT = R;      // [256 rows of the panel][kp]
        for (int cb = 0; cb < N; cb += nt) {
            const int c = cb + tid;
            const bool own = c < N;
            const int cc = own ? c : N - 1;      // (loads stay inside the member's matrix)
            const double qc = ekf_qdiag(cc, N, nz);
            double w[KW];
#pragma unroll
            for (int l = 0; l < KW; ++l) {
                const double v = A[(int64_t)min(l, k - 1) * ld + cc];
                w[l] = l < k ? v : 0.0;
            }
            for (int i0 = 0; i0 < N; i0 += nt) {
                const int rows = min(nt, N - i0);
                __syncthreads();      // (the previous panel, or dx, is no longer read)
                for (int l = 0; l < kp; ++l)
                    WT[tid * kp + l] = l < k && tid < rows ? A[(int64_t)l * ld + i0 + tid] : 0.0;
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
                        if (l0 < kp) {
#pragma unroll
                            for (int u = 0; u < kRowBlock; ++u) {
                                const ekf_d2* Wr = reinterpret_cast<const ekf_d2*>(WT + (ib + u) * kp + l0);
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
                        if (ib + u < rows) Pc[(int64_t)(ib + u) * ld] = (p[u] + (i == c ? qc : 0.0)) - acc[u];
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
        __syncthreads();
        ekf_batch_rows_stepped(a, t, tid, st, P, y, 1, k);
    }
    if (tid == 0) a.nlm[b] = n;
}

template <int MODEL>
void large_launch(void (*kernel)(EkfBatchLargeWindow), bool& once, const EkfBatchLargeWindow& g, int members,
                  hipStream_t s) {
    if (!once) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024);
        once = true;
    }
    hipLaunchKernelGGL(kernel, dim3(members), dim3(kLargeThreads), large_lds_bytes_of<MODEL>(g.w.kmax), s, g);
}

}  // namespace

extern "C" size_t ekf_batch_large_lds_bytes(int model, int kmax) {
    return model == 1 ? large_lds_bytes_of<1>(kmax) : large_lds_bytes_of<0>(kmax);
}

__global__ __launch_bounds__(256) void ekf_batch_large_window_kernel(EkfBatchLargeWindow g) { ekf_batch_large_window<0>(g); }
__global__ __launch_bounds__(256) void ekf_batch_large_rot_window_kernel(EkfBatchLargeWindow g) {
    ekf_batch_large_window<1>(g);
}

void ekf_launch_batch_large_window(int model, const EkfBatchLargeWindow& g, int members, hipStream_t s) {
    static bool once[2] = {false, false};
    if (model == 1)
        large_launch<1>(ekf_batch_large_rot_window_kernel, once[1], g, members, s);
    else
        large_launch<0>(ekf_batch_large_window_kernel, once[0], g, members, s);
}
