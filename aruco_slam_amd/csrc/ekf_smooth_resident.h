// Offline smoothing, the resident pass (include/ekf_slam_hip.h: the smoothing rules): the device
// function that ONE workgroup of EKF_SMOOTH_THREADS runs over ONE table of records, shared by the kernels of ekf_smooth.hip
// (the single filter's, the batch's) and of ekf_batch_smooth_cov.hip (the batch's with the covariances).  Device code only.
#pragma once
#include "ekf_kernels.h"
#include "ekf_smooth_device.h"

// the camera part of x^s_r = inject(x_r, c) and the error dims; xr, cv: the record's state and c (any memory)
__device__ __forceinline__ void ekf_smooth_inject_camera(const double* xr, const double* c7, double* xs) {
    double q[4] = {xr[3], xr[4], xr[5], xr[6]};
    ekf_smooth_quat_inject(q, c7);
    for (int i = 0; i < 4; ++i) xs[3 + i] = q[i];
    for (int i = 0; i < 3; ++i) xs[7 + i] = 0.0;
}

// The hook of a pass that forms nothing but the state: no code.
struct EkfSmoothStateOnly {
    __device__ __forceinline__ void operator()(int, const EkfSmoothRec&, const EkfSmoothRec&, const double*, const double*,
                                               const double*, const EkfMotionF&) const {}
};

// ---- resident tier ------------------------------------------------------------------------------------------------------
// LDS: the packed triangle of nmax dims (dynamic; 103 040 B at 160) and six vectors of 160 doubles.  A Cholesky column j:
// every thread reads the pivot, threads scale the column (the diagonal of L goes to ld_s: nobody overwrites what others
// still read), a barrier, then wave w of the 8 updates the trailing columns j+1+w, j+9+w, ... -- lanes down a column, which is
// contiguous -- and the wave whose turn the "column N" is carries the right-hand side along (forward substitution).  The
// backward substitution runs in ONE wave with y in registers; then P_r is read again from the history into the triangle's
// LDS (L is no longer needed) for c = P_r w.
// The pass itself, for the single filter's kernel and for the batch's (one workgroup of EKF_SMOOTH_THREADS runs it over ONE
// table of R >= 1 records): offsets of the table count doubles from `hist`, rows [lead0, lead1) of `smoothed` repeat
// head[0:7], `tri` is the dynamic LDS.  Returns false at the first P_p with a pivot that is not positive (every thread saw
// the same pivots, so all of them return together); the rows written until then stay.
// `step` is called by every thread once per backward step r+1 -> r, behind the barrier that ends the backward substitution
// and before P_r is loaded over the factor: step(r, table[r], table[r+1], the record's packed triangle in the history, tri,
// ld_s, F).  There L is the packed column-major triangle in `tri` with its diagonal in ld_s (the diagonal words of tri
// hold d, not sqrt(d)), and F is the motion of the step when table[r+1].moved.  It may read all of these, must not write
// them, and must end with a barrier when it reads tri.  The state arithmetic does not depend on it.
template <class Step>
__device__ __forceinline__ bool ekf_smooth_resident_pass(const double* __restrict__ hist, const double* __restrict__ head,
                                                         const EkfSmoothRec* __restrict__ table, int R, int lead0, int lead1,
                                                         double* __restrict__ smoothed, double* tri, const Step& step) {
    __shared__ double xs[EKF_SMOOTH_RESIDENT_DIMS], xr[EKF_SMOOTH_RESIDENT_DIMS], xp[EKF_SMOOTH_RESIDENT_DIMS];
    __shared__ double dv[EKF_SMOOTH_RESIDENT_DIMS], wv[EKF_SMOOTH_RESIDENT_DIMS], ld_s[EKF_SMOOTH_RESIDENT_DIMS];
    __shared__ EkfMotionF F;
    __shared__ double bmat[EKF_CAM][EKF_CAM];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    {
        const EkfSmoothRec last = table[R - 1];
        if (tid < last.dims) xs[tid] = hist[last.off + tid];
        __syncthreads();
        for (int e = tid; e < 7 * (last.frame1 - last.frame0); e += EKF_SMOOTH_THREADS)
            smoothed[(int64_t)7 * last.frame0 + e] = xs[e % 7];
        for (int e = tid; e < 7 * (lead1 - lead0); e += EKF_SMOOTH_THREADS) smoothed[(int64_t)7 * lead0 + e] = head[e % 7];
    }
    for (int r = R - 2; r >= 0; --r) {
        const EkfSmoothRec rec = table[r], nx = table[r + 1];
        const int N = rec.dims, T = (int)ekf_smooth_tri_count(N);
        const double* __restrict__ xg = hist + rec.off;
        const double* __restrict__ pg = xg + N;
        __syncthreads();      // (the step before is over: xs is complete, tri and the vectors are free)
        for (int e = tid; e < T; e += EKF_SMOOTH_THREADS) tri[e] = pg[e];
        if (tid < N) xr[tid] = xp[tid] = xg[tid];
        __syncthreads();
        if (nx.moved) {
            if (tid == 0) ekf_motion_form(xr, nx.u, F);
            __syncthreads();
            double in[EKF_CAM], out[EKF_CAM];
            const int j = EKF_CAM + tid;
            if (j < N) {      // the strip: P[0:10, j] = P[j, 0:10], one thread per column
#pragma unroll
                for (int k = 0; k < EKF_CAM; ++k) in[k] = tri[ekf_smooth_tri(N, j, k)];
                ekf_motion_column(F, in, out);
#pragma unroll
                for (int k = 0; k < EKF_CAM; ++k) tri[ekf_smooth_tri(N, j, k)] = out[k];
            }
            if (tid < EKF_CAM) {      // the block: B = F P_cc, then row i of F P_cc F^T = F B[i, :]^T
#pragma unroll
                for (int k = 0; k < EKF_CAM; ++k) in[k] = tri[ekf_smooth_sym(N, k, tid)];
                ekf_motion_column(F, in, out);
#pragma unroll
                for (int k = 0; k < EKF_CAM; ++k) bmat[k][tid] = out[k];
            }
            __syncthreads();
            if (tid < EKF_CAM) {
#pragma unroll
                for (int k = 0; k < EKF_CAM; ++k) in[k] = bmat[tid][k];
                ekf_motion_column(F, in, out);
                for (int k = 0; k <= tid; ++k) tri[ekf_smooth_tri(N, tid, k)] = out[k];
            }
            if (tid == 0) {
                for (int i = 0; i < 3; ++i) xp[i] = F.c1[i];
                for (int i = 0; i < 4; ++i) xp[3 + i] = F.q1[i];
            }
            __syncthreads();
        }
        if (tid < N) {
            tri[ekf_smooth_tri(N, tid, tid)] += ekf_smooth_qdiag(tid, nx.q);
            dv[tid] = ekf_smooth_residual(tid, xs, xp);
        }
        __syncthreads();
        // right-looking Cholesky of P_p in place, the right-hand side with it
        bool bad = false;
        for (int j = 0; j < N; ++j) {
            const int cj = (int)ekf_smooth_col(N, j);
            const double d = tri[cj];
            const double l = sqrt(d);
            bad = bad || !(d > 0.0);
            const int i = j + 1 + tid;
            if (i < N) tri[cj + i - j] = tri[cj + i - j] / l;
            if (tid == EKF_SMOOTH_THREADS - 1) {
                ld_s[j] = l;
                dv[j] = dv[j] / l;
            }
            __syncthreads();
            for (int c = j + 1 + wave; c < N; c += EKF_SMOOTH_THREADS / 64) {
                const double lc = tri[cj + c - j];
                const int cc = (int)ekf_smooth_col(N, c);
                for (int i2 = c + lane; i2 < N; i2 += 64)
                    tri[cc + i2 - c] = __builtin_fma(-tri[cj + i2 - j], lc, tri[cc + i2 - c]);
            }
            if (((N - j - 1) & (EKF_SMOOTH_THREADS / 64 - 1)) == wave) {
                const double yj = dv[j];
                for (int i2 = j + 1 + lane; i2 < N; i2 += 64) dv[i2] = __builtin_fma(-tri[cj + i2 - j], yj, dv[i2]);
            }
            __syncthreads();
        }
        if (bad) return false;      // (every thread saw the same pivots)
        // L^T y' = y: wave 0, y in registers (lane l holds rows l, l + 64, l + 128), column by column from the last
        if (wave == 0) {
            double y0 = lane < N ? dv[lane] : 0.0, y1 = lane + 64 < N ? dv[lane + 64] : 0.0,
                   y2 = lane + 128 < N ? dv[lane + 128] : 0.0;
            for (int j = N - 1; j >= 0; --j) {
                const int part = j >> 6, jl = j & 63;
                double v = part == 0 ? y0 : (part == 1 ? y1 : y2);
                if (lane == jl) v = v / ld_s[j];
                const double zj = __shfl(v, jl);
                if (lane == jl) {
                    if (part == 0) y0 = zj; else if (part == 1) y1 = zj; else y2 = zj;
                }
                // L[j][i], i < j: column i of the triangle, row j
                if (lane < j) y0 = __builtin_fma(-tri[ekf_smooth_tri(N, j, lane)], zj, y0);
                if (lane + 64 < j) y1 = __builtin_fma(-tri[ekf_smooth_tri(N, j, lane + 64)], zj, y1);
                if (lane + 128 < j) y2 = __builtin_fma(-tri[ekf_smooth_tri(N, j, lane + 128)], zj, y2);
            }
            if (lane < N) dv[lane] = y0;
            if (lane + 64 < N) dv[lane + 64] = y1;
            if (lane + 128 < N) dv[lane + 128] = y2;
        }
        __syncthreads();
        step(r, rec, nx, pg, tri, ld_s, F);      // (the covariances of the step, or nothing)
        // w = F~^T y, and P_r again (through L2) where L was
        if (tid == 0) {
            double y10[EKF_CAM], w10[EKF_CAM];
            for (int i = 0; i < EKF_CAM; ++i) y10[i] = dv[i];
            ekf_smooth_ft(F, nx.moved, y10, w10);
            for (int i = 0; i < EKF_CAM; ++i) wv[i] = w10[i];
        } else if (tid >= EKF_CAM && tid < N) {
            wv[tid] = dv[tid];
        }
        for (int e = tid; e < T; e += EKF_SMOOTH_THREADS) tri[e] = pg[e];
        __syncthreads();
        double c = 0.0;
        if (tid < N) {
            for (int j = 0; j < N; ++j) c = __builtin_fma(tri[ekf_smooth_sym(N, tid, j)], wv[j], c);
        }
        __syncthreads();      // (everybody has read wv and dv)
        if (tid < N) dv[tid] = c;
        __syncthreads();
        if (tid < N && (tid < 3 || tid >= EKF_CAM)) xs[tid] = ekf_smooth_inject_add(xr[tid], c);
        if (tid == 3) ekf_smooth_inject_camera(xr, dv + 7, xs);
        __syncthreads();
        for (int e = tid; e < 7 * (rec.frame1 - rec.frame0); e += EKF_SMOOTH_THREADS)
            smoothed[(int64_t)7 * rec.frame0 + e] = xs[e % 7];
    }
    return true;
}
