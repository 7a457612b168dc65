// Offline smoothing (include/ekf_slam_hip.h: the smoothing rules): the per-element arithmetic of ONE backward
// step of the Rauch-Tung-Striebel pass, shared by the resident kernel, the blocked tier (ekf_smooth.hip) and the host build
// of tests/host/smooth_host_main.hip.  Everything is f64; every sum is one ascending fma chain in the order written here.
//   ekf_smooth_tri        index of P[i][j], i >= j, in a packed lower triangle stored column by column
//   ekf_smooth_qdiag      Q_eff on the diagonal of the prediction
//   ekf_smooth_residual   delta: additive on 0..2 and 10..N-1, zero on 3..6, the rotation vector of q^s (x) q_p^-1 on 7..9
//   ekf_smooth_ft         F~^T y (rows 0..9 only; the rest of y passes through)
//   ekf_smooth_inject     x^s = inject(x_r, c): the filter's scalar-first injection
// (__host__ __device__: the arithmetic of ekf_quat_inject_n, mode 1, is restated here because that one is device-only.)
#pragma once
#include "ekf_motion_device.h"

// A packed lower triangle of an N x N symmetric matrix, column after column: column j holds rows j .. N-1, contiguous.  A
// sweep down a column (the Cholesky scaling, the trailing update of one column, the load of P[:, j]) touches consecutive
// doubles, so consecutive lanes hit consecutive LDS banks.
__host__ __device__ __forceinline__ int64_t ekf_smooth_col(int64_t N, int64_t j) { return j * (2 * N - j + 1) / 2; }
__host__ __device__ __forceinline__ int64_t ekf_smooth_tri(int64_t N, int64_t i, int64_t j) {      // i >= j
    return ekf_smooth_col(N, j) + (i - j);
}
__host__ __device__ __forceinline__ int64_t ekf_smooth_sym(int64_t N, int64_t i, int64_t j) {      // any i, j
    return i >= j ? ekf_smooth_tri(N, i, j) : ekf_smooth_tri(N, j, i);
}
__host__ __device__ __forceinline__ int64_t ekf_smooth_tri_count(int64_t N) { return N * (N + 1) / 2; }

// Q_eff = fl(s_eff q) per entry, formed on the host (q[0] camera position, q[1] error state, q[2] landmarks); the
// quaternion dims get none.
__host__ __device__ __forceinline__ double ekf_smooth_qdiag(int i, const double q[3]) {
    if (i < 3) return q[0];
    if (i < 7) return 0.0;
    if (i < EKF_CAM) return q[1];
    return q[2];
}

// delta[i] of the backward step: xs = x^s_{r+1}, xp = the prediction (camera moved), i < N_r.
__host__ __device__ inline double ekf_smooth_residual(int i, const double* xs, const double* xp) {
#pragma clang fp contract(off)
    if (i < 3 || i >= EKF_CAM) return xs[i] - xp[i];
    if (i < 7) return 0.0;
    // dq = q^s (x) conj(q_p) (the norm of q_p cancels in the quotient): the exact inverse of q <- normalise((1, e/2) (x) q)
    const double w1 = xs[3], x1 = xs[4], y1 = xs[5], z1 = xs[6];
    const double w2 = xp[3], x2 = -xp[4], y2 = -xp[5], z2 = -xp[6];
    const double w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2;
    double v;
    if (i == 7) v = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2;
    else if (i == 8) v = w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2;
    else v = w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2;
    return 2.0 * v / w;
}

// w[0:10] = F^T y[0:10], F = [I G GE; 0 Rm 0; 0 0 I] (ekf_motion_device.h); moved == 0: F = I.
__host__ __device__ inline void ekf_smooth_ft(const EkfMotionF& f, int moved, const double y[EKF_CAM], double w[EKF_CAM]) {
#pragma clang fp contract(off)
    for (int i = 0; i < EKF_CAM; ++i) w[i] = y[i];
    if (!moved) return;
    for (int k = 0; k < 4; ++k) {
        double acc = f.turns ? 0.0 : y[3 + k];
        if (f.turns)
            for (int i = 0; i < 4; ++i) acc = fma(f.rm[i][k], y[3 + i], acc);
        for (int i = 0; i < 3; ++i) acc = fma(f.fg[i][k], y[i], acc);
        w[3 + k] = acc;
    }
    for (int k = 0; k < 3; ++k) {
        double acc = y[7 + k];
        for (int i = 0; i < 3; ++i) acc = fma(f.fg[i][4 + k], y[i], acc);
        w[7 + k] = acc;
    }
}

// The camera quaternion of x^s = inject(x_r, c): q <- normalise((1, e/2) (x) q), scalar first (the expressions of
// ekf_quat_inject_n, mode 1, in their order).
__host__ __device__ inline void ekf_smooth_quat_inject(double q[4], const double err[3]) {
#pragma clang fp contract(off)
    const double nq = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double d[4] = {1.0, 0.5 * err[0], 0.5 * err[1], 0.5 * err[2]};
    const double nd = 1.0 / sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
    const double w1 = d[0] * nd, x1 = d[1] * nd, y1 = d[2] * nd, z1 = d[3] * nd;
    const double w2 = q[0] * nq, x2 = q[1] * nq, y2 = q[2] * nq, z2 = q[3] * nq;
    const double w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2;
    const double x = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2;
    const double y = w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2;
    const double z = w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2;
    const double nr = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    q[0] = w * nr; q[1] = x * nr; q[2] = y * nr; q[3] = z * nr;
}

// x^s[i] for i < 3 or i >= 10: additive.  (3..6: ekf_smooth_quat_inject on c[7:10]; 7..9: the error dims stay 0.)
__host__ __device__ __forceinline__ double ekf_smooth_inject_add(double x, double c) { return x + c; }
