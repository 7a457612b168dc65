// Per-detection chi-square distance: the arithmetic of ONE detection, shared by the single filter's gate kernel
// (ekf_gate.hip) and the batch's gate stage (ekf_batch_impl.h: ekf_batch_gate).  For a detection of landmark columns
// c0 .. c0 + LMD - 1, on the prior P with N state dimensions:
//   r = z - h(x), S_d = H_d (P+Q) H_d^T + R I (or + diag(rows_d)) [RD, RD] from the (10 + LMD)^2 support block of P,
//   S_d = L L^T and d^2 = |L^-1 r|^2, every sum one ascending fma chain, all of it in f64.
// Three stages, each one thread's work on the detection's scratch; the caller owns the threads, the barriers between the
// stages, where z comes from, who is exempt and what a distance decides.  The stages touch nothing but their arguments, so
// a detection's bits depend neither on its caller nor on the detections around it.
#pragma once
#include "ekf_kernels.h"

// Scratch of one detection, in doubles (LDS): J [RD][JC] | T = H_d (P+Q)[:, supp] [RD][JC] | S_d, then L [RD][RD] |
// r, then y = L^-1 r [RD].  90 doubles (EKF), 336 (EKF_Rotations).
template <int MODEL> struct EkfGateScratch {
    static constexpr int RD = EkfModel<MODEL>::RD, JC = EkfModel<MODEL>::JC;
    static constexpr int J = 0, T = RD * JC, S = 2 * RD * JC, R = S + RD * RD;
    static constexpr int DOUBLES = 2 * RD * JC + RD * RD + RD;
};

// Stage 1, one thread per detection: h and dh at the state (dh straight into the scratch: a register copy of 7 x 20 would
// spill) and r = z - h behind them.
template <int MODEL>
__device__ __forceinline__ void ekf_gate_measure(const double* st, int c0, const double* z, double* scr) {
    using G = EkfGateScratch<MODEL>;
    constexpr int RD = G::RD, LMD = EkfModel<MODEL>::LMD, JC = G::JC;
    double cam[EKF_CAM], lm[LMD], h[RD];
    for (int q = 0; q < EKF_CAM; ++q) cam[q] = st[q];
    for (int q = 0; q < LMD; ++q) lm[q] = st[c0 + q];
    ekf_measure_model<MODEL>(cam, lm, h, reinterpret_cast<double(*)[JC]>(scr + G::J));
    for (int r = 0; r < RD; ++r) scr[G::R + r] = z[r] - h[r];
}

// Stage 2, one thread per (detection, support column ci), behind a barrier after stage 1:
// T[:, ci] = H_d (P+Q)[supp, supp[ci]], the column's loads in one round (an f32 P is widened on load).
template <int MODEL, typename T>
__device__ __forceinline__ void ekf_gate_project(const T* P, int64_t ld, int c0, int ci, int N, const EkfNoise& nz,
                                                 double* scr) {
    using G = EkfGateScratch<MODEL>;
    constexpr int RD = G::RD, JC = G::JC;
    const int c = ci < EKF_CAM ? ci : c0 + ci - EKF_CAM;
    const double* Jd = scr + G::J;
    double pc[JC];
#pragma unroll
    for (int si = 0; si < JC; ++si) {
        const int s = si < EKF_CAM ? si : c0 + si - EKF_CAM;
        pc[si] = (double)P[(int64_t)s * ld + c] + (si == ci ? ekf_qdiag(c, N, nz) : 0.0);
    }
#pragma unroll 1
    for (int r = 0; r < RD; ++r) {      // (not unrolled, here and below: the stage stays small in registers and code)
        double acc = 0.0;
#pragma unroll
        for (int si = 0; si < JC; ++si) acc = fma(Jd[r * JC + si], pc[si], acc);
        scr[G::T + r * JC + ci] = acc;
    }
}

// Stage 3, one thread per detection, behind a barrier after stage 2: S_d, its factor and d^2.  Returns whether every
// pivot was positive and finite; only then is d2 the distance.
// rows: the variances of the detection's RD measurement rows (per-detection noise), or null: r_unc on every row.
template <int MODEL>
__device__ __forceinline__ bool ekf_gate_distance(double r_unc, const double* rows, double* scr, double& d2) {
    using G = EkfGateScratch<MODEL>;
    constexpr int RD = G::RD, JC = G::JC;
    const double* Jd = scr + G::J;
    const double* Td = scr + G::T;
    double* Sd = scr + G::S;
    double* rd = scr + G::R;
    // S_d = T H_d^T + R I, lower triangle
#pragma unroll 1
    for (int r = 0; r < RD; ++r)
#pragma unroll 1
        for (int rr = 0; rr <= r; ++rr) {
            double acc = 0.0;
#pragma unroll 4
            for (int ci = 0; ci < JC; ++ci) acc = fma(Td[r * JC + ci], Jd[rr * JC + ci], acc);
            Sd[r * RD + rr] = acc + (r == rr ? (rows ? rows[r] : r_unc) : 0.0);
        }
    // S_d = L L^T row by row (L_ii on the diagonal) with y = L^-1 r behind each row; d^2 = y^T y
    bool ok = true;
    d2 = 0.0;
#pragma unroll 1
    for (int i = 0; i < RD && ok; ++i) {
        double* Li = Sd + i * RD;
#pragma unroll 1
        for (int j = 0; j < i; ++j) {
            const double* Lj = Sd + j * RD;
            double v = Li[j];
            for (int l = 0; l < j; ++l) v = fma(-Li[l], Lj[l], v);
            Li[j] = v / Lj[j];
        }
        double dii = Li[i], y = rd[i];
        for (int l = 0; l < i; ++l) {
            dii = fma(-Li[l], Li[l], dii);
            y = fma(-Li[l], rd[l], y);
        }
        ok = dii > 0.0 && isfinite(dii);
        if (ok) {
            Li[i] = sqrt(dii);
            y = y / Li[i];
            rd[i] = y;
            d2 = fma(y, y, d2);
        }
    }
    return ok;
}
