// Camera motion between frames (include/ekf_slam_hip.h: the motion rules; EKF_FLAG_MOTION): the arithmetic of ONE move,
// shared by the single filter's launch (ekf_motion.hip) and whoever else applies a motion to a (state, P) pair.  For the
// motion u = (d, w) in the camera frame of the pose (c, q):
//   c' = c + R(q) d,  q' = normalised q (x) delta,  delta = (cos(|w|/2), sin(|w|/2) w/|w|)  ((1, 0, 0, 0) for w = 0),
//   P <- F~ P F~^T,  F~ = diag(F, I),  F = [I G G E(q); 0 Rm(delta) 0; 0 0 I]  (10 x 10, columns [c q e]).
// Three stages; the caller owns the threads, the barriers between the stages and where P lives.  The stages touch nothing
// but their arguments, every sum is ONE ascending fma chain in the order written here, all of it in f64: a move's bits
// depend neither on its caller nor on the size of the map.
//   ekf_motion_form    one thread: F, c', q' from (c, q, d, w)
//   ekf_motion_column  one thread per column j of P[0:10, :]: out = F in, in = P[0:10, j]
//   the 10 x 10 block F P_cc F^T is the same function twice: B[:, j] = ekf_motion_column(P_cc[:, j]), a barrier, then row i
//   of the result is ekf_motion_column(B[i, :]) (= F B[i, :]^T); the caller stores its lower triangle and mirrors it.
// F has structure, and the stages use it: the error-state rows of F are unit rows (those rows of P[0:10, j] are COPIED, no
// arithmetic), the quaternion rows are Rm(delta) alone (copied as well when w = 0: delta = (1, 0, 0, 0), Rm = I), and a
// position row is the unit row plus the seven entries of [G | G E].
// (__host__ __device__: tests/host/motion_host_main.hip runs the same stages on the CPU.)
#pragma once
#include "ekf_device.h"

struct EkfMotionF {
    double fg[3][7];      // [G | G E(q)]: G = d(R(q) d)/dq of the NORMALISED R (3 x 4), E(q) = d((1, e) (x) q)/de at 0 (4 x 3)
    double rm[4][4];      // Rm(delta): a (x) delta = Rm(delta) a
    double c1[3], q1[4];  // the moved camera
    int32_t turns;        // w != 0 (0: q' = q and the quaternion rows of P are copied, bit for bit)
};

// Stage 1.  cam = state[0:7] BEFORE the move, u = (d, w).
//   R(q) d = (d0 d + 2 (v.d) v + 2 a (v x d)) / s,  q = (a, v), s = a^2 + v.v, d0 = a^2 - v.v
// (the transpose of the rotation ekf_measure applies: h = R(q)^T (l - c)).
__host__ __device__ inline void ekf_motion_form(const double* cam, const double* u, EkfMotionF& f) {
#pragma clang fp contract(off)      // (the chains are written out: the same bits wherever it is inlined)
    const double a = cam[3];
    const double v[3] = {cam[4], cam[5], cam[6]};
    const double d[3] = {u[0], u[1], u[2]};
    const double w[3] = {u[3], u[4], u[5]};
    const double vv = fma(v[2], v[2], fma(v[1], v[1], v[0] * v[0]));
    const double vd = fma(v[2], d[2], fma(v[1], d[1], v[0] * d[0]));
    const double s = fma(a, a, vv), d0 = fma(a, a, -vv);
    const double is = 1.0 / s;
    const double cx[3] = {fma(v[1], d[2], -(v[2] * d[1])), fma(v[2], d[0], -(v[0] * d[2])), fma(v[0], d[1], -(v[1] * d[0]))};
    double rd[3];
    for (int i = 0; i < 3; ++i) {
        rd[i] = fma(2.0 * a, cx[i], fma(2.0 * vd, v[i], d0 * d[i])) * is;
        f.c1[i] = cam[i] + rd[i];
    }
    // G: column 0 = d/da, column 1 + j = d/dv_j; the quotient rule's second term is -2 q_k (R d) / s
    const double sd[3][3] = {{0.0, -d[2], d[1]}, {d[2], 0.0, -d[0]}, {-d[1], d[0], 0.0}};      // skew(d)
    double g[3][4];
    for (int i = 0; i < 3; ++i) {
        g[i][0] = fma(-2.0 * a, rd[i], fma(2.0, cx[i], 2.0 * a * d[i])) * is;
        for (int j = 0; j < 3; ++j) {
            double acc = i == j ? 2.0 * vd : 0.0;
            acc = fma(-2.0 * a, sd[i][j], acc);
            acc = fma(2.0 * d[j], v[i], acc);
            acc = fma(-2.0 * v[j], d[i], acc);
            acc = fma(-2.0 * v[j], rd[i], acc);
            g[i][1 + j] = acc * is;
        }
    }
    // E(q): row 0 = -v^T, rows 1..3 = a I - skew(v)
    const double e[4][3] = {{-v[0], -v[1], -v[2]}, {a, v[2], -v[1]}, {-v[2], a, v[0]}, {v[1], -v[0], a}};
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 4; ++k) f.fg[i][k] = g[i][k];
        for (int j = 0; j < 3; ++j) {
            double acc = g[i][0] * e[0][j];
            for (int r = 1; r < 4; ++r) acc = fma(g[i][r], e[r][j], acc);
            f.fg[i][4 + j] = acc;
        }
    }
    // delta and Rm(delta).  (|w|^2 that underflows to zero counts as w = 0: the vector part would be below 1e-162.)
    const double th2 = fma(w[2], w[2], fma(w[1], w[1], w[0] * w[0]));
    f.turns = th2 > 0.0;
    double dl[4] = {1.0, 0.0, 0.0, 0.0};
    if (f.turns) {
        const double th = sqrt(th2);
        double sn, cs;
        sincos(0.5 * th, &sn, &cs);
        const double k = sn / th;
        dl[0] = cs;
        dl[1] = k * w[0];
        dl[2] = k * w[1];
        dl[3] = k * w[2];
    }
    const double rm[4][4] = {{dl[0], -dl[1], -dl[2], -dl[3]}, {dl[1], dl[0], dl[3], -dl[2]},
                             {dl[2], -dl[3], dl[0], dl[1]}, {dl[3], dl[2], -dl[1], dl[0]}};
    const double q[4] = {a, v[0], v[1], v[2]};
    double p[4];
    for (int i = 0; i < 4; ++i) {
        for (int k = 0; k < 4; ++k) f.rm[i][k] = rm[i][k];
        double acc = rm[i][0] * q[0];
        for (int k = 1; k < 4; ++k) acc = fma(rm[i][k], q[k], acc);
        p[i] = acc;
    }
    if (f.turns) {      // normalised as the injection normalises its product (ekf_quat_inject_n)
        const double nr = 1.0 / sqrt(fma(p[3], p[3], fma(p[2], p[2], fma(p[1], p[1], p[0] * p[0]))));
        for (int i = 0; i < 4; ++i) f.q1[i] = p[i] * nr;
    } else {
        for (int i = 0; i < 4; ++i) f.q1[i] = q[i];
    }
}

// Stage 2, behind a barrier after stage 1: out = F in for one column in = P[0:10, j] (any j), or one row of F P_cc.
__host__ __device__ __forceinline__ void ekf_motion_column(const EkfMotionF& f, const double in[EKF_CAM], double out[EKF_CAM]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double acc = in[i];
#pragma unroll
        for (int k = 0; k < 7; ++k) acc = fma(f.fg[i][k], in[3 + k], acc);
        out[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double acc = in[3 + i];
        if (f.turns) {
            acc = f.rm[i][0] * in[3];
#pragma unroll
            for (int k = 1; k < 4; ++k) acc = fma(f.rm[i][k], in[3 + k], acc);
        }
        out[3 + i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) out[7 + i] = in[7 + i];
}
