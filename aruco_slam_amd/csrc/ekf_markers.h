// add_marker arithmetic for one new landmark (extended_kalman_filter.py:239-290, ekf_with_rotations.py:275-335).
// Shared by the host-staged launch (ekf_add_markers, ekf_small_kernels.hip) and the gather launch of the log replay
// (ekf_observe_log, ekf_log.hip): the same instructions, only the addressing of the pose differs.
#pragma once
#include "ekf_device.h"

// z of one detection from its logged pose [tvec | rvec] (rd = 3: pose[0:3]; rd = 7: [pose[0:3] | quaternion of
// from_euler("xyz", pose[3:6]), scalar first], ekf_with_rotations.py:216-224).  The quaternion is the host's euler_xyz_to_quat
// (filters/ekf_with_rotations.py) operation for operation -- half angles, q = qz (qy qx) -- with contraction off, so only
// sin / cos can differ in the last place.  Shared by the log replay (ekf_log.hip) and the batch (ekf_batch_impl.h).
__device__ inline void ekf_pose_z(const double* p, int rd, double* zd) {
#pragma clang fp contract(off)
    zd[0] = p[0];
    zd[1] = p[1];
    zd[2] = p[2];
    if (rd == 7) {
        const double ax = 0.5 * p[3], ay = 0.5 * p[4], az = 0.5 * p[5];
        const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
        const double w1 = cy * cx, x1 = cy * sx, y1 = sy * cx, z1 = -(sy * sx);
        zd[3] = cz * w1 - sz * z1;
        zd[4] = cz * x1 - sz * y1;
        zd[5] = cz * y1 + sz * x1;
        zd[6] = cz * z1 + sz * w1;
    }
}

// EKF: t_ml = R(q)^-1 p + c with the camera state in `state`; landmark j goes to column dims + 3 j.
// p = pose[0:3] of the detection; unc = its 3 variances or null (default_unc on the diagonal).
template <typename T>
__device__ inline void ekf_add_marker_xyz(T* P, int64_t ld, double* state, int dims, int j, const double* pp,
                                          const double* unc, double default_unc) {
    double q[4] = {state[3], state[4], state[5], state[6]};
    const double nq = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double a = q[0] * nq, u0 = q[1] * nq, u1 = q[2] * nq, u2 = q[3] * nq;
    const double p[3] = {pp[0], pp[1], pp[2]};
    // rot_cm = R(q)^-1 = R(q)^T  (:264-269);  t_ml = rot_cm p + c  (:272)
    const double d0 = a * a - (u0 * u0 + u1 * u1 + u2 * u2);
    const double up = u0 * p[0] + u1 * p[1] + u2 * p[2];
    const double cx[3] = {u1 * p[2] - u2 * p[1], u2 * p[0] - u0 * p[2], u0 * p[1] - u1 * p[0]};
    const double u[3] = {u0, u1, u2};
    const int c0 = dims + 3 * j;
    for (int d = 0; d < 3; ++d) {
        state[c0 + d] = d0 * p[d] + 2.0 * up * u[d] - 2.0 * a * cx[d] + state[d];
        const double var = unc ? unc[d] : default_unc;
        P[(int64_t)(c0 + d) * ld + c0 + d] = (T)var;
    }
}

// SciPy's from_matrix branch for the largest diagonal entry I of mm (x y z w); compile-time indices keep mm and qx in
// registers wherever ekf_add_marker_pose is inlined
template <int I> __device__ inline void ekf_quat_branch(const double (&mm)[3][3], double tr, double qx[4]) {
    constexpr int J = (I + 1) % 3, K = (I + 2) % 3;
    qx[I] = 1.0 - tr + 2.0 * mm[I][I];
    qx[J] = mm[J][I] + mm[I][J];
    qx[K] = mm[K][I] + mm[I][K];
    qx[3] = mm[K][J] - mm[J][K];
}

// EKF_Rotations: pose = [tvec | rvec], rvec read as extrinsic xyz Euler angles (:307-310); q_ml = from_matrix(R(q)^-1 R_cl)
// with SciPy's branch rule; landmark j goes to column dims + 10 j.  unc = its 10 variances or null.
template <typename T>
__device__ inline void ekf_add_marker_pose(T* P, int64_t ld, double* state, int dims, int j, const double* ps,
                                           const double* unc, double default_unc) {
    double q[4] = {state[3], state[4], state[5], state[6]};
    const double nq = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double a = q[0] * nq, u0 = q[1] * nq, u1 = q[2] * nq, u2 = q[3] * nq;
    // rot_cm = R(q)^T
    const double rcm[3][3] = {
        {a * a + u0 * u0 - u1 * u1 - u2 * u2, 2 * (u0 * u1 + a * u2), 2 * (u0 * u2 - a * u1)},
        {2 * (u0 * u1 - a * u2), a * a - u0 * u0 + u1 * u1 - u2 * u2, 2 * (u1 * u2 + a * u0)},
        {2 * (u0 * u2 + a * u1), 2 * (u1 * u2 - a * u0), a * a - u0 * u0 - u1 * u1 + u2 * u2}};
    const double ca = cos(ps[3]), sa = sin(ps[3]), cb = cos(ps[4]), sb = sin(ps[4]), cc = cos(ps[5]), sc = sin(ps[5]);
    // R_cl = Rz(c) Ry(b) Rx(a)
    const double rcl[3][3] = {{cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa},
                              {sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa},
                              {-sb, cb * sa, cb * ca}};
    double mm[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c2 = 0; c2 < 3; ++c2)
            mm[r][c2] = rcm[r][0] * rcl[0][c2] + rcm[r][1] * rcl[1][c2] + rcm[r][2] * rcl[2][c2];
    // matrix -> quaternion (x y z w), branch on the largest of (M00, M11, M22, trace)
    const double tr = mm[0][0] + mm[1][1] + mm[2][2];
    double dec[4] = {mm[0][0], mm[1][1], mm[2][2], tr};
    int ch = 0;
    for (int e = 1; e < 4; ++e)
        if (dec[e] > dec[ch]) ch = e;
    double qx[4];
    if (ch == 0) {
        ekf_quat_branch<0>(mm, tr, qx);
    } else if (ch == 1) {
        ekf_quat_branch<1>(mm, tr, qx);
    } else if (ch == 2) {
        ekf_quat_branch<2>(mm, tr, qx);
    } else {
        qx[0] = mm[2][1] - mm[1][2];
        qx[1] = mm[0][2] - mm[2][0];
        qx[2] = mm[1][0] - mm[0][1];
        qx[3] = 1.0 + tr;
    }
    const double nn = 1.0 / sqrt(qx[0] * qx[0] + qx[1] * qx[1] + qx[2] * qx[2] + qx[3] * qx[3]);
    const int c0 = dims + 10 * j;
    for (int d = 0; d < 3; ++d)
        state[c0 + d] = rcm[d][0] * ps[0] + rcm[d][1] * ps[1] + rcm[d][2] * ps[2] + state[d];
    state[c0 + 3] = qx[3] * nn;
    state[c0 + 4] = qx[0] * nn;
    state[c0 + 5] = qx[1] * nn;
    state[c0 + 6] = qx[2] * nn;
    for (int d = 7; d < 10; ++d) state[c0 + d] = 0.0;
    for (int d = 0; d < 10; ++d) {
        const double var = unc ? unc[d] : default_unc;
        P[(int64_t)(c0 + d) * ld + c0 + d] = (T)var;
    }
}
