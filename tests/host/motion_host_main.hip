// Host build of the camera-motion stage functions (csrc/ekf_motion_device.h, __host__ __device__), for
// tests/test_motion_cpu.py: one move of a (state, P) pair on the CPU, the stages called in the kernel's order
// (csrc/ekf_motion.hip).  Not part of the library.
//   stdin:  N  f32 (0 / 1: P is rounded to f32 on store, as an f32 covariance is)  u (6)  state[0:7]  P (N x N, row-major)
//   stdout: state[0:7] after the move, then P' row by row, as %.17g
// Host libm differs from the device's: the numbers agree with the kernel's to rounding, not to the bit.
#include <cstdio>
#include <vector>

#include "ekf_motion_device.h"

int main() {
    long n = 0;
    int f32 = 0;
    double u[6], cam[7];
    if (std::scanf("%ld %d", &n, &f32) != 2 || n < EKF_CAM) return 2;
    for (double& x : u)
        if (std::scanf("%lf", &x) != 1) return 2;
    for (double& x : cam)
        if (std::scanf("%lf", &x) != 1) return 2;
    std::vector<double> p((size_t)n * n);
    for (double& x : p)
        if (std::scanf("%lf", &x) != 1) return 2;
    auto store = [&](double v) { return f32 ? (double)(float)v : v; };
    EkfMotionF f;
    ekf_motion_form(cam, u, f);
    double in[EKF_CAM], out[EKF_CAM], b[EKF_CAM][EKF_CAM];
    for (long j = EKF_CAM; j < n; ++j) {      // the strip
        for (int k = 0; k < EKF_CAM; ++k) in[k] = p[(size_t)k * n + j];
        ekf_motion_column(f, in, out);
        for (int k = 0; k < EKF_CAM; ++k) p[(size_t)k * n + j] = p[(size_t)j * n + k] = store(out[k]);
    }
    for (int j = 0; j < EKF_CAM; ++j) {       // the block: B = F P_cc, then row i of F P_cc F^T = F B[i, :]^T
        for (int k = 0; k < EKF_CAM; ++k) in[k] = p[(size_t)k * n + j];
        ekf_motion_column(f, in, out);
        for (int k = 0; k < EKF_CAM; ++k) b[k][j] = out[k];
    }
    for (int i = 0; i < EKF_CAM; ++i) {
        ekf_motion_column(f, b[i], out);
        for (int k = 0; k <= i; ++k) p[(size_t)i * n + k] = p[(size_t)k * n + i] = store(out[k]);
    }
    for (int i = 0; i < 3; ++i) std::printf("%.17g ", f.c1[i]);
    for (int i = 0; i < 4; ++i) std::printf("%.17g ", f.q1[i]);
    std::printf("\n");
    for (long i = 0; i < n; ++i) {
        for (long j = 0; j < n; ++j) std::printf("%.17g ", p[(size_t)i * n + j]);
        std::printf("\n");
    }
    return 0;
}
