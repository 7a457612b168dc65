// Host build of the smoothing step functions (csrc/ekf_smooth_device.h, __host__ __device__), for
// tests/test_smooth_cpu.py.  Not part of the library.
//   stdin:  a command per line
//     "tri N"                 -> "ok" if ekf_smooth_tri enumerates 0 .. N (N + 1) / 2 - 1 column by column without a gap,
//                                ekf_smooth_sym mirrors it and ekf_smooth_col / ekf_smooth_tri_count agree; "bad" otherwise
//     "roundtrip q_p (4) q_s (4)" -> delta[3:10] (7 numbers) of the residual between x_p and x^s, then the quaternion
//                                that the injection of delta[7:10] into q_p gives (4 numbers), as %.17g
// Host libm differs from the device's: the numbers agree with the kernel's to rounding, not to the bit.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ekf_smooth_device.h"

int main() {
    char cmd[32];
    while (std::scanf("%31s", cmd) == 1) {
        if (!std::strcmp(cmd, "tri")) {
            long n = 0;
            if (std::scanf("%ld", &n) != 1 || n < 1) return 2;
            bool ok = ekf_smooth_tri_count(n) == n * (n + 1) / 2;
            int64_t next = 0;
            for (long j = 0; j < n && ok; ++j) {
                ok = ok && ekf_smooth_col(n, j) == next;
                for (long i = j; i < n && ok; ++i, ++next)
                    ok = ekf_smooth_tri(n, i, j) == next && ekf_smooth_sym(n, i, j) == next && ekf_smooth_sym(n, j, i) == next;
            }
            std::printf("%s\n", ok && next == n * (n + 1) / 2 ? "ok" : "bad");
        } else if (!std::strcmp(cmd, "roundtrip")) {
            double xp[EKF_CAM] = {0}, xs[EKF_CAM] = {0};
            for (int i = 0; i < 4; ++i)
                if (std::scanf("%lf", &xp[3 + i]) != 1) return 2;
            for (int i = 0; i < 4; ++i)
                if (std::scanf("%lf", &xs[3 + i]) != 1) return 2;
            double d[EKF_CAM];
            for (int i = 0; i < EKF_CAM; ++i) d[i] = ekf_smooth_residual(i, xs, xp);
            double q[4] = {xp[3], xp[4], xp[5], xp[6]};
            ekf_smooth_quat_inject(q, d + 7);
            for (int i = 3; i < EKF_CAM; ++i) std::printf("%.17g ", d[i]);
            for (int i = 0; i < 4; ++i) std::printf("%.17g ", q[i]);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
