// Host build of the pose front end's device code (csrc/ekf_ippe_device.h, __host__ __device__), for
// tests/test_pose_sweep_cpu.py: ippe_square_pose per marker, on the CPU.  Not part of the library.
//   stdin:  fx fy cx cy  k1 k2 p1 p2 k3 k4 k5 k6  marker_size  count, then count x 8 corner coordinates (pixels)
//   stdout: one line per marker: tvec (3) rvec (3) as %.17g, and the candidate chosen (0 / 1)
// Host FMA contraction and libm differ from the device's: the numbers agree with the kernel's to rounding, not to the bit.
#include <cstdio>
#include <vector>

#include "ekf_ippe_device.h"

int main() {
    EkfCamera cam;
    double size = 0.0;
    long count = 0;
    if (std::scanf("%lf %lf %lf %lf", &cam.fx, &cam.fy, &cam.cx, &cam.cy) != 4) return 2;
    for (int i = 0; i < 8; ++i)
        if (std::scanf("%lf", &cam.k[i]) != 1) return 2;
    if (std::scanf("%lf %ld", &size, &count) != 2 || count < 0) return 2;
    std::vector<double> corners((size_t)count * 8);
    for (double& c : corners)
        if (std::scanf("%lf", &c) != 1) return 2;
    for (long j = 0; j < count; ++j) {
        Vec3 t, r;
        const int best = ippe_square_pose(cam, corners.data() + 8 * j, 0.5 * size, t, r);
        std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %d\n", t.x, t.y, t.z, r.x, r.y, r.z, best);
    }
    return 0;
}
