// Detection -> pose front end, batched: the pose of every detected square marker from its four image corners
// (reference: BaseFilter.estimate_pose_of_markers, filters/base_filter.py:92-171 -- one cv2.solvePnP(...,
// flags=SOLVEPNP_IPPE_SQUARE) per marker in a Python loop).  One thread per marker, f64 throughout.
//
// OpenCV itself is not in the reference tree (a pip dependency) and not in this image; what follows restates the
// PUBLISHED algorithm behind that flag -- Collins & Bartoli, "Infinitesimal Plane-based Pose Estimation", IJCV 2014,
// specialised to a square -- in the order OpenCV documents it:
//   1. pixel corners -> normalised, undistorted image points (pinhole + Brown-Conrady k1 k2 p1 p2 k3 [k4 k5 k6],
//      the fixed-point iteration of cv::undistortPoints, 5 iterations);
//   2. the homography H from the marker plane (corners (-s/2, s/2), (s/2, s/2), (s/2, -s/2), (-s/2, -s/2), the order
//      IPPE_SQUARE prescribes and base_filter.py:113-121 passes) to those points, exact for four points
//      (square -> quadrilateral in closed form);
//   3. IPPE: from the Jacobian J of H at the marker centre and the centre's image v, the rotation R_v that takes the
//      optical axis to the ray through v, the 2x2 factor A = B^-1 J with B = [I | -v] R_v, its largest singular
//      value gamma, and the two rotations whose upper-left 2x2 block is A / gamma;
//   4. for either rotation the translation by linear least squares over the four corners;
//   5. the solution with the smaller reprojection error (normalised image plane) is returned as [tvec | rvec],
//      rvec = axis * angle of the rotation, through its unit quaternion (largest of trace, R00, R11, R22; angle =
//      2 atan2(|v|, w)): exact to rounding for every angle in [0, pi].  A marker that faces a level camera is a rotation
//      by pi or close to it; cv::Rodrigues switches formulas inside |sin| < 1e-5 and is off by up to about 2e-5 rad there,
//      so a cv2 run differs by that much inside cv's own window.
// A degenerate detection (the pixel corners are not those of a strictly convex quadrilateral, or a coordinate is NaN or
// Inf) gets six NaN (ippe_corners_valid, ippe_square_pose in ekf_ippe_device.h).
// No fixture of the reference pins these numbers ("parity unpinned"): tests compare the kernel with a NumPy
// restatement of the same steps (oracle/ippe_numpy.py), with the poses the corners were projected from, and over a table
// of edge geometries with an extended-precision restatement under a conditioned bound (oracle/ippe_extended.py,
// tests/pose_sweep_util.py).
// One KNOWN structural difference to the reference's call: base_filter.py passes float32 corners and object points, and
// cv::undistortPoints returns CV_32F for float32 input, so OpenCV's normalised points are rounded to f32 before IPPE;
// this kernel stays in f64 throughout.  Expect ~1e-7 relative differences in tvec / rvec against a cv2 run (the
// as-written EKF amplifies such differences over long free runs: SURVEY F5).
#include "ekf_ippe_device.h"

namespace {

__global__ __launch_bounds__(64) void ekf_ippe_square_kernel(const double* __restrict__ corners, int count, double half,
                                                             EkfCamera cam, double* __restrict__ out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count) return;
    // the corners in the order (-h, h), (h, h), (h, -h), (-h, -h); steps 1 to 5 in ekf_ippe_device.h
    Vec3 best_t, best_r;
    ippe_square_pose(cam, corners + 8 * j, half, best_t, best_r);
    out[6 * j + 0] = best_t.x;
    out[6 * j + 1] = best_t.y;
    out[6 * j + 2] = best_t.z;
    out[6 * j + 3] = best_r.x;
    out[6 * j + 4] = best_r.y;
    out[6 * j + 5] = best_r.z;
}

}  // namespace

void ekf_launch_ippe_square(const double* corners_dev, int count, double marker_size, const EkfCamera& cam,
                            double* poses_dev, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL(ekf_ippe_square_kernel, dim3((count + 63) / 64), dim3(64), 0, s, corners_dev, count,
                       0.5 * marker_size, cam, poses_dev);
}
