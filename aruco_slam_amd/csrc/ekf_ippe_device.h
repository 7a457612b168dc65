// IPPE for a square marker, the device functions (kernels: ekf_pose_ippe.hip, one thread per marker;
// ekf_batch_corner_replicas.hip, one thread per (replica, detection)).  The steps and their sources are described in
// ekf_pose_ippe.hip; f64 throughout.  One definition for both kernels: a replica whose corner noise is zero gets the bits
// ekf_estimate_poses gives.
#pragma once
#include "ekf_kernels.h"

struct Vec3 { double x, y, z; };

__host__ __device__ __forceinline__ void ippe_undistort(const EkfCamera& cam, double u, double v, double& x, double& y) {
    const double x0 = (u - cam.cx) / cam.fx, y0 = (v - cam.cy) / cam.fy;
    x = x0;
    y = y0;
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icd = (1.0 + ((cam.k[7] * r2 + cam.k[6]) * r2 + cam.k[5]) * r2) /
                           (1.0 + ((cam.k[4] * r2 + cam.k[1]) * r2 + cam.k[0]) * r2);
        const double dx = 2.0 * cam.k[2] * x * y + cam.k[3] * (r2 + 2.0 * x * x);
        const double dy = cam.k[2] * (r2 + 2.0 * y * y) + 2.0 * cam.k[3] * x * y;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
}

// translation for a given rotation: minimise sum_i |(X_i' + t_x, Y_i' + t_y) - (Z_i' + t_z) p_i|^2, P_i' = R P_i
// (normal equations of the 8 x 3 system [1 0 -x_i; 0 1 -y_i] t = [x_i Z' - X'; y_i Z' - Y']), and the reprojection
// error of the resulting pose
__host__ __device__ __forceinline__ double ippe_translation(const double R[3][3], const double px[4],
                                                            const double py[4], double h, Vec3& t) {
    const double ox[4] = {-h, h, h, -h}, oy[4] = {h, h, -h, -h};
    double sxx = 0.0, syy = 0.0, sx = 0.0, sy = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
    double Xr[4], Yr[4], Zr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        Xr[i] = R[0][0] * ox[i] + R[0][1] * oy[i];
        Yr[i] = R[1][0] * ox[i] + R[1][1] * oy[i];
        Zr[i] = R[2][0] * ox[i] + R[2][1] * oy[i];
        const double rx = px[i] * Zr[i] - Xr[i], ry = py[i] * Zr[i] - Yr[i];
        sx += px[i];
        sy += py[i];
        sxx += px[i] * px[i];
        syy += py[i] * py[i];
        bx += rx;
        by += ry;
        bz += -px[i] * rx - py[i] * ry;
    }
    // M = [[4, 0, -sx], [0, 4, -sy], [-sx, -sy, sxx + syy]] (symmetric positive definite): eliminate t_x, t_y
    const double m22 = (sxx + syy) - 0.25 * (sx * sx + sy * sy);
    t.z = (bz + 0.25 * (sx * bx + sy * by)) / m22;
    t.x = 0.25 * (bx + sx * t.z);
    t.y = 0.25 * (by + sy * t.z);
    double err = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double zc = Zr[i] + t.z, ex = (Xr[i] + t.x) / zc - px[i], ey = (Yr[i] + t.y) / zc - py[i];
        err += ex * ex + ey * ey;
    }
    return err;
}

// axis * angle of a rotation matrix (the inverse of Rodrigues' formula), through the unit quaternion: the largest of
// trace, R00, R11, R22 picks the component that is formed as a sum (>= 1 before normalisation, no cancellation), the other
// three are sums and differences of off-diagonal entries; w >= 0 and angle = 2 atan2(|v|, w).  Exact to rounding for every
// angle in [0, pi]: no acos, no threshold window around 0 or pi (cv::Rodrigues has one, |sin| < 1e-5, and is off by up to
// about 2e-5 rad inside it)
__host__ __device__ __forceinline__ Vec3 ippe_rotvec(const double R[3][3]) {
    const double tr = R[0][0] + R[1][1] + R[2][2];
    double w, x, y, z;
    if (tr >= R[0][0] && tr >= R[1][1] && tr >= R[2][2]) {
        w = 1.0 + tr;
        x = R[2][1] - R[1][2];
        y = R[0][2] - R[2][0];
        z = R[1][0] - R[0][1];
    } else if (R[0][0] >= R[1][1] && R[0][0] >= R[2][2]) {
        w = R[2][1] - R[1][2];
        x = 1.0 + R[0][0] - R[1][1] - R[2][2];
        y = R[0][1] + R[1][0];
        z = R[0][2] + R[2][0];
    } else if (R[1][1] >= R[2][2]) {
        w = R[0][2] - R[2][0];
        x = R[0][1] + R[1][0];
        y = 1.0 - R[0][0] + R[1][1] - R[2][2];
        z = R[1][2] + R[2][1];
    } else {
        w = R[1][0] - R[0][1];
        x = R[0][2] + R[2][0];
        y = R[1][2] + R[2][1];
        z = 1.0 - R[0][0] - R[1][1] + R[2][2];
    }
    const double n = sqrt(w * w + x * x + y * y + z * z);
    if (w < 0.0) {
        w = -w;
        x = -x;
        y = -y;
        z = -z;
    }
    w /= n;
    x /= n;
    y /= n;
    z /= n;
    const double v = sqrt(x * x + y * y + z * z);
    if (v == 0.0) return Vec3{0.0, 0.0, 0.0};
    const double f = 2.0 * atan2(v, w) / v;
    return Vec3{x * f, y * f, z * f};
}

// What steps 2 and 3 leave for the two candidates: the rotation Rv that takes the optical axis to the ray through the
// marker centre's image, and the first two columns (r00 r10 +-b0), (r01 r11 +-b1) of R~ (R = Rv R~)
struct IppeFactor {
    double Rv[3][3];
    double r00, r01, r10, r11, b0, b1;
    double den;     // the homography's determinant of corner differences: 0 or not finite for a degenerate detection
};

// steps 2 and 3 from the normalised image points of the corners, in the order (-h, h), (h, h), (h, -h), (-h, -h)
__host__ __device__ __forceinline__ void ippe_factor(const double px[4], const double py[4], double half, IppeFactor& f) {
    // 2. homography: unit square (0,0), (1,0), (1,1), (0,1) <-> corners 3, 2, 1, 0, composed with
    //    (X, Y) -> ((X + h) / 2h, (Y + h) / 2h)
    double H[3][3];
    {
        const double x0 = px[3], y0 = py[3], x1 = px[2], y1 = py[2], x2 = px[1], y2 = py[1], x3 = px[0], y3 = py[0];
        const double dx1 = x1 - x2, dx2 = x3 - x2, sxs = x0 - x1 + x2 - x3;
        const double dy1 = y1 - y2, dy2 = y3 - y2, sys = y0 - y1 + y2 - y3;
        const double den = dx1 * dy2 - dx2 * dy1;
        f.den = den;
        const double g = (sxs * dy2 - dx2 * sys) / den, hh = (dx1 * sys - sxs * dy1) / den;
        const double a = x1 - x0 + g * x1, b = x3 - x0 + hh * x3, d = y1 - y0 + g * y1, e = y3 - y0 + hh * y3;
        const double s = 0.5 / half;                         // columns scaled by 1 / 2h, third = a/2 + b/2 + c ...
        const double h22 = 0.5 * g + 0.5 * hh + 1.0;
        H[0][0] = a * s / h22;
        H[0][1] = b * s / h22;
        H[0][2] = (0.5 * a + 0.5 * b + x0) / h22;
        H[1][0] = d * s / h22;
        H[1][1] = e * s / h22;
        H[1][2] = (0.5 * d + 0.5 * e + y0) / h22;
        H[2][0] = g * s / h22;
        H[2][1] = hh * s / h22;
        H[2][2] = 1.0;
    }
    // 3. IPPE
    const double p = H[0][2], q = H[1][2];
    const double j00 = H[0][0] - H[2][0] * p, j01 = H[0][1] - H[2][1] * p;
    const double j10 = H[1][0] - H[2][0] * q, j11 = H[1][1] - H[2][1] * q;
    {
        const double t = sqrt(p * p + q * q + 1.0), a = p / t, b = q / t, c = 1.0 / t, k = 1.0 / (1.0 + c);
        f.Rv[0][0] = 1.0 - a * a * k;  f.Rv[0][1] = -a * b * k;       f.Rv[0][2] = a;
        f.Rv[1][0] = -a * b * k;       f.Rv[1][1] = 1.0 - b * b * k;  f.Rv[1][2] = b;
        f.Rv[2][0] = -a;               f.Rv[2][1] = -b;               f.Rv[2][2] = c;
    }
    // B = [I | -v] Rv (its first two columns), A = B^-1 J
    const double b00 = f.Rv[0][0] - p * f.Rv[2][0], b01 = f.Rv[0][1] - p * f.Rv[2][1];
    const double b10 = f.Rv[1][0] - q * f.Rv[2][0], b11 = f.Rv[1][1] - q * f.Rv[2][1];
    const double idet = 1.0 / (b00 * b11 - b01 * b10);
    const double a00 = idet * (b11 * j00 - b01 * j10), a01 = idet * (b11 * j01 - b01 * j11);
    const double a10 = idet * (-b10 * j00 + b00 * j10), a11 = idet * (-b10 * j01 + b00 * j11);
    const double ata00 = a00 * a00 + a10 * a10, ata01 = a00 * a01 + a10 * a11, ata11 = a01 * a01 + a11 * a11;
    const double gamma = sqrt(0.5 * (ata00 + ata11 + sqrt((ata00 - ata11) * (ata00 - ata11) + 4.0 * ata01 * ata01)));
    f.r00 = a00 / gamma;
    f.r01 = a01 / gamma;
    f.r10 = a10 / gamma;
    f.r11 = a11 / gamma;
    // third row of the first two columns: b0^2 = 1 - |c0|^2, b1^2 = 1 - |c1|^2, b0 b1 = -c0.c1
    f.b0 = sqrt(fmax(1.0 - f.r00 * f.r00 - f.r10 * f.r10, 0.0));
    f.b1 = sqrt(fmax(1.0 - f.r01 * f.r01 - f.r11 * f.r11, 0.0));
    if (f.r00 * f.r01 + f.r10 * f.r11 > 0.0) f.b1 = -f.b1;
}

// the rotation of candidate `sol` (0: third row (b0, b1), 1: its negative): R~ = [c0 c1 c0 x c1], R = Rv R~
__host__ __device__ __forceinline__ void ippe_candidate(const IppeFactor& f, int sol, double R[3][3]) {
    const double s0 = sol ? -f.b0 : f.b0, s1 = sol ? -f.b1 : f.b1;
    const double c0[3] = {f.r00, f.r10, s0}, c1[3] = {f.r01, f.r11, s1};
    const double c2[3] = {c0[1] * c1[2] - c0[2] * c1[1], c0[2] * c1[0] - c0[0] * c1[2], c0[0] * c1[1] - c0[1] * c1[0]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        R[r][0] = f.Rv[r][0] * c0[0] + f.Rv[r][1] * c0[1] + f.Rv[r][2] * c0[2];
        R[r][1] = f.Rv[r][0] * c1[0] + f.Rv[r][1] * c1[1] + f.Rv[r][2] * c1[2];
        R[r][2] = f.Rv[r][0] * c2[0] + f.Rv[r][1] * c2[1] + f.Rv[r][2] * c2[2];
    }
}

// Whether four pixel corners [4][2] are the corners of a strictly convex quadrilateral, as every image of a square is:
// the cross products of consecutive sides have one sign and each is more than 1e-9 of the sum of the squared sides (exactly
// collinear or coincident f64 corners leave a rounding residue of about 1e-12 of it at most; a marker that thin is within
// about 2e-9 rad of edge-on).  False for a NaN or Inf coordinate.  In pixels, before the undistortion bends a line.
__host__ __device__ __forceinline__ bool ippe_corners_valid(const double* __restrict__ corners) {
    double cr[4], len2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3, k = (i + 2) & 3;
        const double ax = corners[2 * j] - corners[2 * i], ay = corners[2 * j + 1] - corners[2 * i + 1];
        const double bx = corners[2 * k] - corners[2 * j], by = corners[2 * k + 1] - corners[2 * j + 1];
        cr[i] = ax * by - ay * bx;
        len2 += ax * ax + ay * ay;
    }
    const double thr = 1e-9 * len2;
    const bool pos = cr[0] > thr && cr[1] > thr && cr[2] > thr && cr[3] > thr;
    const bool neg = -cr[0] > thr && -cr[1] > thr && -cr[2] > thr && -cr[3] > thr;
    return pos || neg;
}

// Steps 1 to 5 for one marker: the pixel corners [4][2] -> [tvec | rvec] of the candidate with the smaller reprojection
// error.  Returns which candidate that was (0 or 1, in the numbering of ippe_candidate).  A degenerate detection (corners
// that are not those of a strictly convex quadrilateral: collinear, coincident, a NaN or Inf coordinate) gives six NaN.
// fmin / fmax and the comparisons below drop a NaN operand, and the undistortion makes a thin quadrilateral of collinear
// corners, so the outputs alone would not tell: the corners, the homography's determinant and both reprojection errors are
// asked.
__host__ __device__ __forceinline__ int ippe_square_pose(const EkfCamera& cam, const double* __restrict__ corners,
                                                         double half, Vec3& best_t, Vec3& best_r) {
    // 1. normalised image points of the corners
    double px[4], py[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ippe_undistort(cam, corners[2 * i], corners[2 * i + 1], px[i], py[i]);
    IppeFactor f;
    ippe_factor(px, py, half, f);
    double best_err = 0.0;
    int best = 0;
    bool valid = ippe_corners_valid(corners) && __builtin_isfinite(f.den);
    best_t = Vec3{0.0, 0.0, 0.0};
    best_r = Vec3{0.0, 0.0, 0.0};
#pragma unroll
    for (int sol = 0; sol < 2; ++sol) {
        double R[3][3];
        ippe_candidate(f, sol, R);
        // 4. and 5.
        Vec3 t;
        const double err = ippe_translation(R, px, py, half, t);
        valid = valid && __builtin_isfinite(err);
        if (sol == 0 || err < best_err) {
            best_err = err;
            best_t = t;
            best_r = ippe_rotvec(R);
            best = sol;
        }
    }
    if (!valid) {
        const double nan = __builtin_nan("");
        best_t = Vec3{nan, nan, nan};
        best_r = Vec3{nan, nan, nan};
    }
    return best;
}
