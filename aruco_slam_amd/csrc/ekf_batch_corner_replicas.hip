// Replicas of one detection log with the noise where the detector has it, on the four pixel corners of every marker
// (ekf_batch_replica_corners, ekf_batch_observe_corner_replicas in ekf_batch_api.hip): one thread per (replica, detection)
// draws the corner noise, estimates the pose by IPPE (ekf_ippe_device.h, the code of ekf_estimate_poses) and labels the
// pair whose IPPE solution flipped.  The definition is part of the ABI (include/ekf_slam_hip.h):
//   noisy[r][d][i] = corners[d][i] + sigma_px[r] (g_u, g_v),  i < 4, in pixels, before undistortion,
//   (g_u, g_v) = Box-Muller of Philox4x32-10(key (seed_lo, seed_hi), counter (d_lo, d_hi, r0 + r, 4 + i))
// (counter words 4 .. 7: disjoint from the pose noise of ekf_batch_replicas.hip, words 0 .. 2), the pose is IPPE of the
// noisy corners, and
//   flipped[r][d] = trace(R_a R_clean^T) < trace(R_b R_clean^T)
// with R_a / R_b the returned / the other candidate of the noisy corners and R_clean the rotation IPPE returns for the
// corners as logged: the rejected candidate was the one nearer to the clean pose.  A pair (replica, detection) depends on
// nothing else.  Four Philox calls, four f64 log and sin / cos pairs and one IPPE per thread; with `flipped` asked for, the
// clean corners' IPPE and the two noisy rotations once more (no pre-pass over the detections: the replica workspace holds
// no room for R_clean, and this kernel is a small part of a call).  sigma_px of the launch's replicas travels
// in the kernel arguments.
#include "ekf_ippe_device.h"
#include "ekf_philox.h"

namespace {

constexpr int kCornerThreads = 256;

struct CornerReplicaArgs {
    const double* corners;    // [D][4][2] pixels, as logged
    double* poses;            // [count][D][6] or null
    uint8_t* flipped;         // [count][D] or null
    double* noisy;            // [count][D][4][2] or null
    int64_t D;
    uint32_t key0, key1;      // seed_lo, seed_hi
    uint32_t r0;              // replica number of the launch's first replica
    int32_t count;            // replicas of this launch (<= EKF_REPLICA_CHUNK)
    double half;              // marker_size / 2
    EkfCamera cam;
    double sigma[EKF_REPLICA_CHUNK];
};
static_assert(sizeof(CornerReplicaArgs) <= 4096, "kernel arguments");

// the rotation IPPE returns for pixel corners [4][2] (steps 1 to 5 without the rotation vector)
__device__ __forceinline__ void ippe_square_rotation(const EkfCamera& cam, const double* corners, double half,
                                                     double R[3][3]) {
    double px[4], py[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ippe_undistort(cam, corners[2 * i], corners[2 * i + 1], px[i], py[i]);
    IppeFactor f;
    ippe_factor(px, py, half, f);
    double R1[3][3];
    Vec3 t;
    ippe_candidate(f, 0, R);
    ippe_candidate(f, 1, R1);
    const double err0 = ippe_translation(R, px, py, half, t), err1 = ippe_translation(R1, px, py, half, t);
    if (err1 < err0) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i][j] = R1[i][j];
    }
}

__device__ __forceinline__ double trace_abt(const double A[3][3], const double B[3][3]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) s += A[i][j] * B[i][j];
    return s;
}

__global__ __launch_bounds__(kCornerThreads) void ekf_corner_replicas_kernel(CornerReplicaArgs p) {
    const int64_t e = (int64_t)blockIdx.x * kCornerThreads + threadIdx.x;
    if (e >= p.D * p.count) return;
    const int r = (int)(e / p.D);
    const int64_t d = e - (int64_t)r * p.D;
    const double* clean = p.corners + 8 * d;
    const double sg = p.sigma[r];
    double c8[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t c[4] = {(uint32_t)d, (uint32_t)((uint64_t)d >> 32), p.r0 + (uint32_t)r, (uint32_t)(4 + i)};
        philox4x32_10(c, p.key0, p.key1);
        const double ua = unit_open(c[0], c[1]), ub = unit_open(c[2], c[3]);
        const double rad = sqrt(-2.0 * log(ua)), ang = 2.0 * M_PI * ub;
        c8[2 * i] = clean[2 * i] + sg * (rad * cos(ang));
        c8[2 * i + 1] = clean[2 * i + 1] + sg * (rad * sin(ang));
    }
    if (p.noisy) {
#pragma unroll
        for (int i = 0; i < 8; ++i) p.noisy[8 * e + i] = c8[i];
    }
    Vec3 t, rv;
    const int best = ippe_square_pose(p.cam, c8, p.half, t, rv);
    if (p.poses) {
        double* out = p.poses + 6 * e;
        out[0] = t.x;
        out[1] = t.y;
        out[2] = t.z;
        out[3] = rv.x;
        out[4] = rv.y;
        out[5] = rv.z;
    }
    if (p.flipped) {
        double Rc[3][3], Ra[3][3], Rb[3][3];
        ippe_square_rotation(p.cam, clean, p.half, Rc);
        // The two rotations of the noisy corners once more, from copies the compiler cannot tell from new values: sharing
        // the pose path's intermediates would give them more uses there and could change which of its products are
        // contracted into fma, and the pose path has to stay ekf_ippe_square_kernel's to the bit.
        double o8[8], px[4], py[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            o8[i] = c8[i];
            asm volatile("" : "+v"(o8[i]));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) ippe_undistort(p.cam, o8[2 * i], o8[2 * i + 1], px[i], py[i]);
        IppeFactor f;
        ippe_factor(px, py, p.half, f);
        ippe_candidate(f, best, Ra);
        ippe_candidate(f, 1 - best, Rb);
        p.flipped[e] = trace_abt(Ra, Rc) < trace_abt(Rb, Rc) ? 1 : 0;
    }
}

}  // namespace

void ekf_launch_corner_replicas(const double* corners_dev, int64_t D, const double* sigma_px, int32_t count, uint64_t seed,
                                uint32_t r0, double marker_size, const EkfCamera& cam, double* poses_dev,
                                uint8_t* flipped_dev, double* noisy_dev, hipStream_t s) {
    for (int32_t c0 = 0; c0 < count; c0 += EKF_REPLICA_CHUNK) {
        CornerReplicaArgs p{};
        p.corners = corners_dev;
        p.poses = poses_dev ? poses_dev + (size_t)c0 * D * 6 : nullptr;
        p.flipped = flipped_dev ? flipped_dev + (size_t)c0 * D : nullptr;
        p.noisy = noisy_dev ? noisy_dev + (size_t)c0 * D * 8 : nullptr;
        p.D = D;
        p.key0 = (uint32_t)seed;
        p.key1 = (uint32_t)(seed >> 32);
        p.r0 = r0 + (uint32_t)c0;
        p.count = count - c0 < EKF_REPLICA_CHUNK ? count - c0 : EKF_REPLICA_CHUNK;
        p.half = 0.5 * marker_size;
        p.cam = cam;
        for (int r = 0; r < p.count; ++r) p.sigma[r] = sigma_px[c0 + r];
        const int64_t threads = D * p.count;
        if (threads == 0) continue;
        hipLaunchKernelGGL(ekf_corner_replicas_kernel, dim3((unsigned)((threads + kCornerThreads - 1) / kCornerThreads)),
                           dim3(kCornerThreads), 0, s, p);
    }
}
