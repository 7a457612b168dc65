// Replicas of one detection log (ekf_batch_replica_poses, ekf_batch_observe_replicas in ekf_batch_api.hip): the noisy
// poses of every (replica, detection) pair, one thread each.  The noise definition is part of the ABI
// (include/ekf_slam_hip.h):
//   out[r][d][c] = poses[d][c] + sigma[r][c] g_c(seed, r0 + r, d),  c < 6,
//   g_{2j}, g_{2j+1} = Box-Muller of Philox4x32-10(key (seed_lo, seed_hi), counter (d_lo, d_hi, r0 + r, j)), j = 0, 1, 2,
// with u = (((x0 << 32 | x1) >> 11) + 0.5) 2^-53 from each pair of words.  A pair (replica, detection) depends on nothing
// else: not on how many replicas a call holds nor which ones share it.  Three Philox calls, three f64 log and sin / cos
// pairs and 48 bytes stored per thread; sigma of the launch's replicas travels in the kernel arguments.
#include "ekf_kernels.h"
#include "ekf_philox.h"

namespace {

constexpr int kReplicaThreads = 256;

struct ReplicaArgs {
    const double* poses;      // [D][6]
    double* out;              // [count][D][6]
    int64_t D;
    uint32_t key0, key1;      // seed_lo, seed_hi
    uint32_t r0;              // replica number of the launch's first replica
    int32_t count;            // replicas of this launch (<= EKF_REPLICA_CHUNK)
    double sigma[EKF_REPLICA_CHUNK][6];
};
static_assert(sizeof(ReplicaArgs) <= 4096, "kernel arguments");

__global__ __launch_bounds__(kReplicaThreads) void ekf_replica_poses_kernel(ReplicaArgs p) {
    const int64_t e = (int64_t)blockIdx.x * kReplicaThreads + threadIdx.x;
    if (e >= p.D * p.count) return;
    const int r = (int)(e / p.D);
    const int64_t d = e - (int64_t)r * p.D;
    const double* pose = p.poses + 6 * d;
    double* out = p.out + 6 * e;
    for (int j = 0; j < 3; ++j) {
        uint32_t c[4] = {(uint32_t)d, (uint32_t)((uint64_t)d >> 32), p.r0 + (uint32_t)r, (uint32_t)j};
        philox4x32_10(c, p.key0, p.key1);
        const double ua = unit_open(c[0], c[1]), ub = unit_open(c[2], c[3]);
        const double rad = sqrt(-2.0 * log(ua)), ang = 2.0 * M_PI * ub;
        out[2 * j] = pose[2 * j] + p.sigma[r][2 * j] * (rad * cos(ang));
        out[2 * j + 1] = pose[2 * j + 1] + p.sigma[r][2 * j + 1] * (rad * sin(ang));
    }
}

}  // namespace

void ekf_launch_replica_poses(const double* poses_dev, int64_t D, const double* sigma, int32_t count, uint64_t seed,
                              uint32_t r0, double* out_dev, hipStream_t s) {
    for (int32_t c0 = 0; c0 < count; c0 += EKF_REPLICA_CHUNK) {
        ReplicaArgs p{};
        p.poses = poses_dev;
        p.out = out_dev + (size_t)c0 * D * 6;
        p.D = D;
        p.key0 = (uint32_t)seed;
        p.key1 = (uint32_t)(seed >> 32);
        p.r0 = r0 + (uint32_t)c0;
        p.count = count - c0 < EKF_REPLICA_CHUNK ? count - c0 : EKF_REPLICA_CHUNK;
        for (int r = 0; r < p.count; ++r)
            for (int c = 0; c < 6; ++c) p.sigma[r][c] = sigma[(size_t)(c0 + r) * 6 + c];
        const int64_t threads = D * p.count;
        if (threads == 0) continue;
        hipLaunchKernelGGL(ekf_replica_poses_kernel, dim3((unsigned)((threads + kReplicaThreads - 1) / kReplicaThreads)),
                           dim3(kReplicaThreads), 0, s, p);
    }
}
