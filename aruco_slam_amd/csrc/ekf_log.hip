// Kernels of the log replay (ekf_observe_log, ekf_log_api.hip): a whole ragged detection log in one call.
//   prepare     : every detection's measurement z from its logged pose, once per call
//   add_markers : first sightings of a frame, gathered from the logged poses (the add_marker arithmetic of ekf_markers.h)
//   fill_rows   : trajectory rows of frames without detections (the filter is not stepped there)
#include "ekf_kernels.h"
#include "ekf_markers.h"

// z of detection d (ekf_pose_z, ekf_markers.h)
__global__ __launch_bounds__(256) void ekf_log_prepare_kernel(const double* __restrict__ poses, int64_t count, int rd,
                                                              double* __restrict__ z) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= count) return;
    ekf_pose_z(poses + 6 * d, rd, z + rd * d);
}

void ekf_launch_log_prepare(const double* poses_dev, int64_t count, int rd, double* z_dev, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL(ekf_log_prepare_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, poses_dev, count, rd,
                       z_dev);
}

// New landmark j = the detection in slot slots[j] of the log; every one of them sees the camera state that is on the device
// now (the frame's pre-update camera, as in EKF.observe, extended_kalman_filter.py:80-106).  Default uncertainty.
template <typename T, int MODEL>
__global__ void ekf_log_add_markers_kernel(T* P, int64_t ld, double* state, int dims, const double* __restrict__ poses,
                                           const int32_t* __restrict__ slots, double default_unc, int count) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const double* ps = poses + 6 * (int64_t)slots[j];
    if constexpr (MODEL == 0) ekf_add_marker_xyz(P, ld, state, dims, j, ps, nullptr, default_unc);
    else ekf_add_marker_pose(P, ld, state, dims, j, ps, nullptr, default_unc);
}

template <typename T>
void ekf_launch_log_add_markers(int model, void* cov, int64_t ld, double* state, int32_t dims, const double* poses_dev,
                                const int32_t* slots_dev, double default_unc, int32_t count, hipStream_t s) {
    if (model == 1)
        hipLaunchKernelGGL((ekf_log_add_markers_kernel<T, 1>), dim3((count + 63) / 64), dim3(64), 0, s, static_cast<T*>(cov), ld,
                           state, dims, poses_dev, slots_dev, default_unc, count);
    else
        hipLaunchKernelGGL((ekf_log_add_markers_kernel<T, 0>), dim3((count + 63) / 64), dim3(64), 0, s, static_cast<T*>(cov), ld,
                           state, dims, poses_dev, slots_dev, default_unc, count);
}
template void ekf_launch_log_add_markers<float>(int, void*, int64_t, double*, int32_t, const double*, const int32_t*, double,
                                                int32_t, hipStream_t);
template void ekf_launch_log_add_markers<double>(int, void*, int64_t, double*, int32_t, const double*, const int32_t*, double,
                                                 int32_t, hipStream_t);

// pairs [count][2] = (row, source): trajectory row `row` <- row `source`, or state[0:7] where source < 0.  The pairs sit in
// pinned host memory (read once, 8 bytes per empty frame); a source row is always written before the launch is enqueued.
__global__ __launch_bounds__(256) void ekf_log_fill_rows_kernel(double* traj, const int32_t* pairs, int count,
                                                                const double* state) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 7 * count) return;
    const int e = i / 7, c = i % 7;
    const int row = pairs[2 * e], src = pairs[2 * e + 1];
    traj[7 * (int64_t)row + c] = src < 0 ? state[c] : traj[7 * (int64_t)src + c];
}

void ekf_launch_log_fill_rows(double* traj_dev, const int32_t* pairs, int32_t count, const double* state, hipStream_t s) {
    if (count <= 0) return;
    hipLaunchKernelGGL(ekf_log_fill_rows_kernel, dim3((7 * count + 255) / 256), dim3(256), 0, s, traj_dev, pairs, count, state);
}
