// Camera motion between frames of the single filter (include/ekf_slam_hip.h: ekf_move; arithmetic: ekf_motion_device.h).
// P <- F~ P F~^T touches rows and columns 0 .. 9 only: the 10 x (N - 10) strip with its mirror and the 10 x 10 block.
//
// Strip: one thread per column j >= 10.  It loads P[0:10, j] (ten loads, each coalesced across the wave), applies F and
// stores the ten results to P[0:10, j] and, from the same (rounded) values, to P[j, 0:10]: the mirror is a copy, so P stays
// bitwise symmetric.  A column is read and written by its own thread alone, so the strip needs no ordering between threads.
// Block: workgroup 0.  Thread j < 10 leaves column j of B = F P_cc in LDS; behind a barrier thread i < 10 applies F to row i
// of B, which is row i of F P_cc F^T, and stores the lower triangle and its mirror.
// State: every workgroup forms F from the camera state as it was BEFORE the move (one thread, into LDS), so c' and q' may
// be stored only once every workgroup has read it.  A grid of one workgroup (N <= 10 + EKF_MOTION_THREADS) stores them
// itself behind its last barrier; a larger grid leaves the state alone, and a one-thread launch behind it on the same
// stream forms c' and q' again -- the same function on the same input, the same bits -- and stores them.  No counter, no
// wait between workgroups.
// A filter whose status word is set ignores the motion: both kernels return before they write anything.
#include "ekf_motion_device.h"
#include "ekf_kernels.h"

#include <algorithm>

namespace {

__device__ __forceinline__ void ekf_motion_store_state(const EkfMotionArgs& a, const EkfMotionF& f) {
    for (int i = 0; i < 3; ++i) a.state[i] = f.c1[i];
    for (int i = 0; i < 4; ++i) a.state[3 + i] = f.q1[i];
}

template <typename T>
__global__ __launch_bounds__(EKF_MOTION_THREADS) void ekf_motion_kernel(EkfMotionArgs a) {
    __shared__ EkfMotionF f;
    __shared__ double bmat[EKF_CAM][EKF_CAM];
    __shared__ int32_t live;
    const int tid = threadIdx.x;
    if (tid == 0) {
        live = a.status[0] == 0;
        if (live) ekf_motion_form(a.state, a.u, f);
    }
    __syncthreads();
    if (!live) return;
    T* __restrict__ P = static_cast<T*>(a.cov);
    const int64_t ld = a.ld;
    const int64_t j = EKF_CAM + (int64_t)blockIdx.x * EKF_MOTION_THREADS + tid;
    if (j < a.dims) {
        double in[EKF_CAM], out[EKF_CAM];
#pragma unroll
        for (int k = 0; k < EKF_CAM; ++k) in[k] = (double)P[k * ld + j];
        ekf_motion_column(f, in, out);
#pragma unroll
        for (int k = 0; k < EKF_CAM; ++k) {
            const T v = (T)out[k];
            P[k * ld + j] = v;
            P[j * ld + k] = v;
        }
    }
    if (blockIdx.x == 0) {
        double in[EKF_CAM], out[EKF_CAM];
        if (tid < EKF_CAM) {
#pragma unroll
            for (int k = 0; k < EKF_CAM; ++k) in[k] = (double)P[k * ld + tid];
            ekf_motion_column(f, in, out);
#pragma unroll
            for (int k = 0; k < EKF_CAM; ++k) bmat[k][tid] = out[k];
        }
        __syncthreads();      // (B complete; every thread of the block has also loaded its column of P_cc)
        if (tid < EKF_CAM) {
#pragma unroll
            for (int k = 0; k < EKF_CAM; ++k) in[k] = bmat[tid][k];
            ekf_motion_column(f, in, out);
            for (int k = 0; k <= tid; ++k) {
                const T v = (T)out[k];
                P[(int64_t)tid * ld + k] = v;
                P[(int64_t)k * ld + tid] = v;
            }
        }
    }
    if (gridDim.x == 1) {
        __syncthreads();      // (nobody reads the old state any more: F is in LDS)
        if (tid == 0) ekf_motion_store_state(a, f);
    }
}

__global__ __launch_bounds__(64) void ekf_motion_state_kernel(EkfMotionArgs a) {
    if (threadIdx.x != 0 || a.status[0] != 0) return;
    EkfMotionF f;
    ekf_motion_form(a.state, a.u, f);
    ekf_motion_store_state(a, f);
}

}  // namespace

template <typename T>
void ekf_launch_motion(const EkfMotionArgs& a, hipStream_t s) {
    const int strip = a.dims > EKF_CAM ? a.dims - EKF_CAM : 0;
    const unsigned grid = (unsigned)std::max(1, (strip + EKF_MOTION_THREADS - 1) / EKF_MOTION_THREADS);
    hipLaunchKernelGGL(ekf_motion_kernel<T>, dim3(grid), dim3(EKF_MOTION_THREADS), 0, s, a);
    if (grid > 1) hipLaunchKernelGGL(ekf_motion_state_kernel, dim3(1), dim3(64), 0, s, a);
}

template void ekf_launch_motion<float>(const EkfMotionArgs&, hipStream_t);
template void ekf_launch_motion<double>(const EkfMotionArgs&, hipStream_t);
