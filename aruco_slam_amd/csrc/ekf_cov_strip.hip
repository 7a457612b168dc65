// Camera-strip covariance update of a frozen map (include/ekf_slam_hip.h, "Localisation mode"; Schmidt-Kalman update).
//
// A frozen frame keeps the landmarks in the state and in S as uncertain quantities but gives them no gain.  With
// W = L^-1 H (P+Q) the camera rows of the Schmidt update are the arithmetic the full update P <- P + Q - W^T W runs on rows
// 0 .. 9, and everything else of the full update is not done:
//     P'[r][c] = (P[r][c] + Q[r == c]) + sum_k fma(-W[k][r], W[k][c])     r < 10, c < N  (k ascending, from zero, kpad rows)
// and P'[c][r] = P'[r][c]: per element the chain of the full update the handle runs (ekf_cov_update.hip), so the strip has
// the bits of the mapping frame.  The chain step of the matrix-core kernels is one single-rounding fma in the covariance
// dtype; the VALU reference kernel forms its f32 step in f64 and rounds again (`__builtin_fma` on floats), which differs in
// double-rounding ties only.  A handle built with EKF_COVK_VALU and the f32 covariance therefore runs the instance with
// that step (template parameter VALU_STEP); for the f64 covariance the two steps are the same instruction.  P[10:N, 10:N] is
// neither read nor written (no Q_lm is added), nothing at or beyond N is touched: 2 * 10 * N elements instead of N^2.
//
// One thread per column c < N, ten accumulators, EKF_STRIP_THREADS columns per workgroup.
//   * W[k][0:10], the operand every thread shares, is staged once per workgroup into LDS (all its loads in flight at once:
//     one memory round trip) and read from there at wave-uniform addresses (broadcast reads, no bank conflict).
//   * W[k][c] is loaded coalesced along c, EKF_STRIP_ROWS rows per block, and the next block is requested before the chain
//     runs over the current one: two blocks of independent loads are in flight per wave, and the chain over k -- where
//     the time goes: a launch has few waves (49 at n = 1024), so a wave's own latency is the kernel's -- waits for memory
//     kpad / EKF_STRIP_ROWS times instead of kpad times.
//   * Stores: thread c stores P[r][c], r < 10 (ten row stores, each coalesced across the wave); a thread with c >= 10 also
//     stores the mirror P[c][0:10] (ten contiguous elements).  The 10 x 10 block is covered by the row stores of threads
//     0 .. 9 alone -- element (r, c) by thread c, once, and (c, r) by thread r from commuting products, the same bits --
//     so no two threads store to one address and P stays bitwise symmetric.
// In place: thread c reads column c of rows 0 .. 9 only, which nobody else writes, and the mirror rows it writes are read
// by nobody.  A lane beyond N takes part in the staging and the barrier, loads column N - 1 and stores nothing.
// A frame beyond 384 rows runs one launch per row chunk, in order, with Q in the first chunk only, as the full update does;
// a launch never has more than EKF_WIDE_REUSE_ROWS rows, which sizes the LDS copy.
#include <hip/hip_ext.h>
#include "ekf_kernels.h"

#define EKF_STRIP_ROWS 16      // rows of W per block of loads (kpad is a multiple of EKF_RB = 16)
#define EKF_STRIP_PAD 12       // row length of the LDS copy of W[:, 0:10]: rows stay 16-byte aligned in either dtype

// one step of the chain: a single-rounding fma in the covariance dtype (the matrix-core kernels' step), or, VALU_STEP with
// f32, the VALU reference kernel's: the f64 fma of the widened operands, rounded to f32
template <bool VALU_STEP>
__device__ __forceinline__ float ekf_strip_fma(float a, float b, float c) {
    if (VALU_STEP) return (float)__builtin_fma((double)a, (double)b, (double)c);
    return __builtin_fmaf(a, b, c);
}
template <bool VALU_STEP>
__device__ __forceinline__ double ekf_strip_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T, bool VALU_STEP>
__global__ __launch_bounds__(EKF_STRIP_THREADS) void ekf_cov_strip_kernel(EkfFrame fr) {
    __shared__ __attribute__((aligned(16))) T wcam[EKF_WIDE_REUSE_ROWS][EKF_STRIP_PAD];
    const int tid = threadIdx.x;
    const int c = blockIdx.x * EKF_STRIP_THREADS + tid;
    const bool live = c < fr.dims;
    const int cc = live ? c : fr.dims - 1;
    const T* __restrict__ wp = static_cast<const T*>(fr.wpanel);
    T* P = static_cast<T*>(fr.cov);
    const int64_t ld = fr.ld, ldw = fr.ldw;
    const int kpad = fr.kpad;
    // the first block of the column and the ten entries of P go out in front of the staging loads: one round trip for all
    const T* __restrict__ wcol = wp + cc;
    T cur[EKF_STRIP_ROWS], pv[EKF_CAM], acc[EKF_CAM];
#pragma unroll
    for (int u = 0; u < EKF_STRIP_ROWS; ++u) cur[u] = wcol[(int64_t)u * ldw];
#pragma unroll
    for (int r = 0; r < EKF_CAM; ++r) {
        pv[r] = P[r * ld + cc];
        acc[r] = (T)0;
    }
    for (int i = tid; i < kpad * EKF_CAM; i += EKF_STRIP_THREADS) {
        const int k = i / EKF_CAM, r = i - EKF_CAM * k;
        wcam[k][r] = wp[(int64_t)k * ldw + r];
    }
    __syncthreads();
    for (int k0 = 0; k0 < kpad; k0 += EKF_STRIP_ROWS) {
        T nxt[EKF_STRIP_ROWS];
        // the last block asks for its own rows again (in bounds, never used) instead of branching around the loads
        const int kn = (k0 + EKF_STRIP_ROWS < kpad) ? k0 + EKF_STRIP_ROWS : k0;
#pragma unroll
        for (int u = 0; u < EKF_STRIP_ROWS; ++u) nxt[u] = wcol[(int64_t)(kn + u) * ldw];
#pragma unroll
        for (int u = 0; u < EKF_STRIP_ROWS; ++u) {
            const T* wrow = wcam[k0 + u];      // wave-uniform
#pragma unroll
            for (int r = 0; r < EKF_CAM; ++r) acc[r] = ekf_strip_fma<VALU_STEP>(-wrow[r], cur[u], acc[r]);
        }
#pragma unroll
        for (int u = 0; u < EKF_STRIP_ROWS; ++u) cur[u] = nxt[u];
    }
    if (!live) return;
    T out[EKF_CAM];
#pragma unroll
    for (int r = 0; r < EKF_CAM; ++r) {
        T v = pv[r];
        if (r == c) v += (T)ekf_qdiag(r, fr.dims, fr.nz);
        out[r] = v + acc[r];
        P[r * ld + c] = out[r];
    }
    if (c >= EKF_CAM) {
        T* mirror = P + (int64_t)c * ld;
#pragma unroll
        for (int r = 0; r < EKF_CAM; ++r) mirror[r] = out[r];
    }
}

template <typename T, bool VALU_STEP>
static void ekf_cov_strip_go(const EkfFrame& fr, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const dim3 grid((fr.dims + EKF_STRIP_THREADS - 1) / EKF_STRIP_THREADS), block(EKF_STRIP_THREADS);
    // plain launch; with events attached, the dispatch's own start / stop time stamps land in e0 / e1
    if (e0) hipExtLaunchKernelGGL((ekf_cov_strip_kernel<T, VALU_STEP>), grid, block, 0, s, e0, e1, 0, fr);
    else hipLaunchKernelGGL((ekf_cov_strip_kernel<T, VALU_STEP>), grid, block, 0, s, fr);
}

template <typename T>
bool ekf_launch_cov_strip(const EkfFrame& fr, int variant, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (fr.kpad > EKF_WIDE_REUSE_ROWS) return false;      // (the LDS copy holds one row chunk: the caller reports it)
    if constexpr (sizeof(T) == 4) {      // (f64: one step, one instance)
        if (variant == 1) {
            ekf_cov_strip_go<T, true>(fr, s, e0, e1);
            return true;
        }
    }
    ekf_cov_strip_go<T, false>(fr, s, e0, e1);
    return true;
}
template bool ekf_launch_cov_strip<float>(const EkfFrame&, int, hipStream_t, hipEvent_t, hipEvent_t);
template bool ekf_launch_cov_strip<double>(const EkfFrame&, int, hipStream_t, hipEvent_t, hipEvent_t);
