// Offline smoothing: the Rauch-Tung-Striebel backward pass over the records of a recorded replay (include/ekf_slam_hip.h:
// the smoothing rules; per-element arithmetic: ekf_smooth_device.h).  Only the smoothed STATE is formed, so a
// backward step r+1 -> r is one Cholesky solve and one matrix-vector product:
//   x_p = move(x_r, u),  P_p = F~ P_r F~^T + diag(Q_eff),  delta = x^s_{r+1} (-) x_p,  y = P_p^-1 delta,
//   c = P_r (F~^T y),  x^s_r = inject(x_r, c).
//   pack     : one record of a recorded replay: state and the lower triangle of P, packed column by column
//   resident : every record has N <= 160: ONE launch of ONE workgroup runs the whole pass, P_p as a packed triangle in LDS
//   batch    : the resident pass, one workgroup per member of an ekf_batch over the member's own records (grid = members)
//   blocked  : any N: per step expand / move / prepare / the blocked Cholesky of ekf_wide.hip (ncols = 0: the right-hand
//              side rides along as its residual) / backward substitution / matrix-vector product and injection
// Nothing here writes the filter: the history, the table and the workspace are the caller's, and the status word is the
// pass's own.
#include "ekf_kernels.h"
#include "ekf_smooth_device.h"
#include "ekf_smooth_resident.h"

#include <algorithm>

namespace {

// ---- pack ---------------------------------------------------------------------------------------------------------------
// Workgroup j copies column j of the lower triangle: P[j][i], i >= j (P is bitwise symmetric, and row j is contiguous).
__global__ __launch_bounds__(256) void ekf_history_pack_kernel(const double* __restrict__ P, int64_t ld,
                                                               const double* __restrict__ state, int N,
                                                               double* __restrict__ rec) {
    const int j = blockIdx.x;
    double* tri = rec + N + ekf_smooth_col(N, j);
    for (int i = j + threadIdx.x; i < N; i += 256) tri[i - j] = P[(int64_t)j * ld + i];
    if (j == 0)
        for (int i = threadIdx.x; i < N; i += 256) rec[i] = state[i];
}

__global__ __launch_bounds__(64) void ekf_smooth_rows_kernel(const double* __restrict__ src, double* __restrict__ out,
                                                             int f0, int f1) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e < 7 * (f1 - f0)) out[(int64_t)7 * f0 + e] = src[e % 7];
}

// ---- resident tier ------------------------------------------------------------------------------------------------------
// The pass itself is ekf_smooth_resident_pass (ekf_smooth_resident.h: ekf_batch_smooth_cov.hip runs it too, with the
// covariances of every step); the two kernels here form the state only (EkfSmoothStateOnly: a step hook without code).
// the single filter: one workgroup, one table; a bad pivot sets the pass's status word and ends the pass there
__global__ __launch_bounds__(EKF_SMOOTH_THREADS) void ekf_smooth_resident_kernel(const double* __restrict__ hist,
                                                                                 const EkfSmoothRec* __restrict__ table,
                                                                                 int R, int lead_frames,
                                                                                 double* __restrict__ smoothed,
                                                                                 int32_t* status) {
    extern __shared__ double tri[];
    if (!ekf_smooth_resident_pass(hist, hist, table, R, 0, lead_frames, smoothed, tri, EkfSmoothStateOnly{}) &&
        threadIdx.x == 0)
        atomicOr(status, EKF_ST_NOT_SPD);
}

// the batch: workgroup b runs the pass over member b's table and writes the member's own status word; nothing is shared
// between workgroups.  A bad pivot: every row of the member is NaN.  A member that failed in the replay: NaN from its failing
// frame on (its last record's rows end there).  No records: the lead rows only.
__global__ __launch_bounds__(EKF_SMOOTH_THREADS) void ekf_batch_smooth_kernel(const double* __restrict__ hist,
                                                                              const EkfSmoothRec* __restrict__ tables,
                                                                              const EkfBatchSmoothMember* __restrict__ members,
                                                                              double* __restrict__ smoothed,
                                                                              int32_t* __restrict__ status) {
    extern __shared__ double tri[];
    const EkfBatchSmoothMember m = members[blockIdx.x];
    const int tid = threadIdx.x;
    const double nan = __builtin_nan("");
    bool ok = true;
    if (m.records > 0)
        ok = ekf_smooth_resident_pass(hist, hist + m.head, tables + m.table, m.records, m.frame0, m.lead1, smoothed, tri,
                                      EkfSmoothStateOnly{});
    else
        for (int e = tid; e < 7 * (m.lead1 - m.frame0); e += EKF_SMOOTH_THREADS)
            smoothed[(int64_t)7 * m.frame0 + e] = hist[m.head + e % 7];
    const int n0 = ok ? m.nan0 : m.frame0;
    __syncthreads();      // (the NaN rows of a bad member overwrite rows other threads of the pass have written)
    for (int e = tid; e < 7 * (m.frame1 - n0); e += EKF_SMOOTH_THREADS) smoothed[(int64_t)7 * n0 + e] = nan;
    if (tid == 0) status[blockIdx.x] = ok ? 0 : EKF_BATCH_ST_NUMERIC;
}

// ---- blocked tier -------------------------------------------------------------------------------------------------------
// expand: M = P_r unpacked and mirrored, identity beyond N (the padding of the blocked factorisation); xp = x_r
__global__ __launch_bounds__(256) void ekf_smooth_expand_kernel(EkfSmoothBlocked a, int npad) {
    const int N = a.rec.dims, i = blockIdx.x;
    const double* __restrict__ xg = a.history + a.rec.off;
    const double* __restrict__ pg = xg + N;
    for (int j = threadIdx.x; j < npad; j += 256)
        a.M[(int64_t)i * npad + j] = (i < N && j < N) ? pg[ekf_smooth_sym(N, i, j)] : (i == j ? 1.0 : 0.0);
    if (i == 0)
        for (int j = threadIdx.x; j < N; j += 256) a.xp[j] = xg[j];
}

// prepare: Q_eff on the diagonal, delta into the right-hand side (zero in the padding)
__global__ __launch_bounds__(256) void ekf_smooth_prepare_kernel(EkfSmoothBlocked a, int npad) {
    const int N = a.rec.dims, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    if (i < N) a.M[(int64_t)i * npad + i] += ekf_smooth_qdiag(i, a.next.q);
    a.yv[i] = i < N ? ekf_smooth_residual(i, a.xs, a.xp) : 0.0;
}

// L^T y' = y over block columns of EKF_WIDE_BLOCK from the last: wave 0 solves the diagonal block with y in registers,
// then every thread takes the block's contribution out of the rows above it (row j of L is contiguous: coalesced).
// y lives in dynamic LDS [npad].  At the end w = F~^T y' (F formed again from x_r: the same function on the same input).
__global__ __launch_bounds__(EKF_SMOOTH_THREADS) void ekf_smooth_backsub_kernel(EkfSmoothBlocked a, int npad) {
    extern __shared__ double y[];
    __shared__ double zs[EKF_WIDE_BLOCK];
    __shared__ EkfMotionF F;
    const int tid = threadIdx.x, lane = tid & 63, N = a.rec.dims;
    if (a.status[0] != 0) return;
    for (int i = tid; i < npad; i += EKF_SMOOTH_THREADS) y[i] = a.yv[i];
    if (tid == 0 && a.next.moved) ekf_motion_form(a.history + a.rec.off, a.next.u, F);
    __syncthreads();
    for (int B = npad / EKF_WIDE_BLOCK - 1; B >= 0; --B) {
        const int j0 = EKF_WIDE_BLOCK * B;
        if (tid < 64) {
            double v = y[j0 + lane];
            for (int jj = EKF_WIDE_BLOCK - 1; jj >= 0; --jj) {
                const double* lrow = a.M + (int64_t)(j0 + jj) * npad + j0;
                if (lane == jj) v = v / lrow[jj];
                const double zj = __shfl(v, jj);
                if (lane < jj) v = __builtin_fma(-lrow[lane], zj, v);
            }
            y[j0 + lane] = v;
            zs[lane] = v;
        }
        __syncthreads();
        for (int i = tid; i < j0; i += EKF_SMOOTH_THREADS) {
            double acc = y[i];
            for (int jj = EKF_WIDE_BLOCK - 1; jj >= 0; --jj)
                acc = __builtin_fma(-a.M[(int64_t)(j0 + jj) * npad + i], zs[jj], acc);
            y[i] = acc;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double y10[EKF_CAM], w10[EKF_CAM];
        for (int i = 0; i < EKF_CAM; ++i) y10[i] = y[i];
        ekf_smooth_ft(F, a.next.moved, y10, w10);
        for (int i = 0; i < EKF_CAM; ++i) a.wv[i] = w10[i];
    }
    for (int i = EKF_CAM + tid; i < N; i += EKF_SMOOTH_THREADS) a.wv[i] = y[i];
}

// c = P_r w (one ascending chain per row, P_r from the packed record), x^s_r = inject(x_r, c), the record's output rows
__global__ __launch_bounds__(EKF_SMOOTH_THREADS) void ekf_smooth_finish_kernel(EkfSmoothBlocked a) {
    __shared__ double c10[EKF_CAM], x10[EKF_CAM];
    const int tid = threadIdx.x, N = a.rec.dims;
    if (a.status[0] != 0) return;
    const double* __restrict__ xg = a.history + a.rec.off;
    const double* __restrict__ pg = xg + N;
    for (int i = tid; i < N; i += EKF_SMOOTH_THREADS) {
        double c = 0.0;
        for (int j = 0; j < N; ++j) c = __builtin_fma(pg[ekf_smooth_sym(N, i, j)], a.wv[j], c);
        a.cv[i] = c;
        if (i < EKF_CAM) c10[i] = c;
        if (i < 3) x10[i] = ekf_smooth_inject_add(xg[i], c);
        if (i >= EKF_CAM) a.xs[i] = ekf_smooth_inject_add(xg[i], c);
    }
    __syncthreads();
    if (tid == 0) ekf_smooth_inject_camera(xg, c10 + 7, x10);
    __syncthreads();
    if (tid < EKF_CAM) a.xs[tid] = x10[tid];
    for (int e = tid; e < 7 * (a.rec.frame1 - a.rec.frame0); e += EKF_SMOOTH_THREADS)
        a.smoothed[(int64_t)7 * a.rec.frame0 + e] = x10[e % 7];
}

}  // namespace

void ekf_launch_history_pack(const double* cov, int64_t ld, const double* state, int32_t dims, double* record, hipStream_t s) {
    hipLaunchKernelGGL(ekf_history_pack_kernel, dim3(dims), dim3(256), 0, s, cov, ld, state, dims, record);
}

void ekf_launch_smooth_rows(const double* src, double* smoothed, int32_t f0, int32_t f1, hipStream_t s) {
    if (f1 <= f0) return;
    hipLaunchKernelGGL(ekf_smooth_rows_kernel, dim3((7 * (f1 - f0) + 63) / 64), dim3(64), 0, s, src, smoothed, f0, f1);
}

hipError_t ekf_launch_smooth_resident(const double* history, const EkfSmoothRec* table_dev, int32_t records, int32_t nmax,
                                      int32_t lead_frames, double* smoothed, int32_t* status, hipStream_t s) {
    const size_t lds = (size_t)ekf_smooth_tri_count(nmax) * 8;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ekf_smooth_resident_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ekf_smooth_resident_kernel, dim3(1), dim3(EKF_SMOOTH_THREADS), lds, s, history, table_dev, records,
                       lead_frames, smoothed, status);
    return hipSuccess;
}

hipError_t ekf_launch_batch_smooth(const double* history, const EkfSmoothRec* tables_dev, const EkfBatchSmoothMember* members_dev,
                                   int32_t members, int32_t nmax, double* smoothed, int32_t* status, hipStream_t s) {
    const size_t lds = (size_t)ekf_smooth_tri_count(nmax) * 8;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ekf_batch_smooth_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ekf_batch_smooth_kernel, dim3(members), dim3(EKF_SMOOTH_THREADS), lds, s, history, tables_dev,
                       members_dev, smoothed, status);
    return hipSuccess;
}

void ekf_launch_smooth_blocked_prepare(const EkfSmoothBlocked& a, hipStream_t s) {
    const int N = a.rec.dims, npad = (N + EKF_WIDE_BLOCK - 1) / EKF_WIDE_BLOCK * EKF_WIDE_BLOCK;
    hipLaunchKernelGGL(ekf_smooth_expand_kernel, dim3(npad), dim3(256), 0, s, a, npad);
    if (a.next.moved) {      // the filter's own move on (M, xp): P_p before Q, x_p
        EkfMotionArgs m{};
        m.cov = a.M;
        m.ld = npad;
        m.state = a.xp;
        m.dims = N;
        for (int i = 0; i < 6; ++i) m.u[i] = a.next.u[i];
        m.status = a.status;
        ekf_launch_motion<double>(m, s);
    }
    hipLaunchKernelGGL(ekf_smooth_prepare_kernel, dim3((npad + 255) / 256), dim3(256), 0, s, a, npad);
}

void ekf_launch_smooth_blocked_solve(const EkfSmoothBlocked& a, hipStream_t s) {
    const int N = a.rec.dims, npad = (N + EKF_WIDE_BLOCK - 1) / EKF_WIDE_BLOCK * EKF_WIDE_BLOCK;
    hipLaunchKernelGGL(ekf_smooth_backsub_kernel, dim3(1), dim3(EKF_SMOOTH_THREADS), (size_t)npad * 8, s, a, npad);
    hipLaunchKernelGGL(ekf_smooth_finish_kernel, dim3(1), dim3(EKF_SMOOTH_THREADS), 0, s, a);
}

void ekf_launch_smooth_blocked_step(const EkfSmoothBlocked& a, hipStream_t s) {
    const int N = a.rec.dims, npad = (N + EKF_WIDE_BLOCK - 1) / EKF_WIDE_BLOCK * EKF_WIDE_BLOCK;
    ekf_launch_smooth_blocked_prepare(a, s);
    // the blocked Cholesky of the wide frames with no columns of A: L over M, y = L^-1 delta over the right-hand side
    EkfFrame fr{};
    fr.lmat = a.M;
    fr.ldl = npad;
    fr.yvec = a.yv;
    fr.ncols = 0;
    fr.status = a.status;
    ekf_launch_wide_factor(fr, nullptr, a.xinv, npad, s);
    ekf_launch_smooth_blocked_solve(a, s);
}
