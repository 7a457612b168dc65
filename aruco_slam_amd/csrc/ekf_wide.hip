// Wide frames: more detections than the gather kernel and the fused front kernel take (EKF m > 64, EKF_Rotations
// m > 50; up to 1024 detections with EKF_FLAG_WIDE_FRAMES).  Nothing in here sizes LDS or registers by k.
//
//   measure : h, dh, residual and landmark column, one thread per detection              (any m)
//   amat    : A = H (P + Q), column chunks x detection groups                            (k x N)
//   sblock  : lower triangle of S = A H^T + R (identity padding), 16 x 16 blocks: in the `sblk` block layout of the
//             stand-alone solve kernel for kpad <= 384 (solve / panel / covariance update are then the stage kernels,
//             unchanged), else dense into `lmat`
// kpad > 384: blocked right-looking Cholesky in f64 over block columns of 64 rows, three stream-ordered launches each
// (no workgroup ever waits for another one):
//   potrf   : S_BB = L_BB L_BB^T and X = L_BB^-1, one workgroup
//   panel   : L_iB = S_iB X^T (i > B), W_B = X A_B (all columns), y_B = X r_B
//   update  : S_ij -= L_iB L_jB^T (i >= j > B), A_i -= L_iB W_B, r_i -= L_iB y_B   (v_mfma_f64_16x16x4_f64)
// The right-hand sides ride along: the rows of A (a copy in `aw`, so that A stays readable) become W = L^-1 A and the
// residual becomes y = L^-1 (z - h), in place.  Then
//   finish  : W to the covariance-dtype panel (and the f64 debug copy), dx = W^T y, state injection.
// The covariance update P <- P + Q - W^T W is the existing launchers applied to row chunks of W (ekf_frames.hip).
#include "ekf_kernels.h"
#include "ekf_solve_device.h"

#include <algorithm>

typedef double wf64x4 __attribute__((ext_vector_type(4)));
#define WB EKF_WIDE_BLOCK

// --------------------------------------------------------------------------
// (a) measurement model of every detection
// --------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(64) void ekf_wide_measure_kernel(EkfFrame fr, int rp) {
    constexpr int RD = EkfModel<MODEL>::RD, LMD = EkfModel<MODEL>::LMD, JC = EkfModel<MODEL>::JC;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < fr.m) {
        const int c0 = ekf_lm_column(fr, LMD, t, true);
        double cam[EKF_CAM], lm[LMD], h[RD], J[RD][JC];
        for (int a = 0; a < EKF_CAM; ++a) cam[a] = fr.state[a];
        for (int d = 0; d < LMD; ++d) lm[d] = fr.state[c0 + d];
        ekf_measure_model<MODEL>(cam, lm, h, J);
        for (int d = 0; d < RD; ++d) {
            for (int a = 0; a < JC; ++a) fr.jac[(size_t)(RD * t + d) * EKF_JLD + a] = J[d][a];
            const double r = fr.z[RD * t + d] - h[d];         // additive residual, also on q_cl
            fr.resid[RD * t + d] = r;
            fr.yvec[RD * t + d] = r;                          // right-hand side of the blocked factorisation
        }
        fr.lmcol[t] = c0;
    }
    for (int r = fr.k + t; r < rp; r += gridDim.x * 64) fr.yvec[r] = 0.0;
}

// --------------------------------------------------------------------------
// (b) A = H (P + Q): 64 columns x WIDE_G detections per workgroup, one wave per detection (same per-element
// instruction sequence as the gather kernel)
// --------------------------------------------------------------------------
#define WIDE_G 16
template <typename T, int MODEL>
__global__ __launch_bounds__(256) void ekf_wide_amat_kernel(EkfFrame fr, double* aw, int rp) {
    constexpr int RD = EkfModel<MODEL>::RD, LMD = EkfModel<MODEL>::LMD;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);            // < ncols <= ld
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const T* __restrict__ P = static_cast<const T*>(fr.cov);
    const int64_t ld = fr.ld;
    double pc[EKF_CAM];
#pragma unroll
    for (int a = 0; a < EKF_CAM; ++a) pc[a] = (double)P[a * ld + c] + ((a == c) ? ekf_qdiag(a, fr.dims, fr.nz) : 0.0);
    for (int u = 0; u < WIDE_G / 4; ++u) {
        const int j = blockIdx.y * WIDE_G + w + 4 * u;
        if (j >= fr.m) break;
        const int c0 = fr.lmcol[j];
        double pl[LMD];
#pragma unroll
        for (int d = 0; d < LMD; ++d) pl[d] = (double)P[(int64_t)(c0 + d) * ld + c] + ((c0 + d == c) ? fr.nz.q_lm : 0.0);
#pragma unroll
        for (int d = 0; d < RD; ++d) {
            const int r = RD * j + d;
            const double* hr = fr.jac + (size_t)r * EKF_JLD;
            double acc = 0.0;
#pragma unroll
            for (int a = 0; a < EKF_CAM; ++a) acc = __builtin_fma(hr[a], pc[a], acc);
#pragma unroll
            for (int e = 0; e < LMD; ++e) acc = __builtin_fma(hr[10 + e], pl[e], acc);
            fr.amat[(int64_t)r * fr.lda + c] = acc;
            if (aw) aw[(int64_t)r * fr.lda + c] = acc;
        }
    }
    if (blockIdx.y == 0) {
        for (int r = fr.k + w; r < rp; r += 4) {
            fr.amat[(int64_t)r * fr.lda + c] = 0.0;
            if (aw) aw[(int64_t)r * fr.lda + c] = 0.0;
        }
    }
}

// --------------------------------------------------------------------------
// (c) S = A H^T + R, one 16 x 16 block (bi >= bj) per workgroup
// --------------------------------------------------------------------------
__device__ __forceinline__ void ekf_wide_tri_decode(int item, int& i, int& j) {
    int r = (int)((sqrt(8.0 * (double)item + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > item) --r;
    while ((r + 1) * (r + 2) / 2 <= item) ++r;
    i = r;
    j = item - r * (r + 1) / 2;
}

template <int MODEL, bool SBLK>
__global__ __launch_bounds__(256) void ekf_wide_s_kernel(EkfFrame fr) {
    constexpr int RD = EkfModel<MODEL>::RD, JC = EkfModel<MODEL>::JC;
    __shared__ double tile[16 * 17];
    int bi, bj;
    ekf_wide_tri_decode(blockIdx.x, bi, bj);
    const int tid = threadIdx.x, i = tid >> 4, c2 = tid & 15, r1 = 16 * bi + i, r2 = 16 * bj + c2;
    double v;
    if (r1 >= fr.k || r2 >= fr.k) {
        v = (r1 == r2) ? 1.0 : 0.0;                    // identity padding
    } else if (r2 > r1) {
        v = 0.0;                                       // strict upper part of a diagonal block
    } else {
        const double* ar = fr.amat + (int64_t)r1 * fr.lda;
        const double* h2 = fr.jac + (size_t)r2 * EKF_JLD;
        const int c20 = fr.lmcol[r2 / RD];
        double acc = (r1 == r2) ? ekf_row_noise(fr, r1) : 0.0;
#pragma unroll
        for (int b = 0; b < JC; ++b) acc = __builtin_fma(ar[(b < EKF_CAM) ? b : c20 + (b - EKF_CAM)], h2[b], acc);
        v = acc;
    }
    if (SBLK) {
        tile[i * 17 + c2] = v;
        __syncthreads();
        if (tid < 64) sv_sblock_emit<false>(fr.sblk + sv_blk_index(bi, bj), tile, bi == bj, tid);
    } else {
        fr.lmat[(int64_t)r1 * fr.ldl + r2] = v;
    }
}

template <typename T>
void ekf_launch_wide_front(const EkfFrame& fr, double* aw, int rp, hipStream_t s) {
    const int nbs = rp / EKF_RB;
    const bool sblk = fr.kpad <= EKF_WIDE_REUSE_ROWS;
    const dim3 ga(fr.ncols / 64, (fr.m + WIDE_G - 1) / WIDE_G);
    const dim3 gm((std::max(fr.m, rp) + 63) / 64);
    if (fr.model == 1) {
        hipLaunchKernelGGL(ekf_wide_measure_kernel<1>, gm, dim3(64), 0, s, fr, rp);
        hipLaunchKernelGGL((ekf_wide_amat_kernel<T, 1>), ga, dim3(256), 0, s, fr, aw, rp);
        if (sblk) hipLaunchKernelGGL((ekf_wide_s_kernel<1, true>), dim3(nbs * (nbs + 1) / 2), dim3(256), 0, s, fr);
        else hipLaunchKernelGGL((ekf_wide_s_kernel<1, false>), dim3(nbs * (nbs + 1) / 2), dim3(256), 0, s, fr);
    } else {
        hipLaunchKernelGGL(ekf_wide_measure_kernel<0>, gm, dim3(64), 0, s, fr, rp);
        hipLaunchKernelGGL((ekf_wide_amat_kernel<T, 0>), ga, dim3(256), 0, s, fr, aw, rp);
        if (sblk) hipLaunchKernelGGL((ekf_wide_s_kernel<0, true>), dim3(nbs * (nbs + 1) / 2), dim3(256), 0, s, fr);
        else hipLaunchKernelGGL((ekf_wide_s_kernel<0, false>), dim3(nbs * (nbs + 1) / 2), dim3(256), 0, s, fr);
    }
}
template void ekf_launch_wide_front<float>(const EkfFrame&, double*, int, hipStream_t);
template void ekf_launch_wide_front<double>(const EkfFrame&, double*, int, hipStream_t);

// --------------------------------------------------------------------------
// (d) blocked Cholesky, block column B
// --------------------------------------------------------------------------
// potrf: one workgroup.  Right-looking by columns in LDS; X = L_BB^-1 is formed by the same eliminations applied to
// the identity (column j of L scales row j of X, then is subtracted from the rows below), in the same two phases.
__global__ __launch_bounds__(256) void ekf_wide_potrf_kernel(EkfFrame fr, double* xinv, int B) {
    __shared__ double s[WB][WB + 1];
    __shared__ double x[WB][WB + 1];
    __shared__ double ldg[WB];
    const int tid = threadIdx.x, r = tid & (WB - 1), q = tid >> 6;
    double* blk = fr.lmat + (int64_t)(WB * B) * fr.ldl + WB * B;
    for (int e = tid; e < WB * WB; e += 256) {
        const int rr = e / WB, cc = e % WB;
        s[rr][cc] = (cc <= rr) ? blk[(int64_t)rr * fr.ldl + cc] : 0.0;
        x[rr][cc] = (rr == cc) ? 1.0 : 0.0;
    }
    __syncthreads();
    int bad = -1;
    for (int j = 0; j < WB; ++j) {
        // phase 1: pivot, column j of L, row j of X
        const double d = s[j][j];
        const double l = sqrt(d);
        if (!(d > 0.0) && bad < 0) bad = j;
        if (q == 0) {
            if (r > j) s[r][j] = s[r][j] / l;
            if (r == j) ldg[j] = l;
        } else if (q == 1 && r <= j) {
            x[j][r] = x[j][r] / l;
        }
        __syncthreads();
        // phase 2: trailing update of S (columns > j) and elimination in X (columns <= j), rows > j
        if (r > j) {
            const double lr = s[r][j];
            for (int c = j + 1 + q; c <= r; c += 4) s[r][c] = __builtin_fma(-lr, s[c][j], s[r][c]);
            for (int c = q; c <= j; c += 4) x[r][c] = __builtin_fma(-lr, x[j][c], x[r][c]);
        }
        __syncthreads();
    }
    for (int e = tid; e < WB * WB; e += 256) {
        const int rr = e / WB, cc = e % WB;
        blk[(int64_t)rr * fr.ldl + cc] = (cc < rr) ? s[rr][cc] : (cc == rr ? ldg[rr] : 0.0);
        xinv[e] = (cc <= rr) ? x[rr][cc] : 0.0;
    }
    if (bad >= 0 && tid == 0) {
        ekf_raise(fr, EKF_ST_NOT_SPD);
        atomicOr(fr.status + 1, 1);
        atomicCAS(fr.status + 2, 0, 100 + (WB * B + bad) / EKF_RB);
    }
}

// panel: workgroups [0, nrem) one row block of L each, then one per 64 columns of A, then the residual.  Wave w owns
// output columns 16 w .. 16 w + 15 of its 64 x 64 block.
__global__ __launch_bounds__(256) void ekf_wide_panel_kernel(EkfFrame fr, double* aw, const double* xinv, int B, int nbw) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int nrem = nbw - B - 1, nchunk = fr.ncols / 64;
    int bx = blockIdx.x;
    if (bx < nrem) {                                   // L_iB = S_iB X^T   (in place)
        double* blk = fr.lmat + (int64_t)(WB * (B + 1 + bx)) * fr.ldl + WB * B;
        wf64x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = wf64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int k0 = 0; k0 < WB; k0 += 4) {
            const double b = xinv[(16 * wave + c) * WB + k0 + g];                          // B[k][j] = X[j][k]
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const double a = blk[(int64_t)(16 * rt + c) * fr.ldl + k0 + g];             // A[i][k] = S[i][k]
                acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[rt], 0, 0, 0);
            }
        }
        __syncthreads();                               // every wave has read the whole block
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) blk[(int64_t)(16 * rt + g + 4 * r) * fr.ldl + 16 * wave + c] = acc[rt][r];
        return;
    }
    bx -= nrem;
    if (bx < nchunk) {                                 // W_B = X A_B   (in place; a wave reads and writes its own columns)
        double* ab = aw + (int64_t)(WB * B) * fr.lda + 64 * bx + 16 * wave;
        wf64x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = wf64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int k0 = 0; k0 < WB; k0 += 4) {
            const double b = ab[(int64_t)(k0 + g) * fr.lda + c];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const double a = xinv[(16 * rt + c) * WB + k0 + g];
                acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[rt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) ab[(int64_t)(16 * rt + g + 4 * r) * fr.lda + c] = acc[rt][r];
        return;
    }
    double yv = 0.0;                                   // y_B = X r_B
    if (tid < WB) {
        for (int k = 0; k <= tid; ++k) yv = __builtin_fma(xinv[tid * WB + k], fr.yvec[WB * B + k], yv);
    }
    __syncthreads();
    if (tid < WB) fr.yvec[WB * B + tid] = yv;
}

// update: workgroups [0, nrem (nrem + 1) / 2) one lower block S_ij each, then nrem x nchunk blocks of A, then the
// residual.  Everything read here (block column B of L, W_B, y_B) is written by no workgroup of this launch.
__global__ __launch_bounds__(256) void ekf_wide_update_kernel(EkfFrame fr, double* aw, int B, int nbw) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int nrem = nbw - B - 1, nchunk = fr.ncols / 64, ns = nrem * (nrem + 1) / 2;
    int bx = blockIdx.x;
    const double* lcol = fr.lmat + WB * B;             // block column B of L
    if (bx < ns + nrem * nchunk) {
        const double* li;                              // L_iB
        const double* bsrc;                            // B operand: B[k][j] = bsrc[k * bk + j * bj]
        int64_t bk, bj, ldo;
        double* out;                                   // 64 x 64 block, row stride ldo
        if (bx < ns) {
            int ii, jj;
            ekf_wide_tri_decode(bx, ii, jj);
            const int i = B + 1 + ii, j = B + 1 + jj;
            li = lcol + (int64_t)(WB * i) * fr.ldl;
            bsrc = lcol + (int64_t)(WB * j) * fr.ldl;  // B[k][j] = L_jB[j][k]
            bk = 1;
            bj = fr.ldl;
            out = fr.lmat + (int64_t)(WB * i) * fr.ldl + WB * j;
            ldo = fr.ldl;
        } else {
            bx -= ns;
            const int i = B + 1 + bx / nchunk, ch = bx % nchunk;
            li = lcol + (int64_t)(WB * i) * fr.ldl;
            bsrc = aw + (int64_t)(WB * B) * fr.lda + 64 * ch;   // B[k][j] = W_B[k][j]
            bk = fr.lda;
            bj = 1;
            out = aw + (int64_t)(WB * i) * fr.lda + 64 * ch;
            ldo = fr.lda;
        }
        wf64x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[rt][r] = out[(int64_t)(16 * rt + g + 4 * r) * ldo + 16 * wave + c];
#pragma unroll 4
        for (int k0 = 0; k0 < WB; k0 += 4) {
            const double b = bsrc[(int64_t)(k0 + g) * bk + (int64_t)(16 * wave + c) * bj];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const double a = li[(int64_t)(16 * rt + c) * fr.ldl + k0 + g];
                acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a, b, acc[rt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(int64_t)(16 * rt + g + 4 * r) * ldo + 16 * wave + c] = acc[rt][r];
        return;
    }
    // residual rows below block B
    const double* yb = fr.yvec + WB * B;
    for (int r = WB * (B + 1) + tid; r < WB * nbw; r += 256) {
        const double* lr = lcol + (int64_t)r * fr.ldl;
        double v = fr.yvec[r];
        for (int k = 0; k < WB; ++k) v = __builtin_fma(-lr[k], yb[k], v);
        fr.yvec[r] = v;
    }
}

// xinv_stride (doubles): block column B leaves its X = L_BB^-1 at xinv + B * xinv_stride (0: every block in the same place)
void ekf_launch_wide_factor(const EkfFrame& fr, double* aw, double* xinv, int rp, hipStream_t s, int64_t xinv_stride) {
    const int nbw = rp / WB, nchunk = fr.ncols / 64;
    for (int B = 0; B < nbw; ++B, xinv += xinv_stride) {
        const int nrem = nbw - B - 1;
        hipLaunchKernelGGL(ekf_wide_potrf_kernel, dim3(1), dim3(256), 0, s, fr, xinv, B);
        hipLaunchKernelGGL(ekf_wide_panel_kernel, dim3(nrem + nchunk + 1), dim3(256), 0, s, fr, aw, xinv, B, nbw);
        if (nrem > 0)
            hipLaunchKernelGGL(ekf_wide_update_kernel, dim3(nrem * (nrem + 1) / 2 + nrem * nchunk + 1), dim3(256), 0, s,
                               fr, aw, B, nbw);
    }
}

// --------------------------------------------------------------------------
// (e) W into the covariance-dtype panel, dx = W^T y, injection.  64 columns x 16 row slices per workgroup.
// --------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(1024) void ekf_wide_finish_kernel(EkfFrame fr, const double* aw) {
    __shared__ double part_s[16][65];
    const int tid = threadIdx.x, cl = tid & 63, sl = tid >> 6, col = 64 * blockIdx.x + cl;
    T* __restrict__ wp = static_cast<T*>(fr.wpanel);
    double part = 0.0;
    for (int r = sl; r < fr.kpad; r += 16) {
        const double w = aw[(int64_t)r * fr.lda + col];
        part = __builtin_fma(w, fr.yvec[r], part);
        wp[(int64_t)r * fr.ldw + col] = (T)w;
        if (fr.wdbg) fr.wdbg[(int64_t)r * fr.ldw + col] = w;
    }
    part_s[sl][cl] = part;
    __syncthreads();
    if (sl != 0) return;
    double dx = 0.0;
    for (int q = 0; q < 16; ++q) dx += part_s[q][cl];
    if (fr.model == 1) {            // EKF_Rotations: every landmark has a quaternion -> ekf_inject_rot_kernel
        if (col < fr.dims) fr.dxvec[col] = dx;
        return;
    }
    double nv = 0.0;
    if (col < 3 || (col >= EKF_CAM && col < fr.dims && !fr.frozen)) {      // (frozen map: the camera only)
        nv = fr.state[col] + dx;                       // extended_kalman_filter.py:134-135
        fr.state[col] = nv;
    }
    if (blockIdx.x != 0) return;
    const double e0 = __shfl(dx, 7), e1 = __shfl(dx, 8), e2 = __shfl(dx, 9);       // (wave 0 holds columns 0 .. 63)
    const double x0 = __shfl(nv, 0), x1 = __shfl(nv, 1), x2 = __shfl(nv, 2);
    if (cl == 0) {
        const double err[3] = {e0, e1, e2}, x[3] = {x0, x1, x2};
        ekf_inject_camera(fr, err, x);
    }
}

template <typename T>
void ekf_launch_wide_finish(const EkfFrame& fr, const double* aw, hipStream_t s) {
    hipLaunchKernelGGL(ekf_wide_finish_kernel<T>, dim3(fr.ncols / 64), dim3(1024), 0, s, fr, aw);
}
template void ekf_launch_wide_finish<float>(const EkfFrame&, const double*, hipStream_t);
template void ekf_launch_wide_finish<double>(const EkfFrame&, const double*, hipStream_t);
