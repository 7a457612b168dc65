// Offline smoothing, the covariances (include/ekf_slam_hip.h: the covariance rule).  A backward step
// r+1 -> r is the blocked state step of ekf_smooth.hip with N right-hand sides riding along the factorisation, and then
// the N^3 terms of the rule in its subtraction-of-products form, with L L^T = P_p:
//   A = F~ P_r,  W = L^-1 A,  Z = L^-T W (= G_r^T),  T = P^s_{r+1}[0:N, 0:N] Z,  P^s_r = P_r - W^T W + Z^T T.
//   rhs       : A expanded from the packed record, F~ on rows 0..9 (the stage functions of ekf_motion_device.h)
//   (factor)  : ekf_launch_wide_factor with ncols = npad, aw = A, one X = L_BB^-1 kept per block column
//   backsolve : Z, one workgroup per 64 columns walks the block rows from the last (v_mfma_f64_16x16x4_f64)
//   product   : C = C0 + sum of (+-) X^T Y over 64 x 64 tiles, operands staged through LDS; serves T and D = -W^T W + Z^T T
//   finish    : P^s_r = P_r + D on the lower triangle, mirrored, over P^s_{r+1}; the record's rows of the outputs
// Everything is a stream-ordered launch; no workgroup waits for another one.  Every sum is one chain in a fixed order (the
// k order of the MFMA loops), so two runs over one history give the same bits.  The padding (rows and columns N .. npad-1)
// of A, W and Z is exactly zero, so whatever finite values P^s_{r+1} holds there take no part.
#include "ekf_kernels.h"
#include "ekf_smooth_device.h"

typedef double cf64x4 __attribute__((ext_vector_type(4)));
#define CB EKF_WIDE_BLOCK
#define CLD 80      // LDS row stride in doubles: rows k and k + 1 of a tile sit 16 doubles (32 banks) apart modulo the
                    // 64-bank row, so the two k rows a 32-lane group of ds_read_b64 touches never share a bank

namespace {

__host__ __device__ inline int cov_npad(int n) { return (n + CB - 1) / CB * CB; }

// ---- rhs ----------------------------------------------------------------------------------------------------------------
// Workgroup i writes row i of A = F~ P_r (zeros beyond N).  With a motion rows 0..9 are F P_r[0:10, :]: workgroup 0 forms F
// (the same function on the same input as the state step) and applies it column by column; workgroups 1..9 have nothing to do.
__global__ __launch_bounds__(256) void ekf_smooth_cov_rhs_kernel(EkfSmoothCov a, int npad) {
    __shared__ EkfMotionF F;
    const int N = a.b.rec.dims, i = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ xg = a.b.history + a.b.rec.off;
    const double* __restrict__ pg = xg + N;
    if (a.b.next.moved && i < EKF_CAM) {
        if (i != 0) return;
        if (tid == 0) ekf_motion_form(xg, a.b.next.u, F);
        __syncthreads();
        for (int j = tid; j < npad; j += 256) {
            double in[EKF_CAM], out[EKF_CAM];
            if (j < N) {
#pragma unroll
                for (int k = 0; k < EKF_CAM; ++k) in[k] = pg[ekf_smooth_sym(N, k, j)];
                ekf_motion_column(F, in, out);
            } else {
#pragma unroll
                for (int k = 0; k < EKF_CAM; ++k) out[k] = 0.0;
            }
#pragma unroll
            for (int k = 0; k < EKF_CAM; ++k) a.A[(int64_t)k * npad + j] = out[k];
        }
        return;
    }
    for (int j = tid; j < npad; j += 256) a.A[(int64_t)i * npad + j] = (i < N && j < N) ? pg[ekf_smooth_sym(N, i, j)] : 0.0;
}

// ---- backsolve: Z = L^-T W ----------------------------------------------------------------------------------------------
// Workgroup x owns columns 64 x .. 64 x + 63 of Z, wave w 16 of them.  Block row B from the last:
//   Z_B = X_B^T (W_B - sum_{i > B} L_iB^T Z_i),  X_B = L_BB^-1 (kept by the factorisation).
// The Z_i it reads are its own earlier stores (a barrier behind every block row); the difference goes through LDS to
// become the B operand of the product with X_B^T.  MFMA operands: A[m][k] on lane (m = c, k = g), B[k][n] on lane
// (k = g, n = c), D[m][n] in register r of lane (n = c, m = g + 4 r) -- the layout of ekf_wide.hip.
__global__ __launch_bounds__(256) void ekf_smooth_cov_backsolve_kernel(const double* __restrict__ L, const double* __restrict__ xinv,
                                                                       const double* __restrict__ W, double* Z, int npad) {
    __shared__ double t[CB][CLD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int nb = npad / CB, col = CB * blockIdx.x + 16 * wave + c;
    for (int B = nb - 1; B >= 0; --B) {
        cf64x4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[rt][r] = W[(int64_t)(CB * B + 16 * rt + g + 4 * r) * npad + col];
        for (int i = B + 1; i < nb; ++i) {
            const double* li = L + (int64_t)(CB * i) * npad + CB * B;      // L_iB: A[m][k] = L_iB[k][m]
            const double* zi = Z + (int64_t)(CB * i) * npad + col;
#pragma unroll 4
            for (int k0 = 0; k0 < CB; k0 += 4) {
                const double b = zi[(int64_t)(k0 + g) * npad];
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) {
                    const double av = li[(int64_t)(k0 + g) * npad + 16 * rt + c];
                    acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(-av, b, acc[rt], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) t[16 * rt + g + 4 * r][16 * wave + c] = acc[rt][r];
        __syncthreads();      // (a wave reads back its own 16 columns only; the barrier orders the LDS and the Z stores below)
        const double* xb = xinv + (int64_t)B * CB * CB;                    // A[m][k] = X_B[k][m] (zero for k < m)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = cf64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int k0 = 0; k0 < CB; k0 += 4) {
            const double b = t[k0 + g][16 * wave + c];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const double av = xb[(k0 + g) * CB + 16 * rt + c];
                acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b, acc[rt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) Z[(int64_t)(CB * B + 16 * rt + g + 4 * r) * npad + col] = acc[rt][r];
        __syncthreads();      // Z_B is visible to the workgroup, and t is free again
    }
}

// ---- product: C = C0 + sum_p s_p X_p^T Y_p ------------------------------------------------------------------------------
// One 64 x 64 tile of C per workgroup (all nt x nt tiles, or the nt (nt + 1) / 2 lower ones), wave w its columns 16 w ..
// 16 w + 15.  Up to two products are summed into one accumulator chain: p = 0 over k = 0 .. K-1, then p = 1.  Per 16 rows
// of k the two operand strips [16][64] go global -> registers -> LDS (the next strip is in flight while this one is
// multiplied); the MFMA operands come from LDS.
#define CKC 16
struct EkfCovProduct {
    const double *X[2], *Y[2];
    int64_t ldx[2], ldy[2];
    int32_t neg[2];             // s_p = -1
    int32_t terms;              // 1 or 2
    const double* C0;           // or NULL: zero
    double* C;
    int64_t ldc;                // of C0 and C
    int32_t K, nt, lower;
};

__device__ __forceinline__ void cov_tri_decode(int item, int& i, int& j) {
    int r = (int)((sqrt(8.0 * (double)item + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > item) --r;
    while ((r + 1) * (r + 2) / 2 <= item) ++r;
    i = r;
    j = item - r * (r + 1) / 2;
}

__global__ __launch_bounds__(256) void ekf_smooth_cov_product_kernel(EkfCovProduct p) {
    __shared__ double xs[CKC][CLD], ys[CKC][CLD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    int ti, tj;
    if (p.lower) {
        cov_tri_decode(blockIdx.x, ti, tj);
    } else {
        ti = blockIdx.x / p.nt;
        tj = blockIdx.x % p.nt;
    }
    cf64x4 acc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[rt][r] = p.C0 ? p.C0[(int64_t)(CB * ti + 16 * rt + g + 4 * r) * p.ldc + CB * tj + 16 * wave + c] : 0.0;
    const int lr = tid >> 6, lc = tid & 63;      // this thread's element of a strip: rows lr, lr + 4, lr + 8, lr + 12
    for (int term = 0; term < p.terms; ++term) {
        const double* __restrict__ X = p.X[term] + CB * ti;
        const double* __restrict__ Y = p.Y[term] + CB * tj;
        const int64_t ldx = p.ldx[term], ldy = p.ldy[term];
        const bool neg = p.neg[term] != 0;
        double px[4], py[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            px[q] = X[(int64_t)(lr + 4 * q) * ldx + lc];
            py[q] = Y[(int64_t)(lr + 4 * q) * ldy + lc];
        }
        for (int k0 = 0; k0 < p.K; k0 += CKC) {
            __syncthreads();      // the strip before has been read
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                xs[lr + 4 * q][lc] = neg ? -px[q] : px[q];
                ys[lr + 4 * q][lc] = py[q];
            }
            __syncthreads();
            if (k0 + CKC < p.K) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    px[q] = X[(int64_t)(k0 + CKC + lr + 4 * q) * ldx + lc];
                    py[q] = Y[(int64_t)(k0 + CKC + lr + 4 * q) * ldy + lc];
                }
            }
#pragma unroll
            for (int kk = 0; kk < CKC; kk += 4) {
                const double b = ys[kk + g][16 * wave + c];
#pragma unroll
                for (int rt = 0; rt < 4; ++rt)
                    acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[kk + g][16 * rt + c], b, acc[rt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) p.C[(int64_t)(CB * ti + 16 * rt + g + 4 * r) * p.ldc + CB * tj + 16 * wave + c] = acc[rt][r];
}

// ---- finish -------------------------------------------------------------------------------------------------------------
// Workgroup i: row i of the lower triangle, v = P_r[i][j] + D[i][j] (D == NULL: v = P_r[i][j], the last record), written to
// Ps[i][j] and Ps[j][i] -- nobody else writes those two -- and the same way into the outputs: the camera block for every
// frame of the record, first_cov when this is record 0.
__global__ __launch_bounds__(256) void ekf_smooth_cov_finish_kernel(EkfSmoothCov a, const double* __restrict__ D, int npad) {
    const int N = a.b.rec.dims, i = blockIdx.x;
    if (a.b.status[0] != 0) return;
    const double* __restrict__ pg = a.b.history + a.b.rec.off + N;
    for (int j = threadIdx.x; j <= i; j += 256) {
        const double p = pg[ekf_smooth_tri(N, i, j)];
        const double v = D ? p + D[(int64_t)i * npad + j] : p;
        a.Ps[(int64_t)i * a.ldp + j] = v;
        a.Ps[(int64_t)j * a.ldp + i] = v;
        if (a.first && a.first_cov) {
            a.first_cov[(int64_t)i * N + j] = v;
            a.first_cov[(int64_t)j * N + i] = v;
        }
        if (i < EKF_CAM) {
            for (int f = a.b.rec.frame0; f < a.b.rec.frame1; ++f) {
                double* cc = a.cam_cov + (int64_t)f * EKF_CAM * EKF_CAM;
                cc[i * EKF_CAM + j] = v;
                cc[j * EKF_CAM + i] = v;
                if (a.filt_cam_cov) {
                    double* fc = a.filt_cam_cov + (int64_t)f * EKF_CAM * EKF_CAM;
                    fc[i * EKF_CAM + j] = p;
                    fc[j * EKF_CAM + i] = p;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void ekf_smooth_cov_nan_kernel(double* cam_cov, double* filt_cam_cov, int f0, int f1) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, n = (int64_t)(f1 - f0) * EKF_CAM * EKF_CAM;
    if (e >= n) return;
    const double nan = __builtin_nan("");
    cam_cov[(int64_t)f0 * EKF_CAM * EKF_CAM + e] = nan;
    if (filt_cam_cov) filt_cam_cov[(int64_t)f0 * EKF_CAM * EKF_CAM + e] = nan;
}

}  // namespace

void ekf_launch_smooth_cov_nan(double* cam_cov, double* filt_cam_cov, int32_t f0, int32_t f1, hipStream_t s) {
    if (f1 <= f0) return;
    const int64_t n = (int64_t)(f1 - f0) * EKF_CAM * EKF_CAM;
    hipLaunchKernelGGL(ekf_smooth_cov_nan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cam_cov, filt_cam_cov, f0, f1);
}

void ekf_launch_smooth_cov_last(const EkfSmoothCov& a, hipStream_t s) {
    hipLaunchKernelGGL(ekf_smooth_cov_finish_kernel, dim3(a.b.rec.dims), dim3(256), 0, s, a, (const double*)nullptr, 0);
}

void ekf_launch_smooth_cov_step(const EkfSmoothCov& a, hipStream_t s) {
    const int N = a.b.rec.dims, npad = cov_npad(N), nt = npad / CB;
    ekf_launch_smooth_blocked_prepare(a.b, s);
    hipLaunchKernelGGL(ekf_smooth_cov_rhs_kernel, dim3(npad), dim3(256), 0, s, a, npad);
    // the factorisation of the state step with the npad columns of A riding along: L over M, y = L^-1 delta, W = L^-1 A over A
    // (L and y do not depend on the columns that ride along: the state half keeps its bits)
    EkfFrame fr{};
    fr.lmat = a.b.M;
    fr.ldl = npad;
    fr.yvec = a.b.yv;
    fr.ncols = npad;
    fr.lda = npad;
    fr.status = a.b.status;
    ekf_launch_wide_factor(fr, a.A, a.b.xinv, npad, s, (int64_t)CB * CB);
    ekf_launch_smooth_blocked_solve(a.b, s);      // the state half, unchanged; M is free behind the backsolve below
    hipLaunchKernelGGL(ekf_smooth_cov_backsolve_kernel, dim3(nt), dim3(256), 0, s, a.b.M, a.b.xinv, a.A, a.Z, npad);
    EkfCovProduct t{};      // T = P^s_{r+1}[0:npad, 0:npad] Z (P^s is bitwise symmetric: P^s Z = P^s^T Z)
    t.X[0] = a.Ps;
    t.ldx[0] = a.ldp;
    t.Y[0] = a.Z;
    t.ldy[0] = npad;
    t.terms = 1;
    t.C = a.T;
    t.ldc = npad;
    t.K = npad;
    t.nt = nt;
    hipLaunchKernelGGL(ekf_smooth_cov_product_kernel, dim3(nt * nt), dim3(256), 0, s, t);
    EkfCovProduct d{};      // D = -W^T W + Z^T T on the lower tiles, over M
    d.X[0] = a.A;
    d.Y[0] = a.A;
    d.neg[0] = 1;
    d.X[1] = a.Z;
    d.Y[1] = a.T;
    d.ldx[0] = d.ldy[0] = d.ldx[1] = d.ldy[1] = npad;
    d.terms = 2;
    d.C = a.b.M;
    d.ldc = npad;
    d.K = npad;
    d.nt = nt;
    d.lower = 1;
    hipLaunchKernelGGL(ekf_smooth_cov_product_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, d);
    hipLaunchKernelGGL(ekf_smooth_cov_finish_kernel, dim3(N), dim3(256), 0, s, a, (const double*)a.b.M, npad);
}
