// Batch smoothing, the covariances (include/ekf_slam_hip.h, "Batch smoothing, covariances"): the resident
// pass of ekf_smooth_resident.h, one workgroup per member, with the covariance rule inside every backward step.  The state
// step has just factored P_p = L L^T into the packed triangle in LDS; the step hook forms, with N = N_r and nb = the number
// of 16 x 16 block rows,
//   X_B = L_BB^-1,  A = F~ P_r,  W = L^-1 A,  Z = L^-T W (= G_r^T),  T = P^s_{r+1}[0:N, 0:N] Z,  D = -W^T W + Z^T T,
//   P^s_r = P_r + D on the lower triangle, mirrored
// and the state step goes on as if nothing had happened.  L stays in LDS; W, Z, T and P^s live in the member's region of the
// workspace (leading dimension ld, fixed over the pass) and come back through L2.
//   inverses   thread (B, j), 16 nb of them: column j of X_B by a forward substitution in registers; X in LDS
//   rows       with a motion, thread j: ten rows of A, F P_r[0:10, j] (ekf_motion_column with the step's F); in LDS
//   strips     a wave owns whole strips of 16 columns (strip s: wave s mod 8) and keeps the strip in registers, block row
//              after block row -- a D tile of the f64 MFMA (row = (lane >> 4) + 4 reg, col = lane & 15) IS a B operand of
//              four k-steps (k = lane >> 4 of step reg), so nothing is staged and no wave waits for another:
//                W_B = X_B (A_B - sum_{i<B} L_Bi W_i)        block rows ascending
//                Z_B = X_B^T (W_B - sum_{i>B} L_iB^T Z_i)    block rows descending
//                T_B = sum_k P^s_{r+1}[B, k] Z_k             (P^s is bitwise symmetric: read as rows k)
//              W, Z and T are stored as they appear.  With ten strips on eight waves, two waves run two strips: the tail
//              of the round costs one strip's time (DESIGN 4.7.8.1 has the figure).
//   (barrier)  the D tiles read other waves' strips
//   products   lower tile t of the nb (nb + 1) / 2: wave t mod 8; ONE accumulator chain, -W^T W over k ascending and then
//              Z^T T over k ascending; the tile adds P_r from the packed record and writes P^s_r[i][j] and [j][i], the
//              camera block to the record's frame rows, and first_cov at record 0
// Every sum is one chain in a fixed order in a fixed wave: a member's bits do not depend on the batch around it.  Rows and
// columns N .. 16 nb - 1 of A, W and Z are exactly zero, so the finite values P^s holds there take no part; P^s is zeroed
// by the kernel before its first use, and W, Z, T are written before they are read in every step.
#include "ekf_kernels.h"
#include "ekf_smooth_device.h"
#include "ekf_smooth_resident.h"

typedef double bf64x4 __attribute__((ext_vector_type(4)));
#define BT EKF_SMOOTH_COV_TILE
#define BNB (EKF_SMOOTH_RESIDENT_DIMS / BT)      // at most 10 block rows
#define BWAVES (EKF_SMOOTH_THREADS / 64)

namespace {

__host__ __device__ inline int cov_blocks(int n) { return (n + BT - 1) / BT; }

// L[i][j], i > j, j < N, from the packed triangle; a row of the padding is zero
__device__ __forceinline__ double cov_l(const double* tri, int N, int i, int j) {
    return i < N ? tri[j * (2 * N - j + 1) / 2 + (i - j)] : 0.0;
}

struct EkfBatchCovStep {
    double *W, *Z, *T, *Ps;         // the member's region
    int ld;
    double *xinv, *arow;            // LDS: [BNB][16][16], [EKF_CAM][EKF_SMOOTH_RESIDENT_DIMS]
    double *cam_cov, *filt_cam_cov; // the call's
    double* first_cov;              // the member's slab, or NULL
    int first_ld;

    // the record's rows of the outputs and P^s for one entry i >= j of the lower triangle
    __device__ __forceinline__ void put(const EkfSmoothRec& rec, bool first, int i, int j, double p, double v) const {
        Ps[(int64_t)i * ld + j] = v;
        Ps[(int64_t)j * ld + i] = v;
        if (first && first_cov) {
            first_cov[(int64_t)i * first_ld + j] = v;
            first_cov[(int64_t)j * first_ld + i] = v;
        }
        if (i < EKF_CAM) {
            for (int f = rec.frame0; f < rec.frame1; ++f) {
                double* cc = cam_cov + (int64_t)f * EKF_CAM * EKF_CAM;
                cc[i * EKF_CAM + j] = v;
                cc[j * EKF_CAM + i] = v;
                if (filt_cam_cov) {
                    double* fc = filt_cam_cov + (int64_t)f * EKF_CAM * EKF_CAM;
                    fc[i * EKF_CAM + j] = p;
                    fc[j * EKF_CAM + i] = p;
                }
            }
        }
    }

    // A[i][j] = (F~ P_r)[i][j], zero in the padding
    __device__ __forceinline__ double a_entry(const double* __restrict__ pg, int N, int moved, int i, int j) const {
        if (i >= N || j >= N) return 0.0;
        if (moved && i < EKF_CAM) return arow[i * EKF_SMOOTH_RESIDENT_DIMS + j];
        return pg[ekf_smooth_sym(N, i, j)];
    }

    __device__ __forceinline__ void strip(int s, int N, int nb, int moved, int ld, const double* __restrict__ pg,
                                          const double* tri) const {
        // (the lane number is opaque per strip: otherwise the factor's addresses and entries, which do not depend on the
        // strip, are hoisted out of the loop over strips and spill)
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane) : : "memory");
        const int c = lane & 15, g = lane >> 4;
        const int col = BT * s + c;
        bf64x4 t[BNB];
        // W = L^-1 A
#pragma unroll
        for (int B = 0; B < BNB; ++B)
            if (B < nb) {
                asm volatile("" : "+v"(lane));      // (and per block row: addresses are formed where they are used)
                const int c = lane & 15, g = lane >> 4;
                bf64x4 acc;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = a_entry(pg, N, moved, BT * B + g + 4 * r, col);
#pragma unroll
                for (int i = 0; i < BNB; ++i)
                    if (i < B) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double a = cov_l(tri, N, BT * B + c, BT * i + 4 * q + g);
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a, t[i][q], acc, 0, 0, 0);
                        }
                        if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);      // (at most two tiles of L in flight)
                    }
                bf64x4 w = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    w = __builtin_amdgcn_mfma_f64_16x16x4f64(xinv[B * BT * BT + c * BT + 4 * q + g], acc[q], w, 0, 0, 0);
                t[B] = w;
#pragma unroll
                for (int r = 0; r < 4; ++r) W[(int64_t)(BT * B + g + 4 * r) * ld + col] = w[r];
            }
        // Z = L^-T W
#pragma unroll
        for (int B = BNB - 1; B >= 0; --B)
            if (B < nb) {
                asm volatile("" : "+v"(lane));
                const int c = lane & 15, g = lane >> 4;
                bf64x4 acc = t[B];
#pragma unroll
                for (int i = BNB - 1; i >= 0; --i)
                    if (i > B && i < nb) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double a = cov_l(tri, N, BT * i + 4 * q + g, BT * B + c);
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a, t[i][q], acc, 0, 0, 0);
                        }
                        if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);      // (at most two tiles of L in flight)
                    }
                bf64x4 z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    z = __builtin_amdgcn_mfma_f64_16x16x4f64(xinv[B * BT * BT + (4 * q + g) * BT + c], acc[q], z, 0, 0, 0);
                t[B] = z;
#pragma unroll
                for (int r = 0; r < 4; ++r) Z[(int64_t)(BT * B + g + 4 * r) * ld + col] = z[r];
            }
        // T = P^s_{r+1}[0:16 nb, 0:16 nb] Z
        for (int Bi = 0; Bi < nb; ++Bi) {
            bf64x4 acc = {0.0, 0.0, 0.0, 0.0};
            const double* prow = Ps + (int64_t)g * ld + BT * Bi + c;      // (one address per lane, uniform steps from it)
#pragma unroll
            for (int k = 0; k < BNB; ++k)
                if (k < nb) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(*prow, t[k][q], acc, 0, 0, 0);
                        prow += 4 * ld;
                    }
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) T[(int64_t)(BT * Bi + g + 4 * r) * ld + col] = acc[r];
        }
    }

    __device__ __forceinline__ void operator()(int r, const EkfSmoothRec& rec, const EkfSmoothRec& nx,
                                               const double* __restrict__ pg, const double* tri, const double* ld_s,
                                               const EkfMotionF& F) const {
        // (the thread number and the leading dimension are opaque per step: otherwise whatever a lane forms from them, which
        // does not depend on the step, is hoisted out of the loop over the records and lives in registers through the pass)
        int tid = threadIdx.x, ld = this->ld;
        asm volatile("" : "+v"(tid), "+s"(ld));
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, c = lane & 15, g = lane >> 4;
        const int N = rec.dims, nb = cov_blocks(N);
        if (tid < BT * nb) {      // column j of X_B: L_BB x = e_j, the padding of the last block is the identity
            const int B = tid >> 4, j = tid & 15, b0 = BT * B;
            double* x = xinv + B * BT * BT + j;      // x[BT i]: the thread reads back what it has written itself
            for (int i = 0; i < BT; ++i) {
                double s = 0.0;
                for (int k = j; k < i; ++k) s = __builtin_fma(cov_l(tri, N, b0 + i, b0 + k), x[BT * k], s);
                const double d = b0 + i < N ? ld_s[b0 + i] : 1.0;
                x[BT * i] = i < j ? 0.0 : (i == j ? 1.0 : -s) / d;
            }
        }
        if (nx.moved && tid >= EKF_SMOOTH_THREADS / 2 && tid - EKF_SMOOTH_THREADS / 2 < N) {
            const int j = tid - EKF_SMOOTH_THREADS / 2;
            double in[EKF_CAM], out[EKF_CAM];
#pragma unroll
            for (int k = 0; k < EKF_CAM; ++k) in[k] = pg[ekf_smooth_sym(N, k, j)];
            ekf_motion_column(F, in, out);
#pragma unroll
            for (int k = 0; k < EKF_CAM; ++k) arow[k * EKF_SMOOTH_RESIDENT_DIMS + j] = out[k];
        }
        __syncthreads();
        for (int s = wave; s < nb; s += BWAVES) strip(s, N, nb, nx.moved, ld, pg, tri);
        __syncthreads();      // (W, Z and T of every strip are visible to the workgroup)
        const int tiles = nb * (nb + 1) / 2;
        int ti = 0, tj = 0;      // tile `wave` of the lower triangle, row by row
        for (int t = 0; t < wave; ++t)
            if (++tj > ti) ++ti, tj = 0;
        for (int t = wave; t < tiles; t += BWAVES) {
            const double* wi = W + BT * ti + c;
            const double* wj = W + BT * tj + c;
            const double* zi = Z + BT * ti + c;
            const double* tjp = T + BT * tj + c;
            bf64x4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < BT * nb; k0 += BT) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t k = (int64_t)(k0 + 4 * q + g) * ld;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-wi[k], wj[k], acc, 0, 0, 0);
                }
            }
            for (int k0 = 0; k0 < BT * nb; k0 += BT) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t k = (int64_t)(k0 + 4 * q + g) * ld;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(zi[k], tjp[k], acc, 0, 0, 0);
                }
            }
            const int j = BT * tj + c;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = BT * ti + g + 4 * rr;
                if (i < N && j <= i) {
                    const double p = pg[ekf_smooth_tri(N, i, j)];
                    put(rec, r == 0, i, j, p, p + acc[rr]);
                }
            }
            for (int u = 0; u < BWAVES; ++u)
                if (++tj > ti) ++ti, tj = 0;
        }
        __syncthreads();      // (L has been read: the state step may load P_r over it; P^s_r is visible)
    }
};

// One workgroup per member.  P^s <- 0, the last record (P^s_{R-1} = P_{R-1}), the pass with the step above, then the NaN
// rows: a bad pivot -- every row of the member in all three outputs and [0:N_0, 0:N_0] of its first_cov slab; a member that
// failed in the replay -- from its failing frame on; the covariance rows before the first record.
__global__ __launch_bounds__(EKF_SMOOTH_THREADS) void ekf_batch_smooth_cov_kernel(EkfBatchSmoothCov a) {
    extern __shared__ double tri[];
    const EkfBatchSmoothMember m = a.members[blockIdx.x];
    const EkfBatchSmoothCovMember cm = a.cov_members[blockIdx.x];
    const int tid = threadIdx.x;
    const double nan = __builtin_nan("");
    const double* __restrict__ hist = a.history;
    double* first = a.first_cov ? a.first_cov + (int64_t)blockIdx.x * a.first_ld * a.first_ld : nullptr;
    bool ok = true;
    int n0 = 0;
    if (m.records > 0) {
        const int64_t ld2 = (int64_t)cm.ld * cm.ld;
        EkfBatchCovStep step;
        step.W = a.regions + cm.region;
        step.Z = step.W + ld2;
        step.T = step.Z + ld2;
        step.Ps = step.T + ld2;
        step.ld = cm.ld;
        step.xinv = tri + ekf_smooth_tri_count(a.nmax);
        step.arow = step.xinv + cov_blocks(a.nmax) * BT * BT;
        step.cam_cov = a.cam_cov;
        step.filt_cam_cov = a.filt_cam_cov;
        step.first_cov = first;
        step.first_ld = a.first_ld;
        const EkfSmoothRec* table = a.tables + m.table;
        n0 = table[0].dims;
        for (int64_t e = tid; e < ld2; e += EKF_SMOOTH_THREADS) step.Ps[e] = 0.0;
        __syncthreads();
        const EkfSmoothRec last = table[m.records - 1];
        const double* __restrict__ pg = hist + last.off + last.dims;
        for (int e = tid; e < last.dims * last.dims; e += EKF_SMOOTH_THREADS) {
            const int i = e / last.dims, j = e - i * last.dims;
            if (j <= i) {
                const double p = pg[ekf_smooth_tri(last.dims, i, j)];
                step.put(last, m.records == 1, i, j, p, p);
            }
        }
        ok = ekf_smooth_resident_pass(hist, hist + m.head, table, m.records, m.frame0, m.lead1, a.smoothed, tri, step);
    } else {
        for (int e = tid; e < 7 * (m.lead1 - m.frame0); e += EKF_SMOOTH_THREADS)
            a.smoothed[(int64_t)7 * m.frame0 + e] = hist[m.head + e % 7];
    }
    __syncthreads();      // (the NaN rows of a bad member overwrite rows other threads of the pass have written)
    const int CC = EKF_CAM * EKF_CAM;
    const int s0 = ok ? m.nan0 : m.frame0, lead = ok ? m.lead1 : m.frame1;
    for (int e = tid; e < 7 * (m.frame1 - s0); e += EKF_SMOOTH_THREADS) a.smoothed[(int64_t)7 * s0 + e] = nan;
    for (int e = tid; e < CC * (lead - m.frame0); e += EKF_SMOOTH_THREADS) {
        a.cam_cov[(int64_t)CC * m.frame0 + e] = nan;
        if (a.filt_cam_cov) a.filt_cam_cov[(int64_t)CC * m.frame0 + e] = nan;
    }
    for (int e = tid; e < CC * (m.frame1 - m.nan0); e += EKF_SMOOTH_THREADS) {
        a.cam_cov[(int64_t)CC * m.nan0 + e] = nan;
        if (a.filt_cam_cov) a.filt_cam_cov[(int64_t)CC * m.nan0 + e] = nan;
    }
    if (!ok && first)
        for (int e = tid; e < n0 * n0; e += EKF_SMOOTH_THREADS) first[(int64_t)(e / n0) * a.first_ld + e % n0] = nan;
    if (tid == 0) a.status[blockIdx.x] = ok ? 0 : EKF_BATCH_ST_NUMERIC;
}

}  // namespace

size_t ekf_batch_smooth_cov_lds(int32_t nmax) {
    return (size_t)(ekf_smooth_tri_count(nmax) + cov_blocks(nmax) * BT * BT + EKF_CAM * EKF_SMOOTH_RESIDENT_DIMS) * 8;
}

hipError_t ekf_launch_batch_smooth_cov(const EkfBatchSmoothCov& a, int32_t members, hipStream_t s) {
    const size_t lds = ekf_batch_smooth_cov_lds(a.nmax);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ekf_batch_smooth_cov_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ekf_batch_smooth_cov_kernel, dim3(members), dim3(EKF_SMOOTH_THREADS), lds, s, a);
    return hipSuccess;
}
