// Landmark removal (include/ekf_slam_hip.h: ekf_remove_markers / ekf_batch_remove_markers): marginalising landmarks out of
// the Gaussian is deleting their rows and columns of P and their entries of the state.  One launch gathers what is kept
// into a second buffer and zero-fills the capacity padding; pure data movement, bit for bit.
//
// Addressing: destination (i', j') = source (map[i'], map[j']); the map [ld] is built on the host from the sorted removal
// list (ekf_remove.h) and says EKF_REMOVE_NONE from the new state dimension on.
// Destination: a workgroup owns EKF_REMOVE_ROWS rows x 4 KiB of columns per pass (grid-stride over these pieces, so that a
// map of n = 1024 already gives every CU several workgroups); a lane owns 16 bytes of each row, so every store is one
// aligned 16-byte store and a wave writes 1 KiB contiguously.
// Source: runs of whole landmarks between removed ones, so a run starts lmd elements (12 bytes: EKF, f32) off the
// destination's alignment, and no 16-byte load that serves one 16-byte store is aligned in general.  The lanes therefore
// load ELEMENTS (4 x 4 bytes, 2 x 8 bytes) at map[j'] and assemble the vector in registers: the four loads of a wave cover
// the same cache lines, every line is fetched from L2 / HBM once, and nothing depends on where the runs break -- a lane
// whose four columns straddle a removed landmark needs no special case.  The padding is branch-free as well: a lane loads
// element (0, 0) in its place (always there) and stores zero.  The alternative, staging source rows through LDS
// with aligned 16-byte loads and shifting there, moves the same bytes from memory, adds an LDS round trip and a barrier per
// pass, and needs the run structure in the kernel; the map lookup costs one load (16 bytes, f64: 8) per lane and pass, shared by the
// EKF_REMOVE_ROWS rows (their 4 x 8 or 2 x 8 element loads are independent and in flight together).
// The state is gathered by the workgroups with blockIdx.x == 0 (for the single filter also into the pinned host mirror), and
// a batch's device landmark count is stored there too.  The single filter's launch also zeroes the rows and columns that
// the second covariance buffer of the pipelined mode loses (ekf_api.hip: ekf_remove_markers), so the call is one copy and
// one launch.
#include "ekf_remove.h"

namespace {

template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; using index = int4; };
template <> struct Vec16<double> { using type = double2; using index = int2; };

template <typename T>
__global__ __launch_bounds__(EKF_REMOVE_THREADS) void ekf_remove_gather_kernel(EkfRemoveArgs a) {
    constexpr int V = 16 / (int)sizeof(T);
    using vec_t = typename Vec16<T>::type;
    using idx_t = typename Vec16<T>::index;
    const int64_t ld = a.ld;
    const int64_t member = blockIdx.y;
    const T* __restrict__ src = static_cast<const T*>(a.cov_src) + member * ld * ld;
    T* __restrict__ dst = static_cast<T*>(a.cov_dst) + member * ld * ld;
    const int32_t* __restrict__ map = a.map + member * ld;
    const int64_t vecs = ld / V, tiles = ld / EKF_REMOVE_ROWS;      // (ld is a multiple of 32)
    const uint32_t chunks = (uint32_t)((vecs + EKF_REMOVE_THREADS - 1) / EKF_REMOVE_THREADS);
    const uint32_t pieces = (uint32_t)tiles * chunks;      // (ld <= 2^20 or so: far below 2^32 pieces)
    for (uint32_t w = blockIdx.x; w < pieces; w += gridDim.x) {
        const int64_t r0 = (int64_t)(w / chunks) * EKF_REMOVE_ROWS, v = (int64_t)(w % chunks) * EKF_REMOVE_THREADS + threadIdx.x;
        // first element of every source row (wave-uniform); a destination row of the padding reads row 0 and keeps nothing.
        // Every load below is unconditional, at a clamped address, and the select follows it: no branch sits between the
        // EKF_REMOVE_ROWS x V loads of a pass, so they are all in flight before the first store waits.
        int64_t srow[EKF_REMOVE_ROWS];
        bool rkeep[EKF_REMOVE_ROWS];
#pragma unroll
        for (int r = 0; r < EKF_REMOVE_ROWS; ++r) {
            const int32_t si = map[r0 + r];
            rkeep[r] = si >= 0;
            srow[r] = (int64_t)(si < 0 ? 0 : si) * ld;
        }
        if (v < vecs) {
            const idx_t mv = *reinterpret_cast<const idx_t*>(map + v * V);
            int32_t sj[V];
            sj[0] = mv.x;
            sj[1] = mv.y;
            if constexpr (V == 4) {
                sj[2] = mv.z;
                sj[3] = mv.w;
            }
            bool ckeep[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                ckeep[k] = sj[k] >= 0;
                sj[k] = sj[k] < 0 ? 0 : sj[k];
            }
            T e[EKF_REMOVE_ROWS][V];
#pragma unroll
            for (int r = 0; r < EKF_REMOVE_ROWS; ++r)
#pragma unroll
                for (int k = 0; k < V; ++k) e[r][k] = src[srow[r] + sj[k]];
#pragma unroll
            for (int r = 0; r < EKF_REMOVE_ROWS; ++r) {
                vec_t out;
                out.x = rkeep[r] && ckeep[0] ? e[r][0] : T(0);
                out.y = rkeep[r] && ckeep[1] ? e[r][1] : T(0);
                if constexpr (V == 4) {
                    out.z = rkeep[r] && ckeep[2] ? e[r][2] : T(0);
                    out.w = rkeep[r] && ckeep[3] ? e[r][3] : T(0);
                }
                *reinterpret_cast<vec_t*>(dst + (r0 + r) * ld + v * V) = out;
            }
        }
    }
    if (a.cov2) {
        // the fringe of the second covariance buffer: whole rows [n_new, fringe_hi), and those columns of the rows above
        T* __restrict__ c2 = static_cast<T*>(a.cov2);
        const int64_t n_new = a.n_new, hi = a.fringe_hi;
        for (int64_t i = blockIdx.x; i < hi; i += gridDim.x) {
            const int64_t j0 = i < n_new ? n_new : 0, j1 = i < n_new ? hi : ld;
            for (int64_t j = j0 + threadIdx.x; j < j1; j += EKF_REMOVE_THREADS) c2[i * ld + j] = T(0);
        }
    }
    if (blockIdx.x == 0) {
        const double* __restrict__ ssrc = a.state_src + member * ld;
        double* __restrict__ sdst = a.state_dst + member * ld;
        for (int64_t j = threadIdx.x; j < ld; j += EKF_REMOVE_THREADS) {
            const int32_t sj = map[j];
            const double x = sj >= 0 ? ssrc[sj] : 0.0;
            sdst[j] = x;
            if (a.state_host && j < a.n_new) a.state_host[j] = x;
        }
        if (threadIdx.x == 0 && a.nlm) a.nlm[member] = a.nlm_new[member];
    }
}

}  // namespace

template <typename T>
void ekf_launch_remove(const EkfRemoveArgs& a, int members, hipStream_t s) {
    const int64_t vecs = a.ld / (16 / (int64_t)sizeof(T));
    const int64_t pieces = a.ld / EKF_REMOVE_ROWS * ((vecs + EKF_REMOVE_THREADS - 1) / EKF_REMOVE_THREADS);
    const unsigned gx = (unsigned)std::min<int64_t>(pieces, 8192);
    for (int m0 = 0; m0 < members; m0 += 65535) {      // (blockIdx.y carries the member)
        const int count = std::min(65535, members - m0);
        EkfRemoveArgs c = a;
        c.cov_src = static_cast<const T*>(a.cov_src) + (int64_t)m0 * a.ld * a.ld;
        c.cov_dst = static_cast<T*>(a.cov_dst) + (int64_t)m0 * a.ld * a.ld;
        c.state_src = a.state_src + (int64_t)m0 * a.ld;
        c.state_dst = a.state_dst + (int64_t)m0 * a.ld;
        c.map = a.map + (int64_t)m0 * a.ld;
        if (a.nlm) {
            c.nlm = a.nlm + m0;
            c.nlm_new = a.nlm_new + m0;
        }
        hipLaunchKernelGGL(ekf_remove_gather_kernel<T>, dim3(gx, (unsigned)count), dim3(EKF_REMOVE_THREADS), 0, s, c);
    }
}

template void ekf_launch_remove<float>(const EkfRemoveArgs&, int, hipStream_t);
template void ekf_launch_remove<double>(const EkfRemoveArgs&, int, hipStream_t);
