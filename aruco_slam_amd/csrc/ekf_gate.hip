// Per-detection chi-square gate of the single filter (include/ekf_slam_hip.h: ekf_set_gate, ekf_observe_gated,
// ekf_observe_log_gated): ONE launch per frame on the handle's stream, in front of everything else of the frame.
// For detection d of the frame, on the prior P the previous frame left (first sightings added), d^2 is the distance of
// ekf_gate_device.h: the three stages the batch runs as well, so filter and batch test a detection with the same code.
// An exempt detection reports d^2 = 0 and stays; a failed pivot keeps the detection and reports NaN; otherwise the detection
// is rejected iff d^2 > gate.  The survivors' indices and z go, in log order, into the workspace scratch the frame's own
// kernels then read; their number and "some pivot failed" go into a pinned host mirror.
// One workgroup: the frame is walked in chunks of CHUNK detections (one wave holds a chunk's decisions, so a ballot and a
// popcount prefix compact it; the running base makes the order stable across chunks).  A detection's arithmetic is one
// thread's (stages 1 and 3) or one thread's per support column (stage 2) and touches nothing of the other detections: the
// result depends neither on the chunk a detection falls into nor on m.
#include "ekf_gate_device.h"

template <int MODEL> struct EkfGateShape;
// static LDS: CHUNK * EkfGateScratch<MODEL>::DOUBLES * 8 bytes = 46080 (EKF), 43008 (EKF_Rotations)
template <> struct EkfGateShape<0> { static constexpr int CHUNK = 64; };
template <> struct EkfGateShape<1> { static constexpr int CHUNK = 16; };

template <typename T, int MODEL>
__global__ __launch_bounds__(EKF_GATE_THREADS) void ekf_frame_gate_kernel(const EkfGateArgs a) {
    constexpr int RD = EkfModel<MODEL>::RD, LMD = EkfModel<MODEL>::LMD, JC = EkfModel<MODEL>::JC;
    constexpr int CHUNK = EkfGateShape<MODEL>::CHUNK, SCR = EkfGateScratch<MODEL>::DOUBLES;
    static_assert(CHUNK <= 64, "one wave holds the decisions of a chunk");
    __shared__ double scr[CHUNK * SCR];
    __shared__ int col0[CHUNK];
    const int tid = threadIdx.x, nt = blockDim.x;
    const T* P = static_cast<const T*>(a.cov);
    // a sticky error from an earlier frame: nothing is tested any more (d^2 = NaN) and every detection stays, so the frame
    // runs as it does without a gate
    const bool dead = a.status[0] != 0;
    int base = 0;            // survivors of the chunks before this one (wave 0)
    bool pivot_failed = false;
    for (int d0 = 0; d0 < a.m; d0 += CHUNK) {
        const int mc = min(CHUNK, a.m - d0);
        // h, dh and r = z - h of every detection of the chunk (the exempt ones included: the wave does not diverge)
        if (tid < mc && !dead) {
            int i = a.idx[d0 + tid];
            if ((unsigned)i >= (unsigned)a.n_lm) {      // (as ekf_lm_column: clamped, and reported by the next synchronising call)
                atomicOr(a.status, EKF_ST_BAD_INDEX);
                if (a.status_host) __hip_atomic_store(a.status_host, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                i = 0;
            }
            col0[tid] = EKF_CAM + LMD * i;
            ekf_gate_measure<MODEL>(a.state, col0[tid], a.z + (size_t)(d0 + tid) * RD, scr + (size_t)tid * SCR);
        }
        __syncthreads();
        for (int task = tid; task < mc * JC && !dead; task += nt) {
            const int d = task / JC;
            ekf_gate_project<MODEL>(P, a.ld, col0[d], task - d * JC, a.dims, a.nz, scr + (size_t)d * SCR);
        }
        __syncthreads();
        bool keep = false, bad = false;
        if (tid < mc) {
            double out = __builtin_nan("");
            if (!dead) {
                double d2;
                const bool ok = ekf_gate_distance<MODEL>(a.nz.r_unc, a.rows ? a.rows + (size_t)(d0 + tid) * RD : nullptr,
                                                            scr + (size_t)tid * SCR, d2);
                const bool exempt = a.exempt && a.exempt[d0 + tid] != 0;
                out = exempt ? 0.0 : ok ? d2 : __builtin_nan("");
                bad = !exempt && !ok;
            }
            keep = !(out > a.gate);      // (NaN and 0 compare false: kept)
            if (a.mahal) a.mahal[d0 + tid] = out;
            if (a.mahal_host) a.mahal_host[d0 + tid] = out;
        }
        if (tid < 64) {      // wave 0 holds the chunk: stable compaction by ballot and popcount prefix
            const uint64_t mask = __ballot(keep);
            pivot_failed = pivot_failed || __ballot(bad) != 0;
            if (keep) {
                const int pos = base + __popcll(mask & ((1ull << tid) - 1ull));
                a.out_idx[pos] = a.idx[d0 + tid];
                for (int r = 0; r < RD; ++r) a.out_z[(size_t)pos * RD + r] = a.z[(size_t)(d0 + tid) * RD + r];
                if (a.rows)
                    for (int r = 0; r < RD; ++r) a.out_rows[(size_t)pos * RD + r] = a.rows[(size_t)(d0 + tid) * RD + r];
            }
            base += __popcll(mask);
        }
        __syncthreads();      // (the next chunk reuses the scratch)
    }
    if (tid == 0) {
        __hip_atomic_store(a.result_host + 1, pivot_failed ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.result_host, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <typename T> void ekf_launch_frame_gate(int model, const EkfGateArgs& a, hipStream_t s) {
    if (model == 1) hipLaunchKernelGGL((ekf_frame_gate_kernel<T, 1>), dim3(1), dim3(EKF_GATE_THREADS), 0, s, a);
    else hipLaunchKernelGGL((ekf_frame_gate_kernel<T, 0>), dim3(1), dim3(EKF_GATE_THREADS), 0, s, a);
}
template void ekf_launch_frame_gate<float>(int, const EkfGateArgs&, hipStream_t);
template void ekf_launch_frame_gate<double>(int, const EkfGateArgs&, hipStream_t);
