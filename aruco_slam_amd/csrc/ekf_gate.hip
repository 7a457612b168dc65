// Per-detection chi-square gate of the single filter (include/ekf_slam_hip.h: ekf_set_gate, ekf_observe_gated,
// ekf_observe_log_gated): ONE launch per frame on the handle's stream, in front of everything else of the frame.
// For detection d of the frame, on the prior P the previous frame left (first sightings added):
//   r_d = z_d - h_d(x), S_d = H_d (P+Q) H_d^T + R I [RD, RD] from the (10 + LMD)^2 support block of P,
//   S_d = L_d L_d^T and d^2 = |L_d^-1 r_d|^2, every sum one ascending fma chain, all of it in f64 (an f32 P is widened on
//   load): the stages of ekf_batch_gate (ekf_batch_impl.h), operation for operation.
// An exempt detection reports d^2 = 0 and stays; a failed pivot keeps the detection and reports NaN; otherwise the detection
// is rejected iff d^2 > gate.  The survivors' indices and z go, in log order, into the workspace scratch the frame's own
// kernels then read; their number and "some pivot failed" go into a pinned host mirror.
// One workgroup: the frame is walked in chunks of CHUNK detections (one wave holds a chunk's decisions, so a ballot and a
// popcount prefix compact it; the running base makes the order stable across chunks).  A detection's arithmetic is one
// thread's (stages 1 and 3) or one thread's per support column (stage 2) and touches nothing of the other detections: the
// result depends neither on the chunk a detection falls into nor on m.
#include "ekf_kernels.h"

template <int MODEL> struct EkfGateShape;
// static LDS: CHUNK * DOUBLES * 8 bytes = 46080 (EKF), 43008 (EKF_Rotations)
template <> struct EkfGateShape<0> { static constexpr int CHUNK = 64; };
template <> struct EkfGateShape<1> { static constexpr int CHUNK = 16; };

template <typename T, int MODEL>
__global__ __launch_bounds__(EKF_GATE_THREADS) void ekf_frame_gate_kernel(const EkfGateArgs a) {
    constexpr int RD = EkfModel<MODEL>::RD, LMD = EkfModel<MODEL>::LMD, JC = EkfModel<MODEL>::JC;
    constexpr int CHUNK = EkfGateShape<MODEL>::CHUNK;
    // per detection: J [RD][JC] | T = H_d (P+Q)[:, supp] [RD][JC] | S_d [RD][RD] | r_d [RD]
    constexpr int SCR = 2 * RD * JC + RD * RD + RD;
    static_assert(CHUNK <= 64, "one wave holds the decisions of a chunk");
    __shared__ double scr[CHUNK * SCR];
    __shared__ int col0[CHUNK];
    const int tid = threadIdx.x, nt = blockDim.x;
    const T* P = static_cast<const T*>(a.cov);
    const double* st = a.state;
    const int64_t ld = a.ld;
    const int N = a.dims;
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
            const int c0 = EKF_CAM + LMD * i;
            col0[tid] = c0;
            double* Jd = scr + (size_t)tid * SCR;
            double* rd = Jd + 2 * RD * JC + RD * RD;
            double cam[EKF_CAM], lm[LMD], h[RD];
            for (int q = 0; q < EKF_CAM; ++q) cam[q] = st[q];
            for (int q = 0; q < LMD; ++q) lm[q] = st[c0 + q];
            // (the rows go to LDS as the model produces them: a register copy of 7 x 20 would spill)
            ekf_measure_model<MODEL>(cam, lm, h, reinterpret_cast<double(*)[JC]>(Jd));
            for (int r = 0; r < RD; ++r) rd[r] = a.z[(size_t)(d0 + tid) * RD + r] - h[r];
        }
        __syncthreads();
        // T[:, ci] = H_d (P+Q)[supp, supp[ci]]: one thread per (detection, support column), the column's loads in one round
        for (int task = tid; task < mc * JC && !dead; task += nt) {
            const int d = task / JC, ci = task - d * JC;
            const int c0 = col0[d];
            const int c = ci < EKF_CAM ? ci : c0 + ci - EKF_CAM;
            const double* Jd = scr + (size_t)d * SCR;
            double pc[JC];
#pragma unroll
            for (int si = 0; si < JC; ++si) {
                const int s = si < EKF_CAM ? si : c0 + si - EKF_CAM;
                pc[si] = (double)P[(int64_t)s * ld + c] + (si == ci ? ekf_qdiag(c, N, a.nz) : 0.0);
            }
#pragma unroll 1
            for (int r = 0; r < RD; ++r) {
                double acc = 0.0;
#pragma unroll
                for (int si = 0; si < JC; ++si) acc = fma(Jd[r * JC + si], pc[si], acc);
                scr[(size_t)d * SCR + RD * JC + r * JC + ci] = acc;
            }
        }
        __syncthreads();
        bool keep = false, bad = false;
        if (tid < mc) {
            double out = __builtin_nan("");
            if (!dead) {
                const double* Jd = scr + (size_t)tid * SCR;
                const double* Td = Jd + RD * JC;
                double* Sd = scr + (size_t)tid * SCR + 2 * RD * JC;
                double* rd = Sd + RD * RD;
                // S_d = T H_d^T + R I, lower triangle
#pragma unroll 1
                for (int r = 0; r < RD; ++r)
#pragma unroll 1
                    for (int rr = 0; rr <= r; ++rr) {
                        double acc = 0.0;
#pragma unroll 4
                        for (int ci = 0; ci < JC; ++ci) acc = fma(Td[r * JC + ci], Jd[rr * JC + ci], acc);
                        Sd[r * RD + rr] = acc + (r == rr ? a.nz.r_unc : 0.0);
                    }
                // S_d = L L^T row by row (L_ii on the diagonal) with y = L^-1 r behind each row; d^2 = y^T y
                bool ok = true;
                double d2 = 0.0;
#pragma unroll 1
                for (int i = 0; i < RD && ok; ++i) {
                    double* Li = Sd + i * RD;
#pragma unroll 1
                    for (int j = 0; j < i; ++j) {
                        const double* Lj = Sd + j * RD;
                        double v = Li[j];
                        for (int l = 0; l < j; ++l) v = fma(-Li[l], Lj[l], v);
                        Li[j] = v / Lj[j];
                    }
                    double dii = Li[i], y = rd[i];
                    for (int l = 0; l < i; ++l) {
                        dii = fma(-Li[l], Li[l], dii);
                        y = fma(-Li[l], rd[l], y);
                    }
                    ok = dii > 0.0 && isfinite(dii);
                    if (ok) {
                        Li[i] = sqrt(dii);
                        y = y / Li[i];
                        rd[i] = y;
                        d2 = fma(y, y, d2);
                    }
                }
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
