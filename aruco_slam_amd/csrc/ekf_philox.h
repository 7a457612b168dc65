// Counter-based noise of the replica kernels (ekf_batch_replicas.hip: pose noise, ekf_batch_corner_replicas.hip: pixel noise
// on the marker corners): Philox4x32-10 and the word pair -> (0, 1] conversion, one definition for both streams.  The noise
// definitions themselves are part of the ABI (include/ekf_slam_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011): the published round constants
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// (0, 1]: (v + 0.5) 2^-53 in f64 for v the top 53 bits of (hi << 32 | lo) (never 0, so log(u) is finite)
__device__ __forceinline__ double unit_open(uint32_t hi, uint32_t lo) {
    const uint64_t v = ((uint64_t)hi << 32 | lo) >> 11;
    return ((double)v + 0.5) * 0x1.0p-53;
}
