// Landmark removal (ekf_remove.hip; include/ekf_slam_hip.h: ekf_remove_markers, ekf_batch_remove_markers): launch interface
// and the host side both handles share.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

// One launch gathers every member's kept rows and columns: destination (i', j') = source (map[i'], map[j']), 0 where the
// map says EKF_REMOVE_NONE (the capacity padding), likewise the state.  Member b on blockIdx.y.
#define EKF_REMOVE_NONE (-1)
#define EKF_REMOVE_THREADS 256
#define EKF_REMOVE_ROWS 8          // destination rows per workgroup and pass
struct EkfRemoveArgs {
    const void* cov_src;           // [members][ld][ld], T
    void* cov_dst;
    const double* state_src;       // [members][ld]
    double* state_dst;
    int64_t ld;                    // a multiple of 32
    const int32_t* map;            // [members][ld] source index of every destination index, or EKF_REMOVE_NONE
    int32_t* nlm;                  // [members] landmark counts on the device, or null (single filter: the host keeps it)
    const int32_t* nlm_new;        // [members] what the launch stores there
    // single filter only (null / 0 otherwise):
    double* state_host;            // pinned host mirror of the state: receives the first n_new entries of the new state
    void* cov2;                    // second covariance buffer of the pipelined mode [ld][ld], T: its rows and columns
    int32_t n_new, fringe_hi;      // [n_new, fringe_hi) are set to zero (the rest of it is not touched)
};
template <typename T> void ekf_launch_remove(const EkfRemoveArgs& a, int members, hipStream_t s);

// The index map of one filter: out[0 .. ld), from the removal list `rm` [count] of a filter with n_lm landmarks of lmd
// dimensions behind the 10 camera dimensions.  Returns an empty string, or what is wrong with the list (rule 1 of the
// removal semantics: distinct indices in [0, n_lm)).  `sorted` is scratch.
inline std::string ekf_remove_build_map(const int32_t* rm, int64_t count, int n_lm, int lmd, int64_t ld, int32_t* out,
                                        std::vector<int32_t>& sorted) {
    sorted.assign(rm, rm + count);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t i = 0; i < count; ++i) {
        if (sorted[i] < 0 || sorted[i] >= n_lm) return "landmark index out of range in the removal list";
        if (i > 0 && sorted[i] == sorted[i - 1]) return "duplicate landmark index in the removal list";
    }
    if (out == nullptr) return "";
    int64_t at = 0;
    for (; at < 10; ++at) out[at] = (int32_t)at;
    int64_t next = 0;                 // next entry of `sorted` not yet passed
    for (int l = 0; l < n_lm; ++l) {
        if (next < count && sorted[next] == l) {
            ++next;
            continue;
        }
        for (int d = 0; d < lmd; ++d) out[at++] = 10 + lmd * l + d;
    }
    for (; at < ld; ++at) out[at] = EKF_REMOVE_NONE;
    return "";
}
