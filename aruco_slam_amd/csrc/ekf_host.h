// Host helpers shared by the C ABI translation units (the filter handle, ekf_filter.h: ekf_api.hip, ekf_frames.hip,
// ekf_log_api.hip, ekf_smooth_api.hip; the batch handle: ekf_batch_api.hip).
// Not part of the public interface.
#pragma once

#include "../../include/ekf_slam_hip.h"

#include <hip/hip_runtime.h>

#include "ekf_kernels.h"

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

// The library's one error slot (ekf_last_error_string), defined in ekf_api.hip.
extern thread_local std::string g_err __attribute__((visibility("hidden")));

namespace {

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(EKF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

int64_t round_up(int64_t v, int64_t q) { return (v + q - 1) / q * q; }
size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// Carves a buffer into 256-byte aligned pieces, one after the other: take(bytes) returns where the piece starts, `end` is
// where the last one ends.
struct Carve {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t at = end;
        end += align256(bytes);
        return at;
    }
};

// Pinned host memory, freed once with its owner.
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { if (p_) (void)hipHostFree(p_); }
    // At least `bytes`; the contents are not kept.  When the allocation fails, the buffer is as it was.
    int reserve(size_t bytes) {
        if (bytes <= size_) return EKF_OK;
        void* p = nullptr;
        HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        if (p_) (void)hipHostFree(p_);
        p_ = static_cast<char*>(p);
        size_ = bytes;
        return EKF_OK;
    }
    char* get() const { return p_; }
    template <typename P> P* at(size_t off) const { return reinterpret_cast<P*>(p_ + off); }

private:
    char* p_ = nullptr;
    size_t size_ = 0;
};

// Device memory from the caller: none of `bufs` NULL, each 256-byte aligned (every layout is carved in 256-byte pieces),
// and `bytes` at least the `need` that `sizes` (the size query) gave.
int check_device_buffers(std::initializer_list<const void*> bufs, size_t bytes, size_t need, const char* sizes) {
    for (const void* p : bufs)
        if (!p) return fail(EKF_ERR_INVALID, "NULL device buffer");
    if (bytes < need) return fail(EKF_ERR_INVALID, std::string("workspace smaller than ") + sizes);
    for (const void* p : bufs)
        if (reinterpret_cast<uintptr_t>(p) & 0xFF) return fail(EKF_ERR_INVALID, "device buffers must be 256-byte aligned");
    return EKF_OK;
}

// Offsets of a detection log: offsets[0] == 0 and non-decreasing over `count` entries after it (`name` in the messages).
int check_offsets(const int64_t* offsets, int64_t count, const char* name) {
    if (offsets[0] != 0) return fail(EKF_ERR_INVALID, std::string(name) + "[0] must be 0");
    for (int64_t t = 0; t < count; ++t)
        if (offsets[t + 1] < offsets[t]) return fail(EKF_ERR_INVALID, std::string(name) + " must be non-decreasing");
    return EKF_OK;
}

// What a detection log asks of a filter that holds n_lm landmarks (check_log).
struct LogCheck {
    std::vector<int32_t> slots;    // detection of every first sighting, in order
    std::vector<int64_t> new_at;   // [frames + 1]: the first sightings of frame t are slots[new_at[t] .. new_at[t + 1])
    int n = 0;                     // landmarks after the log
    int64_t widest = 0;            // most detections in one frame
};

// Frames [0, frames) of a log whose offsets have passed check_offsets: first sightings numbered n_lm, n_lm + 1, ... in order
// of occurrence (EKF_ERR_INVALID), then at most max_landmarks landmarks and max_visible detections per frame
// (EKF_ERR_CAPACITY).  `log` names the log in the messages.
int check_log(const int32_t* lm_index, const int64_t* offsets, int64_t frames, int n_lm, const ekf_config& cfg,
              const std::string& log, LogCheck* out) {
    *out = LogCheck{{}, std::vector<int64_t>((size_t)frames + 1, 0), n_lm, 0};
    for (int64_t t = 0; t < frames; ++t) {
        out->new_at[t] = (int64_t)out->slots.size();
        for (int64_t d = offsets[t]; d < offsets[t + 1]; ++d) {
            const int32_t i = lm_index[d];
            if (i < 0) return fail(EKF_ERR_INVALID, "negative landmark index in " + log);
            if (i > out->n)
                return fail(EKF_ERR_INVALID, "landmark index beyond the next free one in " + log +
                                                 " (first sightings must be numbered n, n+1, ... in order of first occurrence)");
            if (i == out->n) {
                out->slots.push_back((int32_t)d);
                ++out->n;
            }
        }
        out->widest = std::max<int64_t>(out->widest, offsets[t + 1] - offsets[t]);
    }
    out->new_at[frames] = (int64_t)out->slots.size();
    if (out->n > cfg.max_landmarks) return fail(EKF_ERR_CAPACITY, log + " needs more landmarks than max_landmarks");
    if (out->widest > cfg.max_visible) return fail(EKF_ERR_CAPACITY, "a frame of " + log + " has more detections than max_visible");
    return EKF_OK;
}

// The camera of the pose front end from the C ABI's arguments (row-major 3x3 matrix, 0..8 distortion coefficients).
int make_camera(const double camera_matrix[9], const double* dist_coeffs, int32_t n_dist, EkfCamera* cam) {
    if (!camera_matrix) return fail(EKF_ERR_INVALID, "camera matrix is NULL");
    if (n_dist < 0 || n_dist > 8 || (n_dist > 0 && !dist_coeffs))
        return fail(EKF_ERR_INVALID, "0..8 distortion coefficients (k1 k2 p1 p2 k3 k4 k5 k6) are supported");
    if (!(camera_matrix[0] > 0.0) || !(camera_matrix[4] > 0.0)) return fail(EKF_ERR_INVALID, "focal lengths must be > 0");
    cam->fx = camera_matrix[0];
    cam->fy = camera_matrix[4];
    cam->cx = camera_matrix[2];
    cam->cy = camera_matrix[5];
    for (int i = 0; i < 8; ++i) cam->k[i] = (i < n_dist) ? dist_coeffs[i] : 0.0;
    return EKF_OK;
}

}  // namespace
