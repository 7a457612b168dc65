// Batch of independent EKF filters (ekf_batch_observe_logs, ekf_batch_api.hip): the window kernel of the EKF model (the
// frame body is ekf_batch_impl.h, shared with the EKF_Rotations kernel of ekf_batch_rot.hip).
#include "ekf_batch_impl.h"

extern "C" size_t ekf_batch_lds_bytes(int kmax, int lda) { return ekf_batch_lds_bytes_of<0>(kmax, lda); }

__global__ __launch_bounds__(256) void ekf_batch_window_kernel(EkfBatchWindow a) { ekf_batch_window<0>(a); }

void ekf_launch_batch_window(const EkfBatchWindow& a, int members, hipStream_t s) {
    if (a.frozen) return ekf_launch_batch_frozen_window(0, a, members, s);    // (ekf_batch_frozen.hip)
    if (a.motion) return ekf_launch_batch_moved_window(0, a, members, s);      // (ekf_batch_moved.hip)
    static bool once = false;
    ekf_batch_launch<0>(ekf_batch_window_kernel, once, a, members, s);
}
