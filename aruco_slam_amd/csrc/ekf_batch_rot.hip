// Batch of independent EKF_Rotations filters (ekf_batch_observe_logs, ekf_batch_api.hip): the window kernel of the rotations
// model (RD = 7 rows per detection, LMD = 10 landmark dims, JC = 20 Jacobian columns; frame body: ekf_batch_impl.h).
// Capacity: N = 10 n + 10 <= 256 (n <= 24, one column per thread) and k = 7 m <= 56 (m <= 8): at kmax = 56, lda = 252 the
// dynamic LDS is 149,456 bytes, within the 160 KiB of a CU.
#include "ekf_batch_impl.h"

extern "C" size_t ekf_batch_rot_lds_bytes(int kmax, int lda) { return ekf_batch_lds_bytes_of<1>(kmax, lda); }

__global__ __launch_bounds__(256) void ekf_batch_rot_window_kernel(EkfBatchWindow a) { ekf_batch_window<1>(a); }

void ekf_launch_batch_rot_window(const EkfBatchWindow& a, int members, hipStream_t s) {
    if (a.frozen) return ekf_launch_batch_frozen_window(1, a, members, s);    // (ekf_batch_frozen.hip)
    if (a.motion) return ekf_launch_batch_moved_window(1, a, members, s);      // (ekf_batch_moved.hip)
    static bool once = false;
    ekf_batch_launch<1>(ekf_batch_rot_window_kernel, once, a, members, s);
}
