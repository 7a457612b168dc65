// Batch window kernels with the camera-motion stage at the top of the frame (EkfBatchWindow::motion != null; frame body and
// stage: ekf_batch_impl.h, MOVED = true), EKF and EKF_Rotations.  Instances and a translation unit of their own: a call
// without motions runs the kernels of ekf_batch.hip / ekf_batch_rot.hip, which do not carry the stage's registers.
#include "ekf_batch_impl.h"

__global__ __launch_bounds__(256) void ekf_batch_moved_window_kernel(EkfBatchWindow a) { ekf_batch_window<0, true>(a); }
__global__ __launch_bounds__(256) void ekf_batch_moved_rot_window_kernel(EkfBatchWindow a) { ekf_batch_window<1, true>(a); }

void ekf_launch_batch_moved_window(int model, const EkfBatchWindow& a, int members, hipStream_t s) {
    static bool once[2] = {false, false};
    if (model == 1) ekf_batch_launch<1>(ekf_batch_moved_rot_window_kernel, once[1], a, members, s);
    else ekf_batch_launch<0>(ekf_batch_moved_window_kernel, once[0], a, members, s);
}
