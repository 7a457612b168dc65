// Batch window kernels of a batch with frozen members (EkfBatchWindow::frozen != null; include/ekf_slam_hip.h, "Localisation
// mode"; frame body and strip: ekf_batch_impl.h, FROZEN = true), EKF and EKF_Rotations, with and without the camera-motion
// stage.  Instances and a translation unit of their own: a batch in which no member is frozen runs the kernels of
// ekf_batch.hip / ekf_batch_rot.hip / ekf_batch_moved.hip, which do not carry the branch.
#include "ekf_batch_impl.h"

__global__ __launch_bounds__(256) void ekf_batch_frozen_window_kernel(EkfBatchWindow a) { ekf_batch_window<0, false, true>(a); }
__global__ __launch_bounds__(256) void ekf_batch_frozen_rot_window_kernel(EkfBatchWindow a) { ekf_batch_window<1, false, true>(a); }
__global__ __launch_bounds__(256) void ekf_batch_frozen_moved_window_kernel(EkfBatchWindow a) { ekf_batch_window<0, true, true>(a); }
__global__ __launch_bounds__(256) void ekf_batch_frozen_moved_rot_window_kernel(EkfBatchWindow a) { ekf_batch_window<1, true, true>(a); }

void ekf_launch_batch_frozen_window(int model, const EkfBatchWindow& a, int members, hipStream_t s) {
    static bool once[2][2] = {{false, false}, {false, false}};
    const bool moved = a.motion != nullptr;
    if (model == 1)
        ekf_batch_launch<1>(moved ? ekf_batch_frozen_moved_rot_window_kernel : ekf_batch_frozen_rot_window_kernel,
                            once[1][moved], a, members, s);
    else
        ekf_batch_launch<0>(moved ? ekf_batch_frozen_moved_window_kernel : ekf_batch_frozen_window_kernel, once[0][moved], a,
                            members, s);
}
