// The HBM-resident batch window kernels (large maps, wide frames) with the camera-motion stage at the top of the frame
// (EkfBatchWindow::motion != null): the MOVED = true instances of ekf_batch_wide.hip's frame body, in a translation unit of
// their own; a call without motions runs the kernels of ekf_batch_wide.hip.
#define EKF_BATCH_WIDE_MOVED 1
#include "ekf_batch_wide.hip"
