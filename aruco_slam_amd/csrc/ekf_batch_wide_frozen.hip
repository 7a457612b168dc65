// The HBM-resident batch window kernels (large maps, wide frames) of a batch with frozen members
// (EkfBatchWindow::frozen != null; include/ekf_slam_hip.h, "Localisation mode"): the FROZEN = true instances of
// ekf_batch_wide.hip's frame body, with and without the camera-motion stage, in a translation unit of their own; a batch in
// which no member is frozen runs the kernels of ekf_batch_wide.hip / ekf_batch_wide_moved.hip.
#define EKF_BATCH_WIDE_FROZEN 1
#include "ekf_batch_wide.hip"
