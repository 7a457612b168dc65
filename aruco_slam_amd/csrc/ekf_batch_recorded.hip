// Batch window kernels of a recorded call (ekf_batch_observe_logs_recorded; frame body and the record stage:
// ekf_batch_impl.h, RECORDED = true), EKF only, with and without the camera-motion stage.  Instances and a translation unit
// of their own: a call that does not record runs the kernels it ran before, which carry neither the stage nor its argument.
#include "ekf_batch_impl.h"

__global__ __launch_bounds__(256) void ekf_batch_recorded_window_kernel(EkfBatchWindow a, EkfBatchRecord r) {
    ekf_batch_window<0, false, false, true>(a, &r);
}
__global__ __launch_bounds__(256) void ekf_batch_recorded_moved_window_kernel(EkfBatchWindow a, EkfBatchRecord r) {
    ekf_batch_window<0, true, false, true>(a, &r);
}

void ekf_launch_batch_recorded_window(const EkfBatchWindow& a, const EkfBatchRecord& r, int members, hipStream_t s) {
    static bool once[2] = {false, false};
    void (*kernel)(EkfBatchWindow, EkfBatchRecord) =
        a.motion ? ekf_batch_recorded_moved_window_kernel : ekf_batch_recorded_window_kernel;
    bool& done = once[a.motion ? 1 : 0];
    if (!done) {      // (> 64 KB of dynamic LDS needs the opt-in, once per kernel: as ekf_batch_launch)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        done = true;
    }
    hipLaunchKernelGGL(kernel, dim3(members), dim3(256), ekf_batch_lds_bytes_of<0>(a.kmax, a.lda), s, a, r);
}
