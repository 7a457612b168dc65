/*
 * ekf_slam_hip.h -- C ABI of the MI355X (gfx950) EKF-SLAM update path.
 *
 * Drop-in boundary for the reference filter back-end
 *   /root/reference/filters/extended_kalman_filter.py  (class EKF)
 * as it is driven by
 *   /root/reference/filters/base_filter.py:203-207  (observe, get_poses)
 *   /root/reference/filters/base_filter.py:214-247  (save_map getters)
 *
 * Plain C, no torch / C++ types.  Every function returns 0 (EKF_OK) or a
 * negative error code; ekf_last_error_string() describes the last failure on
 * the calling thread.  A filter handle has exactly one caller thread; all
 * device work is enqueued on the handle's HIP stream; observe calls return
 * before the GPU has finished, getters synchronise.
 *
 * Memory: the covariance, state and workspace live in DEVICE memory owned by
 * the caller (the Python shim passes torch tensor data_ptr()s).  The library
 * never allocates or frees them; they must outlive the handle.
 *
 * State layout (extended_kalman_filter.py:29-34,46-51):
 *   state  f64 [3 n + 10] = [x y z | qw qx qy qz | ex ey ez | l0 | l1 | ...]
 *   cov    f32 or f64, row-major, leading dimension `ld` (capacity-padded to a
 *          multiple of 128; rows/cols >= 3 n + 10 are kept exactly zero)
 */
#ifndef EKF_SLAM_HIP_H
#define EKF_SLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ekf_filter ekf_filter; /* opaque handle */

enum { EKF_COV_F64 = 0, EKF_COV_F32 = 1 };
/* camera quaternion injection (extended_kalman_filter.py:138-149):
 * AS_WRITTEN reproduces the reference exactly (scalar-first arrays passed to
 * SciPy's scalar-last from_quat); SCALAR_FIRST is the consistent convention
 * (what ekf_with_rotations.py:150-151 does). */
enum { EKF_QUAT_AS_WRITTEN = 0, EKF_QUAT_SCALAR_FIRST = 1 };
/* filter model: EKF = extended_kalman_filter.py (landmark xyz, 3 rows per detection);
 * EKF_ROTATIONS = ekf_with_rotations.py (landmark [xyz | quat | err], 10 dims, 7 rows per
 * detection [xyz_cl ; q_cl], consistent quaternion convention, q_cam default 0.2) */
enum { EKF_MODEL_EKF = 0, EKF_MODEL_ROTATIONS = 1 };
/* covariance-update kernel selection (0 = best available: as EKF_COVK_MFMA).  MFMA: the symmetric matrix-core kernels,
 * one wave per 32 x 32 tile, and for the f32 covariance from 3000 tiles of 128 x 128 (n >= 3300 or so) one workgroup per
 * 128 x 128 macro tile with LDS-staged operands; MFMA_TILE / MFMA_MACRO force one of the two (tests, measurements; MACRO:
 * f32 only).  All of them give the same bits as the VALU reference kernel. */
/* ekf_config.flags bit 3: more than 64 (EKF_MODEL_ROTATIONS: 50) detections per frame, up to 1024 */
enum { EKF_FLAG_WIDE_FRAMES = 8 };
/* ekf_config.flags bit 4, read by ekf_batch_* only: dictionary-sized maps in a batch (see there) */
enum { EKF_FLAG_BATCH_LARGE_MAPS = 16 };
/* ekf_config.flags bit 5, read by ekf_batch_* only: up to 64 (EKF_MODEL_ROTATIONS: 50) detections per frame in a batch */
enum { EKF_FLAG_BATCH_WIDE_FRAMES = 32 };
/* ekf_config.flags bit 6, read by ekf_* (the single filter) only: the per-detection chi-square gate (ekf_set_gate) */
enum { EKF_FLAG_GATE = 64 };
/* ekf_config.flags bit 7, read by ekf_* (the single filter) only: per-detection measurement noise (ekf_observe_rows) */
enum { EKF_FLAG_ROW_NOISE = 128 };
/* ekf_config.flags bit 8: per-frame process-noise scale (ekf_observe_scaled, ekf_advance; ekf_batch_observe_logs_scaled) */
enum { EKF_FLAG_FRAME_SCALE = 256 };
/* ekf_config.flags bit 9: per-frame camera motion (ekf_move, ekf_observe_moved; ekf_batch_observe_logs_moved) */
enum { EKF_FLAG_MOTION = 512 };
enum { EKF_COVK_AUTO = 0, EKF_COVK_VALU = 1, EKF_COVK_MFMA = 2, EKF_COVK_MFMA_TILE = 3, EKF_COVK_MFMA_MACRO = 4 };

enum {
    EKF_OK = 0,
    EKF_ERR_INVALID = -1,   /* bad argument */
    EKF_ERR_CAPACITY = -2,  /* more landmarks / observations than configured */
    EKF_ERR_HIP = -3,       /* a HIP runtime call failed */
    EKF_ERR_STATE = -4,     /* buffers not bound, filter not reset, ... */
    EKF_ERR_NUMERIC = -5    /* innovation covariance not positive definite, or an internal integrity check of the
                             * front kernel's in-launch exchange tripped */
};

typedef struct ekf_config {
    int32_t max_landmarks;  /* capacity n_max */
    int32_t max_visible;    /* max observations per frame (<= 64; <= 50 for EKF_MODEL_ROTATIONS: k = 7 m <= 350 rows; beyond k = 192
                             * the frame runs through the stage kernels, in serial order).  With EKF_FLAG_WIDE_FRAMES (flags
                             * bit 3): <= 1024 for both models (k <= 3072 / 7168 rows); a frame with more than 64 (50)
                             * detections then runs through the wide-frame path, in serial order, whatever else is set */
    int32_t cov_dtype;      /* EKF_COV_F64 / EKF_COV_F32 */
    int32_t quat_mode;      /* EKF_QUAT_* */
    int32_t cov_kernel;     /* EKF_COVK_*: covariance-update kernel */
    int32_t model;          /* EKF_MODEL_* */
    int32_t reserved;
    int32_t flags;          /* bits 0-1: pipelined mode of ekf_observe_sequence_device (the front kernel of frame t+1 runs
                             * beside the covariance update of frame t; same results, bit for bit): 0 = chosen by size
                             * (MFMA covariance update only, either dtype; on except above 9000 state dimensions
                             * with more than 32 detections per frame), bit 0 = never, bit 1 = always.  Unless bit 0
                             * is set, a capable configuration adds a second covariance buffer to the workspace
                             * (ekf_query_sizes: + ld^2 elements).  One handle per process pipelines at a time
                             * (ekf_last_sequence_mode).
                             * bit 2: run gather / solve / panel as three separate launches instead of the fused front
                             * kernel (same results, bit for bit; no pipelined mode).
                             * bit 3 (EKF_FLAG_WIDE_FRAMES): max_visible may be up to 1024 (see there); the workspace
                             * of such a configuration also holds an f64 copy of A = H (P+Q) that frames with more than
                             * 384 rows turn into W (ekf_query_sizes: + 8 kmax ld bytes).  Without it, sizes and
                             * limits are as before.
                             * bit 4 (EKF_FLAG_BATCH_LARGE_MAPS), bit 5 (EKF_FLAG_BATCH_WIDE_FRAMES): batches only,
                             * see ekf_batch_query_sizes.
                             * bit 6 (EKF_FLAG_GATE): the filter can gate its detections (ekf_set_gate); the workspace
                             * then also holds the survivors of a frame and its distances (ekf_query_sizes: + 68
                             * max_visible bytes and change).  Without it, sizes, layout and results are as before.
                             * bit 7 (EKF_FLAG_ROW_NOISE): the filter takes per-detection measurement noise
                             * (ekf_observe_rows); with bit 6 the workspace then also holds the survivors' rows of a
                             * gated frame (ekf_query_sizes: + 8 rd max_visible bytes, padded to 256; without bit 6
                             * the size does not change: host rows are staged in pinned memory, device rows are read
                             * where they are).  Without it, sizes, layout and results are as before.
                             * bit 8 (EKF_FLAG_FRAME_SCALE): frames may carry a process-noise scale and the filter keeps a
                             * pending scale (see "Per-frame process-noise scale").  The single filter's sizes do not
                             * change (the pending scale lives on the host); a batch's workspace grows by 8 bytes per
                             * member, padded to 256.  Without it, sizes, layout and results are as before.
                             * bit 9 (EKF_FLAG_MOTION): frames may carry a camera motion (see "Odometry input").  No size
                             * and no layout changes. */
    /* noise constants, defaults = extended_kalman_filter.py:21-27 */
    double initial_camera_uncertainty;   /* 0.1  */
    double initial_landmark_uncertainty; /* 0.7  */
    double r_uncertainty;                /* 0.9  */
    double q_cam;                        /* 0.3  */
    double q_err;                        /* 0.5  */
    double q_lm;                         /* 0.01 */
    void *stream;                        /* hipStream_t, NULL = default */
} ekf_config;

/* Fill `cfg` with the reference's constants (extended_kalman_filter.py:19-34). */
int ekf_default_config(ekf_config *cfg);

/* Sizes of the caller-owned device buffers for this configuration. */
int ekf_query_sizes(const ekf_config *cfg, int64_t *ld, size_t *cov_bytes,
                    size_t *state_bytes, size_t *workspace_bytes);

/* EKF.__init__ (extended_kalman_filter.py:40-56) without the SymPy step. */
int ekf_create(const ekf_config *cfg, ekf_filter **out);
int ekf_destroy(ekf_filter *f);

/* Borrow caller-owned device memory (see ekf_query_sizes). */
int ekf_bind_buffers(ekf_filter *f, void *cov_dev, int64_t ld, double *state_dev,
                     void *workspace_dev, size_t workspace_bytes);

/* Capacity growth.  The reference appends landmarks without limit (extended_kalman_filter.py:274-290: hstack / block
 * matrix per add_marker); here the capacity is fixed by the buffers, and a filter that is about to exceed max_landmarks
 * moves into larger ones (likewise for more detections per frame than max_visible): the caller sizes new buffers with
 * ekf_query_sizes for the same configuration with the new max_landmarks / max_visible (neither may shrink), and the library copies state, covariance (device to device, capacity padding zero) and
 * the status word, re-arms its workspace and borrows the new buffers from then on; the old ones may be freed when the call
 * returns.  The filter continues bit for bit as one that had been created with the larger capacity. */
int ekf_grow(ekf_filter *f, int32_t new_max_landmarks, int32_t new_max_visible, void *cov_dev, int64_t ld,
             double *state_dev, void *workspace_dev, size_t workspace_bytes);

/* state = initial pose, P = 0.1 I_10, no landmarks
 * (extended_kalman_filter.py:46-51). */
int ekf_reset(ekf_filter *f, const double initial_camera_pose[10]);

/* EKF.add_marker for `count` new landmarks (extended_kalman_filter.py:239-290):
 * t_ml = R(q)^-1 * cam_frame_xyz + cam_xyz with the CURRENT camera state,
 * appended to the state; P grows by diag(diag_uncertainty) (or 0.7 I if NULL).
 * Host pointers: cam_frame_xyz [count,3], diag_uncertainty [count,3] or NULL.
 * EKF_MODEL_ROTATIONS (ekf_with_rotations.py:275-335): cam_frame_xyz is the full pose
 * [count,6] = [tvec | rvec] (rvec read as extrinsic xyz Euler angles, :307-310), the new
 * landmark is [t_ml | q_ml | 0 0 0], diag_uncertainty is [count,10].
 * The new landmarks get indices n .. n+count-1 (the marker-id -> index dict
 * stays on the Python side). */
int ekf_add_markers(ekf_filter *f, const double *cam_frame_xyz,
                    const double *diag_uncertainty, int32_t count);

/* EKF.predict + EKF.update for one frame (extended_kalman_filter.py:95-156):
 * lm_index [m] = landmark indices of the visible markers in `ids` order
 * (duplicates legal), z [m,3] = pose[0:3] of every detection (EKF_MODEL_ROTATIONS: z [m,7] =
 * [pose[0:3] | quaternion of from_euler("xyz", pose[3:6]), scalar first], :216-224).
 * ekf_observe takes host pointers (copied during the call; indices are range-checked at once);
 * ekf_observe_device takes device pointers that must stay valid until the
 * stream has consumed them.  Device-resident indices are range-checked BY THE KERNELS: an index
 * outside [0, num_landmarks) is clamped (nothing is read or written out of bounds) and reported as
 * EKF_ERR_INVALID by the next synchronising call (ekf_sync, any getter); the error is sticky until
 * ekf_reset, because the frames computed from clamped indices have already changed the filter. */
int ekf_observe(ekf_filter *f, const int32_t *lm_index, const double *z, int32_t m);
int ekf_observe_device(ekf_filter *f, const int32_t *lm_index_dev,
                       const double *z_dev, int32_t m);

/* `frames` consecutive observe() calls on device-resident detections
 * lm_index_dev [frames,m], z_dev [frames,m,3]; after every frame the camera
 * pose state[0:7] is appended to trajectory_dev [frames,7] (may be NULL).
 * Pipelined mode (see ekf_config.flags): the covariance update of frame t runs on an internal
 * second stream BESIDE frame t+1's front kernel.  The covariance ping-pongs between the caller's
 * buffer and a second one in the workspace (the update reads P_t and writes P_{t+1} elsewhere), and
 * the front kernel of frame t+1 completes the few rows of P_{t+1} it reads from P_t and W_t on the
 * fly, with the update's own per-element instruction sequence: results are bitwise those of
 * per-frame ekf_observe calls.  The two streams are ordered by one-wave gate kernels on the
 * device, every wait bounded.  The last update of a call runs on the handle's stream again, so after the
 * call that stream alone orders everything that follows, and the covariance is back in the caller's buffer. */
int ekf_observe_sequence_device(ekf_filter *f, const int32_t *lm_index_dev,
                                const double *z_dev, int32_t m, int32_t frames,
                                double *trajectory_dev);
/* What the last ekf_observe_sequence_device call of this handle did (results are the same bits in every mode):
 * PIPELINED; SERIAL (not asked for / not chosen for this size, fewer than 2 frames, kernel timing on, stage kernels);
 * SERIAL_ONE_QUEUE: asked for, but the handle's two streams share one hardware queue (found by a self-test on first use);
 * SERIAL_OTHER_HANDLE: asked for, but another handle of the process has a pipelined call in flight -- the device-side
 * gates of two handles could wait for each other across the shared hardware queues, so only one handle pipelines at a time. */
enum { EKF_SEQ_NONE = 0, EKF_SEQ_SERIAL = 1, EKF_SEQ_PIPELINED = 2, EKF_SEQ_SERIAL_ONE_QUEUE = 3, EKF_SEQ_SERIAL_OTHER_HANDLE = 4 };
int ekf_last_sequence_mode(const ekf_filter *f);

/* Log replay: BaseFilter.process_detections with should_filter=True over a whole recorded log in one call
 * (base_filter.py:196-212, extended_kalman_filter.py:58-156, ekf_with_rotations.py:66-181).  EKF_MODEL_EKF: the same bits
 * as the per-frame ekf_add_markers / ekf_observe loop; EKF_MODEL_ROTATIONS: z is formed on the device, and its quaternion
 * may differ from the host's in the last place (device sin / cos).
 *
 * ekf_log_workspace_bytes: device scratch a log of `detections` detections needs (caller-owned, like the workspace).
 *
 * ekf_observe_log:
 *   lm_index [D]   HOST  landmark index of every detection, frame after frame.  An index >= the number of landmarks at the
 *                        start of its frame is a first sighting; first sightings must be numbered n, n+1, ... in order of
 *                        first occurrence (the Python id -> index dict assigns them).  Duplicates within a frame are legal.
 *   offsets [F+1]  HOST  offsets[0] = 0, non-decreasing, offsets[F] = D.  An empty frame is NOT stepped (no predict); its
 *                        trajectory row repeats the previous one (the camera state at the call for the first frames).
 *   poses_dev [D,6] DEVICE  [tvec | rvec] exactly as logged; valid until the handle's stream has consumed it.
 *   log_ws         DEVICE  256-byte aligned, ekf_log_workspace_bytes(D); valid until the stream has consumed it.
 *   trajectory_dev [F,7] DEVICE or NULL  state[0:7] after every frame.
 * Everything is validated on the host before anything is enqueued: a bad log returns EKF_ERR_INVALID, a log that needs more
 * landmarks or more detections per frame than the buffers hold EKF_ERR_CAPACITY, and the filter is left untouched (the
 * library never grows inside the call: ekf_grow first).
 * Device work, on the handle's stream: one copy of the indices, one prepare kernel (z of the whole log), then frame after
 * frame.  A frame with first sightings adds them with one gather launch, reading the camera state the previous frame left.
 * Consecutive frames that the rule of ekf_observe_sequence_device would pipeline on their own, with one kpad (3 m or 7 m
 * rounded up to 16) and no first sighting but in the first, run in the pipelined mode as one run; a first sighting or a
 * change of kpad ends the run.  Wide frames and frames the rule keeps serial run in serial order.  Like every observe call,
 * a frame whose tile count of the macro-tile covariance update (f32, 3000 tiles or more: state dimension >= ~9 700)
 * differs from the last one synchronises the stream once, to rebuild the launch table.
 * The host side stages the indices in pinned memory, two buffers used by turns: a call returns once its work is enqueued, and
 * only waits for the device to have finished the call before the previous one.  A getter after the call waits for all of
 * it (there is no shortcut through an earlier frame's event). */
int ekf_log_workspace_bytes(const ekf_filter *f, int64_t detections, size_t *bytes);
int ekf_observe_log(ekf_filter *f, const int32_t *lm_index, const int64_t *offsets, int32_t frames,
                    const double *poses_dev, void *log_ws, size_t log_ws_bytes, double *trajectory_dev);
/* What the last ekf_observe_log did: out[0] frames stepped, out[1] frames run in the pipelined mode, out[2] pipelined runs,
 * out[3] landmarks added. */
int ekf_last_log_stats(const ekf_filter *f, int64_t out[4]);

/* EKF.get_poses / get_lm_uncertainties (extended_kalman_filter.py:84-93).
 * Synchronise and copy to host.  ekf_get_camera / ekf_get_state directly after ekf_observe / ekf_observe_device wait
 * for the part of that frame that produces the state (and the status word) only -- the front kernel leaves the state in a
 * pinned host mirror, so nothing is copied -- and the covariance update of the frame may still be running when they return.  ekf_get_cov_diag / ekf_get_cov / ekf_sync wait for everything. */
int ekf_get_camera(ekf_filter *f, double out[10]);
int ekf_get_state(ekf_filter *f, double *out, int32_t count);
int ekf_get_cov_diag(ekf_filter *f, double *out, int32_t count);
/* Full covariance as host f64 [dims,dims] (tests, checkpointing). */
int ekf_get_cov(ekf_filter *f, double *out, int32_t dims);

/* Restore (state, P) from host f64 (map restore / teacher-forced tests).
 * cov is [dims,dims] with dims = 3*num_landmarks+10; it is symmetrised
 * ((P+P^T)/2) on upload. */
int ekf_set_state(ekf_filter *f, const double *state, int32_t num_landmarks);
int ekf_set_cov(ekf_filter *f, const double *cov, int32_t dims);

int ekf_num_landmarks(const ekf_filter *f);
int ekf_sync(ekf_filter *f);

/* Front part of the update (measurement model, S, Cholesky, W, dx, injection): enable != 0 = the
 * fused front kernel (default), 0 = the three stage kernels (gather / solve / panel).  Same results,
 * bit for bit; may be switched between any two frames (same as ekf_config.flags bit 2). */
int ekf_set_fused(ekf_filter *f, int32_t enable);

/* Per-kernel device timing with HIP events on the handle's stream.
 * which: 0 gather, 1 solve, 2 panel, 3 covariance update.  Wide frames: 0 measurement, A and S; 1 factorisation;
 * 2 W, dx and injection; 3 covariance update (beyond 384 rows: all of its row-chunk launches, events around them).
 * enable: 0 off, 1 all four kernels (5 events per frame), 2 covariance update only
 * (2 events per frame: least perturbation of the pipeline).
 * ekf_get_kernel_timing synchronises, returns the mean duration [us] and the
 * launch count since the last enable, then clears the accumulated events. */
int ekf_set_kernel_timing(ekf_filter *f, int32_t enable);
int ekf_get_kernel_timing(ekf_filter *f, int32_t which, double *mean_us, int64_t *launches);

/* Last frame's intermediates as host f64 (tests): what = 0 Jacobian blocks
 * [k,13], 1 residual [k], 2 Cholesky factor L [kpad,kpad], 3 whitened panel
 * W = L^-1 H P [kpad,dims], 4 A = H (P+Q) [k,dims].  `count` = capacity of out.
 * Items 2 and 3 need ekf_debug_fetch(f, -1, ..) before the frame (item 2 always holds L after a wide frame of more
 * than 384 rows: the blocked factorisation works in place there); all five are valid after a wide frame. */
int ekf_debug_fetch(ekf_filter *f, int32_t what, double *out, size_t count);

/* Detection -> pose front end, batched (replaces the per-marker loop of cv2.solvePnP(..., SOLVEPNP_IPPE_SQUARE) in
 * BaseFilter.estimate_pose_of_markers, filters/base_filter.py:92-171).  Stateless: no filter handle.
 * corners [count,4,2]: pixel coordinates of each marker's corners in the detector's order (top-left, top-right,
 * bottom-right, bottom-left = object points (-s/2, s/2), (s/2, s/2), (s/2, -s/2), (-s/2, -s/2), base_filter.py:113-121);
 * camera_matrix: row-major 3x3 (fx, cx, fy, cy are read); dist_coeffs: n_dist <= 8 values k1 k2 p1 p2 k3 k4 k5 k6;
 * poses [count,6] = [tvec | rvec] per marker, the layout observe() takes (base_filter.py:166-171).
 * rvec = axis * angle, through the unit quaternion of the rotation: exact to rounding for every angle in [0, pi], the
 * angle pi of a marker that faces a level camera included (cv::Rodrigues has a window |sin| < 1e-5 there: a cv2 run differs
 * by up to about 2e-5 rad inside it).
 * A degenerate detection -- the four pixel corners are not those of a strictly convex quadrilateral (collinear,
 * coincident, a consecutive triple spanning less than 1e-9 of the squared side lengths), or a coordinate is NaN or Inf --
 * gets six NaN: a pose is valid exactly if all six values are finite.  The call still returns EKF_OK and no other marker of
 * the batch is affected.  count = 0 does nothing.
 * The `_device` form enqueues one kernel on `stream` (device pointers); the host form copies, runs and synchronises. */
int ekf_estimate_poses_device(const double *corners_dev, int32_t count, double marker_size,
                              const double camera_matrix[9], const double *dist_coeffs, int32_t n_dist,
                              double *poses_dev, void *stream);
int ekf_estimate_poses(const double *corners, int32_t count, double marker_size,
                       const double camera_matrix[9], const double *dist_coeffs, int32_t n_dist,
                       double *poses, void *stream);

/* ---- Batch of independent filters: many detection logs replayed at once (parameter sweeps, evaluation sets, Monte-Carlo
 * runs: ekf_batch_observe_replicas below).  Every member is BaseFilter.process_detections with should_filter=True over its own log, exactly as
 * ekf_observe_log does it; one workgroup owns one member for a window of frames, members never wait for each other.
 *
 * cfg, by model (every member of a batch has the batch's model):
 *   EKF_MODEL_EKF:       cov_dtype EKF_COV_F64, max_landmarks <= 82, max_visible <= 16 (N = 3 n + 10 <= 256, k = 3 m <= 48),
 *                        either quat_mode;
 *   EKF_MODEL_ROTATIONS: cov_dtype EKF_COV_F64, max_landmarks <= 24, max_visible <= 8 (N = 10 n + 10 <= 256, k = 7 m <= 56),
 *                        quat_mode EKF_QUAT_SCALAR_FIRST (EKF_Rotations' convention);
 * anything else is EKF_ERR_INVALID.
 * flags bit 4 (EKF_FLAG_BATCH_LARGE_MAPS): dictionary-sized maps, N <= 1024 and ld = round_up(N, 32) <= 1024:
 *   EKF_MODEL_EKF max_landmarks <= 338, EKF_MODEL_ROTATIONS max_landmarks <= 101; max_visible and every other rule as
 *   above.  Every call then runs the large-map kernel (A / W in HBM, LDS independent of the map), whatever the map size,
 *   with the same arithmetic in the same order: where both kernels run, the results are the same bits.  The workspace
 *   grows by members * rd * max_visible * ld * 8 bytes (rd = 3: EKF, 7: EKF_Rotations).
 * flags bit 5 (EKF_FLAG_BATCH_WIDE_FRAMES): wide frames, max_visible <= 64 (EKF_MODEL_EKF, k = 3 m <= 192) or <= 50
 *   (EKF_MODEL_ROTATIONS, k = 7 m <= 350), the single filter's limits without EKF_FLAG_WIDE_FRAMES; max_landmarks follows
 *   the large-map limits above (338 / 101, N <= 1024, ld = round_up(N, 32)) whether bit 4 is set or not; every other rule
 *   as above.  Every call then runs the wide-frame kernel, whatever the frame widths and the map size.  It keeps A / W
 *   [k][ld] in HBM (the workspace, as bit 4: members * rd * max_visible * ld * 8 bytes more, with this max_visible) and
 *   factorises a frame in blocks of 16 (EKF) / 8 (EKF_Rotations) detections in log order; the off-diagonal factor rows
 *   L_ji = H_j W_i^T are formed from the W rows in HBM as they are needed, one block at a time in LDS, and not stored.
 *   A frame of at most 16 / 8 detections is one block and gives the same bits as without the flag.  P and the state are
 *   written only after every pivot of the frame has passed, so a failing pivot in any block leaves them as they were.
 * The other flag bits and cov_kernel are ignored; the noise constants of cfg are every member's defaults.
 * Below, lmd = 3 (EKF) or 10 (EKF_Rotations) landmark dims: a member's state is [lmd n + 10].
 * Memory is the caller's, as for single filters: cov [B, ld, ld] f64, state [B, ld] f64 (capacity padding exactly zero),
 * a workspace of workspace_bytes, all 256-byte aligned.  ekf_batch_bind_buffers resets every member to the identity pose.
 * A batch never grows. */
typedef struct ekf_batch ekf_batch; /* opaque handle */
int ekf_batch_query_sizes(const ekf_config *cfg, int32_t members, int64_t *ld, size_t *cov_bytes, size_t *state_bytes,
                          size_t *workspace_bytes);
int ekf_batch_create(const ekf_config *cfg, int32_t members, ekf_batch **out);
int ekf_batch_bind_buffers(ekf_batch *b, double *cov_dev, int64_t ld, double *state_dev, void *ws_dev, size_t ws_bytes);
int ekf_batch_destroy(ekf_batch *b);
/* noise [B,6] per member in ekf_config order: initial_camera_uncertainty, initial_landmark_uncertainty, r_uncertainty,
 * q_cam, q_err, q_lm (initial_camera_uncertainty takes effect at the next reset). */
int ekf_batch_set_noise(ekf_batch *b, const double *noise);
/* state = initial pose, P = initial_camera_uncertainty I_10, no landmarks, status cleared.
 * member = -1: every member, initial_poses [B,10]; member >= 0: that member, initial_poses [10]. */
int ekf_batch_reset(ekf_batch *b, int32_t member, const double *initial_poses);
/* one member from host f64: state [lmd n + 10], cov [lmd n + 10, lmd n + 10] (symmetrised on upload); clears its status */
int ekf_batch_set_member(ekf_batch *b, int32_t member, const double *state, int32_t num_landmarks, const double *cov);
/* state[0:count] and, unless cov is NULL, the covariance [dims, dims] (dims = lmd n + 10) of one member; synchronises */
int ekf_batch_get_member(ekf_batch *b, int32_t member, double *state, int32_t count, double *cov /* or NULL */, int32_t dims);
int ekf_batch_num_landmarks(const ekf_batch *b, int32_t *out /* [B] */);
/* out [B]: 0, or EKF_ERR_NUMERIC for a member whose innovation covariance had a non-positive or non-finite pivot: that
 * member stopped at that frame (its update left state and covariance as they were, the frame's first sightings stay
 * added) and its remaining trajectory rows are NaN, until ekf_batch_reset or ekf_batch_set_member.  Synchronises. */
int ekf_batch_status(ekf_batch *b, int32_t *out /* [B] */);
int ekf_batch_log_workspace_bytes(const ekf_batch *b, int64_t detections, int64_t frames, size_t *bytes);
/* One log per member, in one call:
 *   lm_index [D]            HOST  landmark index of every detection, same rules as ekf_observe_log, per member
 *   frame_offsets [Ftot+1]  HOST  detection offsets, frame after frame, member after member
 *   member_frames [B+1]     HOST  frame offsets per member (equal entries: no log for that member)
 *   poses_dev [D,6]         DEVICE [tvec | rvec] as logged
 *   log_ws                  DEVICE 256-byte aligned, ekf_batch_log_workspace_bytes(D, Ftot)
 *   trajectory_dev [Ftot,7] DEVICE or NULL  state[0:7] after every frame
 * Everything is validated on the host before anything is enqueued (EKF_ERR_INVALID / EKF_ERR_CAPACITY; no member
 * changes).  Then, on the batch's stream, one copy of indices and offsets and one launch per window of 64 frames per
 * member (with EKF_FLAG_BATCH_WIDE_FRAMES: 64 / ceil(widest frame of the call / 16) frames, EKF_Rotations
 * 64 / ceil(widest / 8); where windows split does not change any result).  Returns once the work is enqueued; the
 * getters synchronise. */
int ekf_batch_observe_logs(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets, const int64_t *member_frames,
                           const double *poses_dev, void *log_ws, size_t log_ws_bytes, double *trajectory_dev);
/* ekf_batch_observe_logs with the filter's own statistics per frame, next to the trajectory rows (either may be NULL;
 * with both NULL this IS ekf_batch_observe_logs, to the bit):
 *   nis_dev [Ftot]              DEVICE  normalised innovation squared (z-h)^T S^-1 (z-h) = y^T y, y = L^-1 (z-h) the
 *                                       whitened residual, summed i = 0 .. k-1 in one fma chain; 0 for a frame without
 *                                       detections.  Its expected value is the frame's row count k = 3 m (EKF) or 7 m
 *                                       (EKF_MODEL_ROTATIONS, where the unit-quaternion rows make the chi^2 reading
 *                                       approximate).
 *   cam_cov_dev [Ftot,10,10]    DEVICE  P[0:10, 0:10] after every frame (repeated by a frame without detections).
 * A member's failing frame and every later one give NaN, as the trajectory rows. */
int ekf_batch_observe_logs_diag(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets,
                                const int64_t *member_frames, const double *poses_dev, void *log_ws, size_t log_ws_bytes,
                                double *trajectory_dev, double *nis_dev, double *cam_cov_dev);

/* ---- Monte-Carlo replicas of ONE log with detection noise generated on the device.
 * Noise definition (part of the ABI): replica r, detection d, pose component c < 6 ([tvec | rvec]) gets
 *     pose[d][c] + sigma[r][c] * g_c(seed, r, d)
 * where g_0 .. g_5 are standard normals from three Philox4x32-10 calls (Salmon et al., SC 2011, the published constants)
 * with key (seed_lo, seed_hi) = (seed & 0xffffffff, seed >> 32) and counter (d_lo, d_hi, r, j), j = 0, 1, 2: each call
 * gives words x0 .. x3, u_a = (((x0 << 32 | x1) >> 11) + 0.5) 2^-53 and u_b likewise from (x2, x3), then
 *     g_{2j} = sqrt(-2 ln u_a) cos(2 pi u_b),  g_{2j+1} = sqrt(-2 ln u_a) sin(2 pi u_b)
 * (f64 throughout; evaluated as pose + sigma * (sqrt(..) * cos(..))).  The noise of (r, d) depends on nothing else: not on
 * how many replicas a call holds nor on which replicas share it.  EKF reads only the tvec; EKF_MODEL_ROTATIONS reads both.
 * A first sighting is placed from its noisy pose (that pose is the detection).
 *
 * ekf_batch_replica_poses: out_dev [R, D, 6] = the poses replicas first_replica .. first_replica + R - 1 consume, from
 * poses_dev [D, 6] (DEVICE) and sigma [R, 6] (HOST, finite, >= 0), enqueued on `stream`; first_replica + R <= 2^32.
 * No handle: it is the code ekf_batch_observe_replicas runs. */
int ekf_batch_replica_poses(const double *poses_dev, int64_t detections, const double *sigma, int32_t replicas, uint64_t seed,
                            uint32_t first_replica, double *out_dev, void *stream);
/* bytes of the replica workspace for a log of `detections` and `frames`: B D (48 + 4) + B (F + 1) 8 bytes and change */
int ekf_batch_replica_workspace_bytes(const ekf_batch *b, int64_t detections, int64_t frames, size_t *bytes);
/* Member b replays the log as replica first_replica + b, with its own sigma[b] and noise constants:
 *   lm_index [D], frame_offsets [F+1]   HOST  the log, rules of ekf_batch_observe_logs, checked for every member
 *   poses_dev [D,6]                     DEVICE the log's poses
 *   sigma [B,6]                         HOST  finite, >= 0 (sigma = 0: exactly the log's poses)
 *   ws                                  DEVICE 256-byte aligned, ekf_batch_replica_workspace_bytes(D, F)
 *   trajectory_dev [B,F,7], nis_dev [B,F], cam_cov_dev [B,F,10,10]   DEVICE or NULL, as ekf_batch_observe_logs_diag
 * first_replica + B <= 2^32.  Everything is validated on the host before anything is enqueued (EKF_ERR_INVALID /
 * EKF_ERR_CAPACITY; no member changes).  Then, on the batch's stream: one copy of the log's indices and offsets tiled B
 * times (member b: frames b F .., detections b D ..), the noise kernel writing the B D noisy poses into ws, and the window
 * launches of ekf_batch_observe_logs: every member gives the bits of ekf_batch_observe_logs on the poses
 * ekf_batch_replica_poses returns for its replica.  Returns once the work is enqueued. */
int ekf_batch_observe_replicas(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets, int64_t frames,
                               const double *poses_dev, const double *sigma, uint64_t seed, uint32_t first_replica, void *ws,
                               size_t ws_bytes, double *trajectory_dev, double *nis_dev, double *cam_cov_dev);

/* ---- Per-detection chi-square gate (individual compatibility) and Mahalanobis distance output.
 * Semantics (part of the ABI).  Member b has a constant gate[b]: +inf, or no gate set, is off; otherwise finite and > 0.
 * For every detection d of a frame that would be stepped, AFTER the frame's first sightings are added and BEFORE anything
 * else of the frame (rd = 3: EKF, 7: EKF_MODEL_ROTATIONS):
 *   1. r_d = z_d - h_d(x);
 *   2. S_d = H_d (P+Q) H_d^T + r_uncertainty I  [rd, rd], with P the covariance the previous frame left plus this frame's
 *      first sightings: the diagonal block the joint S would have, independent of the other detections;
 *   3. S_d = L_d L_d^T and d^2_d = |L_d^-1 r_d|^2, by ONE device routine of fixed operation order (ascending fma chains):
 *      every window kernel gives the same bits for it;
 *   4. a detection that is the first occurrence of a landmark first sighted in this frame is exempt: d^2 = 0 is reported
 *      and it is never rejected (its z = h by construction);
 *   5. a detection is rejected iff every pivot of S_d was positive and finite and d^2 > gate[b]; after a failed pivot the
 *      detection is kept, its distance is NaN, and the joint factorisation fails as it does without a gate;
 *   6. the frame runs on the surviving detections, in log order: state, P, landmark count, trajectory, nis and cam_cov are
 *      bit for bit those of replaying, with the gate off, the log from which the rejected detections have been deleted
 *      (with EKF_FLAG_BATCH_WIDE_FRAMES the blocks of 16 / 8 detections are formed from the survivors).  A frame with no
 *      survivor is not stepped (no predict, its rows repeat, nis = 0), exactly like a frame without detections;
 *   7. nis is over the survivors: its degrees of freedom are rd times their number.
 * chi^2 quantiles users want for gate: 3 dof (EKF) 7.815 (95 %), 11.345 (99 %), 16.266 (99.9 %); 7 dof
 * (EKF_MODEL_ROTATIONS, approximate: the unit-quaternion rows are not independent) 14.067, 18.475, 24.322.
 *
 * ekf_batch_set_gate: gate [B] HOST, or NULL = no gate.  Persistent like ekf_batch_set_noise and honoured by every
 * observe call of the batch; NaN, <= 0 or -inf gives EKF_ERR_INVALID and nothing changes.  While a gate is set the log and
 * replica workspaces hold the B gates too (8 B bytes and change more): size them after setting the gate.
 * The ..._gated calls are ekf_batch_observe_logs_diag / ekf_batch_observe_replicas with one more nullable output:
 *   mahal_dev [D] (logs) or [B,D] (replicas)  DEVICE  d^2 of every tested detection, indexed like lm_index; 0 for an exempt
 *       detection; NaN after a failed pivot, for every frame AFTER a member's failing frame (the failing frame keeps the
 *       values that were computed) and for frames not stepped for other reasons.  It may be requested with the gate off:
 *       the distances are reported and nothing is rejected.  rejected = mahal > gate[b].
 * With no gate set and mahal_dev NULL they are the calls above, to the bit. */
int ekf_batch_set_gate(ekf_batch *b, const double *gate /* [B] or NULL */);
int ekf_batch_observe_logs_gated(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets,
                                 const int64_t *member_frames, const double *poses_dev, void *log_ws, size_t log_ws_bytes,
                                 double *trajectory_dev, double *nis_dev, double *cam_cov_dev, double *mahal_dev);
int ekf_batch_observe_replicas_gated(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets, int64_t frames,
                                     const double *poses_dev, const double *sigma, uint64_t seed, uint32_t first_replica,
                                     void *ws, size_t ws_bytes, double *trajectory_dev, double *nis_dev,
                                     double *cam_cov_dev, double *mahal_dev);

/* ---- Monte-Carlo replicas with the noise on the marker corners, in pixels, where the detector has it: IPPE turns it into
 * what pose noise never gives (a depth error that grows with distance, an error that depends on the marker's tilt, and now
 * and then the other of its two solutions), and every such flip is labelled.
 * Noise and flip definition (part of the ABI).  Replica r, detection d, corner i = 0 .. 3 (the detector's order, as
 * ekf_estimate_poses takes them):
 *     noisy[r][d][i] = corners[d][i] + sigma_px[r] * (g_u, g_v)        in pixels, before undistortion
 * with (g_u, g_v) = (sqrt(-2 ln u_a) cos(2 pi u_b), sqrt(-2 ln u_a) sin(2 pi u_b)) from ONE Philox4x32-10 call with key
 * (seed_lo, seed_hi) and counter (d_lo, d_hi, r, 4 + i), u_a / u_b from its words exactly as for the pose noise above
 * (evaluated as corner + sigma_px * (sqrt(..) * cos(..))).  Counter words 4 .. 7 keep this stream disjoint from the pose
 * stream (words 0 .. 2).  The noise of (r, d) depends on nothing else: not on how many replicas a call holds nor on which
 * replicas share it.
 * The pose of (r, d) is IPPE-square of the noisy corners, the steps of ekf_estimate_poses by the same device code:
 * sigma_px = 0 gives the bits of ekf_estimate_poses on the corners as logged.
 * flipped[r][d] is defined with three rotations: R_clean, the rotation IPPE returns for the corners as logged; R_a, the
 * returned candidate (the smaller reprojection error) for the noisy corners; R_b, the other candidate for the noisy corners:
 *     flipped = trace(R_a R_clean^T) < trace(R_b R_clean^T),
 * the rejected candidate was the one nearer to the clean pose.
 *
 * ekf_batch_replica_corners: what replicas first_replica .. first_replica + R - 1 consume, from corners_dev [D,4,2] (DEVICE,
 * pixels) and sigma_px [R] (HOST, finite, >= 0), enqueued on `stream`; first_replica + R <= 2^32; marker_size > 0; camera
 * arguments as ekf_estimate_poses (n_dist <= 8).  Outputs, each DEVICE or NULL: poses_dev [R,D,6] = [tvec | rvec],
 * flipped_dev [R,D] bytes (0 / 1), noisy_corners_dev [R,D,4,2].  R = 0 does nothing.  No handle: it is the code
 * ekf_batch_observe_corner_replicas runs.  Corners noisy enough to give a degenerate quadrilateral give the non-finite
 * poses ekf_estimate_poses would give. */
int ekf_batch_replica_corners(const double *corners_dev, int64_t detections, const double *sigma_px, int32_t replicas,
                              uint64_t seed, uint32_t first_replica, double marker_size, const double camera_matrix[9],
                              const double *dist_coeffs, int32_t n_dist, double *poses_dev, uint8_t *flipped_dev,
                              double *noisy_corners_dev, void *stream);
/* ekf_batch_observe_replicas_gated on a log of corners: member b replays the log as replica first_replica + b with its own
 * sigma_px[b] (HOST [B]); corners_dev [D,4,2] DEVICE; ws as ekf_batch_replica_workspace_bytes(D, F), unchanged: the poses
 * the kernel estimates take the place of the noisy poses.  Outputs as there, and flipped_dev [B,D] bytes DEVICE or NULL,
 * indexed like lm_index.  Everything, the noise and camera arguments included, is validated on the host before anything is
 * enqueued; a gate that is set acts as in every observe call.  Every member gives the bits of ekf_batch_observe_logs_gated
 * on the poses ekf_batch_replica_corners returns for its replica. */
int ekf_batch_observe_corner_replicas(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets, int64_t frames,
                                      const double *corners_dev, const double *sigma_px, uint64_t seed,
                                      uint32_t first_replica, double marker_size, const double camera_matrix[9],
                                      const double *dist_coeffs, int32_t n_dist, void *ws, size_t ws_bytes,
                                      double *trajectory_dev, double *nis_dev, double *cam_cov_dev, double *mahal_dev,
                                      uint8_t *flipped_dev);

/* ---- The same gate for the single filter (ekf_config.flags bit 6, EKF_FLAG_GATE).  Without the flag ekf_set_gate,
 * ekf_observe_gated and ekf_observe_log_gated with mahal_dev given return EKF_ERR_STATE; ekf_observe_log_gated with
 * mahal_dev NULL is ekf_observe_log, and ekf_last_gate_stats reports 0 / 0.
 * Semantics: rules 1 - 7 of "Per-detection chi-square gate" above, with "member" read as "filter" and the one constant
 * gate of the handle: per detection S_d = H_d (P+Q) H_d^T + r_uncertainty I from the (10 + lmd)^2 support block of the
 * prior P, d^2 = |L_d^-1 r_d|^2; a detection is rejected iff every pivot was positive and finite and d^2 > gate; after a
 * failed pivot the detection is kept, its distance is NaN and the frame fails as it does without a gate
 * (EKF_ERR_NUMERIC at the next synchronising call); the frame runs on the survivors in log order; a frame with no survivor
 * is not stepped (no predict; its trajectory row repeats); an exempt detection reports d^2 = 0 and is never rejected.
 * Once the filter carries a sticky error, nothing is tested any more: the distances are NaN and every detection stays.
 * State, P, landmark count and trajectory of a gated frame are bit for bit those of the same call on the frame with the
 * rejected detections deleted, at every map size, either covariance dtype (all gate arithmetic is f64: an f32 P is widened
 * on load) and every frame width: one kernel (ekf_gate.hip) in front of everything else of the frame tests the detections
 * and compacts the survivors, the host waits for their number, and the frame's ordinary kernels run on them.  A gated
 * frame therefore costs one host round trip, and gated sequence and log calls run frame by frame in serial order
 * (ekf_last_sequence_mode: EKF_SEQ_SERIAL; ekf_last_log_stats: 0 pipelined frames).
 *
 * ekf_set_gate: +inf is off, the state after ekf_create; NaN, <= 0 or -inf gives EKF_ERR_INVALID and nothing changes.  The
 *   gate is persistent: ekf_reset and ekf_grow keep it.  ekf_observe, ekf_observe_device and
 *   ekf_observe_sequence_device honour a set gate, with no exemptions; ekf_observe_log too, with those below.
 * ekf_observe_gated: ekf_observe (host pointers) with exempt [m] bytes or NULL (non-zero: exempt; BaseFilter.observe passes
 *   the markers it has just added), mahal [m] or NULL (d^2 of every detection) and survivors or NULL (how many stayed).
 *   With the gate off and mahal requested, the distances are reported and nothing is rejected.
 * ekf_observe_log_gated: ekf_observe_log with mahal_dev [D] DEVICE or NULL, indexed like lm_index.  The first occurrence
 *   of a landmark first sighted in its frame is exempt (rule 4; decided on the host).  mahal_dev: 0 for an exempt
 *   detection, NaN after a failed pivot and for every frame after the failing one; a frame whose detections were all
 *   rejected keeps their distances.  With the gate off and mahal_dev NULL it IS ekf_observe_log, to the bit, pipelined runs
 *   included.
 * ekf_last_gate_stats: out[0] detections tested (exempt ones not counted), out[1] detections rejected by the last observe
 *   call of any kind. */
int ekf_set_gate(ekf_filter *f, double gate);
int ekf_observe_gated(ekf_filter *f, const int32_t *lm_index, const double *z, int32_t m, const uint8_t *exempt /* [m] or NULL */,
                      double *mahal /* [m] host or NULL */, int32_t *survivors /* or NULL */);
int ekf_observe_log_gated(ekf_filter *f, const int32_t *lm_index, const int64_t *offsets, int32_t frames,
                          const double *poses_dev, void *log_ws, size_t log_ws_bytes, double *trajectory_dev,
                          double *mahal_dev /* [D] or NULL */);
int ekf_last_gate_stats(const ekf_filter *f, int64_t out[2]);

/* ---- Per-detection measurement noise (heteroscedastic R; ekf_config.flags bit 7, EKF_FLAG_ROW_NOISE for the single filter;
 * a batch needs no flag).  Every update forms S = H (P+Q) H^T + r_uncertainty I.  With rows it forms
 *     S = H (P+Q) H^T + diag(rows)
 * Semantics (part of the ABI):
 *   1. Detection d of a frame may carry rows[d][0 .. rd-1], the variances of its rd measurement rows in the order of z:
 *      x y z in the camera frame (EKF, rd = 3), then qw qx qy qz (EKF_MODEL_ROTATIONS, rd = 7).  Nothing else of the frame
 *      changes.  The per-detection S_d of the gate (rule 2 there) uses the same rows.
 *   2. Rows are data of the frame, like z; they are not state of the handle.  rows = NULL is the call without rows: the same
 *      code path, the same bits.  First sightings are added as before (initial_landmark_uncertainty).
 *   3. Rows all equal to c, whatever the filter's r_uncertainty, give bit for bit the plain call on a filter configured with
 *      r_uncertainty = c: state, P, trajectory and d^2; every path, model and covariance dtype.
 *   4. Gate and rows compose: a gated frame with rows is bit for bit the ungated call on the survivors with the survivors'
 *      rows (the gate kernel compacts the rows together with lm_index and z).
 *   5. Host-pointer entry points reject a row that is NaN, Inf or <= 0 with EKF_ERR_INVALID before anything is enqueued.
 *      Device arrays are the caller's contract: an S they make non-positive-definite fails as without rows
 *      (EKF_ERR_NUMERIC, sticky).
 *   6. Every rule of the calls they extend holds with rows present: the EKF log replay is bitwise the per-frame loop, the
 *      pipelined sequence is bitwise the serial order, batch large-map and wide-frame kernels are bitwise the one-column
 *      kernel where both run.
 * rows given to a filter created without EKF_FLAG_ROW_NOISE: EKF_ERR_STATE.
 * ekf_observe_rows: ekf_observe_gated with rows [m, rd] HOST or NULL.  Usable without EKF_FLAG_GATE when exempt and mahal
 *   are NULL (survivors, if given, is then m).
 * ekf_observe_sequence_device_rows: ekf_observe_sequence_device with rows_dev [frames, m, rd] DEVICE or NULL; pipelined
 *   where that call would be.
 * ekf_observe_log_rows: ekf_observe_log_gated with rows_dev [D, rd] DEVICE or NULL, indexed like lm_index; with no gate set
 *   and mahal_dev NULL the runs pipeline as ekf_observe_log plans them.
 * ekf_batch_observe_logs_rows: ekf_batch_observe_logs_gated with rows_dev [D, rd] DEVICE or NULL, indexed like lm_index;
 *   valid for the one-column, large-map and wide-frame kernels; nis, cam_cov and mahal stay available.  The batch workspace
 *   does not change, so a batch takes rows without a flag.
 * The replica entry points (ekf_batch_observe_replicas*, ekf_batch_observe_corner_replicas) keep the constant
 * r_uncertainty of their members. */
int ekf_observe_rows(ekf_filter *f, const int32_t *lm_index, const double *z, const double *rows /* [m, rd] host or NULL */,
                     int32_t m, const uint8_t *exempt /* [m] or NULL */, double *mahal /* [m] host or NULL */,
                     int32_t *survivors /* or NULL */);
int ekf_observe_sequence_device_rows(ekf_filter *f, const int32_t *lm_index_dev, const double *z_dev,
                                     const double *rows_dev /* [frames, m, rd] or NULL */, int32_t m, int32_t frames,
                                     double *trajectory_dev);
int ekf_observe_log_rows(ekf_filter *f, const int32_t *lm_index, const int64_t *offsets, int32_t frames,
                         const double *poses_dev, const double *rows_dev /* [D, rd] or NULL */, void *log_ws,
                         size_t log_ws_bytes, double *trajectory_dev, double *mahal_dev /* [D] or NULL */);
int ekf_batch_observe_logs_rows(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets,
                                const int64_t *member_frames, const double *poses_dev,
                                const double *rows_dev /* [D, rd] or NULL */, void *log_ws, size_t log_ws_bytes,
                                double *trajectory_dev, double *nis_dev, double *cam_cov_dev, double *mahal_dev);

/* ---- Landmark removal (map pruning).  Deleting landmarks from a Gaussian is marginalisation: their rows and columns of P
 * and their entries of the state go, nothing else changes.  The calling pattern is that of ekf_grow at unchanged capacity:
 * the caller hands in a second covariance and a second state buffer of the sizes ekf_query_sizes gives for the filter's own
 * configuration (which are what they were), the library gathers what is kept into them on the handle's stream (one launch)
 * and borrows them from then on; the old ones may be freed once the stream has passed the call.  remove_ws: caller-owned
 * device scratch for the index map, 256-byte aligned, ekf_remove_workspace_bytes(count); valid until the stream has passed
 * the call.
 * Semantics (part of the ABI):
 *   1. lm_index [count] HOST holds distinct indices in [0, num_landmarks), in any order.  A duplicate, an index out of
 *      range, a negative count, a NULL or misaligned buffer, a new buffer that is the current one, or a wrong ld returns
 *      EKF_ERR_INVALID; a remove_ws smaller than ekf_remove_workspace_bytes returns EKF_ERR_CAPACITY; both before anything
 *      is enqueued: the filter, its buffers and its bindings are untouched.  count == 0 returns EKF_OK and does nothing: no
 *      rebinding, the new buffers are not written.
 *   2. Kept landmarks keep their relative order: new index = old index - (number of removed indices below it);
 *      num_landmarks drops by count.  Removing every landmark leaves the camera block (state[0:10], P[0:10, 0:10]).
 *   3. The whole new covariance buffer [ld, ld] and the whole new state buffer are written: the kept N' x N' block and N'
 *      state entries (N' = lmd (n - count) + 10) are bit for bit the old values, everything else is exactly zero (the
 *      capacity padding every update kernel relies on).  The result is bit for bit the filter ekf_set_state + ekf_set_cov
 *      build from the host arrays with those rows and columns deleted (P is bitwise symmetric, so the upload's
 *      (P + P^T) / 2 is the identity on it), either model, either covariance dtype, and every later call of any kind
 *      continues bit for bit as on that twin.
 *   4. Pure data movement, enqueued on the handle's stream.  The call does not wait for the device's work: the only host
 *      wait it can make is for its own staging, the index map goes through two pinned buffers used by turns, so a call
 *      waits for the upload of the removal before the previous one and for nothing else.  The sticky status word, the gate,
 *      the noise constants and the sequence-mode state stay as they are; NaNs of a failed filter move like any other value.
 *      The pinned host mirror of the state is refreshed by the launch, so a getter after the call returns the new state.
 * ekf_batch_remove_markers: the same per member, ragged like the log calls: member b removes
 * lm_index[offsets[b] : offsets[b + 1]] (offsets [B+1] HOST, offsets[0] = 0, non-decreasing), checked against the landmark
 * counts the library reads back from the device first (this call waits for the batch's stream, as every batch call does).
 * Members with an empty list are copied unchanged; no list at all (offsets[B] == 0) does nothing.  cov_dev_new [B, ld, ld],
 * state_dev_new [B, ld] as ekf_batch_query_sizes sizes them; the launch also stores the new landmark counts on the device;
 * a member's status stays.  One-column, large-map and wide-frame batches alike. */
int ekf_remove_workspace_bytes(const ekf_filter *f, int32_t count, size_t *bytes);
int ekf_remove_markers(ekf_filter *f, const int32_t *lm_index /* [count] HOST */, int32_t count, void *cov_dev_new, int64_t ld,
                       double *state_dev_new, void *remove_ws, size_t remove_ws_bytes);
int ekf_batch_remove_workspace_bytes(const ekf_batch *b, int64_t total, size_t *bytes);
int ekf_batch_remove_markers(ekf_batch *b, const int32_t *lm_index /* [total] HOST */, const int64_t *offsets /* [B+1] HOST */,
                             double *cov_dev_new, int64_t ld, double *state_dev_new, void *remove_ws, size_t remove_ws_bytes);

/* ---- Per-frame process-noise scale (time-aware predict; ekf_config.flags bit 8, EKF_FLAG_FRAME_SCALE, single filter and
 * batch).  Every update steps the covariance with P + Q, Q = diag(q_cam, 0 (quaternion), q_err, q_lm ...).  With a scale the
 * frame's Q is multiplied by the time that has passed, in units the caller chooses (frames of a nominal rate, say), and time
 * that passes without an update is kept and added to the next update.
 * Semantics (part of the ABI):
 *   1. A frame may carry a scale s (f64, finite, >= 0).  It is data of the frame, like z and the rows, not a noise constant.
 *      A frame WITHOUT a scale (the calls that take none; scale = NULL in those that do) is the frame as it ever was:
 *      stepped, it runs with s_eff = p + 1 (and p = 0 afterwards); not stepped, it leaves p alone.
 *   2. The filter (every member of a batch) carries one more number, the pending scale p: f64, >= 0, 0 after create and
 *      after reset.
 *   3. A frame that is STEPPED runs with s_eff = p + s (one f64 addition) and
 *          Q_eff = diag(fl(s_eff q_cam), 0 (quaternion), fl(s_eff q_err), fl(s_eff q_lm) ...),
 *      every entry one f64 multiplication, rounded before it is added to anything.  Q_eff is used wherever the frame uses Q:
 *      the gate's S_d, A = H (P+Q), S, and the diagonal of the covariance update.  After the frame p = 0.
 *   4. A frame that is NOT stepped (no detections, or no detection survived the gate) sets p = p + s and changes nothing
 *      else: its trajectory row repeats, its nis is 0, its distances are reported as ever.  A failed filter or a failed
 *      member ignores scales, as it ignores everything.
 *   5. Bit rules.  (a) No scale given (p = 0), or every scale exactly 1.0 with no frame that is not stepped, is bit for bit
 *      the call without scales.  (b) A stepped frame with s_eff is bit for bit the plain frame on a filter configured with
 *      (fl(s_eff q_cam), fl(s_eff q_err), fl(s_eff q_lm)): state, P, trajectory, d^2 and nis.  (c) A log is bit for bit the
 *      log with its frames that are not stepped deleted and their scales folded into the next stepped frame by rule 3's
 *      addition, in log order.  (d) Rule 6 of the gate and rules 3, 4 and 6 of the per-detection noise hold unchanged with
 *      scales present.  (e) With scales present the log replay is bitwise the per-frame loop, the pipelined sequence is
 *      bitwise the serial order, and the batch large-map and wide-frame kernels are bitwise the one-column kernel where
 *      both run.
 *   6. s = 0 is legal: that frame adds no process noise.  First sightings are added as before (initial_landmark_uncertainty)
 *      and, under rule 3, see the whole s_eff on their diagonal like every other state dimension.
 *   7. The covariance getters return P of the last stepped frame; p is reported separately (ekf_get_pending_scale).
 * Without EKF_FLAG_FRAME_SCALE a call that is given a scale returns EKF_ERR_STATE (ekf_get_pending_scale reports 0); a scale
 * that is NaN, Inf or negative gives EKF_ERR_INVALID; both before anything is enqueued.
 * Single filter: the scales are HOST data and p is kept on the host, which launches every frame and already plans empty
 * frames and the gate's round trips.  ekf_reset and ekf_set_state zero p; ekf_grow and ekf_remove_markers keep it.
 *   ekf_advance: rule 4 with no frame (time passes, nothing is observed): p = p + scale.
 *   ekf_observe_scaled: ekf_observe_rows with the frame's scale.
 *   ekf_observe_sequence_device_scaled: ekf_observe_sequence_device_rows with scale [frames] HOST or NULL; pipelined where
 *     that call would be (the front kernel of frame t+1 completes its rows of P_{t+1} with frame t's Q_eff and predicts with
 *     its own).
 *   ekf_observe_log_scaled: ekf_observe_log_rows with scale [F] HOST or NULL, one entry per frame, empty frames included.
 * Batch: the flag gives every member a pending scale on the device ([B] doubles in the batch workspace), loaded by a window
 * kernel at its start and stored at its end.  ekf_batch_reset zeroes it (of the members it resets), ekf_batch_set_member
 * zeroes the member's, ekf_batch_remove_markers keeps it.
 *   ekf_batch_observe_logs_scaled: ekf_batch_observe_logs_rows with scale_dev [Ftot] DEVICE or NULL, indexed like the frames
 *     (frame_offsets); the caller's contract, like rows_dev: finite and >= 0.  The kernels form fl(s_eff q) with an explicitly
 *     rounded multiply once per frame.
 *   ekf_batch_get_pending_scale / ekf_batch_set_pending_scale: member = -1: every member, [B]; member >= 0: that one, [1].
 *     Both synchronise.
 * The replica entry points keep scale 1, as they keep the constant r_uncertainty (a member's pending scale goes into its
 * first stepped frame, by rule 1). */
int ekf_advance(ekf_filter *f, double scale);
int ekf_get_pending_scale(const ekf_filter *f, double *out);
int ekf_set_pending_scale(ekf_filter *f, double pending);
int ekf_observe_scaled(ekf_filter *f, const int32_t *lm_index, const double *z, const double *rows /* [m, rd] host or NULL */,
                       int32_t m, const uint8_t *exempt /* [m] or NULL */, double *mahal /* [m] host or NULL */,
                       int32_t *survivors /* or NULL */, double scale);
int ekf_observe_sequence_device_scaled(ekf_filter *f, const int32_t *lm_index_dev, const double *z_dev,
                                       const double *rows_dev /* [frames, m, rd] or NULL */,
                                       const double *scale /* [frames] HOST or NULL */, int32_t m, int32_t frames,
                                       double *trajectory_dev);
int ekf_observe_log_scaled(ekf_filter *f, const int32_t *lm_index, const int64_t *offsets, int32_t frames,
                           const double *poses_dev, const double *rows_dev /* [D, rd] or NULL */,
                           const double *scale /* [F] HOST or NULL */, void *log_ws, size_t log_ws_bytes,
                           double *trajectory_dev, double *mahal_dev /* [D] or NULL */);
int ekf_batch_observe_logs_scaled(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets,
                                  const int64_t *member_frames, const double *poses_dev,
                                  const double *rows_dev /* [D, rd] or NULL */, const double *scale_dev /* [Ftot] or NULL */,
                                  void *log_ws, size_t log_ws_bytes, double *trajectory_dev, double *nis_dev,
                                  double *cam_cov_dev, double *mahal_dev);
int ekf_batch_get_pending_scale(ekf_batch *b, int32_t member, double *out);
int ekf_batch_set_pending_scale(ekf_batch *b, int32_t member, const double *pending);

/* ---- Odometry input: per-frame camera motion in the predict step (ekf_config.flags bit 9, EKF_FLAG_MOTION; single filter
 * and batch).  Every update predicts with a camera that stands still, x_{t+1|t} = x_t; with the reference's noise constants
 * the gain on the camera is small, and a moving camera is tracked with a lag that grows with its speed.  A motion makes the
 * camera's movement between two frames data of the frame: wheel or visual odometry, an IMU pre-integration, a commanded
 * motion.
 * Semantics (part of the ABI):
 *   1. A frame may carry a motion u = (d, w): six f64, d a translation and w a rotation vector (radians), both expressed in
 *      the camera frame of the previous pose.  It is data of the frame, not state of the handle.
 *   2. State.  R(q) is the normalised rotation matrix of the scalar-first quaternion q = state[3:7], the camera-to-map
 *      rotation of the measurement model h = R(q)^T (l - c), whatever ekf_config.quat_mode says about the injection.
 *      delta = (cos(|w|/2), sin(|w|/2) w/|w|), and delta = (1, 0, 0, 0) exactly when w = 0.  The move is c' = c + R(q) d, then
 *      q' = q (x) delta (Hamilton product; then normalised, q' / |q'|, as the injection normalises its product; with w = 0
 *      q' = q, bit for bit).  The error state stays 0 and the landmarks are untouched.
 *   3. Covariance.  P <- F~ P F~^T, F~ = diag(F, I), F the 10 x 10 Jacobian of (c, q, e) -> (c + R((1,e) (x) q) d, q (x) delta, e)
 *      at e = 0 in the state's column order [c q e]:
 *          F = [ I   G      G E(q) ]      G    = d(R(q) d)/dq  (3 x 4, R normalised)
 *              [ 0   Rm(d)  0      ]      E(q) = d((1,e) (x) q)/de at 0  (4 x 3)
 *              [ 0   0      I      ]      Rm(delta): a (x) delta = Rm(delta) a
 *      Only rows and columns 0 .. 9 of P change.  All arithmetic is f64, every sum one ascending fma chain (the order is
 *      stated in csrc/ekf_motion_device.h); an f32 P is widened on load and rounded once on store.  P stays bitwise
 *      symmetric (one triangle of the 10 x 10 block is computed and mirrored; every strip entry and its mirror are stores of
 *      the same value), nothing at or beyond N is written, and the capacity padding stays exactly zero.
 *   4. Order inside a frame: the motion first, then first sightings (placed from the moved camera), then the gate (on the
 *      moved prior), then predict and update with Q_eff as ever.  A frame that is not stepped (no detections, or none
 *      survived the gate) is still moved: its trajectory row is the moved pose.  The pending scale is untouched by a motion.
 *   5. A failed filter ignores motions, as it ignores everything.
 *   6. Bit rules.  (a) motion = NULL, or a motion whose six numbers are all exactly 0, is the call without it: nothing is
 *      enqueued for it, the same bits.  (b) ekf_observe_moved(..., u) is ekf_move(u) followed by ekf_observe_scaled(...).
 *      (c) A log replay is the per-frame loop, and a sequence call is the loop (EKF_Rotations: as without motions, a log
 *      replay forms z from the logged poses on the device, so it is bit for bit the loop that is fed the same z, and
 *      agrees with a loop whose z was formed on the host to rounding).  (d) The batch large-map and wide-frame kernels are
 *      bit for bit the one-column kernel where both run.  (e) With w = 0 the quaternion and its four
 *      rows and columns of P are unchanged bit for bit, apart from the G terms in the position rows and columns.  (f) Gate,
 *      rows and scales compose: a gated frame with a motion is bit for bit the ungated call with the same motion on the
 *      survivors, and rule 5(b) of the frame scale holds on a moved frame.
 *   7. The host-pointer entry points reject a NaN or Inf motion with EKF_ERR_INVALID and a motion given to a handle without
 *      the flag with EKF_ERR_STATE, both before anything is enqueued.
 * The flag changes no size and no layout: a motion travels in the kernel arguments.
 *   ekf_move: the motion alone (rules 2 and 3), on the handle's stream; a state getter that follows returns the moved pose.
 *   ekf_observe_moved: ekf_observe_scaled with the frame's motion [6] HOST or NULL.  Like ekf_observe_scaled it always
 *     carries a scale, so the handle needs EKF_FLAG_FRAME_SCALE as well (EKF_ERR_STATE otherwise); a handle with
 *     EKF_FLAG_MOTION alone calls ekf_move and then the observe call of its choice, which rule 6(b) makes the same thing.
 *     The frame's landmarks are in the map
 *     already; a caller with first sightings calls ekf_move, ekf_add_markers and then an observe call (rule 4).
 *   ekf_observe_sequence_device_moved: ekf_observe_sequence_device_scaled with motion [frames, 6] HOST or NULL.
 *   ekf_observe_log_moved: ekf_observe_log_scaled with motion [F, 6] HOST or NULL, one row per frame, empty frames included.
 * A pipelined run completes P_{t+1} from P_t and W_t inside the next front kernel, which a motion between the two frames
 * invalidates: a sequence or log call that is given a motion array (not NULL) runs its frames in serial order, reports
 * EKF_SEQ_SERIAL, and ekf_last_log_stats reports 0 pipelined frames, as gated calls do.  A call without one pipelines as ever.
 * Batch: a motion stage at the top of the frame in all three window kernels runs the same stage functions on the member's
 * P; an empty frame with a motion moves the member and its trajectory row, a failed member ignores motions.  The flag
 * changes no size.
 *   ekf_batch_observe_logs_moved: ekf_batch_observe_logs_scaled with motion_dev [Ftot, 6] DEVICE or NULL, indexed like the
 *     frames (frame_offsets); the caller's contract, like rows_dev and scale_dev: finite.  Without the flag: EKF_ERR_STATE.
 * The replica entry points take no motion, as they take no rows and no scales. */
int ekf_move(ekf_filter *f, const double motion[6]);
int ekf_observe_moved(ekf_filter *f, const int32_t *lm_index, const double *z, const double *rows /* [m, rd] host or NULL */,
                      int32_t m, const uint8_t *exempt /* [m] or NULL */, double *mahal /* [m] host or NULL */,
                      int32_t *survivors /* or NULL */, double scale, const double *motion /* [6] HOST or NULL */);
int ekf_observe_sequence_device_moved(ekf_filter *f, const int32_t *lm_index_dev, const double *z_dev,
                                      const double *rows_dev /* [frames, m, rd] or NULL */,
                                      const double *scale /* [frames] HOST or NULL */,
                                      const double *motion /* [frames, 6] HOST or NULL */, int32_t m, int32_t frames,
                                      double *trajectory_dev);
int ekf_observe_log_moved(ekf_filter *f, const int32_t *lm_index, const int64_t *offsets, int32_t frames,
                          const double *poses_dev, const double *rows_dev /* [D, rd] or NULL */,
                          const double *scale /* [F] HOST or NULL */, const double *motion /* [F, 6] HOST or NULL */,
                          void *log_ws, size_t log_ws_bytes, double *trajectory_dev, double *mahal_dev /* [D] or NULL */);
int ekf_batch_observe_logs_moved(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets,
                                 const int64_t *member_frames, const double *poses_dev,
                                 const double *rows_dev /* [D, rd] or NULL */, const double *scale_dev /* [Ftot] or NULL */,
                                 const double *motion_dev /* [Ftot, 6] or NULL */, void *log_ws, size_t log_ws_bytes,
                                 double *trajectory_dev, double *nis_dev, double *cam_cov_dev, double *mahal_dev);

/* ---- Localisation mode: a frozen map, Schmidt-Kalman ("consider") update of the camera (the single filter here; the members
 * of a batch: "Localisation mode of a batch" below).  A filter can build
 * a map, restore one (ekf_set_state / ekf_set_cov, ekf_add_markers with the stored variances), prune it and gate against it;
 * frozen, it uses the map without changing it.  The landmarks stay in the state and in S as uncertain quantities, but
 * their gain rows are zero: the camera state, P_cc and the cross-covariances P_cl are updated, the landmark state and P_ll
 * are not, and P stays a valid joint covariance, so the filter can be unfrozen and go on mapping.
 * With W = L^-1 H (P+Q) the Schmidt update of the camera rows is the arithmetic the full update runs on rows 0 .. 9, and
 * the rest of the full update is not done: a frozen frame writes about 2 * 10 * N elements of P instead of N^2.
 * Semantics (part of the ABI).  A filter has a persistent boolean, "map frozen", off after ekf_create.  While it is on:
 *   1. The frame sees exactly the prior a mapping frame sees: the motion first, then the gate on P+Q, then A = H (P+Q), S,
 *      L, y, W with the frame's Q_eff, rows and scale.  Everything up to and including W and dx has the bits of the mapping
 *      frame.
 *   2. State.  Only the camera is injected: dx[0:3], the quaternion rule on dx[7:10] and state[7:10] = 0, as ever, in either
 *      quaternion mode; EKF_MODEL_ROTATIONS: block 0 of the injection only.  state[10:] keeps its bits, and so does the
 *      pinned host mirror of it.
 *   3. Covariance.  For r < 10 and every c < N, P[r][c] and P[c][r] get the value the full update gives that element: the
 *      same dtype, the same k-ascending fma chain from zero over kpad rows, v = P (+ Q on the diagonal) and then v + acc.  A
 *      frame beyond 384 rows runs the same row chunks in the same order, Q with the first chunk only.  P[10:N, 10:N] is
 *      neither predicted (no Q_lm is added) nor downdated: it keeps its bits.  The capacity padding stays exactly zero.  The
 *      update is in place on the current buffer.  q_lm therefore acts as a per-frame inflation of the map's uncertainty
 *      inside S and inside the gate that does not accumulate: every frozen frame sees P_ll + Q_lm, and none stores it.
 *   4. A frozen filter adds nothing through observation: an entry point that would add landmarks as part of an observe
 *      call -- ekf_observe_log* with first-sighting slots -- returns EKF_ERR_STATE before anything is enqueued.  Explicit
 *      ekf_add_markers, ekf_remove_markers, ekf_set_state, ekf_set_cov and ekf_grow work as ever and keep the flag.
 *      ekf_reset clears it: a reset filter has no map.
 *   5. A frozen frame that is not stepped (empty, or nothing survived the gate) behaves as an unstepped frame does: it is
 *      still moved, and its scale goes to the pending scale.  Gate, rows, scale and motion compose exactly as for mapping
 *      frames: a gated frozen frame is bit for bit the ungated frozen frame on the survivors.
 *   6. Run order.  Frozen sequence and log calls run frame by frame in serial order: ekf_last_sequence_mode reports
 *      EKF_SEQ_SERIAL (1) and ekf_last_log_stats 0 pipelined frames, as for gated and moved calls.  A filter that is not
 *      frozen runs the kernels and the pipelined mode it ran before, to the bit.
 *   7. Unfreezing.  Mapping continues from the state and P the frozen frames left, bit for bit like a filter that
 *      ekf_set_state / ekf_set_cov restore from those arrays.
 * No config flag, no size and no layout change: the flag travels in the kernel arguments.
 *   ekf_set_map_frozen: frozen != 0 freezes, 0 unfreezes, from the next frame on (a bound, reset filter).
 *   ekf_get_map_frozen: 1 / 0, or EKF_ERR_INVALID for a NULL handle. */
int ekf_set_map_frozen(ekf_filter *f, int32_t frozen);
int ekf_get_map_frozen(const ekf_filter *f);

/* ---- Localisation mode of a batch: per-member frozen maps.  Every member of an ekf_batch has its own persistent boolean
 * "map frozen": off after ekf_batch_create; ekf_batch_reset clears it for the members it resets; ekf_batch_set_member,
 * ekf_batch_remove_markers, ekf_batch_set_gate, ekf_batch_set_noise and ekf_batch_set_pending_scale keep it.  No config flag.
 * A frozen member's frame follows rules 1, 2, 3 and 5 above with the batch's arithmetic:
 *   - the motion, the first-sighting check, the gate on P+Q, A, S, L, y, W, dx[0:10] and the per-frame outputs (trajectory
 *     row, NIS, dof, cam_cov, mahal) have the bits of the member's mapping frame from the same prior;
 *   - only the camera is injected (EKF: dx[0:3], the quaternion rule, state[7:10] = 0; EKF_MODEL_ROTATIONS: block 0);
 *   - for r < 10 and every c < N, P[r][c] and P[c][r] get the value the member's mapping frame gives that element (the same
 *     l-ascending fma chain from zero, then (P + Q on the diagonal) - acc; in the HBM-resident kernel one pass per block of
 *     detections in block order, Q in the first pass); state[10:] and P[10:N, 10:N] keep their bits, the padding stays
 *     zero and P stays bitwise symmetric;
 *   - a frame that is not stepped is still moved and leaves its scale pending; a frame whose pivot fails leaves state and P
 *     as it found them and sets the member's status (EKF_ERR_NUMERIC), as for a mapping member.
 * A frozen member adds nothing through observation: if, in any ekf_batch_observe_logs*, ekf_batch_observe_replicas* or
 * ekf_batch_observe_corner_replicas call, the log of a frozen member holds an index at or beyond that member's landmark
 * count, the call returns EKF_ERR_STATE before anything is enqueued, and no member changes.
 * Unfreezing: mapping continues from the state and P the frozen frames left, bit for bit the member ekf_batch_set_member
 * restores from those arrays.  Frozen and mapping members run side by side in one call; a batch in which no member is
 * frozen launches the kernel instances it launched before the flag existed and produces the same bits.
 * Storage: the flags live on the host in the handle and, for the kernels, as [B] int32 in the batch workspace, directly
 * behind the [B] status words and in their 256-byte-aligned piece: that piece holds 8 B bytes instead of 4 B, so
 * workspace_bytes of ekf_batch_query_sizes grows by exactly round_up(8 B, 256) - round_up(4 B, 256) bytes (nothing for
 * B <= 32).  cov_bytes, state_bytes, ld and what ekf_batch_log_workspace_bytes, ekf_batch_replica_workspace_bytes and
 * ekf_batch_remove_workspace_bytes report do not change.
 *   ekf_batch_set_map_frozen: frozen[b] != 0 freezes member b, 0 unfreezes it, from the next call on; NULL: no member is
 *     frozen.  Waits for the batch's stream.
 *   ekf_batch_get_map_frozen: out[b] = 1 / 0. */
int ekf_batch_set_map_frozen(ekf_batch *b, const int32_t *frozen /* [B] HOST, or NULL: none */);
int ekf_batch_get_map_frozen(const ekf_batch *b, int32_t *out /* [B] */);

/* ---- Offline smoothing: a Rauch-Tung-Striebel backward pass over a recorded log replay.  A recorded replay
 * keeps, on the device, the filter as it was right after every frame that changed it; the backward pass turns those records
 * into the trajectory that ALL the data supports.  ekf_smooth_history forms the smoothed state only; ekf_smooth_history_cov
 * ("Smoothed covariances" below) forms the smoothed covariance with it.
 *
 * The smoothing rules.
 *   A RECORD r holds the state x_r (N_r doubles) and P_r right after a frame that changed the filter: a frame that was
 *   stepped, or moved by a non-zero motion, or both.  The TRANSITION into record r+1 is what that frame did before its
 *   update: (1) the move u_{r+1} (possibly zero), (2) the first sightings, appended with a block-diagonal P (uncorrelated
 *   with the old dims), (3) the predict with Q_eff = fl(s_eff q) if the frame was stepped (s_eff = 0 if it was only moved).
 *   Backward step for r = R-2 .. 0, x^s_{R-1} = x_{R-1}, N = N_r (the dims a later frame added are dropped, which is exact
 *   under the block-diagonal augmentation):
 *     prediction   x_p = move(x_r, u_{r+1}) (x_p = x_r for a zero motion); P_p = F~ P_r F~^T + diag(Q_eff), F~ of the motion
 *                  rules above (rows and columns 0 .. 9 only); Q_eff is 0 on the quaternion dims 3 .. 6.
 *     residual     delta[0:3] = x^s_{r+1}[0:3] - x_p[0:3], delta[10:N] likewise, delta[3:7] = 0 (the filter never applies an
 *                  additive quaternion correction), delta[7:10] = 2 vec(dq) / dq_w with dq = q^s_{r+1} (x) q_p^-1: the exact
 *                  inverse of the scalar-first injection q <- normalise((1, e/2) (x) q).
 *     solve        y = P_p^-1 delta by a Cholesky factorisation in f64 and the two substitutions; c = P_r F~^T y.
 *     inject       x^s_r = inject(x_r, c) with the filter's own injection: additive on 0 .. 2 and 10 .. N-1, c[3:7] dropped,
 *                  the quaternion rule on c[7:10], the error dims stay 0.
 *     output       frame t of the log gets x^s[0:7] of the last record at or before t; frames before the first record repeat
 *                  the camera state at the start of the recorded call, as the filtered trajectory does.
 *   Every sum is one ascending fma chain: two runs over the same history give the same bits.
 * Supported: EKF_MODEL_EKF with EKF_COV_F64 and EKF_QUAT_SCALAR_FIRST; mapping logs with any mix of gate, per-detection
 * noise, frame scale and motion.  REFUSED with EKF_ERR_STATE before anything is enqueued: EKF_QUAT_AS_WRITTEN (the
 * as-written injection reads scalar-first arrays as scalar-last and writes scalar-first: it is not a group action and has
 * no inverse), the f32 covariance, EKF_MODEL_ROTATIONS, a frozen map, and a filter that ekf_remove_markers (or ekf_reset)
 * touched between the recording and the smoothing.
 *
 * Recording.  ekf_observe_log_recorded takes the arguments of ekf_observe_log_moved plus the history buffer.  It runs the
 * frame-by-frame serial replay (ekf_last_sequence_mode: 1) and enqueues, behind every frame that changed the filter, ONE
 * pack launch that copies state[0:N] and the lower triangle of P -- packed column by column, f64 -- into the next record
 * (256-byte aligned).  Bit rule: trajectory, final state, final P, d^2 and ekf_last_log_stats are bit for bit those of the
 * same call through ekf_observe_log_moved / ekf_observe_log_gated: recording only reads.  (Of the stats, frames_pipelined
 * and pipelined_runs are 0 in a recorded call: a plain call without gate and motions may run pipelined, with the same
 * bits.)  The handle keeps the table of the call on the host (per record: frame, N_r, offset, s_eff, motion; per frame:
 * its record).
 *   history layout  [256 B: state[0:7] at the start of the call | record 0 | record 1 | ...], record = [state N | triangle
 *                   N (N + 1) / 2] doubles, rounded up to 256 bytes (ekf_history_record_bytes)
 *   ekf_history_bytes   an upper bound from the log alone: the header and one record per frame at the dims that frame
 *                       ends with (the log is checked as ekf_observe_log checks it)
 *   ekf_history_info    *records = R and, where the arrays are not NULL (capacity >= R entries each): per record the frame,
 *                       N_r, s_eff (0: only moved), the motion [6] and whether it was stepped; frame_record [frames]: the
 *                       record of every frame (-1: before the first).  Host getter.
 *   ekf_history_record  record r unpacked and mirrored: state_out [dims], cov_out [dims][dims] (either may be NULL); waits
 *                       for the handle's stream.  Host getter.
 *
 * The backward pass.  ekf_smooth_history runs on the handle's stream, over the handle's LAST recorded call and that buffer
 * (anything else: EKF_ERR_STATE), and writes smoothed_dev [frames][7].  It never writes the filter: state and P keep their
 * bits, and its status word is its own -- a P_p that is not positive definite returns EKF_ERR_NUMERIC and leaves no sticky
 * error on the filter.  The pass ends at that step r: the rows written until then stay (the frames before the first record
 * and the frames of the records behind r), the rows of the records up to r are left unwritten, in both tiers and in every
 * output of ekf_smooth_history_cov, first_cov_dev included.  It waits for the stream before it returns.  Two tiers, chosen
 * per call by the largest record:
 *   resident   every N_r <= 160 (n <= 50): ONE launch of ONE workgroup runs the whole pass, P_p as a packed triangle in LDS
 *   blocked    any larger N_r (up to 8064 dims), or flags bit 0: per step a short launch sequence around the blocked f64
 *              Cholesky of the wide frames
 *
 * Smoothed covariances.  ekf_smooth_history_cov runs the same backward pass and the covariance recursion with it.
 *   The covariance rule.  Records, transitions, F~, Q_eff, P_p and the dropping of dims that a later frame added are those
 *   of the smoothing rules.  With N = N_r and G_r = P_r F~^T P_p^-1:
 *     P^s_{R-1} = P_{R-1},   P^s_r = P_r + G_r (P^s_{r+1}[0:N, 0:N] - P_p) G_r^T,   r = R-2 .. 0
 *   (restricting P^s_{r+1} to the first N_r dims is exact: first sightings are appended block-diagonally).  The device
 *   evaluates the subtraction-of-products form, with L L^T = P_p, W = L^-1 F~ P_r and Z = L^-T W (= G_r^T):
 *     P^s_r = P_r - W^T W + Z^T (P^s_{r+1}[0:N, 0:N] Z)
 *   Only the lower triangle is computed and then mirrored: P^s_r is bitwise symmetric.  Every sum is one chain in a fixed
 *   order: two runs over the same history give the same bits.  Outputs for frame t come from the last record at or before
 *   t, as the poses; frames BEFORE THE FIRST RECORD get NaN in the covariance outputs (the history header keeps only the
 *   camera state of the call's start).
 *   Outputs: smoothed_dev [frames][7], bit for bit what ekf_smooth_history writes with flags bit 0 (the blocked tier);
 *   cam_cov_dev [frames][10][10] = P^s[0:10, 0:10]; filt_cam_cov_dev [frames][10][10] = P_r[0:10, 0:10] (or NULL);
 *   first_cov_dev [N_0][N_0] = P^s_0, mirrored (or NULL).  The last record's cam_cov rows are its filtered ones.
 *   Preconditions and refusals are those of ekf_smooth_history (the handle's last recorded call; EKF_MODEL_EKF, f64
 *   covariance, scalar-first, not frozen, not touched by removal), checked before anything is enqueued; a workspace
 *   smaller than ekf_smooth_cov_workspace_bytes is EKF_ERR_INVALID.  The pass has its own status word and never writes
 *   the filter: a P_p that is not positive definite returns EKF_ERR_NUMERIC and leaves nothing sticky.  One tier for every
 *   N: a launch sequence per step (the right-hand sides F~ P_r ride along the blocked f64 Cholesky, then a block backward
 *   substitution and three N x N x N products on the f64 matrix cores); records of up to 8064 dims, larger ones
 *   EKF_ERR_CAPACITY.  `flags` is reserved (0).
 * Not in this interface: recording from per-frame ekf_observe calls; for the covariances of the single filter: a resident
 * one-workgroup form, EKF_MODEL_ROTATIONS and the f32 covariance (ekf_batch has the resident form: "Batch smoothing,
 * covariances" below). */
int ekf_observe_log_recorded(ekf_filter *f, const int32_t *lm_index, const int64_t *offsets, int32_t frames,
                             const double *poses_dev, const double *rows_dev, const double *scale, const double *motion,
                             void *log_ws, size_t log_ws_bytes, double *trajectory_dev, double *mahal_dev,
                             void *history_dev, size_t history_bytes);
int ekf_history_record_bytes(int32_t dims, size_t *bytes);
int ekf_history_bytes(const ekf_filter *f, const int32_t *lm_index, const int64_t *offsets, int32_t frames, size_t *bytes);
int ekf_history_info(const ekf_filter *f, int32_t *records, int32_t capacity, int32_t *frame, int32_t *dims, double *s_eff,
                     double *motion /* [capacity][6] */, int32_t *stepped, int32_t *frame_record /* [frames] */);
int ekf_history_record(ekf_filter *f, const void *history_dev, int32_t r, double *state_out, double *cov_out, int32_t dims);
int ekf_smooth_workspace_bytes(const ekf_filter *f, size_t *bytes);
int ekf_smooth_history(ekf_filter *f, const void *history_dev, size_t history_bytes, void *ws, size_t ws_bytes, int32_t flags,
                       double *smoothed_dev /* [frames][7] */);
int ekf_smooth_cov_workspace_bytes(const ekf_filter *f, size_t *bytes);
int ekf_smooth_history_cov(ekf_filter *f, const void *history_dev, size_t history_bytes, void *ws, size_t ws_bytes,
                           int32_t flags, double *smoothed_dev        /* [frames][7]                           */,
                           double *cam_cov_dev                        /* [frames][10][10]  P^s[0:10,0:10]       */,
                           double *filt_cam_cov_dev                   /* [frames][10][10]  P_r[0:10,0:10], NULL */,
                           double *first_cov_dev                      /* [N_0][N_0]  P^s_0 mirrored, or NULL    */);

/* ---- Batch smoothing: recorded replays of an ekf_batch, one backward pass per member.  The smoothing rules
 * above, applied per member with the member's own q_cam / q_err / q_lm, with these additions.
 *   When a frame is recorded.  A member's frame is recorded when it changed the member: it was stepped, or moved by a motion
 *   with any non-zero component, or both.  Which frames the gate left unstepped and -- the motions being a device array --
 *   which motions are non-zero is known on the device only.  So the HOST gives a record slot to every frame that can change
 *   the member: every frame with detections, and every frame at all when the call carries motions; a slot has the size of
 *   the dims that frame ends with (first sightings are validated on the host, so the plan knows them).  The DEVICE writes,
 *   for every frame of the call, flag (0: no record, 1: stepped, 2: moved only, -1: the member has failed, at this frame or
 *   before) and s_eff as f64 (the scale the frame was stepped with: 1.0 in a batch without EKF_FLAG_FRAME_SCALE; 0 for a frame
 *   that was not stepped).  The frame on which a member fails (EKF_ERR_NUMERIC) writes no record, and no later frame does.
 *   History layout.  One region per member, member after member: [256 B: state[0:7] at the start of the call | slots], a slot
 *   [state N | triangle N (N + 1) / 2] doubles packed column by column and rounded up to 256 bytes (ekf_history_record_bytes,
 *   unchanged); a member without a log has its 256 bytes.  Behind the last region the words of the call, each piece rounded up
 *   to 256 bytes: the regions' offsets [B] i64, the slots' offsets [Ftot] i64, flag [Ftot] i32, s_eff [Ftot] f64 and, in a
 *   call with motions, a copy of the motions [Ftot][6] f64.
 *   Smoothed rows.  After the replay the host reads flag, s_eff and the motions back and builds one table per member: frame,
 *   dims, slot, Q_eff = fl(s_eff q) with the member's q, the motion.  Frame t gets x^s[0:7] of the member's last record at or
 *   before it; frames before the first record repeat the member's camera at the start of the call.  A member that failed in
 *   the replay has NaN rows from its failing frame on, as its trajectory has; its records before that frame are smoothed from
 *   the last good one.  A member with a P_p that is not positive definite has NaN on ALL its rows and EKF_ERR_NUMERIC in its
 *   entry of the pass's status [B]; no other member notices, the call still returns EKF_OK, and the pass never writes state, P
 *   or the replay status of any member.
 *   One workgroup per member runs the resident pass of the single filter (the same device function) over the member's own
 *   records; more members than compute units run as further rounds of workgroups; nothing synchronises across workgroups.
 *   Every sum is one ascending fma chain in a fixed thread: a member's smoothed rows do not depend on the batch around it.
 * Bit rule of the recording: trajectory, nis, cam_cov, d^2, state, P, landmark counts, pending scales and status of a recorded
 * call are bit for bit those of ekf_batch_observe_logs_moved: recording only reads the members.  A call that does not record
 * launches the kernels it launched before.
 * Supported: EKF_MODEL_EKF, EKF_QUAT_SCALAR_FIRST, mapping members that end the call with at most 50 landmarks (every record
 * has N_r <= 160: the resident tier), the one-column window kernel (max_visible <= 16), any mix of per-member gate, row noise,
 * frame scale, motion, per-member noise constants and initial poses, members without a log.
 * REFUSED with EKF_ERR_STATE before anything is enqueued, nothing changed: EKF_MODEL_ROTATIONS, EKF_QUAT_AS_WRITTEN, a batch
 * with EKF_FLAG_BATCH_LARGE_MAPS or EKF_FLAG_BATCH_WIDE_FRAMES, a frozen member with a log, a plan that takes a member past 50
 * landmarks; a history buffer smaller than ekf_batch_history_bytes: EKF_ERR_CAPACITY.
 * Binding: the pass and the getters run over the handle's LAST recorded call and that buffer only (EKF_ERR_STATE otherwise),
 * and are refused after ekf_batch_reset, ekf_batch_set_member or ekf_batch_remove_markers touched any member since.
 *   ekf_batch_history_bytes          the size of the history from the logs alone (checked as ekf_batch_observe_logs checks
 *                                    them); with_motion != 0: the call will carry motions.  Waits for the stream.
 *   ekf_batch_observe_logs_recorded  ekf_batch_observe_logs_moved plus the history buffer; rows, scale, motion, nis, cam_cov
 *                                    and mahal may each be NULL.
 *   ekf_batch_history_info           the fields of ekf_history_info for one member, frames counted within its log.  Waits for
 *                                    the stream (the first getter after a recording copies the call's words back).
 *   ekf_batch_history_record         record r of a member, unpacked and mirrored.
 *   ekf_batch_history_table          the table builder alone, no handle and no device: from flag / s_eff / motion (or NULL)
 *                                    [Ftot], slot / dims [Ftot], member_frames [B + 1] and noise [B][6] (ekf_config order) it
 *                                    gives per member (records, first row, end of the lead rows, first NaN row, end row) and,
 *                                    per record in member order, its member, its rows [frame0, frame1), Q_eff [3], moved.
 *   ekf_batch_smooth_workspace_bytes, ekf_batch_smooth_history: the pass; smoothed_dev [Ftot][7], status_out [B] on the host
 *                                    (or NULL).  Waits for the stream before it returns.
 * Batch smoothing, covariances.  ekf_batch_smooth_history_cov runs the same pass and, inside it, the covariance rule above
 * (P^s_{R-1} = P_{R-1}, P^s_r = P_r + G_r (P^s_{r+1}[0:N, 0:N] - P_p) G_r^T, in its subtraction-of-products form) per member
 * with the member's own Q_eff = fl(s_eff q): the smoothed covariances of every member in ONE launch, one workgroup per member.
 * The factor L of P_p is the one the state step has just formed in LDS -- P_p is not factored twice and the state arithmetic is
 * that of ekf_batch_smooth_history: smoothed_dev has its bits.  W = L^-1 F~ P_r, Z = L^-T W, T = P^s_{r+1} Z and P^s live in the
 * member's own region of the workspace ([ld][ld] each, ld = the dims of the member's largest record rounded up to 16; at most
 * 819 200 bytes per member); the products run on the f64 matrix cores, every sum is one chain in a fixed order in a fixed wave,
 * and P^s is zeroed by the kernel before its first use: the bits of a member depend neither on the batch around it nor on
 * what the workspace held.  Only the lower triangle is computed and mirrored: cam_cov and first_cov are bitwise symmetric.
 *   Outputs: smoothed_dev [Ftot][7]; cam_cov_dev [Ftot][10][10] = P^s[0:10, 0:10] of the member's last record at or before the
 *   frame; filt_cam_cov_dev [Ftot][10][10] = that record's P[0:10, 0:10] (or NULL); first_cov_dev [B][first_ld][first_ld]: member
 *   b's slab holds P^s_0 in [0:N_0, 0:N_0] with leading dimension first_ld, the rest of the slab is not written (or NULL).  The
 *   last record's cam_cov rows are its filtered ones.  Frames before a member's first record: the pose rows repeat the start
 *   camera, the covariance rows are NaN.  A member with no record: its first_cov slab is NOT written.
 *   Failures.  A member with a P_p that is not positive definite has NaN on all its rows of all three per-frame outputs, NaN in
 *   [0:N_0, 0:N_0] of its first_cov slab and EKF_ERR_NUMERIC in its entry of status_out; no other member notices and the call
 *   returns EKF_OK.  A member that failed in the replay has NaN from its failing frame on in all three outputs.  The pass
 *   never writes state, P or the replay status of any member.
 *   Binding and refusals are those of ekf_batch_smooth_history; in addition a workspace below
 *   ekf_batch_smooth_cov_workspace_bytes, a first_ld below some member's N_0 (with first_cov_dev given) and non-zero flags
 *   (reserved) are EKF_ERR_INVALID before anything is enqueued.  Waits for the stream before it returns.
 * Not in this interface: a blocked tier for batches (members beyond 50 landmarks), recording in the HBM-resident window
 * kernels (large maps, wide frames), smoothed landmark outputs. */
int ekf_batch_history_bytes(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets, const int64_t *member_frames,
                            int32_t with_motion, size_t *bytes);
int ekf_batch_observe_logs_recorded(ekf_batch *b, const int32_t *lm_index, const int64_t *frame_offsets,
                                    const int64_t *member_frames, const double *poses_dev, const double *rows_dev,
                                    const double *scale_dev, const double *motion_dev, void *log_ws, size_t log_ws_bytes,
                                    double *trajectory_dev, double *nis_dev, double *cam_cov_dev, double *mahal_dev,
                                    void *history_dev, size_t history_bytes);
int ekf_batch_history_info(ekf_batch *b, int32_t member, int32_t *records, int32_t capacity, int32_t *frame, int32_t *dims,
                           double *s_eff, double *motion /* [capacity][6] */, int32_t *stepped,
                           int32_t *frame_record /* [F_b] */);
int ekf_batch_history_record(ekf_batch *b, const void *history_dev, int32_t member, int32_t r, double *state_out,
                             double *cov_out, int32_t dims);
int ekf_batch_history_table(int32_t members, const int64_t *member_frames, const int64_t *slot, const int32_t *dims,
                            const int32_t *flag, const double *s_eff, const double *motion, const double *noise,
                            int32_t capacity, int32_t *total, int32_t *member_rows /* [B][5] */,
                            int32_t *rec_member /* [capacity] */, int32_t *rec_rows /* [capacity][2] */,
                            double *rec_q /* [capacity][3] */, int32_t *rec_moved /* [capacity] */);
int ekf_batch_smooth_workspace_bytes(ekf_batch *b, size_t *bytes);
int ekf_batch_smooth_history(ekf_batch *b, const void *history_dev, size_t history_bytes, void *ws, size_t ws_bytes,
                             double *smoothed_dev /* [Ftot][7] */, int32_t *status_out /* [B] host, or NULL */);
int ekf_batch_smooth_cov_workspace_bytes(ekf_batch *b, size_t *bytes);
int ekf_batch_smooth_history_cov(ekf_batch *b, const void *history_dev, size_t history_bytes, void *ws, size_t ws_bytes,
                                 int32_t flags /* reserved, 0 */, double *smoothed_dev /* [Ftot][7] */,
                                 double *cam_cov_dev /* [Ftot][10][10] */, double *filt_cam_cov_dev /* or NULL */,
                                 double *first_cov_dev /* [B][first_ld][first_ld], or NULL */, int32_t first_ld,
                                 int32_t *status_out /* [B] host, or NULL */);

const char *ekf_last_error_string(void);

#ifdef __cplusplus
}
#endif
#endif /* EKF_SLAM_HIP_H */
