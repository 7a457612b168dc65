"""ctypes binding of the C ABI in ``include/ekf_slam_hip.h``.

PyTorch is used for exactly three things: owning the device buffers
(covariance, state, workspace, resident detection arrays), providing the HIP
stream, and ``torch.distributed`` for the final gather.  All arithmetic runs in
the HIP library; there is no CPU fallback -- a missing library or a missing GPU
raises.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from ._build import LIB_PATH

EKF_COV_F64, EKF_COV_F32 = 0, 1
EKF_QUAT_AS_WRITTEN, EKF_QUAT_SCALAR_FIRST = 0, 1
EKF_FLAG_WIDE_FRAMES = 8       # ekf_config.flags bit 3: up to 1024 detections per frame
EKF_FLAG_BATCH_LARGE_MAPS = 16  # ekf_config.flags bit 4 (batches): up to 1024 state dims per member
EKF_FLAG_BATCH_WIDE_FRAMES = 32  # ekf_config.flags bit 5 (batches): up to 64 (EKF) / 50 (EKF_Rotations) detections per frame
EKF_FLAG_GATE = 64             # ekf_config.flags bit 6: the per-detection chi-square gate of the single filter
EKF_FLAG_ROW_NOISE = 128       # ekf_config.flags bit 7: per-detection measurement noise of the single filter (rows=)
EKF_FLAG_FRAME_SCALE = 256     # ekf_config.flags bit 8: per-frame process-noise scale and the pending scale (scale=)
EKF_FLAG_MOTION = 512          # ekf_config.flags bit 9: per-frame camera motion of the single filter (motion=, move)
EKF_COVK_AUTO, EKF_COVK_VALU, EKF_COVK_MFMA, EKF_COVK_MFMA_TILE, EKF_COVK_MFMA_MACRO = 0, 1, 2, 3, 4

# frames in the end-gate ring of ekf_debug_fetch item 6 (csrc/ekf_kernels.h: EKF_GATE_LOG_FRAMES)
GATE_LOG_FRAMES = 2048

# every symbol include/ekf_slam_hip.h declares
EXPORTED_SYMBOLS = (
    "ekf_default_config", "ekf_query_sizes", "ekf_create", "ekf_destroy", "ekf_bind_buffers",
    "ekf_reset", "ekf_grow", "ekf_add_markers", "ekf_observe", "ekf_observe_device",
    "ekf_observe_sequence_device", "ekf_last_sequence_mode", "ekf_get_camera", "ekf_get_state", "ekf_get_cov_diag",
    "ekf_get_cov", "ekf_set_state", "ekf_set_cov", "ekf_num_landmarks", "ekf_sync",
    "ekf_set_fused", "ekf_set_kernel_timing", "ekf_get_kernel_timing", "ekf_debug_fetch",
    "ekf_estimate_poses_device", "ekf_estimate_poses", "ekf_last_error_string",
    "ekf_log_workspace_bytes", "ekf_observe_log", "ekf_last_log_stats",
    "ekf_batch_query_sizes", "ekf_batch_create", "ekf_batch_bind_buffers", "ekf_batch_destroy", "ekf_batch_set_noise",
    "ekf_batch_reset", "ekf_batch_set_member", "ekf_batch_get_member", "ekf_batch_num_landmarks", "ekf_batch_status",
    "ekf_batch_log_workspace_bytes", "ekf_batch_observe_logs", "ekf_batch_observe_logs_diag", "ekf_batch_replica_poses",
    "ekf_batch_replica_workspace_bytes", "ekf_batch_observe_replicas",
    "ekf_batch_set_gate", "ekf_batch_observe_logs_gated", "ekf_batch_observe_replicas_gated",
    "ekf_batch_replica_corners", "ekf_batch_observe_corner_replicas",
    "ekf_set_gate", "ekf_observe_gated", "ekf_observe_log_gated", "ekf_last_gate_stats",
    "ekf_remove_workspace_bytes", "ekf_remove_markers", "ekf_batch_remove_workspace_bytes", "ekf_batch_remove_markers",
    "ekf_observe_rows", "ekf_observe_sequence_device_rows", "ekf_observe_log_rows", "ekf_batch_observe_logs_rows",
    "ekf_advance", "ekf_get_pending_scale", "ekf_set_pending_scale", "ekf_observe_scaled",
    "ekf_observe_sequence_device_scaled", "ekf_observe_log_scaled", "ekf_batch_observe_logs_scaled",
    "ekf_batch_get_pending_scale", "ekf_batch_set_pending_scale",
    "ekf_move", "ekf_observe_moved", "ekf_observe_sequence_device_moved", "ekf_observe_log_moved",
    "ekf_batch_observe_logs_moved",
    "ekf_set_map_frozen", "ekf_get_map_frozen",
    "ekf_batch_set_map_frozen", "ekf_batch_get_map_frozen",
    "ekf_observe_log_recorded", "ekf_history_record_bytes", "ekf_history_bytes", "ekf_history_info", "ekf_history_record",
    "ekf_smooth_workspace_bytes", "ekf_smooth_history", "ekf_smooth_cov_workspace_bytes", "ekf_smooth_history_cov",
    "ekf_batch_history_bytes", "ekf_batch_observe_logs_recorded", "ekf_batch_history_info", "ekf_batch_history_record",
    "ekf_batch_history_table", "ekf_batch_smooth_workspace_bytes", "ekf_batch_smooth_history",
    "ekf_batch_smooth_cov_workspace_bytes", "ekf_batch_smooth_history_cov",
)


class EkfConfig(C.Structure):
    _fields_ = [
        ("max_landmarks", C.c_int32), ("max_visible", C.c_int32), ("cov_dtype", C.c_int32),
        ("quat_mode", C.c_int32), ("cov_kernel", C.c_int32), ("model", C.c_int32), ("reserved", C.c_int32), ("flags", C.c_int32),
        ("initial_camera_uncertainty", C.c_double), ("initial_landmark_uncertainty", C.c_double),
        ("r_uncertainty", C.c_double), ("q_cam", C.c_double), ("q_err", C.c_double),
        ("q_lm", C.c_double), ("stream", C.c_void_p),
    ]


class EkfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ekf_slam_hip error {code}: {msg}")
        self.code = code


_lib = None


def load_library(path: str | Path | None = None):
    """dlopen the in-tree library; raises if it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise FileNotFoundError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the EKF update path)")
    # torch ships its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  Import
    # torch FIRST so the library below binds to that already-loaded runtime: a
    # second HIP runtime in the process sees no device.
    import torch  # noqa: F401
    lib = C.CDLL(str(p))
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    sig = {
        "ekf_default_config": [C.POINTER(EkfConfig)],
        "ekf_query_sizes": [C.POINTER(EkfConfig), C.POINTER(C.c_int64), C.POINTER(C.c_size_t),
                            C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
        "ekf_create": [C.POINTER(EkfConfig), C.POINTER(vp)],
        "ekf_destroy": [vp],
        "ekf_bind_buffers": [vp, vp, C.c_int64, vp, vp, C.c_size_t],
        "ekf_reset": [vp, dp],
        "ekf_grow": [vp, C.c_int32, C.c_int32, vp, C.c_int64, vp, vp, C.c_size_t],
        "ekf_add_markers": [vp, dp, dp, C.c_int32],
        "ekf_observe": [vp, ip, dp, C.c_int32],
        "ekf_observe_device": [vp, vp, vp, C.c_int32],
        "ekf_observe_sequence_device": [vp, vp, vp, C.c_int32, C.c_int32, vp],
        "ekf_get_camera": [vp, dp],
        "ekf_get_state": [vp, dp, C.c_int32],
        "ekf_get_cov_diag": [vp, dp, C.c_int32],
        "ekf_get_cov": [vp, dp, C.c_int32],
        "ekf_set_state": [vp, dp, C.c_int32],
        "ekf_set_cov": [vp, dp, C.c_int32],
        "ekf_num_landmarks": [vp],
        "ekf_last_sequence_mode": [vp],
        "ekf_sync": [vp],
        "ekf_set_fused": [vp, C.c_int32],
        "ekf_set_kernel_timing": [vp, C.c_int32],
        "ekf_get_kernel_timing": [vp, C.c_int32, dp, C.POINTER(C.c_int64)],
        "ekf_debug_fetch": [vp, C.c_int32, dp, C.c_size_t],
        "ekf_estimate_poses_device": [vp, C.c_int32, C.c_double, dp, dp, C.c_int32, vp, vp],
        "ekf_estimate_poses": [dp, C.c_int32, C.c_double, dp, dp, C.c_int32, dp, vp],
        "ekf_log_workspace_bytes": [vp, C.c_int64, C.POINTER(C.c_size_t)],
        "ekf_observe_log": [vp, ip, C.POINTER(C.c_int64), C.c_int32, vp, vp, C.c_size_t, vp],
        "ekf_last_log_stats": [vp, C.POINTER(C.c_int64)],
        "ekf_set_gate": [vp, C.c_double],
        "ekf_observe_gated": [vp, ip, dp, C.c_int32, C.POINTER(C.c_uint8), dp, ip],
        "ekf_observe_log_gated": [vp, ip, C.POINTER(C.c_int64), C.c_int32, vp, vp, C.c_size_t, vp, vp],
        "ekf_last_gate_stats": [vp, C.POINTER(C.c_int64)],
        "ekf_observe_rows": [vp, ip, dp, dp, C.c_int32, C.POINTER(C.c_uint8), dp, ip],
        "ekf_observe_sequence_device_rows": [vp, vp, vp, vp, C.c_int32, C.c_int32, vp],
        "ekf_observe_log_rows": [vp, ip, C.POINTER(C.c_int64), C.c_int32, vp, vp, vp, C.c_size_t, vp, vp],
        "ekf_batch_observe_logs_rows": [vp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp, vp, vp, C.c_size_t, vp, vp,
                                        vp, vp],
        "ekf_advance": [vp, C.c_double],
        "ekf_get_pending_scale": [vp, dp],
        "ekf_set_pending_scale": [vp, C.c_double],
        "ekf_observe_scaled": [vp, ip, dp, dp, C.c_int32, C.POINTER(C.c_uint8), dp, ip, C.c_double],
        "ekf_observe_sequence_device_scaled": [vp, vp, vp, vp, dp, C.c_int32, C.c_int32, vp],
        "ekf_observe_log_scaled": [vp, ip, C.POINTER(C.c_int64), C.c_int32, vp, vp, dp, vp, C.c_size_t, vp, vp],
        "ekf_batch_observe_logs_scaled": [vp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp, vp, vp, vp, C.c_size_t, vp,
                                          vp, vp, vp],
        "ekf_batch_get_pending_scale": [vp, C.c_int32, dp],
        "ekf_batch_set_pending_scale": [vp, C.c_int32, dp],
        "ekf_move": [vp, dp],
        "ekf_observe_moved": [vp, ip, dp, dp, C.c_int32, C.POINTER(C.c_uint8), dp, ip, C.c_double, dp],
        "ekf_observe_sequence_device_moved": [vp, vp, vp, vp, dp, dp, C.c_int32, C.c_int32, vp],
        "ekf_observe_log_moved": [vp, ip, C.POINTER(C.c_int64), C.c_int32, vp, vp, dp, dp, vp, C.c_size_t, vp, vp],
        "ekf_batch_observe_logs_moved": [vp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp, vp, vp, vp, vp, C.c_size_t,
                                         vp, vp, vp, vp],
        "ekf_set_map_frozen": [vp, C.c_int32],
        "ekf_get_map_frozen": [vp],
        "ekf_batch_set_map_frozen": [vp, ip],
        "ekf_batch_get_map_frozen": [vp, ip],
        "ekf_observe_log_recorded": [vp, ip, C.POINTER(C.c_int64), C.c_int32, vp, vp, dp, dp, vp, C.c_size_t, vp, vp, vp,
                                     C.c_size_t],
        "ekf_history_record_bytes": [C.c_int32, C.POINTER(C.c_size_t)],
        "ekf_history_bytes": [vp, ip, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_size_t)],
        "ekf_history_info": [vp, ip, C.c_int32, ip, ip, dp, dp, ip, ip],
        "ekf_history_record": [vp, vp, C.c_int32, dp, dp, C.c_int32],
        "ekf_smooth_workspace_bytes": [vp, C.POINTER(C.c_size_t)],
        "ekf_smooth_history": [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int32, vp],
        "ekf_smooth_cov_workspace_bytes": [vp, C.POINTER(C.c_size_t)],
        "ekf_smooth_history_cov": [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int32, vp, vp, vp, vp],
        "ekf_batch_history_bytes": [vp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_size_t)],
        "ekf_batch_observe_logs_recorded": [vp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp, vp, vp, vp, vp, C.c_size_t,
                                            vp, vp, vp, vp, vp, C.c_size_t],
        "ekf_batch_history_info": [vp, C.c_int32, ip, C.c_int32, ip, ip, dp, dp, ip, ip],
        "ekf_batch_history_record": [vp, vp, C.c_int32, C.c_int32, dp, dp, C.c_int32],
        "ekf_batch_history_table": [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), ip, ip, dp, dp, dp, C.c_int32, ip,
                                    ip, ip, ip, dp, ip],
        "ekf_batch_smooth_workspace_bytes": [vp, C.POINTER(C.c_size_t)],
        "ekf_batch_smooth_history": [vp, vp, C.c_size_t, vp, C.c_size_t, vp, ip],
        "ekf_batch_smooth_cov_workspace_bytes": [vp, C.POINTER(C.c_size_t)],
        "ekf_batch_smooth_history_cov": [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int32, vp, vp, vp, vp, C.c_int32, ip],
        "ekf_remove_workspace_bytes": [vp, C.c_int32, C.POINTER(C.c_size_t)],
        "ekf_remove_markers": [vp, ip, C.c_int32, vp, C.c_int64, vp, vp, C.c_size_t],
        "ekf_batch_remove_workspace_bytes": [vp, C.c_int64, C.POINTER(C.c_size_t)],
        "ekf_batch_remove_markers": [vp, ip, C.POINTER(C.c_int64), vp, C.c_int64, vp, vp, C.c_size_t],
        "ekf_batch_query_sizes": [C.POINTER(EkfConfig), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_size_t),
                                  C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
        "ekf_batch_create": [C.POINTER(EkfConfig), C.c_int32, C.POINTER(vp)],
        "ekf_batch_bind_buffers": [vp, vp, C.c_int64, vp, vp, C.c_size_t],
        "ekf_batch_destroy": [vp],
        "ekf_batch_set_noise": [vp, dp],
        "ekf_batch_reset": [vp, C.c_int32, dp],
        "ekf_batch_set_member": [vp, C.c_int32, dp, C.c_int32, dp],
        "ekf_batch_get_member": [vp, C.c_int32, dp, C.c_int32, dp, C.c_int32],
        "ekf_batch_num_landmarks": [vp, ip],
        "ekf_batch_status": [vp, ip],
        "ekf_batch_log_workspace_bytes": [vp, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)],
        "ekf_batch_observe_logs": [vp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp, vp, C.c_size_t, vp],
        "ekf_batch_observe_logs_diag": [vp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp, vp, C.c_size_t, vp, vp,
                                        vp],
        "ekf_batch_replica_poses": [vp, C.c_int64, dp, C.c_int32, C.c_uint64, C.c_uint32, vp, vp],
        "ekf_batch_replica_workspace_bytes": [vp, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)],
        "ekf_batch_observe_replicas": [vp, ip, C.POINTER(C.c_int64), C.c_int64, vp, dp, C.c_uint64, C.c_uint32, vp,
                                       C.c_size_t, vp, vp, vp],
        "ekf_batch_set_gate": [vp, dp],
        "ekf_batch_observe_logs_gated": [vp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), vp, vp, C.c_size_t, vp, vp,
                                         vp, vp],
        "ekf_batch_observe_replicas_gated": [vp, ip, C.POINTER(C.c_int64), C.c_int64, vp, dp, C.c_uint64, C.c_uint32, vp,
                                             C.c_size_t, vp, vp, vp, vp],
        "ekf_batch_replica_corners": [vp, C.c_int64, dp, C.c_int32, C.c_uint64, C.c_uint32, C.c_double, dp, dp, C.c_int32,
                                      vp, vp, vp, vp],
        "ekf_batch_observe_corner_replicas": [vp, ip, C.POINTER(C.c_int64), C.c_int64, vp, dp, C.c_uint64, C.c_uint32,
                                              C.c_double, dp, dp, C.c_int32, vp, C.c_size_t, vp, vp, vp, vp, vp],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.ekf_last_error_string.argtypes = []
    lib.ekf_last_error_string.restype = C.c_char_p
    if path is None:
        _lib = lib
    return lib


def check_gate(gate):
    """``gate`` (None, or a number > 0; ``inf``: off) as None or a float; ``ValueError`` otherwise."""
    if gate is None:
        return None
    g = float(gate)
    if not g > 0.0:
        raise ValueError("gate must be > 0 (inf: off) and not NaN")
    return g


def row_noise_array(noise, count: int, rd: int, what: str = "noise"):
    """Per-detection measurement noise as the C ABI takes it: ``noise`` is [count] (one variance per detection, broadcast
    over its ``rd`` rows) or [count, rd] (one per measurement row, in the order of z); returns a contiguous float64
    [count, rd] array.  Another shape, or an entry that is not finite and > 0, raises ``ValueError``."""
    try:
        v = np.asarray(noise, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what} must be numbers of shape ({count},) or ({count}, {rd})") from e
    if v.shape == (count,):
        v = np.repeat(v[:, None], rd, axis=1)
    elif v.shape != (count, rd):
        raise ValueError(f"{what} must have shape ({count},) or ({count}, {rd}), got {v.shape}")
    if not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError(f"{what} must be finite and > 0")
    return np.ascontiguousarray(v)


def frame_scale_array(scale, count: int | None = None, what: str = "scale"):
    """Per-frame process-noise scales as the C ABI takes them: a number (``count`` None) as a float, or [count] as a
    contiguous float64 array.  Another shape, or an entry that is NaN, Inf or negative, raises ``ValueError``."""
    try:
        v = np.asarray(scale, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what} must be a number" if count is None else f"{what} must be numbers of shape ({count},)") from e
    if v.shape != (() if count is None else (count,)):
        raise ValueError(f"{what} must be a number, got shape {v.shape}" if count is None
                         else f"{what} must have shape ({count},), got {v.shape}")
    if not (np.isfinite(v).all() and (v >= 0).all()):
        raise ValueError(f"{what} must be finite and >= 0")
    return float(v) if count is None else np.ascontiguousarray(v)


def motion_array(motion, count: int | None = None, what: str = "motion"):
    """Camera motions as the C ABI takes them: ``(d, w)`` -- six numbers, a translation and a rotation vector in the camera
    frame of the previous pose -- as a contiguous float64 [6] (``count`` None) or [count, 6] array.  Another shape, or an
    entry that is NaN or Inf, raises ``ValueError``."""
    shape = (6,) if count is None else (count, 6)
    try:
        v = np.asarray(motion, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what} must be numbers of shape {shape}") from e
    if v.shape != shape:
        raise ValueError(f"{what} must have shape {shape}, got {v.shape}")
    if not np.isfinite(v).all():
        raise ValueError(f"{what} must be finite")
    return np.ascontiguousarray(v)


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _iptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _lptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def estimate_poses(corners, marker_size: float, camera_matrix, dist_coeffs=None, device="cuda:0") -> np.ndarray:
    """Batched IPPE-square pose of every detected marker on the GPU (ekf_estimate_poses; replaces the per-marker
    cv2.solvePnP loop of base_filter.py:92-171).  corners: array-like [m,4,2] (or cv2's list of [1,4,2]) of pixel
    coordinates; returns [m,6] = [tvec | rvec].  No CPU fallback."""
    import torch
    lib = load_library()
    if not torch.cuda.is_available():
        raise RuntimeError("the pose front end needs a HIP device (no CPU fallback)")
    c = np.ascontiguousarray(np.asarray(corners, dtype=np.float64).reshape(-1, 4, 2))
    k = np.ascontiguousarray(np.asarray(camera_matrix, dtype=np.float64).reshape(3, 3))
    d = np.ascontiguousarray(np.asarray([] if dist_coeffs is None else dist_coeffs, dtype=np.float64).reshape(-1))
    out = np.zeros((c.shape[0], 6))
    with torch.cuda.device(torch.device(device)):
        rc = lib.ekf_estimate_poses(_dptr(c), c.shape[0], float(marker_size), _dptr(k), _dptr(d) if d.size else None,
                                    int(d.size), _dptr(out), None)
    if rc != 0:
        raise EkfError(rc, lib.ekf_last_error_string().decode())
    return out


class HipEkf:
    """One filter instance = one C handle + the torch tensors it borrows."""

    KERNEL_NAMES = ("gather", "solve", "panel", "cov_update")
    # detections per frame (by landmark width: EKF / EKF_Rotations).  Beyond 64 (50) a frame runs through the wide-frame
    # path (EKF_FLAG_WIDE_FRAMES, set in every configuration made here: grow() carries it along in self.cfg)
    MAX_VISIBLE_LIMIT = {3: 1024, 10: 1024}

    def __init__(self, max_landmarks: int, max_visible: int, cov_dtype="float64",
                 quat_mode="as_written", cov_kernel="auto", device="cuda:0", noise=None,
                 lookahead=None, model="ekf", fused=True, gate=None, row_noise=False, frame_scale=False, motion=False):
        """``gate``: None = a filter without the per-detection gate (sizes and results as ever); a number > 0 = the
        chi-square gate on every detection's own d^2 (``set_gate``; ``inf``: the filter can gate and report distances, but
        the gate is off).
        ``row_noise``: the filter takes per-detection measurement noise (``rows=`` of the observe calls); without it,
        sizes and results as ever.
        ``frame_scale``: frames may carry a process-noise scale (``scale=`` of the observe calls, ``advance``) and the
        filter keeps a pending scale; without it, results as ever.
        ``motion``: frames may carry a camera motion (``motion=`` of the observe calls, ``move``); without it, results as
        ever."""
        import torch
        self._torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("the EKF update path needs a HIP device (no CPU fallback)")
        self.device = torch.device(device)
        cfg = EkfConfig()
        self._check(self.lib.ekf_default_config(C.byref(cfg)))
        cfg.max_landmarks = int(max_landmarks)
        cfg.max_visible = int(max_visible)
        cfg.cov_dtype = {"float64": EKF_COV_F64, "float32": EKF_COV_F32}[str(cov_dtype)]
        cfg.quat_mode = {"as_written": EKF_QUAT_AS_WRITTEN,
                         "scalar_first": EKF_QUAT_SCALAR_FIRST}[quat_mode]
        kern = {"auto": EKF_COVK_AUTO, "valu": EKF_COVK_VALU, "mfma": EKF_COVK_MFMA, "mfma_tile": EKF_COVK_MFMA_TILE,
                "mfma_macro": EKF_COVK_MFMA_MACRO}
        cfg.cov_kernel = kern[cov_kernel]
        cfg.flags = {None: 0, False: 1, True: 2}[lookahead]   # None: pipelined sequence mode where it wins (by size); False: never; True: always
        if not fused:
            cfg.flags |= 4        # separate gather / solve / panel launches
        cfg.flags |= EKF_FLAG_WIDE_FRAMES
        gate = check_gate(gate)
        if gate is not None:
            cfg.flags |= EKF_FLAG_GATE
        if row_noise:
            cfg.flags |= EKF_FLAG_ROW_NOISE
        if frame_scale:
            cfg.flags |= EKF_FLAG_FRAME_SCALE
        if motion:
            cfg.flags |= EKF_FLAG_MOTION
        self.fused = bool(fused)  # ("force" of earlier versions == True: there is no automatic fallback any more)
        self._last_m = 1
        cfg.model = {"ekf": 0, "ekf_rotations": 1}[model]
        self.lm_dims, self.rows_per_detection = (10, 7) if cfg.model == 1 else (3, 3)
        for key, val in (noise or {}).items():
            setattr(cfg, key, float(val))
        self.cov_dtype = str(cov_dtype)
        self.max_landmarks, self.max_visible = int(max_landmarks), int(max_visible)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(device=self.device)
            cfg.stream = self.stream.cuda_stream
            ld, cb, sb, wb = C.c_int64(), C.c_size_t(), C.c_size_t(), C.c_size_t()
            self._check(self.lib.ekf_query_sizes(C.byref(cfg), C.byref(ld), C.byref(cb),
                                                 C.byref(sb), C.byref(wb)))
            self.ld = ld.value
            tdt = torch.float64 if cfg.cov_dtype == EKF_COV_F64 else torch.float32
            self.cov_t = torch.zeros((self.ld, self.ld), dtype=tdt, device=self.device)
            self.state_t = torch.zeros((sb.value // 8,), dtype=torch.float64, device=self.device)
            self.ws_t = torch.zeros((wb.value,), dtype=torch.uint8, device=self.device)
            torch.cuda.synchronize(self.device)
            handle = C.c_void_p()
            self._check(self.lib.ekf_create(C.byref(cfg), C.byref(handle)))
            self.h = handle
            self._check(self.lib.ekf_bind_buffers(self.h, self.cov_t.data_ptr(), self.ld,
                                                  self.state_t.data_ptr(), self.ws_t.data_ptr(),
                                                  wb.value))
        self.cfg = cfg
        self._map_frozen = False      # (off after ekf_create)
        self._history_frames = 0      # frames of the last recorded replay (observe_log(history=))
        self.gate = None      # None: built without the gate; inf: off
        if gate is not None:
            self.set_gate(gate)

    @property
    def can_gate(self) -> bool:
        return bool(self.cfg.flags & EKF_FLAG_GATE)

    @property
    def can_row_noise(self) -> bool:
        return bool(self.cfg.flags & EKF_FLAG_ROW_NOISE)

    @property
    def can_frame_scale(self) -> bool:
        return bool(self.cfg.flags & EKF_FLAG_FRAME_SCALE)

    @property
    def can_motion(self) -> bool:
        return bool(self.cfg.flags & EKF_FLAG_MOTION)

    @property
    def map_frozen(self) -> bool:
        """Whether the map is frozen (ekf_set_map_frozen): frames update the camera, P_cc and the cross-covariances and
        leave the landmarks and P_ll alone.  The handle's flag as this object set it (``observe`` asks every frame)."""
        return self._map_frozen

    def set_map_frozen(self, frozen) -> None:
        """Freeze (localisation on the map as it is: the Schmidt-Kalman update of the camera) or unfreeze the map from the
        next frame on (ekf_set_map_frozen).  Persistent until ``reset``; nothing is enqueued."""
        self._check(self.lib.ekf_set_map_frozen(self.h, int(bool(frozen))))
        self._map_frozen = self.lib.ekf_get_map_frozen(self.h) == 1

    def _motion(self, motion, count: int | None = None):
        """``motion`` of a call as a contiguous [6] (``count`` None) or [count, 6] array (``motion_array``); a filter built
        without ``motion=True`` raises ``ValueError``."""
        if not self.can_motion:
            raise ValueError("this filter was built without camera motions: construct it with motion=True")
        return motion_array(motion, count)

    def move(self, motion) -> None:
        """The camera moves by ``motion = (d, w)`` in its own frame (ekf_move): state and P on the device, nothing is
        synchronised; six exact zeros enqueue nothing."""
        self._check(self.lib.ekf_move(self.h, _dptr(self._motion(motion))))

    def _scale(self, scale, count: int | None = None):
        """``scale`` of an observe call as a float (``count`` None) or a contiguous [count] array (``frame_scale_array``);
        a filter built without ``frame_scale=True`` raises ``ValueError``."""
        if not self.can_frame_scale:
            raise ValueError("this filter was built without per-frame scales: construct it with frame_scale=True")
        return frame_scale_array(scale, count)

    def advance(self, scale) -> None:
        """Time passes without a frame (ekf_advance): ``scale`` is added to the pending scale, which the next stepped
        frame adds to its own."""
        self._check(self.lib.ekf_advance(self.h, self._scale(scale)))

    @property
    def pending_scale(self) -> float:
        """The process-noise scale that has accumulated since the last stepped frame (ekf_get_pending_scale); 0 for a
        filter built without ``frame_scale=True``."""
        out = C.c_double()
        self._check(self.lib.ekf_get_pending_scale(self.h, C.byref(out)))
        return out.value

    @pending_scale.setter
    def pending_scale(self, value) -> None:
        self._check(self.lib.ekf_set_pending_scale(self.h, self._scale(value)))

    def _rows(self, rows, count: int):
        """``rows`` of an observe call as a contiguous [count, rd] array (``row_noise_array``); a filter built without
        ``row_noise=True`` raises ``ValueError``."""
        if not self.can_row_noise:
            raise ValueError("this filter was built without per-detection noise: construct it with row_noise=True")
        return row_noise_array(rows, count, self.rows_per_detection, "rows")

    def set_gate(self, gate) -> None:
        """The chi-square gate on every detection's own Mahalanobis distance (ekf_set_gate): a number > 0, ``inf`` or
        None = off.  Needs a filter constructed with ``gate=`` (``inf`` will do); persistent across ``reset``."""
        g = check_gate(gate)
        if g is None:
            if not self.can_gate:
                return
            g = float("inf")
        if not self.can_gate:
            raise ValueError("this filter was built without the gate: construct it with gate=... (gate=float('inf'): off)")
        self._check(self.lib.ekf_set_gate(self.h, g))
        self.gate = g

    def last_gate_stats(self) -> dict:
        """Detections the last observe call tested and rejected (ekf_last_gate_stats)."""
        out = (C.c_int64 * 2)()
        self._check(self.lib.ekf_last_gate_stats(self.h, out))
        return {"tested": int(out[0]), "rejected": int(out[1])}

    def _check(self, rc):
        if rc != 0:
            raise EkfError(rc, self.lib.ekf_last_error_string().decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ekf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- filter operations -------------------------------------------------
    @property
    def num_landmarks(self) -> int:
        return self.lib.ekf_num_landmarks(self.h)

    @property
    def dims(self) -> int:
        return self.lm_dims * self.num_landmarks + 10

    def reset(self, initial_pose):
        p = np.ascontiguousarray(initial_pose, dtype=np.float64)
        assert p.shape == (10,)
        self._check(self.lib.ekf_reset(self.h, _dptr(p)))
        self._map_frozen = False      # (ekf_reset clears the flag: a reset filter has no map)

    def grow(self, new_max_landmarks: int | None = None, new_max_visible: int | None = None):
        """Move the filter into buffers for a larger capacity (ekf_grow): new tensors sized by ekf_query_sizes, the library
        copies state / covariance device to device and re-binds; the old tensors are released afterwards."""
        torch = self._torch
        cfg = self.cfg
        new_max_landmarks = self.max_landmarks if new_max_landmarks is None else int(new_max_landmarks)
        new_max_visible = self.max_visible if new_max_visible is None else int(new_max_visible)
        ncfg = EkfConfig()
        C.memmove(C.byref(ncfg), C.byref(cfg), C.sizeof(EkfConfig))
        ncfg.max_landmarks = int(new_max_landmarks)
        ncfg.max_visible = int(new_max_visible)
        with torch.cuda.device(self.device):
            ld, cb, sb, wb = C.c_int64(), C.c_size_t(), C.c_size_t(), C.c_size_t()
            self._check(self.lib.ekf_query_sizes(C.byref(ncfg), C.byref(ld), C.byref(cb), C.byref(sb), C.byref(wb)))
            cov_t = torch.empty((ld.value, ld.value), dtype=self.cov_t.dtype, device=self.device)
            state_t = torch.empty((sb.value // 8,), dtype=torch.float64, device=self.device)
            ws_t = torch.empty((wb.value,), dtype=torch.uint8, device=self.device)
            torch.cuda.synchronize(self.device)
            self._check(self.lib.ekf_grow(self.h, int(new_max_landmarks), int(new_max_visible), cov_t.data_ptr(), ld.value,
                                          state_t.data_ptr(), ws_t.data_ptr(), wb.value))
        self.cov_t, self.state_t, self.ws_t, self.ld = cov_t, state_t, ws_t, ld.value
        self.cfg = ncfg
        self.max_landmarks, self.max_visible = int(new_max_landmarks), int(new_max_visible)

    def remove_markers(self, indices):
        """Delete the landmarks with these indices (distinct, any order) from state and covariance on the device
        (ekf_remove_markers): new tensors of the filter's own sizes, allocated on the filter's stream, receive the kept
        rows and columns, the library borrows them, and ``cov_t`` / ``state_t`` are swapped.  Kept landmarks keep their
        order: new index = old index - (removed indices below it).  Nothing is synchronised."""
        torch = self._torch
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            cov_t, state_t = torch.empty_like(self.cov_t), torch.empty_like(self.state_t)
        self._remove_into(indices, cov_t, state_t)

    def _remove_into(self, indices, cov_t, state_t):
        """``remove_markers`` into tensors of the caller (shapes and dtypes of ``cov_t`` / ``state_t``), which the filter
        keeps; an empty list leaves them unwritten and unused."""
        torch = self._torch
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        assert cov_t.shape == self.cov_t.shape and cov_t.dtype == self.cov_t.dtype and cov_t.is_contiguous()
        assert state_t.shape == self.state_t.shape and state_t.dtype == self.state_t.dtype
        nbytes = C.c_size_t()
        self._check(self.lib.ekf_remove_workspace_bytes(self.h, idx.shape[0], C.byref(nbytes)))
        # (the new tensors may have been filled on the caller's current stream)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=self.device)
            self._check(self.lib.ekf_remove_markers(self.h, _iptr(idx), idx.shape[0], cov_t.data_ptr(), self.ld,
                                                    state_t.data_ptr(), ws.data_ptr(), nbytes.value))
            if idx.shape[0] == 0:
                return
            # (old and new tensors may come from another stream: the allocator keeps them until this one has passed the call)
            for t in (cov_t, state_t, self.cov_t, self.state_t):
                t.record_stream(self.stream)
        self.cov_t, self.state_t = cov_t, state_t

    def add_markers(self, xyz, uncertainty=None):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 6 if self.lm_dims == 10 else 3)
        if self.num_landmarks + xyz.shape[0] > self.max_landmarks:      # the reference appends without limit (:274-290)
            self.grow(max(2 * self.max_landmarks, self.num_landmarks + xyz.shape[0]))
        unc = None
        if uncertainty is not None:
            unc = np.ascontiguousarray(
                np.broadcast_to(np.asarray(uncertainty, dtype=np.float64), (xyz.shape[0], self.lm_dims)))
        self._check(self.lib.ekf_add_markers(self.h, _dptr(xyz), _dptr(unc) if unc is not None else None,
                                             xyz.shape[0]))

    def observe(self, lm_index, z, exempt=None, mahal=False, rows=None, scale=None, motion=None):
        """One frame.  With ``exempt`` (bool [m]: detections the gate leaves alone, d^2 = 0) or ``mahal=True`` the frame
        goes through ekf_observe_gated (a filter built with ``gate=``) and returns every detection's d^2 [m]; a set gate
        acts either way.
        ``rows`` ([m] or [m, rd] variances; a filter built with ``row_noise=True``): the frame's measurement noise is
        diag(rows) instead of r_uncertainty I (ekf_observe_rows).
        ``scale`` (a number >= 0; a filter built with ``frame_scale=True``): the frame's process-noise scale
        (ekf_observe_scaled); None: the frame carries none.
        ``motion`` ([6] = (d, w); a filter built with ``motion=True``): the camera moves first (ekf_observe_moved; without
        a scale ekf_move and then the call without it, which is the same thing); None: the frame carries none."""
        idx = np.ascontiguousarray(lm_index, dtype=np.int32)
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, self.rows_per_detection)
        assert idx.shape[0] == z.shape[0]
        self._last_m = idx.shape[0]
        if idx.shape[0] > self.max_visible:      # the reference takes any number of detections per frame (:158-200)
            self.grow(new_max_visible=min(self.MAX_VISIBLE_LIMIT[self.lm_dims], max(2 * self.max_visible, idx.shape[0])))
        if rows is not None:
            rows = self._rows(rows, idx.shape[0])
        if scale is not None:
            scale = self._scale(scale)
        if motion is not None:
            motion = self._motion(motion)
            if scale is None:
                self._check(self.lib.ekf_move(self.h, _dptr(motion)))
                motion = None
        if exempt is None and not mahal and rows is None and scale is None:
            self._check(self.lib.ekf_observe(self.h, _iptr(idx), _dptr(z), idx.shape[0]))
            return None
        ex = None
        if exempt is not None:
            ex = np.ascontiguousarray(exempt, dtype=np.uint8).reshape(-1)
            assert ex.shape[0] == idx.shape[0]
        d2 = np.empty(idx.shape[0]) if mahal else None
        if scale is not None:
            self._check(self.lib.ekf_observe_moved(self.h, _iptr(idx), _dptr(z),
                                                   _dptr(rows) if rows is not None else None, idx.shape[0],
                                                   ex.ctypes.data_as(C.POINTER(C.c_uint8)) if ex is not None else None,
                                                   _dptr(d2) if mahal else None, None, scale,
                                                   _dptr(motion) if motion is not None else None))
            return d2
        if rows is not None:
            self._check(self.lib.ekf_observe_rows(self.h, _iptr(idx), _dptr(z), _dptr(rows), idx.shape[0],
                                                  ex.ctypes.data_as(C.POINTER(C.c_uint8)) if ex is not None else None,
                                                  _dptr(d2) if mahal else None, None))
            return d2
        self._check(self.lib.ekf_observe_gated(self.h, _iptr(idx), _dptr(z), idx.shape[0],
                                               ex.ctypes.data_as(C.POINTER(C.c_uint8)) if ex is not None else None,
                                               _dptr(d2) if mahal else None, None))
        return d2

    def observe_sequence(self, idx_t, z_t, traj_t=None, rows=None, scale=None, motion=None):
        """idx_t int32 [F,m], z_t float64 [F,m,3] device tensors (resident
        detections); traj_t float64 [F,7] or None; rows: float64 device tensor [F,m,rd] of row variances (the caller's
        contract: finite, > 0; a filter built with ``row_noise=True``) or None; scale: [F] numbers >= 0 on the host (a
        filter built with ``frame_scale=True``) or None; motion: [F, 6] camera motions on the host (a filter built with
        ``motion=True``: serial order) or None.  Every call is ekf_observe_sequence_device_moved, NULL for what is None."""
        frames, m = idx_t.shape
        assert idx_t.is_cuda and z_t.is_cuda and idx_t.is_contiguous() and z_t.is_contiguous()
        assert tuple(z_t.shape) == (frames, m, self.rows_per_detection)
        self._last_m = m
        if motion is not None:
            motion = self._motion(motion, frames)
        if scale is not None:
            scale = self._scale(scale, frames)
        if rows is not None:
            if not self.can_row_noise:
                raise ValueError("this filter was built without per-detection noise: construct it with row_noise=True")
            assert rows.is_cuda and rows.dtype == self._torch.float64 and rows.is_contiguous()
            assert tuple(rows.shape) == tuple(z_t.shape)
        # (the narrower entry points are this one with NULL for what they lack)
        self._check(self.lib.ekf_observe_sequence_device_moved(
            self.h, idx_t.data_ptr(), z_t.data_ptr(), rows.data_ptr() if rows is not None else None,
            _dptr(scale) if scale is not None else None, _dptr(motion) if motion is not None else None, m, frames,
            traj_t.data_ptr() if traj_t is not None else None))

    def observe_log(self, lm_index, offsets, poses, traj=None, mahal=None, rows=None, scale=None, motion=None, history=None):
        """A whole detection log in one call (ekf_observe_log): lm_index int [D] landmark index of every detection (first
        sightings numbered n, n+1, ... in order of first occurrence), offsets int [F+1], poses [D,6] ``[tvec | rvec]`` as a
        NumPy array (uploaded once) or a contiguous float64 device tensor on this filter's device; traj: float64 device
        tensor [F,7] that receives state[0:7] after every frame, or None; mahal: float64 device tensor [D] that receives
        every detection's d^2 (ekf_observe_log_gated; a filter built with ``gate=``), or None; rows: [D] or [D, rd] row
        variances, indexed like lm_index (NumPy, validated and uploaded; a filter built with ``row_noise=True``), or None;
        scale: [F] numbers >= 0, one per frame, empty frames included (a filter built with ``frame_scale=True``;
        ekf_observe_log_scaled), or None; motion: [F, 6] camera motions, one per frame, empty frames included (a filter
        built with ``motion=True``; ekf_observe_log_moved: serial order), or None; history: a uint8 device tensor of at
        least ``history_bytes(lm_index, offsets)`` bytes that receives the records of the call (ekf_observe_log_recorded:
        serial order, the same bits; ``smooth_history`` runs the backward pass over it), or None.
        Capacity must already suffice (grow() first)."""
        torch = self._torch
        idx = np.ascontiguousarray(lm_index, dtype=np.int32).reshape(-1)
        offs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if offs.shape[0] < 1:
            raise ValueError("offsets needs F+1 >= 1 entries")
        frames = offs.shape[0] - 1
        if isinstance(poses, torch.Tensor):
            if not (poses.is_cuda and poses.device == self.device):
                raise ValueError(f"poses must be on {self.device} (got {poses.device})")
            if poses.dtype != torch.float64 or not poses.is_contiguous():
                raise ValueError("poses must be a contiguous float64 tensor")
        else:
            poses = np.ascontiguousarray(poses, dtype=np.float64)
        if tuple(poses.shape) != (idx.shape[0], 6):
            raise ValueError(f"poses must have shape ({idx.shape[0]}, 6), got {tuple(poses.shape)}")
        if traj is not None:
            assert traj.is_cuda and traj.dtype == torch.float64 and traj.is_contiguous()
            assert tuple(traj.shape) == (frames, 7)
        if mahal is not None:
            assert mahal.is_cuda and mahal.dtype == torch.float64 and mahal.is_contiguous()
            assert tuple(mahal.shape) == (idx.shape[0],)
        if rows is not None:
            rows = self._rows(rows, idx.shape[0])
        if scale is not None:
            scale = self._scale(scale, frames)
        if motion is not None:
            motion = self._motion(motion, frames)
        nbytes = C.c_size_t()
        self._check(self.lib.ekf_log_workspace_bytes(self.h, idx.shape[0], C.byref(nbytes)))
        # device tensors of the caller (poses, traj) were produced on its current stream
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            # (allocated and uploaded on the filter's stream: the caching allocator keeps them until it has passed them)
            if isinstance(poses, torch.Tensor):
                poses.record_stream(self.stream)
                poses_t = poses
            else:
                poses_t = torch.from_numpy(poses).to(self.device, non_blocking=False)
            ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=self.device)
            if traj is not None:
                traj.record_stream(self.stream)
            if mahal is not None:
                mahal.record_stream(self.stream)
            rows_t = torch.from_numpy(rows).to(self.device, non_blocking=False) if rows is not None else None
            args = (self.h, _iptr(idx), _lptr(offs), frames, poses_t.data_ptr() if idx.shape[0] else None,
                    rows_t.data_ptr() if rows_t is not None and idx.shape[0] else None,
                    _dptr(scale) if scale is not None and frames else None,
                    _dptr(motion) if motion is not None and frames else None, ws.data_ptr(), nbytes.value,
                    traj.data_ptr() if traj is not None else None,
                    mahal.data_ptr() if mahal is not None and idx.shape[0] else None)
            if history is None:
                self._check(self.lib.ekf_observe_log_moved(*args))
            else:
                assert history.is_cuda and history.dtype == torch.uint8 and history.is_contiguous()
                history.record_stream(self.stream)
                self._check(self.lib.ekf_observe_log_recorded(*args, history.data_ptr(), history.numel()))
                self._history_frames = frames
        self._log_keep = (poses_t, ws, rows_t)     # (released by the next call; record_stream already guards the allocator)
        m = np.diff(offs)
        if m.size and m.max() > 0:
            self._last_m = int(m[m > 0][-1])

    # -- offline smoothing (include/ekf_slam_hip.h, "Offline smoothing") --------------------------------------------------
    def history_bytes(self, lm_index, offsets) -> int:
        """Upper bound of the history a recorded replay of this log needs, from the log alone (ekf_history_bytes)."""
        idx = np.ascontiguousarray(lm_index, dtype=np.int32).reshape(-1)
        offs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        out = C.c_size_t()
        self._check(self.lib.ekf_history_bytes(self.h, _iptr(idx), _lptr(offs), offs.shape[0] - 1, C.byref(out)))
        return out.value

    def new_history(self, lm_index, offsets):
        """A uint8 device tensor of ``history_bytes`` bytes, allocated on the filter's stream."""
        torch = self._torch
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            return torch.empty((self.history_bytes(lm_index, offsets),), dtype=torch.uint8, device=self.device)

    def history_info(self) -> dict:
        """The table of the last recorded replay (ekf_history_info): {"frame", "dims", "s_eff", "motion" [R, 6], "stepped"}
        per record and "frame_record" [F] (-1: before the first record)."""
        count = C.c_int32()
        self._check(self.lib.ekf_history_info(self.h, C.byref(count), 0, None, None, None, None, None, None))
        r = count.value
        frame, dims, stepped = (np.zeros(max(r, 1), dtype=np.int32) for _ in range(3))
        s_eff, motion = np.zeros(max(r, 1)), np.zeros((max(r, 1), 6))
        frec = np.zeros(max(self._history_frames, 1), dtype=np.int32)
        self._check(self.lib.ekf_history_info(self.h, C.byref(count), max(r, 1), _iptr(frame), _iptr(dims), _dptr(s_eff),
                                              _dptr(motion), _iptr(stepped), _iptr(frec)))
        return {"frame": frame[:r], "dims": dims[:r], "s_eff": s_eff[:r], "motion": motion[:r], "stepped": stepped[:r].astype(bool),
                "frame_record": frec[:self._history_frames]}

    def history_record(self, history, r: int, dims: int):
        """(state [dims], P [dims, dims]) of record r, unpacked and mirrored (ekf_history_record)."""
        state, cov = np.empty(dims), np.empty((dims, dims))
        self._check(self.lib.ekf_history_record(self.h, history.data_ptr(), int(r), _dptr(state), _dptr(cov), int(dims)))
        return state, cov

    def smooth_history(self, history, frames: int, blocked: bool = False):
        """The backward pass over the last recorded replay (ekf_smooth_history): a float64 device tensor [frames, 7] of
        smoothed poses.  ``blocked``: force the blocked tier (flags bit 0).  Waits for the filter's stream."""
        torch = self._torch
        nbytes = C.c_size_t()
        self._check(self.lib.ekf_smooth_workspace_bytes(self.h, C.byref(nbytes)))
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=self.device)
            out = torch.empty((frames, 7), dtype=torch.float64, device=self.device)
            history.record_stream(self.stream)
            self._check(self.lib.ekf_smooth_history(self.h, history.data_ptr(), history.numel(), ws.data_ptr(), nbytes.value,
                                                    int(bool(blocked)), out.data_ptr() if frames else None))
        return out

    def smooth_history_cov(self, history, frames: int, ws_bytes=None):
        """The backward pass with the smoothed covariances (ekf_smooth_history_cov): float64 device tensors {"smoothed"
        [frames, 7], "cam_cov" [frames, 10, 10] (P^s[0:10, 0:10] of every frame's record), "filt_cam_cov" [frames, 10, 10]
        (P_r[0:10, 0:10]), "first_cov" [N_0, N_0] (P^s_0; None without records)}.  Covariance rows of frames before the
        first record are NaN.  ``ws_bytes``: the workspace size to pass (default: what the library asks for).  Waits for
        the filter's stream."""
        torch = self._torch
        nbytes = C.c_size_t()
        self._check(self.lib.ekf_smooth_cov_workspace_bytes(self.h, C.byref(nbytes)))
        count = C.c_int32()
        self._check(self.lib.ekf_history_info(self.h, C.byref(count), 0, None, None, None, None, None, None))
        n0 = int(self.history_info()["dims"][0]) if count.value else 0
        given = nbytes.value if ws_bytes is None else int(ws_bytes)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            ws = torch.empty((max(given, nbytes.value),), dtype=torch.uint8, device=self.device)
            out = {"smoothed": torch.empty((frames, 7), dtype=torch.float64, device=self.device),
                   "cam_cov": torch.empty((frames, 10, 10), dtype=torch.float64, device=self.device),
                   "filt_cam_cov": torch.empty((frames, 10, 10), dtype=torch.float64, device=self.device),
                   "first_cov": torch.empty((n0, n0), dtype=torch.float64, device=self.device) if n0 else None}
            history.record_stream(self.stream)
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
            self._check(self.lib.ekf_smooth_history_cov(self.h, history.data_ptr(), history.numel(), ws.data_ptr(), given, 0,
                                                        ptr(out["smoothed"]), ptr(out["cam_cov"]), ptr(out["filt_cam_cov"]),
                                                        ptr(out["first_cov"])))
        return out

    LOG_STATS = ("frames_stepped", "frames_pipelined", "pipelined_runs", "markers_added")

    def last_log_stats(self) -> dict:
        """What the last observe_log call did (ekf_last_log_stats)."""
        out = (C.c_int64 * 4)()
        self._check(self.lib.ekf_last_log_stats(self.h, out))
        return dict(zip(self.LOG_STATS, (int(v) for v in out)))

    SEQUENCE_MODES = {0: "none", 1: "serial", 2: "pipelined", 3: "serial (the two streams share one hardware queue)",
                      4: "serial (another handle of the process is pipelining)"}

    def last_sequence_mode(self) -> str:
        """What the last observe_sequence call did (ekf_last_sequence_mode)."""
        return self.SEQUENCE_MODES[self.lib.ekf_last_sequence_mode(self.h)]

    def sync(self):
        self._check(self.lib.ekf_sync(self.h))

    def get_state(self, count=None):
        n = self.dims if count is None else count
        out = np.empty(n)
        self._check(self.lib.ekf_get_state(self.h, _dptr(out), n))
        return out

    def get_cov_diag(self):
        out = np.empty(self.dims)
        self._check(self.lib.ekf_get_cov_diag(self.h, _dptr(out), self.dims))
        return out

    def get_cov(self):
        n = self.dims
        out = np.empty((n, n))
        self._check(self.lib.ekf_get_cov(self.h, _dptr(out), n))
        return out

    def set_state_cov(self, state, cov):
        state = np.ascontiguousarray(state, dtype=np.float64)
        n_lm = (state.shape[0] - 10) // self.lm_dims
        if n_lm > self.max_landmarks:
            self.grow(n_lm)
        self._check(self.lib.ekf_set_state(self.h, _dptr(state), n_lm))
        cov = np.ascontiguousarray(cov, dtype=np.float64)
        assert cov.shape == (state.shape[0], state.shape[0])
        self._check(self.lib.ekf_set_cov(self.h, _dptr(cov), state.shape[0]))

    # -- instrumentation -----------------------------------------------------
    def set_kernel_timing(self, enable):
        """False/0 off, True/1 all kernels, 2 covariance update only."""
        self._check(self.lib.ekf_set_kernel_timing(self.h, int(enable)))

    def kernel_timing(self):
        out = {}
        for i, name in enumerate(self.KERNEL_NAMES):
            us, cnt = C.c_double(), C.c_int64()
            self._check(self.lib.ekf_get_kernel_timing(self.h, i, C.byref(us), C.byref(cnt)))
            out[name] = (us.value, cnt.value)
        if self.fused:
            # one launch: slot 0 is the whole front kernel, slots 1-2 are empty event gaps
            out = {"front": out["gather"], "cov_update": out["cov_update"]}
        return out

    def set_fused(self, enable: bool):
        """Fused front kernel (True) or the three stage kernels (False) from the next frame on."""
        self._check(self.lib.ekf_set_fused(self.h, int(bool(enable))))
        # the library flips flags bit 2 of its own copy of the configuration; grow() sizes the new workspace from this one
        # (the second covariance buffer of the pipelined sequence mode exists only without bit 2), so keep them in step
        if enable:
            self.cfg.flags &= ~4
        else:
            self.cfg.flags |= 4
        self.fused = bool(enable)

    def debug_enable_w(self):
        dummy = np.zeros(1)
        self._check(self.lib.ekf_debug_fetch(self.h, -1, _dptr(dummy), 1))

    def debug_enable_stamps(self, light: bool = False):
        """In-kernel time stamps of the front kernel without the debug copies of W / L (production code path).
        `light`: only the stamps at the start / end of the roles (the others perturb what they measure)."""
        dummy = np.zeros(1)
        self._check(self.lib.ekf_debug_fetch(self.h, -3 if light else -2, _dptr(dummy), 1))

    def debug_fetch(self, what: str, m: int):
        rd = self.rows_per_detection
        k, kp, n = rd * m, -(-rd * m // 16) * 16, self.dims
        shape = {"jac": (k, 20 if rd == 7 else 13), "resid": (k,), "L": (kp, kp), "W": (kp, n), "A": (k, n),
                 "stamps": (64,), "gate_log": (GATE_LOG_FRAMES, 4)}[what]
        code = {"jac": 0, "resid": 1, "L": 2, "W": 3, "A": 4, "stamps": 5, "gate_log": 6}[what]
        out = np.empty(shape)
        self._check(self.lib.ekf_debug_fetch(self.h, code, _dptr(out), out.size))
        return out
