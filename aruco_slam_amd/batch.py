"""``EKFBatch``: many independent ``EKF`` or ``EKF_Rotations`` filters replayed at once on one GPU (the batch C ABI of
``include/ekf_slam_hip.h``, kernels ``csrc/ekf_batch.hip`` and ``csrc/ekf_batch_rot.hip``).

What users of a filter of this size run is many sequences: a set of recorded runs, a sweep of the noise constants, Monte-Carlo
studies on re-noised detections.  Each member is ``BaseFilter.process_detection_log`` with ``should_filter=True`` over its
own log, with its own initial pose, noise constants and marker-id -> landmark-index table; one workgroup owns one member, so
a batch fills the GPU where a single filter of this size leaves it almost idle.  All members share the model, the quaternion
convention, an f64 covariance and the capacity: ``model="ekf"`` (``EKF``) holds ``max_landmarks`` <= 82 and ``max_visible``
<= 16, ``model="ekf_rotations"`` (``EKF_Rotations``, scalar-first quaternions only) ``max_landmarks`` <= 24 and
``max_visible`` <= 8.  With ``large_maps`` (``EKF_FLAG_BATCH_LARGE_MAPS``, kernel ``csrc/ekf_batch_wide.hip``) the maps
grow to dictionary size: ``max_landmarks`` <= 338 (``EKF``) or <= 101 (``EKF_Rotations``), same ``max_visible``.  With
``wide_frames`` (``EKF_FLAG_BATCH_WIDE_FRAMES``, the same kernel) a frame may hold as many detections as
a default single filter takes: ``max_visible`` <= 64 (``EKF``) or <= 50 (``EKF_Rotations``), on the large-map limits of
``max_landmarks``; a frame is factorised in blocks of 16 / 8 detections, and one of at most 16 / 8 detections gives the same
bits as a batch without the flag.  A batch never grows; there is no CPU fallback.

Monte-Carlo studies need no host-side re-noising: ``replay_replicas`` replays ONE log in every member, each as a numbered
replica whose detection noise the device draws (``csrc/ekf_batch_replicas.hip``; ``replica_poses`` returns exactly the
poses a replica consumed).  Runs and sweeps are judged by the filter's own statistics: with ``nis`` / ``cam_cov`` both replay
calls also return every frame's normalised innovation squared and camera covariance P[0:10, 0:10].

The detector's noise is on the four pixel corners of a marker, and IPPE turns it into what pose noise never gives: a depth
error that grows with distance, an error that depends on the marker's tilt and, now and then, the other of its two
solutions.  ``replay_corner_replicas`` replays a log of ``corners`` the same way, the noise drawn in pixels and every pose
estimated on the device (``csrc/ekf_batch_corner_replicas.hip``, the IPPE of ``hip_backend.estimate_poses``), and returns
``flipped``: which (replica, detection) pairs got the flipped solution, the ground truth for tuning the gate below.
``replica_corner_poses`` / ``replica_corners`` return what a replica consumed.  With ``set_camera``,
``process_detection_logs`` takes logs of ``corners`` as well.

Outliers (IPPE's flipped poses, mis-decoded ids) are kept out by the per-detection chi-square gate: ``gate`` / ``set_gate``
make every member reject the detections whose own Mahalanobis distance d^2 = r^T S_d^-1 r exceeds its threshold before the
frame is updated, and ``mahal=True`` returns every detection's d^2, gate or no gate (``ekf_batch_set_gate`` in
``include/ekf_slam_hip.h`` has the exact semantics).

Localisation studies run on a surveyed map that must not move: ``freeze_map`` / ``unfreeze_map`` / ``map_frozen`` give every
member the single filter's localisation mode (``BaseFilter.freeze_map``; "Localisation mode of a batch" in
``include/ekf_slam_hip.h``).  A frozen member updates its camera, P_cc and the cross-covariances and leaves its landmarks and
P_ll alone; its frames cost the 10 x N camera strip of P instead of the N x N sweep.  Frozen and mapping members run side by
side in one call.  Detections of ids a frozen member's map does not hold are dropped and reported in ``last_ignored``.

Offline studies ask for the trajectory that a whole log supports: ``smooth_detection_logs`` replays the logs recorded --
the window kernel packs every member behind each frame that changed it -- and runs one Rauch-Tung-Striebel backward pass per
member, one workgroup each ("Batch smoothing" in ``include/ekf_slam_hip.h``; ``EKF.smooth_detection_log`` per member, in one
call).  ``smooth_replicas`` does the same for Monte-Carlo replicas of one log, ``history_records`` returns what was recorded.
With ``cov=True`` both also return the camera blocks of the filtered and the smoothed covariance per frame
(``smooth_history_cov``: the same launch forms ``P^s`` of every member, "Batch smoothing, covariances" in the header).
``model="ekf"`` with ``quat_update="scalar_first"``, at most 50 landmarks per member, without ``large_maps`` / ``wide_frames``.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from .filters.base_filter import plan_detection_log
from .hip_backend import (EKF_FLAG_BATCH_LARGE_MAPS, EKF_FLAG_BATCH_WIDE_FRAMES, EKF_FLAG_FRAME_SCALE, EKF_FLAG_MOTION,
                          EKF_QUAT_AS_WRITTEN, EKF_QUAT_SCALAR_FIRST, EkfConfig, EkfError, _dptr, _iptr, _lptr,
                          frame_scale_array, load_library, motion_array, row_noise_array)

NOISE_KEYS = ("initial_camera_uncertainty", "initial_landmark_uncertainty", "r_uncertainty", "q_cam", "q_err", "q_lm")
EKF_ERR_NUMERIC = -5
QUAT_MODES = {"as_written": EKF_QUAT_AS_WRITTEN, "scalar_first": EKF_QUAT_SCALAR_FIRST}
MODELS = {"ekf": 0, "ekf_rotations": 1}
LM_DIMS = {"ekf": 3, "ekf_rotations": 10}      # landmark dims: a member's state is [LM_DIMS n + 10]
# max_landmarks of the one-column kernels (N <= 256) and of the large-map kernel (N <= 1024)
COLUMN_MAX_LANDMARKS = {"ekf": 82, "ekf_rotations": 24}
LARGE_MAX_LANDMARKS = {"ekf": 338, "ekf_rotations": 101}
# max_visible of the kernels without wide frames and of the wide-frame kernel (the single filter's default limits)
COLUMN_MAX_VISIBLE = {"ekf": 16, "ekf_rotations": 8}
WIDE_MAX_VISIBLE = {"ekf": 64, "ekf_rotations": 50}


def use_large_maps(model: str, max_landmarks: int, large_maps: bool | None = None) -> bool:
    """Whether a batch sets ``EKF_FLAG_BATCH_LARGE_MAPS``: ``None`` only when ``max_landmarks`` exceeds the one-column
    kernel's limit of the model, ``True`` / ``False`` always / never (then a larger map raises as the library rules)."""
    if large_maps is None:
        return int(max_landmarks) > COLUMN_MAX_LANDMARKS[model]
    return bool(large_maps)


def use_wide_frames(model: str, max_visible: int, wide_frames: bool | None = None) -> bool:
    """Whether a batch sets ``EKF_FLAG_BATCH_WIDE_FRAMES``: ``None`` only when ``max_visible`` exceeds the limit of the
    model without the flag (16 / 8), ``True`` / ``False`` always / never (then a wider frame raises as the library rules)."""
    if wide_frames is None:
        return int(max_visible) > COLUMN_MAX_VISIBLE[model]
    return bool(wide_frames)


RD = {"ekf": 3, "ekf_rotations": 7}         # measurement rows per detection: a frame of m detections has RD m rows


class BatchReplay(NamedTuple):
    """``process_detection_logs(..., nis=True / cam_cov=True)``: per-member lists.  ``trajectory[b]`` [F_b, 7]; ``nis[b]``
    [F_b] (None unless asked); ``dof[b]`` [F_b] the frame's row count (3 m or 7 m, duplicate detections counted, 0 for an
    empty frame); ``cam_cov[b]`` [F_b, 10, 10] (None unless asked)."""
    trajectory: list
    nis: list | None
    dof: list
    cam_cov: list | None


class ReplicaReplay(NamedTuple):
    """``replay_replicas``: ``trajectory`` [B, F, 7], ``nis`` [B, F] (None unless asked), ``dof`` [F], ``cam_cov``
    [B, F, 10, 10] (None unless asked)."""
    trajectory: np.ndarray
    nis: np.ndarray | None
    dof: np.ndarray
    cam_cov: np.ndarray | None


class GatedBatchReplay(NamedTuple):
    """``process_detection_logs`` with ``mahal=True`` or a gate set: ``BatchReplay``'s fields (``dof[b]`` counts the
    surviving detections only), then per member ``mahal[b]`` [D_b], every detection's d^2 aligned with the log's own
    detections (0: exempt first sighting; NaN: not tested, dropped by the planner included), and ``rejected[b]`` [D_b]
    bool, ``mahal[b] > gate[b]``."""
    trajectory: list
    nis: list | None
    dof: list
    cam_cov: list | None
    mahal: list
    rejected: list


class GatedReplicaReplay(NamedTuple):
    """``replay_replicas`` with ``mahal=True`` or a gate set: ``ReplicaReplay``'s fields with ``dof`` [B, F] counting each
    member's surviving detections, then ``mahal`` [B, D] and ``rejected`` [B, D] as in ``GatedBatchReplay``."""
    trajectory: np.ndarray
    nis: np.ndarray | None
    dof: np.ndarray
    cam_cov: np.ndarray | None
    mahal: np.ndarray
    rejected: np.ndarray


class CornerReplicaReplay(NamedTuple):
    """``replay_corner_replicas``: ``trajectory`` [B, F, 7], ``nis`` [B, F] and ``cam_cov`` [B, F, 10, 10] (None unless
    asked), ``dof`` [F], ``mahal`` and ``rejected`` None; with ``mahal=True`` or a gate set ``dof`` [B, F] counts each
    member's surviving detections and ``mahal`` / ``rejected`` are [B, D] as in ``GatedReplicaReplay``.  ``flipped`` [B, D]
    bool, aligned with the log's own detections: IPPE returned the candidate farther from the clean pose (the definition
    in ``include/ekf_slam_hip.h``); False for the detections the planner dropped."""
    trajectory: np.ndarray
    nis: np.ndarray | None
    dof: np.ndarray
    cam_cov: np.ndarray | None
    mahal: np.ndarray | None
    rejected: np.ndarray | None
    flipped: np.ndarray


def gate_array(gate, members: int):
    """``gate`` (None, a scalar or [members]) as None or a contiguous [members] array; every entry must be > 0 (``inf``:
    that member's gate is off); ``ValueError`` otherwise."""
    if gate is None:
        return None
    g = np.asarray(gate, dtype=np.float64)
    if g.ndim == 0:
        g = np.broadcast_to(g, (members,))
    elif g.shape != (members,):
        raise ValueError(f"gate must be a scalar or [{members}], got shape {g.shape}")
    if not (g > 0).all():
        raise ValueError("gate must be > 0 (inf: off) and not NaN")
    return np.ascontiguousarray(g)


def _surviving_dof(rd: int, offsets: np.ndarray, rejected: np.ndarray) -> np.ndarray:
    """Rows per frame over the detections that were not rejected (offsets [F+1] into rejected [D])."""
    kept = np.concatenate([np.zeros(1, np.int64), np.cumsum(~rejected, dtype=np.int64)])
    return rd * (kept[offsets[1:]] - kept[offsets[:-1]])


def replica_sigma(sigma, replicas: int) -> np.ndarray:
    """``sigma`` (a scalar, [6] or [replicas, 6]; finite, >= 0) as a contiguous [replicas, 6] array; ``ValueError``
    otherwise."""
    s = np.asarray(sigma, dtype=np.float64)
    if s.ndim == 0 or s.shape == (6,):
        s = np.broadcast_to(s, (replicas, 6))
    elif s.shape != (replicas, 6):
        raise ValueError(f"sigma must be a scalar, [6] or [{replicas}, 6], got shape {s.shape}")
    if not np.isfinite(s).all() or (s < 0).any():
        raise ValueError("sigma must be finite and >= 0")
    return np.ascontiguousarray(s)


def replica_sigma_px(sigma_px, replicas: int) -> np.ndarray:
    """``sigma_px`` (a scalar or [replicas]; finite, >= 0) as a contiguous [replicas] array; ``ValueError`` otherwise."""
    s = np.asarray(sigma_px, dtype=np.float64)
    if s.ndim == 0:
        s = np.broadcast_to(s, (replicas,))
    elif s.shape != (replicas,):
        raise ValueError(f"sigma_px must be a scalar or [{replicas}], got shape {s.shape}")
    if not np.isfinite(s).all() or (s < 0).any():
        raise ValueError("sigma_px must be finite and >= 0")
    return np.ascontiguousarray(s)


def camera_arrays(camera_matrix, dist_coeffs=None, marker_size: float = 0.16):
    """The camera of the pose front end as the C ABI takes it: (camera matrix [9], distortion coefficients [0..8],
    marker size); ``ValueError`` for another shape, non-finite values, focal lengths or a marker size that are not > 0."""
    k = np.asarray(camera_matrix, dtype=np.float64)
    if k.shape != (3, 3):
        raise ValueError(f"camera_matrix must be 3 x 3, got shape {k.shape}")
    d = np.asarray([] if dist_coeffs is None else dist_coeffs, dtype=np.float64).reshape(-1)
    if d.size > 8:
        raise ValueError(f"0..8 distortion coefficients (k1 k2 p1 p2 k3 k4 k5 k6) are supported, got {d.size}")
    if not (np.isfinite(k).all() and np.isfinite(d).all()):
        raise ValueError("camera_matrix and dist_coeffs must be finite")
    if not (k[0, 0] > 0 and k[1, 1] > 0):
        raise ValueError("focal lengths must be > 0")
    size = float(marker_size)
    if not (np.isfinite(size) and size > 0):
        raise ValueError(f"marker_size must be > 0, got {marker_size}")
    return np.ascontiguousarray(k.reshape(9)), np.ascontiguousarray(d), size


def _replica_range(first_replica, replicas: int) -> int:
    r0 = int(first_replica)
    if r0 < 0 or r0 + int(replicas) > 2 ** 32:
        raise ValueError(f"first_replica must be >= 0 with first_replica + {replicas} <= 2**32, got {r0}")
    return r0


def _seed(seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2**64)")
    return seed


def replica_poses(poses, sigma, seed: int, *, replicas: int | None = None, first_replica: int = 0,
                  device: str = "cuda:0") -> np.ndarray:
    """The noisy poses [R, D, 6] that replicas ``first_replica`` .. ``first_replica + R - 1`` of a log with ``poses`` [D, 6]
    consume in ``EKFBatch.replay_replicas`` (``ekf_batch_replica_poses``, the same device code): ``poses[d][c] +
    sigma[r][c] g_c(seed, r, d)`` with the Philox4x32-10 / Box-Muller normals defined in ``include/ekf_slam_hip.h``.
    ``sigma``: a scalar, [6] or [R, 6]; R = ``replicas``, or sigma's rows."""
    import torch
    lib = load_library()
    if not torch.cuda.is_available():
        raise RuntimeError("replica noise is generated on a HIP device (no CPU fallback)")
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    if poses.ndim != 2 or poses.shape[1] != 6:
        raise ValueError(f"poses must have shape (D, 6), got {poses.shape}")
    if replicas is None:
        s = np.asarray(sigma)
        if s.ndim != 2:
            raise ValueError("give replicas= unless sigma is [R, 6]")
        replicas = s.shape[0]
    sig = replica_sigma(sigma, int(replicas))
    r0, seed = _replica_range(first_replica, replicas), _seed(seed)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        src = torch.from_numpy(poses).to(dev)
        out = torch.empty((int(replicas), poses.shape[0], 6), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev)
        rc = lib.ekf_batch_replica_poses(src.data_ptr() if poses.shape[0] else None, poses.shape[0], _dptr(sig),
                                         int(replicas), seed, r0, out.data_ptr() if out.numel() else None,
                                         stream.cuda_stream)
        if rc != 0:
            raise EkfError(rc, lib.ekf_last_error_string().decode())
        stream.synchronize()
    return out.cpu().numpy()


def _replica_corner_outputs(want, corners, sigma_px, seed, camera_matrix, dist_coeffs, marker_size, replicas, first_replica,
                            device):
    """``ekf_batch_replica_corners`` with the outputs named in ``want`` (of "poses", "flipped", "noisy"), as host arrays."""
    import torch
    lib = load_library()
    if not torch.cuda.is_available():
        raise RuntimeError("replica noise is generated on a HIP device (no CPU fallback)")
    corners = np.ascontiguousarray(corners, dtype=np.float64)
    if corners.ndim != 3 or corners.shape[1:] != (4, 2):
        raise ValueError(f"corners must have shape (D, 4, 2), got {corners.shape}")
    if replicas is None:
        if np.ndim(sigma_px) != 1:
            raise ValueError("give replicas= unless sigma_px is [R]")
        replicas = np.shape(sigma_px)[0]
    R, D = int(replicas), corners.shape[0]
    sig = replica_sigma_px(sigma_px, R)
    r0, seed = _replica_range(first_replica, R), _seed(seed)
    k, d, size = camera_arrays(camera_matrix, dist_coeffs, marker_size)
    dev = torch.device(device)
    shapes = {"poses": ((R, D, 6), torch.float64), "flipped": ((R, D), torch.uint8), "noisy": ((R, D, 4, 2), torch.float64)}
    with torch.cuda.device(dev):
        src = torch.from_numpy(corners).to(dev)
        out = {name: torch.empty(shapes[name][0], dtype=shapes[name][1], device=dev) for name in want}
        ptr = (lambda name: out[name].data_ptr() if name in out and out[name].numel() else None)
        stream = torch.cuda.current_stream(dev)
        rc = lib.ekf_batch_replica_corners(src.data_ptr() if D else None, D, _dptr(sig), R, seed, r0, size, _dptr(k),
                                           _dptr(d) if d.size else None, int(d.size), ptr("poses"), ptr("flipped"),
                                           ptr("noisy"), stream.cuda_stream)
        if rc != 0:
            raise EkfError(rc, lib.ekf_last_error_string().decode())
        stream.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


def replica_corner_poses(corners, sigma_px, seed: int, camera_matrix, dist_coeffs=None, marker_size: float = 0.16, *,
                         replicas: int | None = None, first_replica: int = 0, flipped: bool = False,
                         device: str = "cuda:0"):
    """The poses [R, D, 6] that replicas ``first_replica`` .. ``first_replica + R - 1`` of a log with ``corners`` [D, 4, 2]
    (pixels) consume in ``EKFBatch.replay_corner_replicas`` (``ekf_batch_replica_corners``, the same device code): IPPE of
    ``corners[d][i] + sigma_px[r] (g_u, g_v)`` with the Philox4x32-10 / Box-Muller normals defined in
    ``include/ekf_slam_hip.h``.  ``sigma_px``: a scalar or [R]; R = ``replicas``, or sigma_px's length.  With ``flipped``
    it returns ``(poses, flipped [R, D] bool)``: the pairs for which IPPE returned the candidate farther from the pose of
    the clean corners."""
    out = _replica_corner_outputs(("poses", "flipped") if flipped else ("poses",), corners, sigma_px, seed, camera_matrix,
                                  dist_coeffs, marker_size, replicas, first_replica, device)
    return (out["poses"], out["flipped"].astype(bool)) if flipped else out["poses"]


def replica_corners(corners, sigma_px, seed: int, camera_matrix, dist_coeffs=None, marker_size: float = 0.16, *,
                    replicas: int | None = None, first_replica: int = 0, device: str = "cuda:0") -> np.ndarray:
    """The noisy corners [R, D, 4, 2] behind ``replica_corner_poses`` (same arguments)."""
    return _replica_corner_outputs(("noisy",), corners, sigma_px, seed, camera_matrix, dist_coeffs, marker_size, replicas,
                                   first_replica, device)["noisy"]


def corner_row_noise(log, sigma_px, seed: int, replicas: int, camera_matrix, dist_coeffs=None, marker_size: float = 0.16,
                     model: str = "ekf", *, device: str = "cuda:0") -> np.ndarray:
    """Per-detection measurement noise [D, RD] of a log of ``corners`` [D, 4, 2] from its own Monte-Carlo front end: the
    variance over ``replicas`` corner replicas (``replica_corner_poses`` with one ``sigma_px`` for all of them: pixel
    noise on the corners, IPPE on the device) of the z each model forms from a pose -- ``EKF``: the tvec; ``EKF_Rotations``:
    ``[tvec | quaternion of the xyz Euler angles rvec]``, the mapping ``EKF_Rotations.observe`` uses.  ``numpy.var`` over
    the replica axis (host arithmetic on device-drawn poses).  Depth rows grow with distance and tilt, and a detection whose
    IPPE solution flips in some replicas gets large quaternion rows: what ``noise=`` of the observe calls and ``"noise"``
    of a batch log take.  A variance that comes out zero (``sigma_px = 0``) is not a valid row."""
    if model not in MODELS:
        raise ValueError(f"model must be one of {sorted(MODELS)}, got {model!r}")
    if int(replicas) < 2:
        raise ValueError("a variance needs at least 2 replicas")
    poses = replica_corner_poses(log["corners"], float(sigma_px), seed, camera_matrix, dist_coeffs, marker_size,
                                 replicas=int(replicas), device=device)
    return np.var(replica_z(poses, model), axis=0)


def replica_z(poses, model: str) -> np.ndarray:
    """z [..., RD] of poses [..., 6] as the model's filter forms it (``EKF``: tvec; ``EKF_Rotations``: tvec and the
    scalar-first quaternion of the xyz Euler angles)."""
    poses = np.asarray(poses, dtype=np.float64)
    if model == "ekf":
        return poses[..., :3].copy()
    from .filters.ekf_with_rotations import euler_xyz_to_quat
    quat = euler_xyz_to_quat(poses[..., 3:6].reshape(-1, 3)).reshape(poses.shape[:-1] + (4,))
    return np.concatenate((poses[..., :3], quat), axis=-1)


class EKFBatch:
    """``members`` filters of ``model`` (``"ekf"``: ``EKF``, ``"ekf_rotations"``: ``EKF_Rotations``).
    ``initial_camera_pose``: [10] for all or [B, 10]; ``quat_update``: None for the model's convention (``"as_written"`` for
    ``EKF``; ``EKF_Rotations`` has only ``"scalar_first"``); ``noise``: dict of scalars or length-B arrays keyed by
    ``NOISE_KEYS`` (missing keys: the model's constants); ``large_maps``: see ``use_large_maps`` (the choice is kept in
    ``self.large_maps``); ``wide_frames``: see ``use_wide_frames`` (kept in ``self.wide_frames``); ``gate``: see
    ``set_gate`` (kept in ``self.gate``); ``row_noise``: the logs may carry per-detection measurement noise (``"noise"`` in
    ``process_detection_logs``, ``noise=`` of ``observe_indexed``; kept in ``self.row_noise``); ``frame_scale``: the logs
    may carry a process-noise scale per frame (``"scale"`` in ``process_detection_logs``, ``scale=`` of ``observe_indexed``)
    and every member keeps a pending scale (``pending_scale``; kept in ``self.frame_scale``); ``motion``: the logs may carry
    the camera's motion before every frame (``"motion"`` in ``process_detection_logs``, ``motion=`` of ``observe_indexed``;
    kept in ``self.motion``)."""

    gate = None        # [B] chi-square gate per member, or None: no gate (set_gate)
    # per member, the marker ids the last process_detection_logs / replay_replicas / replay_corner_replicas call dropped
    # because the member's map is frozen and does not hold them (a tuple per member, in log order; () for a mapping member)
    last_ignored = ()
    _frozen = None     # [B] bool mirror of the handle's "map frozen" flags as this object set them, or None: none is frozen
    camera = None      # (camera matrix [9], distortion coefficients, marker size) of corner logs, or None (set_camera)
    last_history = None          # uint8 device tensor: the history of the last recorded call (smooth_detection_logs), or None
    _history_frames = None       # [B + 1]: member_frames of that call
    last_smooth_status = None    # [B] int32 of the last backward pass: 0, or EKF_ERR_NUMERIC (smooth_history)

    def __init__(self, members: int, initial_camera_pose, *, max_landmarks: int = 50, max_visible: int = 16,
                 quat_update: str | None = None, noise=None, device: str = "cuda:0", model: str = "ekf",
                 large_maps: bool | None = None, wide_frames: bool | None = None, gate=None, row_noise: bool = False,
                 frame_scale: bool = False, motion: bool = False) -> None:
        import torch
        gate = gate_array(gate, int(members))
        if model not in MODELS:
            raise ValueError(f"model must be one of {sorted(MODELS)}, got {model!r}")
        if quat_update is None:
            quat_update = "scalar_first" if model == "ekf_rotations" else "as_written"
        if quat_update not in QUAT_MODES:
            raise ValueError(f"quat_update must be one of {sorted(QUAT_MODES)}, got {quat_update!r}")
        if model == "ekf_rotations" and quat_update != "scalar_first":
            raise ValueError(f"EKF_Rotations batches take quat_update \"scalar_first\" (or None), got {quat_update!r}")
        unknown = set(noise or {}) - set(NOISE_KEYS)
        if unknown:
            raise ValueError(f"unknown noise constants {sorted(unknown)}; known: {list(NOISE_KEYS)}")
        self._torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("the EKF update path needs a HIP device (no CPU fallback)")
        self.members = int(members)
        self.row_noise = bool(row_noise)
        self.frame_scale = bool(frame_scale)
        self.motion = bool(motion)
        self.device = torch.device(device)
        self.model = model
        self.lm_dims = LM_DIMS[model]
        self.quat_update = quat_update
        cfg = EkfConfig()
        self._check(self.lib.ekf_default_config(C.byref(cfg)))
        cfg.max_landmarks, cfg.max_visible = int(max_landmarks), int(max_visible)
        cfg.quat_mode = QUAT_MODES[quat_update]
        cfg.model = MODELS[model]
        self.large_maps = use_large_maps(model, max_landmarks, large_maps)
        if self.large_maps:
            cfg.flags |= EKF_FLAG_BATCH_LARGE_MAPS
        self.wide_frames = use_wide_frames(model, max_visible, wide_frames)
        if self.wide_frames:
            cfg.flags |= EKF_FLAG_BATCH_WIDE_FRAMES
        if self.frame_scale:
            cfg.flags |= EKF_FLAG_FRAME_SCALE
        if self.motion:
            cfg.flags |= EKF_FLAG_MOTION
        if model == "ekf_rotations":
            from .filters import ekf_with_rotations as rot
            for key, val in zip(NOISE_KEYS, (rot.INITIAL_CAMERA_UNCERTAINTY, rot.INITIAL_LANDMARK_UNCERTAINTY,
                                             rot.R_UNCERTAINTY, rot.Q_UNCERTAINTY_CAM, rot.Q_ERROR_UNCERTAINTY_CAM,
                                             rot.Q_UNCERTAINTY_LM_XYZ)):
                setattr(cfg, key, val)
        self.max_landmarks, self.max_visible = int(max_landmarks), int(max_visible)
        defaults = np.array([getattr(cfg, k) for k in NOISE_KEYS])
        self.noise = np.tile(defaults, (self.members, 1))
        for key, val in (noise or {}).items():
            self.noise[:, NOISE_KEYS.index(key)] = np.broadcast_to(np.asarray(val, dtype=np.float64), (self.members,))
        self._initial_poses = np.ascontiguousarray(
            np.broadcast_to(np.asarray(initial_camera_pose, dtype=np.float64), (self.members, 10)))
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(device=self.device)
            cfg.stream = self.stream.cuda_stream
            ld, cb, sb, wb = C.c_int64(), C.c_size_t(), C.c_size_t(), C.c_size_t()
            self._check(self.lib.ekf_batch_query_sizes(C.byref(cfg), self.members, C.byref(ld), C.byref(cb), C.byref(sb),
                                                       C.byref(wb)))
            self.ld = ld.value
            self.cov_t = torch.zeros((self.members, self.ld, self.ld), dtype=torch.float64, device=self.device)
            self.state_t = torch.zeros((self.members, self.ld), dtype=torch.float64, device=self.device)
            self.ws_t = torch.zeros((wb.value,), dtype=torch.uint8, device=self.device)
            torch.cuda.synchronize(self.device)
            handle = C.c_void_p()
            self._check(self.lib.ekf_batch_create(C.byref(cfg), self.members, C.byref(handle)))
            self.h = handle
            self._check(self.lib.ekf_batch_bind_buffers(self.h, self.cov_t.data_ptr(), self.ld, self.state_t.data_ptr(),
                                                        self.ws_t.data_ptr(), wb.value))
            self._check(self.lib.ekf_batch_set_noise(self.h, _dptr(np.ascontiguousarray(self.noise))))
        self.cfg = cfg
        self.landmarks = [{} for _ in range(self.members)]
        self.num_landmarks = [0] * self.members
        self.gate = None
        self.last_ignored = [()] * self.members
        self.set_gate(gate)
        self.reset()

    def _check(self, rc):
        if rc != 0:
            raise EkfError(rc, self.lib.ekf_last_error_string().decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ekf_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_gate(self, gate) -> None:
        """The chi-square gate of every member: ``None`` (no gate), a scalar or [B]; ``inf`` switches one member's gate
        off.  Persistent like the noise constants, so a threshold sweep is one call.  Before a frame is updated, every
        detection's own d^2 = r^T S_d^-1 r (r = z - h, S_d = H_d (P+Q) H_d^T + R I, after the frame's first sightings) is
        compared with the member's gate and the frame runs on the survivors only; first sightings are exempt.  The usual
        thresholds are chi^2 quantiles of the detection's row count: 3 dof for ``EKF`` (95 %: 7.815, 99 %: 11.345, 99.9 %:
        16.266), 7 dof for ``EKF_Rotations`` (14.067, 18.475, 24.322; approximate, as for NIS: the unit-quaternion rows
        are not independent).  ``mahal=True`` on a replay call returns the distances with the gate off, to choose a
        threshold from data.  A bad gate raises ``ValueError`` and nothing changes."""
        g = gate_array(gate, self.members)
        self._check(self.lib.ekf_batch_set_gate(self.h, _dptr(g) if g is not None else None))
        self.gate = g

    # -- localisation mode ----------------------------------------------------------------------------------------------
    @property
    def map_frozen(self) -> np.ndarray:
        """[B] bool: which members' maps are frozen (the handle's flags, ``ekf_batch_get_map_frozen``, as this object set
        them: a copy)."""
        return np.zeros(self.members, dtype=bool) if self._frozen is None else self._frozen.copy()

    def _set_map_frozen(self, b, value: bool) -> None:
        flags = self.map_frozen
        if b is None:
            flags[:] = value
        else:
            flags[self._member(b)] = value
        self._check(self.lib.ekf_batch_set_map_frozen(self.h, _iptr(np.ascontiguousarray(flags, dtype=np.int32))))
        out = np.zeros(self.members, dtype=np.int32)
        self._check(self.lib.ekf_batch_get_map_frozen(self.h, _iptr(out)))
        self._frozen = out != 0

    def freeze_map(self, b=None) -> None:
        """Freeze the map of member b (None: of every member) from the next call on: localisation on the map as it is, the
        Schmidt-Kalman update of the camera (``BaseFilter.freeze_map``).  The member's frames update the camera state,
        P[0:10, :] and P[:, 0:10] with the bits of its mapping frame and leave the landmarks and P[10:, 10:] alone.
        Persistent until ``unfreeze_map`` or ``reset``; ``set_member``, ``remove_markers``, ``set_gate`` and
        ``set_pending_scale`` keep it.  Detections of ids the map does not hold are dropped by the replay calls (reported in
        ``last_ignored``); ``observe_indexed`` with an index beyond a frozen member's landmarks raises ``EkfError``
        (EKF_ERR_STATE) and nothing changes."""
        self._set_map_frozen(b, True)

    def unfreeze_map(self, b=None) -> None:
        """Member b (None: every member) maps again, from the state and P its frozen frames left: bit for bit the member
        ``set_member`` restores from those arrays."""
        self._set_map_frozen(b, False)

    def set_camera(self, camera_matrix, dist_coeffs=None, marker_size: float = 0.16) -> None:
        """The camera and marker size of logs that carry ``corners`` (``process_detection_logs``,
        ``replay_corner_replicas``): the arguments of ``hip_backend.estimate_poses``, kept on the host.  Bad values raise
        ``ValueError`` and nothing changes."""
        self.camera = camera_arrays(camera_matrix, dist_coeffs, marker_size)

    def _rejected(self, mahal: np.ndarray, member) -> np.ndarray:
        """``mahal > gate`` of the detections' members (NaN and 0 are never rejected)."""
        gate = self.gate
        if gate is None:
            return np.zeros(mahal.shape, dtype=bool)
        with np.errstate(invalid="ignore"):
            return mahal > gate[member]

    def _member(self, b) -> int:
        b = int(b)
        if not 0 <= b < self.members:
            raise IndexError(f"member {b} out of range 0..{self.members - 1}")
        return b

    # -- replay ------------------------------------------------------------------------------------------------------
    def process_detection_logs(self, logs, *, nis: bool = False, cam_cov: bool = False, mahal: bool = False,
                               record: bool = False):
        """One log per member (``None``: no log), each a dict of the replay layout ``ids [D]``, ``poses [D,6]``,
        ``offsets [F+1]`` and optionally ``has_detections [F]``.  After ``set_camera`` a log may carry ``corners [D,4,2]``
        (pixels) instead of ``poses``: the corner logs of a call are estimated by one ``ekf_estimate_poses_device`` launch on
        the batch's stream and their poses never leave the device; a log with both keys or with neither is a ``ValueError``.
        Returns the camera pose ``state[0:7]`` after every frame, one ``(F_b, 7)`` array per member.  A malformed log raises ``ValueError``, a log that needs more landmarks or
        detections per frame than the batch holds ``EkfError`` (EKF_ERR_CAPACITY); either way before anything runs, and no
        member (``landmarks`` included) changes.
        With ``nis`` or ``cam_cov`` it returns a ``BatchReplay`` of per-member lists instead: the trajectories, each
        frame's normalised innovation squared (z-h)^T S^-1 (z-h) (0 for a frame that is not stepped), its row count
        ``dof`` (the NIS's chi^2 degrees of freedom; approximate for EKF_Rotations, whose unit-quaternion rows are not
        independent) and P[0:10, 0:10] after it.  A member's failing frame and every later one give NaN.
        With ``mahal``, or with a gate set (``set_gate``), it returns a ``GatedBatchReplay``: the same fields with ``dof``
        over the surviving detections, every detection's d^2 and whether the gate rejected it.
        A log may carry ``noise`` ([D] or [D, RD], aligned with ``ids``; a batch built with ``row_noise=True``): the
        variances of its detections' measurement rows, in place of the member's ``r_uncertainty``.  A member whose log
        carries none keeps its constant (the same bits as without any ``noise`` in the call).
        A log may carry ``scale`` ([F], one per frame, empty frames included; a batch built with ``frame_scale=True``): the
        frames' process-noise scales.  A frame that is not stepped leaves its scale in the member's pending scale, which the
        next stepped frame adds to its own.  Either every log of a call carries scales or none does.
        A log may carry ``motion`` ([F, 6], one row per frame, empty frames included; a batch built with ``motion=True``):
        the camera's motion ``(d, w)`` before every frame, in the camera frame of the previous pose.  A frame that is not
        stepped is still moved.  Either every log of a call carries motions or none does.
        A member whose map is frozen (``freeze_map``) drops the detections of ids its map does not hold, as a frozen filter's
        ``process_detection_log`` does: a frame left with nothing is a frame that is not stepped, ``self.last_ignored[b]``
        lists the dropped ids of member b in log order (() for a mapping member and after a call that raised), and ``mahal``
        / ``rejected`` stay indexed like the log's own rows (NaN / False for a dropped one)."""
        gated = mahal or self.gate is not None
        frozen = self.map_frozen
        self.last_ignored = [()] * self.members
        if len(logs) != self.members:
            raise ValueError(f"need {self.members} logs (None for a member without one), got {len(logs)}")
        plans, index, offsets, frames, poses = [], [], [], [0], []
        rows, any_rows = [], any(log is not None and log.get("noise") is not None for log in logs)
        if any_rows and not self.row_noise:
            raise ValueError("a log with noise needs a batch built with row_noise=True")
        with_scale = [log is not None and log.get("scale") is not None for log in logs]
        if any(with_scale):
            if not self.frame_scale:
                raise ValueError("a log with scale needs a batch built with frame_scale=True")
            if not all(w for w, log in zip(with_scale, logs) if log is not None):
                raise ValueError("either every log of a call carries scale or none does")
        with_motion = [log is not None and log.get("motion") is not None for log in logs]
        if any(with_motion):
            if not self.motion:
                raise ValueError("a log with motion needs a batch built with motion=True")
            if not all(w for w, log in zip(with_motion, logs) if log is not None):
                raise ValueError("either every log of a call carries motion or none does")
        scales, motions = [], []
        corner_parts = []       # (first row, kept corners [n,4,2]) of every log that carries corners
        base = 0
        for b, log in enumerate(logs):
            if log is None:
                plans.append(None)
                frames.append(frames[-1])
                continue
            plan = plan_detection_log(self.landmarks[b], self.num_landmarks[b], log["ids"], log["offsets"],
                                      log.get("has_detections"), frozen=bool(frozen[b]))
            if ("poses" in log) == ("corners" in log):
                raise ValueError(f"member {b}: a log carries either poses [D,6] or corners [D,4,2]")
            if "corners" in log:
                if self.camera is None:
                    raise ValueError(f"member {b}: a log of corners needs set_camera() first")
                c = np.asarray(log["corners"], dtype=np.float64)
                if c.shape != (plan.keep.shape[0], 4, 2):
                    raise ValueError(f"member {b}: corners must have shape ({plan.keep.shape[0]}, 4, 2), got {c.shape}")
                corner_parts.append((base, c[plan.keep]))
                p = np.zeros((plan.keep.shape[0], 6))       # (filled on the device: _estimate_corner_logs)
            else:
                p = np.asarray(log["poses"], dtype=np.float64)
                if p.shape != (plan.keep.shape[0], 6):
                    raise ValueError(f"member {b}: poses must have shape ({plan.keep.shape[0]}, 6), got {p.shape}")
            if any_rows:
                if log.get("noise") is not None:
                    r = row_noise_array(log["noise"], plan.keep.shape[0], RD[self.model], f"member {b}: noise")
                else:
                    r = np.full((plan.keep.shape[0], RD[self.model]), self.noise[b, NOISE_KEYS.index("r_uncertainty")])
                rows.append(r[plan.keep])
            if with_scale[b]:
                scales.append(frame_scale_array(log["scale"], plan.offsets.shape[0] - 1, f"member {b}: scale"))
            if with_motion[b]:
                motions.append(motion_array(log["motion"], plan.offsets.shape[0] - 1, f"member {b}: motion"))
            plans.append(plan)
            index.append(plan.index)
            offsets.append(plan.offsets[1:] + base)
            base += plan.index.shape[0]
            frames.append(frames[-1] + plan.offsets.shape[0] - 1)
            poses.append(p[plan.keep])
        index = np.concatenate(index).astype(np.int32) if index else np.zeros(0, np.int32)
        offsets = np.concatenate([np.zeros(1, np.int64)] + offsets).astype(np.int64)
        poses = np.ascontiguousarray(np.concatenate(poses) if poses else np.zeros((0, 6)))
        if sum(c.shape[0] for _, c in corner_parts):
            poses = self._estimate_corner_logs(poses, corner_parts)
        # only what the caller set travels as a keyword (no rows: the call as it ever was)
        given = {"noise": np.concatenate(rows)} if any_rows and rows else {}
        if scales:
            given["scale"] = np.concatenate(scales)
        if motions:
            given["motion"] = np.concatenate(motions)
        if record:      # (the recorded call: the same outputs, and the history in last_history)
            given["record"] = True
        if gated or nis or cam_cov:
            given.update(nis=nis, cam_cov=cam_cov)
        if gated:
            given["mahal"] = True
        out = self.observe_indexed(index, offsets, np.asarray(frames, dtype=np.int64), poses, **given)
        # an array, (trajectory, nis, cam_cov) or (trajectory, nis, cam_cov, mahal)
        traj, nis_v, cov_v, mahal_v = (tuple(out) + (None,))[:4] if isinstance(out, tuple) else (out, None, None, None)
        self._adopt_plans(plans)
        self.last_ignored = [() if plan is None else tuple(plan.ignored) for plan in plans]
        split = [slice(frames[b], frames[b + 1]) for b in range(self.members)]
        if gated:
            member = np.repeat(np.arange(self.members), np.diff(offsets[np.asarray(frames)]))
            rej_v = self._rejected(mahal_v, member)
            dof = _surviving_dof(RD[self.model], offsets, rej_v)
            mahal_l, rej_l = [], []
            for b, plan in enumerate(plans):      # back to the log's own detections (the planner's drops: NaN)
                keep = np.zeros(0, dtype=bool) if plan is None else np.asarray(plan.keep, dtype=bool)
                dsl = slice(offsets[frames[b]], offsets[frames[b + 1]])
                full = np.full(keep.shape[0], np.nan)
                full[keep] = mahal_v[dsl]
                rej = np.zeros(keep.shape[0], dtype=bool)
                rej[keep] = rej_v[dsl]
                mahal_l.append(full)
                rej_l.append(rej)
            return GatedBatchReplay([traj[sl] for sl in split], [nis_v[sl] for sl in split] if nis else None,
                                    [dof[sl] for sl in split], [cov_v[sl] for sl in split] if cam_cov else None,
                                    mahal_l, rej_l)
        if not (nis or cam_cov):
            return [traj[sl] for sl in split]
        dof = RD[self.model] * np.diff(offsets)
        return BatchReplay([traj[sl] for sl in split], [nis_v[sl] for sl in split] if nis else None,
                           [dof[sl] for sl in split], [cov_v[sl] for sl in split] if cam_cov else None)

    def _estimate_corner_logs(self, poses: np.ndarray, corner_parts):
        """``poses`` [D, 6] of a call as a device tensor whose rows ``first .. first + n`` of every ``(first, corners
        [n,4,2])`` in ``corner_parts`` hold the IPPE poses of those corners: one ``ekf_estimate_poses_device`` launch for
        all of them on the batch's stream, then one device-to-device copy per corner log (none if every log has corners)."""
        torch = self._torch
        k, d, size = self.camera
        corners = np.ascontiguousarray(np.concatenate([c for _, c in corner_parts]))
        count = corners.shape[0]
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            corners_t = torch.from_numpy(corners).to(self.device)
            est = torch.empty((count, 6), dtype=torch.float64, device=self.device)
            self._check(self.lib.ekf_estimate_poses_device(corners_t.data_ptr(), count, size, _dptr(k),
                                                           _dptr(d) if d.size else None, int(d.size), est.data_ptr(),
                                                           self.stream.cuda_stream))
            if count == poses.shape[0]:
                return est
            poses_t = torch.from_numpy(poses).to(self.device)
            at = 0
            for first, c in corner_parts:
                poses_t[first:first + c.shape[0]].copy_(est[at:at + c.shape[0]])
                at += c.shape[0]
        return poses_t

    def _adopt_plans(self, plans) -> None:
        """Landmark tables after a call, from the planned first sightings and the device's counts."""
        counts = self._num_landmarks_device()
        for b, plan in enumerate(plans):
            if plan is not None:        # (a member that failed keeps the landmarks it added before it stopped)
                self.landmarks[b].update((k, j) for k, j in plan.new_landmarks.items() if j < counts[b])
            self.num_landmarks[b] = int(counts[b])

    def replay_replicas(self, log, sigma, seed: int, *, first_replica: int = 0, nis: bool = False,
                        cam_cov: bool = False, mahal: bool = False):
        """Monte-Carlo replicas of ONE log: member b replays ``log`` (the layout of ``process_detection_logs``) as replica
        ``first_replica + b``, every detection's pose re-noised on the device as ``pose + sigma[b] * g`` with the
        standard normals g of ``replica_poses`` (Philox4x32-10 / Box-Muller, defined in ``include/ekf_slam_hip.h``; a
        replica's noise depends on its number, the detection and ``seed`` only, not on the batch size).  ``sigma``: a
        scalar, [6] or [B, 6] over ``[tvec | rvec]`` (EKF reads only the tvec); each member keeps its own noise
        constants, so a sweep x Monte-Carlo grid is one call.  The log is planned once: every member's landmark table must
        be the same (after ``reset()`` they are all empty), else ``ValueError``.
        Returns a ``ReplicaReplay``: ``trajectory`` [B, F, 7], ``dof`` [F] (the frame's row count 3 m / 7 m, duplicate
        detections counted) and, if asked, ``nis`` [B, F] and ``cam_cov`` [B, F, 10, 10] as in ``process_detection_logs``.
        Mean NIS over replicas against the chi^2(dof) bounds tunes the noise constants without ground truth; for
        EKF_Rotations the unit-quaternion rows make that chi^2 reading approximate.  Bad arguments raise before anything
        runs, and no member changes.  Either every member's map is frozen or none is (``ValueError`` otherwise: the log is
        planned once); with all of them frozen the log is planned as a frozen filter plans it (``last_ignored``).
        With ``mahal``, or with a gate set (``set_gate``), it returns a ``GatedReplicaReplay`` instead: ``dof`` [B, F] over
        each member's surviving detections, ``mahal`` [B, D] and ``rejected`` [B, D] aligned with the log's detections."""
        gated = mahal or self.gate is not None
        sig = replica_sigma(sigma, self.members)
        r0, seed = _replica_range(first_replica, self.members), _seed(seed)
        plan, poses, idx, fo = self._plan_replica_log(log, "poses", (6,), "replay_replicas")
        out = self._run_replicas(plan, poses, idx, fo, nis, cam_cov, gated, lambda head, outputs:
                                 self.lib.ekf_batch_observe_replicas_gated(*head, _dptr(sig), seed, r0, *outputs))
        return GatedReplicaReplay(*out) if gated else ReplicaReplay(*out[:4])

    def _run_replicas(self, plan, src, idx, fo, nis: bool, cam_cov: bool, gated: bool, launch):
        """What the replica calls share once their arguments have passed and the log is planned: ``src`` (the kept poses or
        corners) uploaded, the workspace and the outputs allocated on the batch's stream, ``launch(head, outputs)`` checked
        -- head: (handle, indices, offsets, F, src); outputs: (workspace, its bytes, trajectory, nis, cam_cov, mahal), NULL for
        what is not asked -- the stream synchronised and the plan adopted.  Returns the host arrays (trajectory, nis, dof,
        cam_cov, mahal, rejected): ``dof`` [F] and no ``mahal`` / ``rejected``, or with ``gated`` ``_replica_gate_outputs``."""
        F, D, B = fo.shape[0] - 1, idx.shape[0], self.members
        torch = self._torch
        nbytes = C.c_size_t()
        self._check(self.lib.ekf_batch_replica_workspace_bytes(self.h, D, F, C.byref(nbytes)))
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            new = (lambda want, *shape: torch.empty(shape, dtype=torch.float64, device=self.device) if want else None)
            src_t = torch.from_numpy(src).to(self.device)
            ws = torch.empty((max(nbytes.value, 1),), dtype=torch.uint8, device=self.device)
            traj, nis_t, cov_t, mahal_t = new(True, B, F, 7), new(nis, B, F), new(cam_cov, B, F, 10, 10), new(gated, B, D)
            ptr = (lambda t: t.data_ptr() if t is not None and F else None)
            self._check(launch((self.h, _iptr(idx), _lptr(fo), F, src_t.data_ptr() if D else None),
                               (ws.data_ptr(), nbytes.value, ptr(traj), ptr(nis_t), ptr(cov_t),
                                mahal_t.data_ptr() if gated and D else None)))
            self.stream.synchronize()
        self._adopt_plans([plan] * B)
        self.last_ignored = [tuple(plan.ignored)] * B
        host = (lambda t: None if t is None else t.cpu().numpy())
        full, rej, dof = self._replica_gate_outputs(plan, fo, host(mahal_t)) if gated else \
            (None, None, RD[self.model] * np.diff(fo))
        return host(traj), host(nis_t), dof, host(cov_t), full, rej

    def _plan_replica_log(self, log, key: str, tail: tuple, what: str):
        """The one log of a replica call planned on the members' common landmark table: (plan, the kept rows of
        ``log[key]`` [D, *tail], landmark indices [D], frame offsets [F+1]); ``ValueError`` if the tables differ or the
        array has another shape."""
        if any(t != self.landmarks[0] for t in self.landmarks[1:]) or len(set(self.num_landmarks)) > 1:
            raise ValueError(f"{what} needs every member's landmark table to be the same (reset() first)")
        frozen = self.map_frozen
        if frozen.any() != frozen.all():
            raise ValueError(f"{what} plans its one log once: every member's map must be frozen, or none "
                             "(freeze_map() / unfreeze_map() without a member)")
        self.last_ignored = [()] * self.members
        plan = plan_detection_log(self.landmarks[0], self.num_landmarks[0], log["ids"], log["offsets"],
                                  log.get("has_detections"), frozen=bool(frozen.all()))
        v = np.asarray(log[key], dtype=np.float64)
        if v.shape != (plan.keep.shape[0],) + tail:
            raise ValueError(f"{key} must have shape {(plan.keep.shape[0],) + tail}, got {v.shape}")
        return (plan, np.ascontiguousarray(v[plan.keep]), np.ascontiguousarray(plan.index, dtype=np.int32),
                np.ascontiguousarray(plan.offsets, dtype=np.int64))

    def _replica_gate_outputs(self, plan, fo: np.ndarray, mahal_v: np.ndarray):
        """(mahal [B, D], rejected [B, D], dof [B, F]) of a replica call from the device's distances over the planned
        detections: back on the log's own detections (the planner's drops: NaN / False)."""
        B, keep = self.members, np.asarray(plan.keep, dtype=bool)
        rej_v = self._rejected(mahal_v, np.arange(B)[:, None])
        full = np.full((B, keep.shape[0]), np.nan)
        full[:, keep] = mahal_v
        rej = np.zeros((B, keep.shape[0]), dtype=bool)
        rej[:, keep] = rej_v
        dof = np.stack([_surviving_dof(RD[self.model], fo, r) for r in rej_v]) if B else np.zeros((0, fo.shape[0] - 1), np.int64)
        return full, rej, dof

    def replay_corner_replicas(self, log, sigma_px, seed: int, *, first_replica: int = 0, nis: bool = False,
                               cam_cov: bool = False, mahal: bool = False) -> CornerReplicaReplay:
        """``replay_replicas`` with the noise where the detector has it: ``log`` carries ``corners`` [D, 4, 2] (pixels)
        instead of ``poses``, member b replays it as replica ``first_replica + b`` with every corner moved by
        ``sigma_px[b] * (g_u, g_v)`` pixels and every pose estimated from the noisy corners by IPPE on the device, with
        the camera of ``set_camera`` (``replica_corner_poses`` returns exactly the poses a replica consumed; the noise
        and the flip are defined in ``include/ekf_slam_hip.h``).  ``sigma_px``: a scalar or [B].  The same landmark-table
        precondition as ``replay_replicas``; bad arguments raise before anything runs, and no member changes.
        Returns a ``CornerReplicaReplay``: the fields of ``replay_replicas`` (``mahal`` and ``rejected`` None, and ``dof``
        [F], unless ``mahal=True`` or a gate is set: then ``dof`` is [B, F]) and ``flipped`` [B, D] bool aligned with
        the log's own detections: the (replica, detection) pairs whose IPPE solution flipped, the outliers a gate should
        catch.  Very large ``sigma_px`` can make a quadrilateral degenerate: its pose is non-finite, as from
        ``estimate_poses``, and the member stops there (``status``)."""
        gated = mahal or self.gate is not None
        sig = replica_sigma_px(sigma_px, self.members)
        r0, seed = _replica_range(first_replica, self.members), _seed(seed)
        if self.camera is None:
            raise ValueError("replay_corner_replicas needs set_camera() first")
        if "poses" in log:
            raise ValueError("replay_corner_replicas takes a log of corners [D,4,2], not of poses (replay_replicas)")
        plan, corners, idx, fo = self._plan_replica_log(log, "corners", (4, 2), "replay_corner_replicas")
        k, d, size = self.camera
        D, B = idx.shape[0], self.members
        flip = []      # (allocated with the other outputs, on the batch's stream)

        def launch(head, outputs):
            flip.append(self._torch.zeros((B, D), dtype=self._torch.uint8, device=self.device))
            return self.lib.ekf_batch_observe_corner_replicas(
                *head, _dptr(sig), seed, r0, size, _dptr(k), _dptr(d) if d.size else None, int(d.size), *outputs,
                flip[0].data_ptr() if D else None)
        out = self._run_replicas(plan, corners, idx, fo, nis, cam_cov, gated, launch)
        keep = np.asarray(plan.keep, dtype=bool)
        flipped = np.zeros((B, keep.shape[0]), dtype=bool)
        flipped[:, keep] = flip[0].cpu().numpy().astype(bool)
        return CornerReplicaReplay(*out, flipped)

    # -- offline smoothing ---------------------------------------------------------------------------------------------
    def smooth_detection_logs(self, logs, *, mahal: bool = False, cov: bool = False):
        """``process_detection_logs(logs)`` recorded, then one Rauch-Tung-Striebel backward pass per member on the device
        ("Batch smoothing" in ``include/ekf_slam_hip.h``): returns ``(filtered, smoothed)``, per-member lists of
        ``(F_b, 7)``.  ``filtered`` has the bits of ``process_detection_logs`` and the batch is left where that call
        leaves it; ``smoothed[b][t]`` is the camera pose of frame t that ALL of member b's data supports.  The logs may carry
        what ``process_detection_logs`` takes (noise, scale, motion, corners after ``set_camera``, ``None`` members).  With
        ``mahal`` or a gate set a third value ``(mahal, rejected)`` follows, the per-member lists of ``GatedBatchReplay``.
        A member that failed in the replay has NaN rows from its failing frame on; ``last_smooth_status[b]`` is
        EKF_ERR_NUMERIC (-5) for a member whose backward pass met a covariance that is not positive definite (all its rows
        NaN), else 0.  A batch of ``model="ekf"``, ``quat_update="scalar_first"``, without ``large_maps`` / ``wide_frames``,
        mapping members of at most 50 landmarks; anything else raises ``EkfError`` (EKF_ERR_STATE) and nothing changes.

        Keyword-only ``cov=True`` (default False): the pass forms the smoothed covariances as well (``smooth_history_cov``) and
        the call returns ``(filtered, smoothed, filtered_cov, smoothed_cov)`` (plus ``(mahal, rejected)``), as
        ``EKF.smooth_detection_log(cov=True)`` does: per-member lists of ``(F_b, 10, 10)``, the camera blocks of ``P`` and
        ``P^s`` per frame, NaN before a member's first record."""
        gated = mahal or self.gate is not None
        out = self.process_detection_logs(logs, mahal=mahal, record=True)
        filtered = out.trajectory if gated else out
        if cov:
            smoothed, smoothed_cov, filtered_cov = self.smooth_history_cov()
            res = (filtered, smoothed, filtered_cov, smoothed_cov)
        else:
            res = (filtered, self.smooth_history())
        return res + ((out.mahal, out.rejected),) if gated else res

    def _history_open(self, history, workspace_bytes):
        """The opening of both backward passes: (the history buffer, workspace bytes from ``workspace_bytes``, a zeroed status
        [B], the frames of the recorded call, the split of its rows per member)."""
        history = self.last_history if history is None else history
        if history is None:
            raise ValueError("no recorded call yet (smooth_detection_logs, or observe_indexed(record=True))")
        nbytes = C.c_size_t()
        self._check(workspace_bytes(self.h, C.byref(nbytes)))
        mf = self._history_frames
        return (history, max(nbytes.value, 256), np.zeros(self.members, dtype=np.int32), int(mf[-1]),
                lambda a: [a[mf[b]:mf[b + 1]] for b in range(self.members)])

    def smooth_history(self, history=None) -> list:
        """The backward pass over the last recorded call (``ekf_batch_smooth_history``; ``history``: its buffer, default
        ``self.last_history``): per member the smoothed rows ``(F_b, 7)``.  Sets ``last_smooth_status``.  Reads the members
        only; the same history gives the same bits every time."""
        torch = self._torch
        history, nbytes, status, frames, cut = self._history_open(history, self.lib.ekf_batch_smooth_workspace_bytes)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
            out = torch.empty((frames, 7), dtype=torch.float64, device=self.device)
            self._check(self.lib.ekf_batch_smooth_history(self.h, history.data_ptr(), history.numel(), ws.data_ptr(),
                                                          ws.numel(), out.data_ptr() if frames else None, _iptr(status)))
            self.stream.synchronize()
        self.last_smooth_status = status
        return cut(out.cpu().numpy())

    def smooth_history_cov(self, history=None, first: bool = False):
        """The backward pass with the smoothed covariances over the last recorded call (``ekf_batch_smooth_history_cov``,
        "Batch smoothing, covariances" in ``include/ekf_slam_hip.h``): ``(smoothed, cam_cov, filt_cam_cov)``, per-member
        lists of ``(F_b, 7)``, ``(F_b, 10, 10)`` and ``(F_b, 10, 10)`` -- the rows of ``smooth_history``, bit for bit, the camera
        block of ``P^s`` and the one of the filtered ``P`` of the record a frame belongs to (NaN before the first record).  With
        ``first`` a fourth list follows: ``P^s_0`` of every member, ``(N_0, N_0)`` (``(0, 0)`` for a member without a record).
        Sets ``last_smooth_status``; a member with EKF_ERR_NUMERIC there has NaN everywhere.  Reads the members only."""
        torch = self._torch
        history, nbytes, status, frames, cut = self._history_open(history, self.lib.ekf_batch_smooth_cov_workspace_bytes)
        n0 = np.zeros(self.members, dtype=np.int64)
        if first:
            for b in range(self.members):
                dims = self._history_info(b)[1]
                n0[b] = dims[0] if dims.size else 0
        first_ld = int(n0.max()) if first and self.members else 0
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
            out = torch.empty((frames, 7), dtype=torch.float64, device=self.device)
            cam = torch.empty((frames, 10, 10), dtype=torch.float64, device=self.device)
            filt = torch.empty((frames, 10, 10), dtype=torch.float64, device=self.device)
            slab = torch.empty((self.members, first_ld, first_ld), dtype=torch.float64, device=self.device) if first_ld else None
            self._check(self.lib.ekf_batch_smooth_history_cov(
                self.h, history.data_ptr(), history.numel(), ws.data_ptr(), ws.numel(), 0, out.data_ptr() if frames else None,
                cam.data_ptr() if frames else None, filt.data_ptr() if frames else None,
                slab.data_ptr() if slab is not None else None, first_ld, _iptr(status)))
            self.stream.synchronize()
        self.last_smooth_status = status
        rows, cam, filt = out.cpu().numpy(), cam.cpu().numpy(), filt.cpu().numpy()
        if not first:
            return cut(rows), cut(cam), cut(filt)
        slabs = slab.cpu().numpy() if slab is not None else np.zeros((self.members, 0, 0))
        return cut(rows), cut(cam), cut(filt), [slabs[b, :n0[b], :n0[b]].copy() for b in range(self.members)]

    def _history_info(self, b: int):
        """(frame, dims, s_eff, motion [R, 6], stepped) of member b's R records in the last recorded call
        (``ekf_batch_history_info``: the count first, then the arrays)."""
        count = C.c_int32()
        self._check(self.lib.ekf_batch_history_info(self.h, b, C.byref(count), 0, None, None, None, None, None, None))
        r = count.value
        frame, dims, stepped = (np.zeros(max(r, 1), dtype=np.int32) for _ in range(3))
        s_eff, motion = np.zeros(max(r, 1)), np.zeros((max(r, 1), 6))
        self._check(self.lib.ekf_batch_history_info(self.h, b, C.byref(count), max(r, 1), _iptr(frame), _iptr(dims),
                                                    _dptr(s_eff), _dptr(motion), _iptr(stepped), None))
        return frame[:r], dims[:r], s_eff[:r], motion[:r], stepped[:r]

    def history_records(self, b) -> list:
        """The records of member b in the last recorded call, as ``tests/smooth_util.device_records`` lists a single filter's:
        dicts ``frame`` (within the member's log), ``dims``, ``s_eff``, ``u`` [6], ``stepped``, ``x`` [N], ``P`` [N, N]."""
        b = self._member(b)
        records = []
        for i, (frame, n, s_eff, motion, stepped) in enumerate(zip(*self._history_info(b))):
            x, p = np.empty(n), np.empty((n, n))
            self._check(self.lib.ekf_batch_history_record(self.h, self.last_history.data_ptr(), b, i, _dptr(x), _dptr(p),
                                                          int(n)))
            records.append({"frame": int(frame), "dims": int(n), "s_eff": float(s_eff), "u": motion.copy(),
                            "stepped": bool(stepped), "x": x, "P": p})
        return records

    def smooth_replicas(self, log, sigma, seed: int, *, first_replica: int = 0, cov: bool = False):
        """``replay_replicas(log, sigma, seed)`` recorded and smoothed: every member replays ONE log as replica
        ``first_replica + b`` (the poses of ``replica_poses``, drawn on the device) and gets its own backward pass.  Returns
        ``(filtered [B, F, 7], smoothed [B, F, 7])``; ``filtered`` has the bits of ``replay_replicas``' trajectories on an
        equal batch.  "How much does smoothing buy at this noise level, this gate, these noise constants" is one call.
        Keyword-only ``cov=True``: ``(filtered, smoothed, filtered_cov [B, F, 10, 10], smoothed_cov [B, F, 10, 10])`` -- "is the
        smoothed uncertainty honest" (the NEES of the smoothed pose over the replicas) is the same call."""
        torch = self._torch
        B = self.members
        sig = replica_sigma(sigma, B)
        r0, seed = _replica_range(first_replica, B), _seed(seed)
        plan, poses, idx, fo = self._plan_replica_log(log, "poses", (6,), "smooth_replicas")
        F, D = fo.shape[0] - 1, idx.shape[0]
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            src = torch.from_numpy(poses).to(self.device)
            noisy = torch.empty((B * D, 6), dtype=torch.float64, device=self.device)
            self._check(self.lib.ekf_batch_replica_poses(src.data_ptr() if D else None, D, _dptr(sig), B, seed, r0,
                                                         noisy.data_ptr() if D else None, self.stream.cuda_stream))
        offsets = np.concatenate([fo[:-1] + b * D for b in range(B)] + [np.array([B * D], dtype=np.int64)])
        traj = self.observe_indexed(np.tile(idx, B), offsets, F * np.arange(B + 1, dtype=np.int64), noisy, record=True)
        self._adopt_plans([plan] * B)
        self.last_ignored = [tuple(plan.ignored)] * B
        if not cov:
            return traj.reshape(B, F, 7), np.stack(self.smooth_history()) if B else np.zeros((0, F, 7))
        smoothed, smoothed_cov, filtered_cov = self.smooth_history_cov()
        return traj.reshape(B, F, 7), np.stack(smoothed), np.stack(filtered_cov), np.stack(smoothed_cov)

    def observe_indexed(self, lm_index, frame_offsets, member_frames, poses, *, nis: bool = False, cam_cov: bool = False,
                        mahal: bool = False, noise=None, scale=None, motion=None, record: bool = False):
        """The C call behind ``process_detection_logs`` (ekf_batch_observe_logs_moved, NULL for what is not given or not
        asked; landmark indices already assigned; ``landmarks`` is not touched): lm_index [D], frame_offsets [Ftot+1],
        member_frames [B+1] on the host, poses [D,6] on the host or a contiguous float64 tensor on the batch's device,
        produced on the batch's stream.  Returns the trajectory [Ftot, 7]; with ``nis`` or ``cam_cov`` the tuple (trajectory, nis [Ftot] or None, cam_cov [Ftot, 10, 10]
        or None); with ``mahal`` the tuple (trajectory, nis or None, cam_cov or None, mahal [D]).  A gate that is set acts
        on every call, whatever it returns.  ``noise``: [D] or [D, RD] row variances indexed like lm_index (a batch built
        with ``row_noise=True``), or None: every member's ``r_uncertainty``.  ``scale``: [Ftot] process-noise scales, one
        per frame, indexed like frame_offsets (a batch built with ``frame_scale=True``), or None: no frame carries one.
        ``motion``: [Ftot, 6] camera motions, one per frame, indexed like frame_offsets (a batch built with
        ``motion=True``), or None.
        ``record``: the recorded call (ekf_batch_observe_logs_recorded): the same outputs, bit for bit, and the history of
        the call in ``self.last_history`` for ``smooth_history`` / ``history_records`` (True: a buffer of
        ``ekf_batch_history_bytes`` is allocated; a uint8 tensor on the batch's device: that buffer)."""
        torch = self._torch
        idx = np.ascontiguousarray(lm_index, dtype=np.int32).reshape(-1)
        if noise is not None:
            if not self.row_noise:
                raise ValueError("noise= needs a batch built with row_noise=True")
            noise = row_noise_array(noise, idx.shape[0], RD[self.model])
        if scale is not None and not self.frame_scale:
            raise ValueError("scale= needs a batch built with frame_scale=True")
        if motion is not None and not self.motion:
            raise ValueError("motion= needs a batch built with motion=True")
        fo = np.ascontiguousarray(frame_offsets, dtype=np.int64).reshape(-1)
        mf = np.ascontiguousarray(member_frames, dtype=np.int64).reshape(-1)
        on_device = isinstance(poses, torch.Tensor)
        if on_device:
            if not poses.is_cuda or poses.dtype != torch.float64 or not poses.is_contiguous() or poses.ndim != 2 \
                    or poses.shape[1] != 6:
                raise ValueError(f"device poses must be a contiguous float64 [D, 6] tensor on {self.device}")
        else:
            poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 6)
        if mf.shape[0] != self.members + 1 or mf[0] != 0 or (np.diff(mf) < 0).any():
            raise ValueError(f"member_frames must be {self.members + 1} non-decreasing offsets from 0")
        frames = int(mf[-1])
        if fo.shape[0] != frames + 1:
            raise ValueError(f"frame_offsets must have {frames + 1} entries")
        if poses.shape[0] != idx.shape[0] or (frames and fo[-1] != idx.shape[0]):
            raise ValueError("frame_offsets, lm_index and poses do not match")
        if scale is not None:
            scale = frame_scale_array(scale, frames)
        if motion is not None:
            motion = motion_array(motion, frames)
        D = idx.shape[0]
        nbytes = C.c_size_t()
        self._check(self.lib.ekf_batch_log_workspace_bytes(self.h, D, frames, C.byref(nbytes)))
        hbytes = C.c_size_t()
        recording = isinstance(record, torch.Tensor) or bool(record)
        if recording:
            self._check(self.lib.ekf_batch_history_bytes(self.h, _iptr(idx), _lptr(fo), _lptr(mf), int(motion is not None),
                                                         C.byref(hbytes)))
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            # (a device tensor comes from this batch's stream: _estimate_corner_logs)
            poses_t = poses if on_device else torch.from_numpy(poses).to(self.device)
            ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=self.device)
            new = (lambda want, *shape: torch.empty(shape, dtype=torch.float64, device=self.device) if want else None)
            up = (lambda a: torch.from_numpy(a).to(self.device) if a is not None else None)
            rows_t, scale_t, motion_t = up(noise), up(scale), up(motion)
            traj, nis_t, cov_t, mahal_t = new(True, frames, 7), new(nis, frames), new(cam_cov, frames, 10, 10), new(mahal, D)
            # one call path: NULL for every input and output that is not given or not asked (what the narrower entry points
            # of the C ABI forward), per frame only with frames and per detection only with detections
            ptr = (lambda t, count: t.data_ptr() if t is not None and count else None)
            args = (self.h, _iptr(idx), _lptr(fo), _lptr(mf), ptr(poses_t, D), ptr(rows_t, D), ptr(scale_t, frames),
                    ptr(motion_t, frames), ws.data_ptr(), nbytes.value, ptr(traj, frames), ptr(nis_t, frames),
                    ptr(cov_t, frames), ptr(mahal_t, D))
            if recording:
                history = record if isinstance(record, torch.Tensor) else \
                    torch.empty((max(hbytes.value, 256),), dtype=torch.uint8, device=self.device)
                self._check(self.lib.ekf_batch_observe_logs_recorded(*args, history.data_ptr(), history.numel()))
                self.last_history, self._history_frames = history, mf.copy()
            else:
                self._check(self.lib.ekf_batch_observe_logs_moved(*args))
            self.stream.synchronize()
        host = (lambda t: None if t is None else t.cpu().numpy())
        out = (host(traj), host(nis_t), host(cov_t))
        if mahal:
            return out + (host(mahal_t),)
        return out if (nis or cam_cov) else out[0]

    # -- per-member state ---------------------------------------------------------------------------------------------
    def _num_landmarks_device(self) -> np.ndarray:
        out = np.zeros(self.members, dtype=np.int32)
        self._check(self.lib.ekf_batch_num_landmarks(self.h, _iptr(out)))
        return out

    def status(self) -> list:
        """Per member: 0, or EKF_ERR_NUMERIC (-5) for a member stopped by a non-positive pivot of its innovation
        covariance (until ``reset`` or ``set_member``)."""
        out = np.zeros(self.members, dtype=np.int32)
        self._check(self.lib.ekf_batch_status(self.h, _iptr(out)))
        return [int(v) for v in out]

    def get_state(self, b) -> np.ndarray:
        b = self._member(b)
        out = np.empty(self.lm_dims * self.num_landmarks[b] + 10)
        self._check(self.lib.ekf_batch_get_member(self.h, b, _dptr(out), out.shape[0], None, 0))
        return out

    def get_cov(self, b) -> np.ndarray:
        b = self._member(b)
        dims = self.lm_dims * self.num_landmarks[b] + 10
        out = np.empty((dims, dims))
        self._check(self.lib.ekf_batch_get_member(self.h, b, None, 0, _dptr(out), dims))
        return out

    def get_poses(self, b):
        """``get_poses`` of the model's filter for member b: camera state [10], landmarks [n, 3] (EKF) or [n, 10]
        (EKF_Rotations)."""
        state = self.get_state(b)
        return state[:10], state[10:].reshape(-1, self.lm_dims)

    def get_lm_uncertainties(self, b, predicted: bool = False) -> np.ndarray:
        """diag(P) of member b's landmarks; ``predicted=True`` adds fl(pending scale * q_lm) on the host."""
        out = np.diagonal(self.get_cov(b))[10:].reshape(-1, self.lm_dims).copy()
        if predicted:
            out += float(self.pending_scale[self._member(b)]) * float(self.noise[self._member(b), NOISE_KEYS.index("q_lm")])
        return out

    @property
    def pending_scale(self) -> np.ndarray:
        """[B]: every member's pending process-noise scale (ekf_batch_get_pending_scale; zeros for a batch built without
        ``frame_scale=True``).  Synchronises."""
        out = np.zeros(self.members)
        self._check(self.lib.ekf_batch_get_pending_scale(self.h, -1, _dptr(out)))
        return out

    def set_pending_scale(self, pending, b=None) -> None:
        """The pending scale of member b (a number), or of every member (None: a number or [B]); a batch built with
        ``frame_scale=True``.  Values that are not finite and >= 0 raise ``ValueError`` and nothing changes."""
        if not self.frame_scale:
            raise ValueError("a pending scale needs a batch built with frame_scale=True")
        if b is None:
            v = frame_scale_array(np.broadcast_to(np.asarray(pending, dtype=np.float64), (self.members,)), self.members,
                                  "pending")
            self._check(self.lib.ekf_batch_set_pending_scale(self.h, -1, _dptr(v)))
        else:
            v = np.array([frame_scale_array(pending, None, "pending")])
            self._check(self.lib.ekf_batch_set_pending_scale(self.h, self._member(b), _dptr(v)))

    def set_member(self, b, state, cov, marker_ids) -> None:
        """Member b from host ``(state [l n + 10], cov [l n + 10, l n + 10], marker ids in landmark-index order)`` with
        l = ``lm_dims`` (3 for EKF, 10 for EKF_Rotations); clears its status.  cov is symmetrised on upload."""
        b = self._member(b)
        state = np.ascontiguousarray(state, dtype=np.float64).reshape(-1)
        ids = [int(k) for k in marker_ids]
        dims = self.lm_dims * len(ids) + 10
        if state.shape[0] != dims:
            raise ValueError(f"state has {state.shape[0]} entries, {dims} expected for {len(ids)} markers")
        cov = np.ascontiguousarray(cov, dtype=np.float64)
        if cov.shape != (state.shape[0], state.shape[0]):
            raise ValueError(f"cov must be {state.shape[0]} x {state.shape[0]}")
        self._check(self.lib.ekf_batch_set_member(self.h, b, _dptr(state), len(ids), _dptr(cov)))
        self.landmarks[b] = {k: i for i, k in enumerate(ids)}
        self.num_landmarks[b] = len(ids)

    def remove_markers(self, per_member_ids) -> None:
        """Take landmarks out of the members' maps (``ekf_batch_remove_markers``; ``BaseFilter.remove_markers`` per member,
        in one launch): ``per_member_ids`` is a list of B marker-id lists (empty or None: that member is left alone), or a
        dict ``member -> ids``.  Every member's other landmarks keep their order and move up; ``landmarks`` and
        ``num_landmarks`` follow.  An unknown id raises ``KeyError`` and a duplicate ``ValueError`` before anything runs, and
        no member changes."""
        from .filters.map_management import renumber_landmarks
        torch = self._torch
        if isinstance(per_member_ids, dict):
            lists = [[] for _ in range(self.members)]
            for b, ids in per_member_ids.items():
                lists[self._member(b)] = [int(k) for k in ids]
        else:
            if len(per_member_ids) != self.members:
                raise ValueError(f"need {self.members} id lists (empty for a member that keeps its map), got {len(per_member_ids)}")
            lists = [[] if ids is None else [int(k) for k in ids] for ids in per_member_ids]
        index, tables = [], []
        for b, ids in enumerate(lists):
            for marker in ids:
                if marker not in self.landmarks[b]:
                    raise KeyError(f"member {b}: marker {marker} is not in the map")
            if len(set(ids)) != len(ids):
                raise ValueError(f"member {b}: duplicate marker id in the removal list")
            index.append([self.landmarks[b][marker] for marker in ids])
            tables.append(renumber_landmarks(self.landmarks[b], index[-1]))
        offsets = np.concatenate([[0], np.cumsum([len(i) for i in index])]).astype(np.int64)
        if offsets[-1] == 0:
            return
        flat = np.ascontiguousarray(np.concatenate([np.asarray(i, dtype=np.int32) for i in index]), dtype=np.int32)
        nbytes = C.c_size_t()
        self._check(self.lib.ekf_batch_remove_workspace_bytes(self.h, int(offsets[-1]), C.byref(nbytes)))
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            cov_t, state_t = torch.empty_like(self.cov_t), torch.empty_like(self.state_t)
            ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=self.device)
            self._check(self.lib.ekf_batch_remove_markers(self.h, _iptr(flat), _lptr(offsets), cov_t.data_ptr(), self.ld,
                                                          state_t.data_ptr(), ws.data_ptr(), nbytes.value))
            # (the old tensors may come from another stream: the allocator keeps them until this one has passed the call)
            self.cov_t.record_stream(self.stream)
            self.state_t.record_stream(self.stream)
        self.cov_t, self.state_t = cov_t, state_t
        for b, ids in enumerate(lists):
            self.landmarks[b] = tables[b]
            self.num_landmarks[b] -= len(ids)

    def _filter_class(self):
        from .filters.ekf_with_rotations import EKF_Rotations
        from .filters.extended_kalman_filter import EKF
        return EKF_Rotations if self.model == "ekf_rotations" else EKF

    def load_filter(self, b, ekf) -> None:
        """Member b from an ordinary filter of the batch's model (``EKF`` or ``EKF_Rotations``): its state, covariance and
        landmark table, with the batch's quaternion convention.  The member keeps its own noise constants (a sweep loads
        one filter into members that differ in nothing else) and takes the filter's gate, if the filter was built with one:
        a filter whose gate is ``inf`` switches that member's gate OFF, also where the member had a finite one (``set_gate``
        afterwards to keep it); a filter built without ``gate=`` leaves the member's gate as it is.  The member takes the
        filter's ``map_frozen``."""
        cls = self._filter_class()
        if not isinstance(ekf, cls):
            raise ValueError(f"a batch of model {self.model!r} holds {cls.__name__} filters, got {type(ekf).__name__}")
        if ekf.backend.cfg.quat_mode != QUAT_MODES[self.quat_update]:
            raise ValueError(f"the filter's quaternion convention differs from the batch's ({self.quat_update!r})")
        if ekf.backend.can_row_noise and not self.row_noise:
            raise ValueError("the filter takes per-detection noise: load it into a batch built with row_noise=True")
        if ekf.backend.can_frame_scale and not self.frame_scale:
            raise ValueError("the filter takes per-frame scales: load it into a batch built with frame_scale=True")
        if ekf.backend.can_motion and not self.motion:
            raise ValueError("the filter takes camera motions: load it into a batch built with motion=True")
        pending = ekf.backend.pending_scale
        ids = [k for k, _ in sorted(ekf.get_lm_estimates(), key=lambda kv: kv[1])]
        self.set_member(b, np.asarray(ekf.state, dtype=np.float64), ekf.uncertainty, ids)
        if self.frame_scale:      # (set_member has zeroed it; a filter without the capability has 0)
            self.set_pending_scale(pending, b)
        self._set_map_frozen(b, bool(ekf.map_frozen))      # (the member takes the filter's flag, on or off)
        if ekf.gate is not None and not (self.gate is None and np.isinf(ekf.gate)):
            gates = np.full(self.members, np.inf) if self.gate is None else self.gate.copy()
            gates[self._member(b)] = ekf.gate
            self.set_gate(gates)

    def to_filter(self, b):
        """An ordinary filter of the batch's model (``EKF`` or ``EKF_Rotations``, f64 covariance) with member b's quaternion
        convention, noise constants, gate (a batch with a gate gives a filter built with ``gate=``), per-detection-noise
        capability (a batch built with ``row_noise=True`` gives a filter built the same way), per-frame-scale capability and
        pending scale (likewise, ``frame_scale=True``), camera-motion capability (likewise, ``motion=True``), state, covariance,
        landmark table and ``map_frozen`` (a frozen member gives a frozen filter); ``observe`` (and for ``EKF`` ``save_map`` and ``save_checkpoint``) work on it."""
        b = self._member(b)
        state, cov = self.get_state(b), self.get_cov(b)
        n = self.num_landmarks[b]
        noise = dict(zip(NOISE_KEYS, (float(v) for v in self.noise[b])))
        gate = None if self.gate is None else float(self.gate[b])
        if self.model == "ekf_rotations":
            from .filters.ekf_with_rotations import EKF_Rotations
            ekf = EKF_Rotations(state[:10], max_landmarks=max(n, 1), max_visible=self.max_visible, cov_dtype="float64",
                                device=str(self.device), noise=noise, gate=gate, row_noise=self.row_noise,
                                frame_scale=self.frame_scale, motion=self.motion)
        else:
            from .filters.extended_kalman_filter import EKF
            ekf = EKF(state[:10], max_landmarks=max(n, 1), max_visible=self.max_visible, cov_dtype="float64",
                      quat_update=self.quat_update, device=str(self.device), noise=noise, gate=gate, row_noise=self.row_noise,
                      frame_scale=self.frame_scale, motion=self.motion)
        pending = float(self.pending_scale[b]) if self.frame_scale else 0.0
        ekf.backend.set_state_cov(state, cov)
        if self.frame_scale:
            ekf.backend.pending_scale = pending
        ekf.landmarks = dict(self.landmarks[b])
        ekf.num_landmarks = n
        if self.map_frozen[b]:
            ekf.freeze_map()
        return ekf

    def reset(self, b=None) -> None:
        """Member b (all members: None) back to its initial pose, no landmarks, status cleared, map not frozen."""
        if b is None:
            self._check(self.lib.ekf_batch_reset(self.h, -1, _dptr(self._initial_poses)))
            members = range(self.members)
        else:
            b = self._member(b)
            self._check(self.lib.ekf_batch_reset(self.h, b, _dptr(np.ascontiguousarray(self._initial_poses[b]))))
            members = (b,)
        ignored = list(self.last_ignored) if len(self.last_ignored) == self.members else [()] * self.members
        for m in members:
            self.landmarks[m] = {}
            self.num_landmarks[m] = 0
            ignored[m] = ()
            if self._frozen is not None:      # (ekf_batch_reset has cleared the member's flag)
                self._frozen[m] = False
        self.last_ignored = ignored
