"""Filter boundary: host-side mirror of reference ``BaseFilter``
(/root/reference/filters/base_filter.py:35-381).

Only the boundary is in scope: the abstract filter API,
the ``process_frame`` driver contract (observe only when something was
detected, ``get_poses`` every frame -- base_filter.py:194-212) and the map file
format (``save_map`` :214-247).  The ArUco detector is OpenCV work and is not
re-implemented (used as the reference does when ``cv2`` is importable; otherwise
frames of pre-computed detections are fed through ``process_detections``); the
per-marker solvePnP that follows it is one batched HIP kernel
(``estimate_pose_of_markers``).
"""
from __future__ import annotations

from pathlib import Path
from typing import NamedTuple

import numpy as np

try:  # the image has no OpenCV; the boundary does not need it
    import cv2  # type: ignore
except ImportError:  # pragma: no cover
    cv2 = None

CALIB_MTX_FILE = "./calibration/camera_matrix.npy"      # base_filter.py:12
DIST_COEFFS_FILE = "./calibration/dist_coeffs.npy"      # base_filter.py:13

KALMAN_FILTER = "ekf"
FACTOR_GRAPH = "factorgraph"

NOT_IMPLEMENTED_ERROR = """
                        This method is not implemented in the base class and
                        should be implemented in a subclass.
                        """

CAM_DIMS = 10
XYZ_DIMS = slice(0, 3)
QUAT_DIMS = slice(3, 7)
ERROR_DIMS = slice(7, 10)

# markers in the predefined dictionaries, by OpenCV's enumeration (cv2.aruco.DICT_4X4_50 = 0 ... DICT_ARUCO_MIP_36h12 = 21):
# how many landmarks a map built with that dictionary can hold (the filters size their first buffers for it; they grow
# if more show up).  The reference's default is DICT_5X5_50 (base_filter.py:81-82).
ARUCO_DICT_SIZES = {0: 50, 1: 100, 2: 250, 3: 1000, 4: 50, 5: 100, 6: 250, 7: 1000, 8: 50, 9: 100, 10: 250, 11: 1000,
                    12: 50, 13: 100, 14: 250, 15: 1000, 16: 1024, 17: 30, 18: 35, 19: 2320, 20: 587, 21: 250}
DEFAULT_ARUCO_DICT = 4      # cv2.aruco.DICT_5X5_50


def dictionary_size(aruco_dict) -> int:
    """Number of marker ids of the dictionary the filter was constructed with (None: the reference's default)."""
    if aruco_dict is None:
        aruco_dict = DEFAULT_ARUCO_DICT
    try:
        return ARUCO_DICT_SIZES[int(aruco_dict)]
    except (KeyError, TypeError, ValueError):
        return ARUCO_DICT_SIZES[DEFAULT_ARUCO_DICT]


class DetectionLogPlan(NamedTuple):
    index: np.ndarray          # int32 [D'] landmark index of every detection that is replayed
    offsets: np.ndarray        # int64 [F+1] frame boundaries in `index` (frames without detections are empty)
    keep: np.ndarray           # bool [D] rows of the input log that are replayed
    new_landmarks: dict        # marker id -> landmark index of the ids the log adds, in order of first occurrence
    num_landmarks: int         # landmarks after the log
    widest: int                # most detections in one frame
    ignored: tuple = ()        # frozen map: the marker ids of the rows that were dropped because the map does not hold them, in order


def plan_detection_log(landmarks, num_landmarks, ids, offsets, has_detections=None, frozen=False) -> DetectionLogPlan:
    """Host side of ``process_detection_log``: check the CSR log and map marker ids to landmark indices as ``observe`` does
    frame by frame (known ids keep their index, new ones are numbered ``num_landmarks``, ``+1``, ... in order of first
    occurrence, duplicates of a new id inside its frame share its index).  ``landmarks`` is not modified.  Raises
    ``ValueError`` for a malformed log.  ``frozen`` (a frozen map): detections of ids that are not in ``landmarks`` are
    dropped as ``observe`` drops them -- their rows get ``keep = False``, ``ignored`` lists their ids in order,
    ``new_landmarks`` is empty -- and a frame left with nothing is an empty frame."""
    offsets = np.asarray(offsets)
    if offsets.ndim != 1 or offsets.shape[0] < 1 or (offsets.size > 1 and offsets.dtype.kind not in "iu"):
        raise ValueError("offsets must be a 1-D integer array of F+1 entries")
    offsets = offsets.astype(np.int64)
    ids = np.asarray(ids).reshape(-1)
    if ids.size and ids.dtype.kind not in "iu":
        raise ValueError("ids must be integers")
    frames = offsets.shape[0] - 1
    counts = np.diff(offsets)
    if offsets[0] != 0 or (counts < 0).any():
        raise ValueError("offsets must start at 0 and be non-decreasing")
    if offsets[-1] != ids.shape[0]:
        raise ValueError(f"offsets[-1] = {int(offsets[-1])} but there are {ids.shape[0]} ids")
    if has_detections is None:
        has = counts > 0
    else:
        has = np.asarray(has_detections, dtype=bool).reshape(-1)
        if has.shape[0] != frames:
            raise ValueError(f"has_detections must have {frames} entries")
    empty = np.nonzero(has & (counts == 0))[0]
    if empty.size:
        raise ValueError(f"frame {int(empty[0])} has detections but no ids: observe() needs at least one detection")
    keep = np.repeat(has, counts)
    counts = np.where(has, counts, 0)
    ignored = ()
    if frozen:
        unknown = keep & ~np.fromiter((marker in landmarks for marker in ids.tolist()), dtype=bool, count=ids.shape[0])
        ignored = tuple(ids[unknown].tolist())
        keep = keep & ~unknown
        kept = np.concatenate(([0], np.cumsum(keep))).astype(np.int64)
        counts = kept[offsets[1:]] - kept[offsets[:-1]]
    new, n = {}, int(num_landmarks)
    index = np.empty(int(counts.sum()), dtype=np.int32)
    for k, marker in enumerate(ids[keep].tolist()):
        j = landmarks.get(marker)
        if j is None:
            j = new.get(marker)
            if j is None:
                j = new[marker] = n
                n += 1
        index[k] = j
    return DetectionLogPlan(index, np.concatenate(([0], np.cumsum(counts))).astype(np.int64), keep, new, n,
                            int(counts.max()) if frames else 0, ignored)


class BaseFilter:
    """Front-end + abstract back-end API (names and semantics of the reference)."""

    # (class-level defaults: subclasses that build themselves without this constructor prune nothing)
    _tentative = None       # confirm=(hits, window): the TentativeLandmarks policy (_init_confirm)
    _pruned = False         # landmarks have been removed: with none left, `state` is still the device's
    _moved = False          # the camera has been moved (move, motion=): with no landmark yet, `state` is the device's
    last_ignored = ()       # frozen map: the marker ids the last observe / log call dropped because the map does not hold them

    def __init__(self, initial_pose, map_file=None, aruco_dict=None) -> None:
        self.calib_matrix = None
        self.dist_coeffs = None
        self.detector = None
        if cv2 is not None:
            # same contract as base_filter.py:55-67
            if not Path(CALIB_MTX_FILE).exists():
                raise FileNotFoundError("Camera matrix not found. Run calibration.py first.")
            if not Path(DIST_COEFFS_FILE).exists():
                raise FileNotFoundError(
                    "Distortion coefficients not found. Run calibration.py first.")
            self.calib_matrix = np.load(CALIB_MTX_FILE)
            self.dist_coeffs = np.load(DIST_COEFFS_FILE)
            self.detector = self.init_aruco_detector(aruco_dict)
        self.camera_pose = initial_pose
        self._map_file = map_file
        # per detection of the last observed frame, indexed like its ``ids`` (filters built with ``gate=``; else None):
        # Mahalanobis distance d^2 (0: a marker the frame added, NaN: not tested) and whether the gate rejected it
        self.last_mahal = None
        self.last_rejected = None

    def _init_confirm(self, confirm) -> None:
        """``confirm=(hits, window)`` of the subclass constructors, once the initial map is loaded: a landmark that is not
        seen again in ``hits`` later frames within ``window`` frames of its first sighting is removed again
        (``map_management.TentativeLandmarks``, fed by ``process_detections``).  None: off, nothing changes.  Landmarks the
        filter holds already (map file) are confirmed from the start, and so are the landmarks a ``process_detection_log``
        replay adds: the replay is one device call that the policy does not see frame by frame."""
        if confirm is None:
            return
        from .map_management import TentativeLandmarks
        hits, window = confirm
        self._tentative = TentativeLandmarks(hits, window)
        self._tentative.confirm(self.landmarks)

    def _load_initial_map(self):
        """Subclasses call this once their back-end exists (the reference calls
        load_map from the base ctor, base_filter.py:71-72, before the subclass
        state exists -- one reason its load_map never worked)."""
        if self._map_file is not None:
            self.load_map(self._map_file)

    def init_aruco_detector(self, aruco_dict):
        """base_filter.py:74-90 (needs OpenCV)."""
        if cv2 is None:
            raise RuntimeError("OpenCV (cv2) is not available: feed detections via "
                               "process_detections()")
        if aruco_dict is None:
            aruco_dict = cv2.aruco.DICT_5X5_50
        aruco_dict = cv2.aruco.getPredefinedDictionary(aruco_dict)
        params = cv2.aruco.DetectorParameters()
        params.cornerRefinementMethod = cv2.aruco.CORNER_REFINE_SUBPIX
        params.cornerRefinementWinSize = 3
        params.cornerRefinementMaxIterations = 3
        params.adaptiveThreshWinSizeMin = 3
        params.adaptiveThreshWinSizeMax = 30
        return cv2.aruco.ArucoDetector(aruco_dict, params)

    def estimate_pose_of_markers(self, corners, ids, marker_size):
        """base_filter.py:92-171: IPPE-square PnP of every detected marker -> (m,6) [tvec|rvec].  The reference
        loops over the markers with cv2.solvePnP(flags=SOLVEPNP_IPPE_SQUARE); here all markers of the frame go
        through one HIP kernel (csrc/ekf_pose_ippe.hip) with the same object-point order (:113-121), camera matrix
        and distortion coefficients.  `corners` as the detector returns them (one [1,4,2] array per marker)."""
        if self.calib_matrix is None:
            raise RuntimeError("no camera calibration: set calib_matrix / dist_coeffs (calibration/*.npy)")
        from aruco_slam_amd import hip_backend
        if len(ids) == 0:
            return np.zeros((0, 6))
        backend = getattr(self, "_hip", None)        # (the filter's own GPU: one sequence per GPU)
        device = str(backend.device) if backend is not None else "cuda:0"
        return hip_backend.estimate_poses(corners, marker_size, self.calib_matrix, self.dist_coeffs, device=device)

    def process_frame(self, frame, should_filter=True, iteration=0, marker_size=0.16):
        """base_filter.py:173-212."""
        if self.detector is None:
            raise RuntimeError("no ArUco detector (cv2 missing): use process_detections()")
        corners, ids, _ = tuple(self.detector.detectMarkers(frame))
        detected_poses = np.array([])
        if ids is not None:
            frame = cv2.aruco.drawDetectedMarkers(frame, corners, ids)
            ids = ids.flatten()
            detected_poses = self.estimate_pose_of_markers(corners, ids, marker_size)
        _, camera_pose, marker_poses, detected_poses = self.process_detections(
            ids, detected_poses, should_filter, iteration)
        return frame, camera_pose, marker_poses, detected_poses

    def process_detections(self, ids, detected_poses, should_filter=True, iteration=0, noise=None, scale=None, motion=None):
        """The part of ``process_frame`` behind the detector
        (base_filter.py:196-212): ``ids`` is None for a frame without
        detections, in which case the filter is NOT stepped (no predict).  ``noise``: the frame's per-detection
        measurement noise, as ``observe`` takes it (a filter built with ``row_noise=True``).  ``scale``: the frame's
        process-noise scale, as ``observe`` takes it (a filter built with ``frame_scale=True``); a frame without
        detections advances the pending scale by it (``advance``), so the time it took is not lost.  ``motion``: the
        camera's motion since the previous frame, as ``observe`` takes it (a filter built with ``motion=True``); a frame
        without detections moves the camera all the same."""
        if ids is None:
            detected_poses = np.array([])
            if should_filter:
                scale, motion = self._frame_scale(scale), self._frame_motion(motion)      # (both checked before either acts)
                if motion is not None:
                    self._move(motion)
                if scale is not None:
                    self.advance(scale)
        elif should_filter and (noise is not None or scale is not None or motion is not None):
            extra = {} if noise is None else {"noise": noise}
            if scale is not None:
                extra["scale"] = scale
            if motion is not None:
                extra["motion"] = motion
            self.observe(ids, detected_poses, **extra)
        elif should_filter:
            self.observe(ids, detected_poses)
        if should_filter and self._tentative is not None and not self.map_frozen:      # (a frozen map is not pruned either)
            self._prune_tentative(ids)
        if should_filter:
            camera_pose, marker_poses = self.get_poses()
        else:
            _, marker_poses = self.get_poses()
            camera_pose = self.get_cam_estimate(iteration)
        return None, camera_pose, marker_poses, detected_poses

    # -- localisation mode: a frozen map (ekf_set_map_frozen) -------------------------------------
    @property
    def map_frozen(self) -> bool:
        """Whether the map is frozen: frames localise the camera on the map as it is (Schmidt-Kalman update: the camera,
        P_cc and the cross-covariances change, the landmarks and their covariance block keep their bits)."""
        return bool(getattr(getattr(self, "backend", None), "map_frozen", False))

    def freeze_map(self) -> None:
        """Freeze the map from the next frame on: ``observe`` / ``process_detections`` / ``process_detection_log`` update
        the camera only and drop detections of markers the map does not hold (``last_ignored``) instead of adding them.
        P stays a valid joint covariance: ``unfreeze_map`` goes on mapping from it.  Explicit ``add_marker``,
        ``remove_markers`` and ``load_checkpoint`` work as ever; ``reset`` unfreezes."""
        self.backend.set_map_frozen(True)

    def unfreeze_map(self) -> None:
        """Back to mapping, from the state and the covariance the frozen frames left."""
        self.backend.set_map_frozen(False)

    def _observe_frozen(self, ids, poses, rows, scale, motion) -> None:
        """``observe`` on a frozen map, arguments validated: detections of unknown ids are dropped (``last_ignored``, in
        order), the rest is the frame.  A frame left with nothing is not stepped: it is still moved, and its scale goes
        to the pending scale.  ``last_mahal`` / ``last_rejected`` stay indexed like ``ids`` (NaN / False for a dropped
        detection)."""
        known = self.landmarks
        sel = np.fromiter((marker in known for marker in ids), dtype=bool, count=len(ids))
        self.last_ignored = tuple(marker for marker, k in zip(ids, sel) if not k)
        if motion is not None:
            self._move(motion)
        backend = self.backend
        if backend.can_gate:
            self.last_mahal, self.last_rejected = np.full(len(ids), np.nan), np.zeros(len(ids), dtype=bool)
        if not sel.any():
            if scale is not None:
                backend.advance(scale)
            return
        index = [known[marker] for marker, k in zip(ids, sel) if k]
        z = self._measurements(poses[sel])
        rows = None if rows is None else rows[sel]
        if not backend.can_gate:
            backend.observe(index, z, rows=rows, scale=scale)
            return
        self._observe_gated(index, z, None, rows, scale)
        d2, rejected = np.full(len(ids), np.nan), np.zeros(len(ids), dtype=bool)
        d2[sel], rejected[sel] = self.last_mahal, self.last_rejected
        self.last_mahal, self.last_rejected = d2, rejected

    # -- the per-detection chi-square gate (ekf_set_gate) ----------------------------------------
    @property
    def gate(self):
        """The gate: None (a filter built without it), ``inf`` (off) or the threshold on d^2."""
        return self.backend.gate

    def set_gate(self, gate) -> None:
        """Reject every detection whose own squared Mahalanobis distance on the prior exceeds ``gate`` before the frame
        is updated (one flipped IPPE pose otherwise bends the whole map); None or ``inf``: off.  The filter must have been
        constructed with ``gate=`` (``inf`` will do).  A bad gate raises ``ValueError`` and nothing changes."""
        self.backend.set_gate(gate)

    # -- per-frame process-noise scale (ekf_advance, ekf_observe_scaled) ----------------------------
    def advance(self, scale) -> None:
        """Time passes without a frame: ``scale`` (a number >= 0, in the unit of the frames' scales) is added to the pending
        scale, and the next stepped frame runs with pending + its own scale.  A filter built with ``frame_scale=True``;
        anything else raises ``ValueError`` and nothing changes."""
        self.backend.advance(self._frame_scale(scale))

    @property
    def pending_scale(self) -> float:
        """The process-noise scale accumulated by frames that were not stepped (no detections, or none that survived the
        gate) and by ``advance`` since the last stepped frame; 0 after a stepped frame, after ``reset`` and for a filter built
        without ``frame_scale=True``."""
        return self.backend.pending_scale

    def _frame_scale(self, scale):
        """``scale=`` of ``observe`` / ``advance``: None, or a float.  ``ValueError`` for anything that is not a finite
        number >= 0 and for a filter built without ``frame_scale=True``; checked before the frame changes anything."""
        if scale is None:
            return None
        from ..hip_backend import frame_scale_array
        if not self.backend.can_frame_scale:
            raise ValueError("scale= needs a filter built with frame_scale=True")
        return frame_scale_array(scale)

    # -- odometry input: the camera's motion between frames (ekf_move) ---------------------------------
    def move(self, d, w) -> None:
        """The camera has moved by the translation ``d`` and the rotation vector ``w`` (radians), both in its own frame
        before the move: the pose is moved and P is propagated through the move's Jacobian on the device (nothing is
        synchronised).  A filter built with ``motion=True``; anything that is not two finite 3-vectors raises
        ``ValueError`` and nothing changes."""
        if np.shape(d) != (3,) or np.shape(w) != (3,):
            raise ValueError(f"motion: d and w must have shape (3,), got {np.shape(d)} and {np.shape(w)}")
        self._move(self._frame_motion(np.concatenate((d, w))))

    def _move(self, motion) -> None:
        self.backend.move(motion)
        self._moved = True

    def _frame_motion(self, motion):
        """``motion=`` of ``observe`` / ``process_detections``: None, or a float64 [6] array.  ``ValueError`` for another
        shape, a NaN or Inf entry and a filter built without ``motion=True``; checked before the frame changes anything."""
        if motion is None:
            return None
        from ..hip_backend import motion_array
        if not self.backend.can_motion:
            raise ValueError("motion= needs a filter built with motion=True")
        return motion_array(motion)

    def _lm_variances(self, lm_dims: int, predicted: bool) -> np.ndarray:
        """The landmark part of diag(P), [n, lm_dims]: P of the last stepped frame, or with ``predicted`` what the next
        stepped frame would start from if no more time passed, diag(P) + fl(pending_scale q_lm) (formed on the host)."""
        out = self.backend.get_cov_diag()[CAM_DIMS:].reshape(-1, lm_dims)
        if predicted:
            out = out + self.backend.pending_scale * float(self.backend.cfg.q_lm)
        return out

    # -- map pruning (ekf_remove_markers) ----------------------------------------------------------
    def remove_marker(self, marker_id) -> None:
        """``remove_markers([marker_id])``."""
        self.remove_markers([marker_id])

    def remove_markers(self, ids) -> None:
        """Take the landmarks of these marker ids out of the map: their rows and columns of P and their state entries are
        deleted on the device (marginalisation; nothing else changes, nothing is synchronised), the other landmarks keep
        their order and move up (new index = old index - removed indices below it).  An unknown id raises ``KeyError``
        and a duplicate ``ValueError`` before anything runs.  A removed id that is seen again is a first sighting: a new
        landmark at the end, exempt from the gate like any other."""
        ids = [int(i) for i in np.asarray(ids).reshape(-1).tolist()] if isinstance(ids, np.ndarray) else [int(i) for i in ids]
        for marker in ids:
            if marker not in self.landmarks:
                raise KeyError(f"marker {marker} is not in the map")
        if len(set(ids)) != len(ids):
            raise ValueError("duplicate marker id in the removal list")
        if not ids:
            return
        self.backend.remove_markers([self.landmarks[marker] for marker in ids])
        self._drop_from_table(ids)

    def _drop_from_table(self, ids) -> None:
        """Host side of a removal the back-end has enqueued: the id table, the count and the policy."""
        from .map_management import renumber_landmarks
        self.landmarks = renumber_landmarks(self.landmarks, [self.landmarks[marker] for marker in ids])
        self.num_landmarks -= len(ids)
        self._pruned = True
        if self._tentative is not None:
            self._tentative.forget(ids)

    def _prune_tentative(self, ids) -> None:
        """End of a frame of ``process_detections`` under ``confirm=``: feed the policy the frame's ids and which of its
        detections the gate let through, and remove what it gives up on (one ``remove_markers`` call, if any)."""
        if ids is None:
            stale = self._tentative.end_frame()
        else:
            ids = [int(i) for i in np.asarray(ids).reshape(-1).tolist()]
            rejected = self.last_rejected if self.backend.can_gate else None
            stale = self._tentative.end_frame(ids, None if rejected is None else ~np.asarray(rejected, dtype=bool))
        if stale:
            self.remove_markers(stale)

    @staticmethod
    def _first_occurrences(ids, fresh):
        """bool [m]: the first detection of every marker in ``fresh`` (the markers the frame has just added)."""
        left, out = set(fresh), np.zeros(len(ids), dtype=bool)
        for j, marker in enumerate(ids):
            if marker in left:
                left.discard(marker)
                out[j] = True
        return out

    def _frame_noise(self, noise, count: int):
        """``noise=`` of ``observe``: None, or the frame's row variances [count, rd] from [count] (one variance per
        detection, broadcast over its rows) or [count, rd].  ``ValueError`` for anything else, for an entry that is not
        finite and > 0, and for a filter built without ``row_noise=True``; checked before the frame changes anything."""
        if noise is None:
            return None
        from ..hip_backend import row_noise_array
        backend = self.backend
        if not backend.can_row_noise:
            raise ValueError("noise= needs a filter built with row_noise=True")
        return row_noise_array(noise, count, backend.rows_per_detection)

    def _observe_gated(self, index, z, exempt, rows=None, scale=None) -> None:
        backend = self.backend
        d2 = backend.observe(index, z, exempt=exempt, mahal=True, rows=rows, scale=scale)
        self.last_mahal = d2
        self.last_rejected = d2 > backend.gate      # (NaN and 0 compare false; gate inf: nothing)

    def process_detection_log(self, ids, poses, offsets, has_detections=None, mahal=False, noise=None, scale=None,
                              motion=None):
        """``process_detections(ids_t, poses_t)`` with ``should_filter=True`` for every frame of a recorded log, in ONE call
        that runs predict / update of every frame on the device (ekf_observe_log).  The log is a CSR batch as in a replay
        file (``main/run_slam.py: detection_frames``): ``ids [D]``, ``poses [D,6]`` ``[tvec | rvec]`` (NumPy, or a
        float64 tensor on the filter's device), ``offsets [F+1]``, ``has_detections [F]`` (None: every non-empty frame).
        A frame without detections is not stepped.  Marker ids are mapped to landmark indices here (``plan_detection_log``);
        the buffers grow first if the log needs more landmarks or detections per frame.  Returns the camera pose
        ``state[0:7]`` after every frame, ``(F, 7)``.  A malformed log raises ``ValueError`` before anything runs, and the
        filter (``landmarks`` included) is left as it was.  A gate that is set (``set_gate``) acts on every frame, with
        the first occurrence of every marker the log adds exempt; ``mahal=True`` (a filter built with ``gate=``) returns
        ``(trajectory, d2 [D])`` with every detection's squared Mahalanobis distance, indexed like ``ids`` (NaN for the
        rows of frames without detections), gate or no gate; ``d2 > gate`` are the rejected ones.  ``noise``: per-detection
        measurement noise of the log, [D] or [D, rd] aligned with ``ids`` (a filter built with ``row_noise=True``).
        ``scale``: the frames' process-noise scales, [F], one per frame of the log (a filter built with
        ``frame_scale=True``): a frame that is not stepped leaves its scale pending for the next stepped one.
        ``motion``: the camera's motion before every frame, [F, 6], one row per frame of the log, empty frames included (a
        filter built with ``motion=True``); such a replay runs its frames in serial order.
        On a frozen map (``freeze_map``) detections of ids the map does not hold are dropped (``last_ignored``; their d2 is
        NaN), nothing is added, and the replay runs its frames in serial order."""
        return self._replay_detection_log(ids, poses, offsets, has_detections, mahal, noise, scale, motion, False)

    def _replay_detection_log(self, ids, poses, offsets, has_detections, mahal, noise, scale, motion, smooth):
        """``process_detection_log``; ``smooth``: the replay is recorded (``observe_log(history=)``), the backward pass runs
        over the records, and the smoothed trajectory comes back behind the filtered one (``EKF.smooth_detection_log``);
        ``smooth="cov"``: the pass forms the covariances too, and ``filtered_cov``, ``smoothed_cov`` [F, 10, 10] follow."""
        import torch
        backend = self.backend
        plan = plan_detection_log(self.landmarks, self.num_landmarks, ids, offsets, has_detections, self.map_frozen)
        if isinstance(poses, torch.Tensor):
            if not poses.is_cuda or poses.device != backend.device:
                raise ValueError(f"poses must be on {backend.device} (got {poses.device})")
            if poses.dtype != torch.float64:
                raise ValueError("poses must be float64")
        else:
            poses = np.asarray(poses, dtype=np.float64)
        if tuple(poses.shape) != (plan.keep.shape[0], 6):
            raise ValueError(f"poses must have shape ({plan.keep.shape[0]}, 6), got {tuple(poses.shape)}")
        rows = self._frame_noise(noise, plan.keep.shape[0])
        if rows is not None:
            rows = rows[plan.keep]
        if scale is not None:
            from ..hip_backend import frame_scale_array
            if not backend.can_frame_scale:
                raise ValueError("scale= needs a filter built with frame_scale=True")
            scale = frame_scale_array(scale, plan.offsets.shape[0] - 1)
        if motion is not None:
            from ..hip_backend import motion_array
            if not backend.can_motion:
                raise ValueError("motion= needs a filter built with motion=True")
            motion = motion_array(motion, plan.offsets.shape[0] - 1)
        if not plan.keep.all():      # (rows of frames without detections, if there are any, are not part of the replay)
            poses = poses[torch.from_numpy(plan.keep).to(poses.device)] if isinstance(poses, torch.Tensor) else poses[plan.keep]
        if isinstance(poses, torch.Tensor):
            poses = poses.contiguous()
        if plan.num_landmarks > backend.max_landmarks:
            backend.grow(plan.num_landmarks)
        if plan.widest > backend.max_visible:
            backend.grow(new_max_visible=min(backend.MAX_VISIBLE_LIMIT[backend.lm_dims], plan.widest))
        traj = torch.empty((plan.offsets.shape[0] - 1, 7), dtype=torch.float64, device=backend.device)
        mahal_t = torch.empty((plan.index.shape[0],), dtype=torch.float64, device=backend.device) if mahal else None
        history = backend.new_history(plan.index, plan.offsets) if smooth else None
        backend.observe_log(plan.index, plan.offsets, poses, traj, mahal_t, rows, scale, motion,
                            **({"history": history} if smooth else {}))
        backend.sync()
        if motion is not None and motion.any():
            self._moved = True
        self.last_ignored = plan.ignored
        self.landmarks.update(plan.new_landmarks)
        self.num_landmarks = plan.num_landmarks
        if self._tentative is not None:      # (confirm=: the policy sees per-frame calls only; what a replay adds stays)
            self._tentative.confirm(plan.new_landmarks)
        out = (traj.cpu().numpy(),)
        if smooth:
            self._smoothed_cov = None
            if smooth == "cov":
                res = backend.smooth_history_cov(history, traj.shape[0])
                self._smoothed = res["smoothed"].cpu().numpy()
                self._smoothed_cov = res["cam_cov"].cpu().numpy()
                out += (self._smoothed, res["filt_cam_cov"].cpu().numpy(), self._smoothed_cov)
            else:
                self._smoothed = backend.smooth_history(history, traj.shape[0]).cpu().numpy()
                out += (self._smoothed,)
        if mahal:
            d2 = np.full(plan.keep.shape[0], np.nan)
            d2[plan.keep] = mahal_t.cpu().numpy()
            out += (d2,)
        return out[0] if len(out) == 1 else out

    def save_map(self, filename: str) -> None:
        """Map text format of base_filter.py:214-247: three comment lines and a
        blank, then one record per landmark in index order -- marker id, pose
        numbers, their variances (each ``", "``-separated through ``str()``) and a
        blank line."""
        _, rows = self.get_poses()
        variances = self.get_lm_uncertainties()
        marker_of = dict((index, marker) for marker, index in self.get_lm_estimates())

        def record(index):
            pose = rows[index]
            numbers = (pose, variances[index, :len(pose)])
            return "\n".join([str(marker_of[index])] + [", ".join(str(v) for v in vals) for vals in numbers]) + "\n\n"

        header = "# landmark_id\n# x y z\n# uncertainty\n\n"
        Path(filename).write_text(header + "".join(record(i) for i in range(len(rows))), encoding="utf-8")

    def load_map(self, filename: str) -> None:
        """Reader for the ``save_map`` format (base_filter.py:249-272: skip 4
        header lines, stride 4).  The reference's version ends in
        ``self.filter.add_marker`` (an AttributeError, :272); this one calls the
        intended restore hook ``self.add_marker(id, pose, uncertainty)``."""
        with Path(filename).open("r", encoding="utf-8") as file:
            lines = file.readlines()[4:]
        for i in range(0, len(lines) - 2, 4):
            id_ = int(lines[i].strip())
            pose = np.array(lines[i + 1].strip().split(", "), np.float64)
            uncertainty = np.array(lines[i + 2].strip().split(", "), np.float64)
            self.add_marker(id_, pose, uncertainty)
        if self._tentative is not None:      # landmarks restored from a map file are confirmed from the start
            self._tentative.confirm(self.landmarks)

    def reset(self) -> None:
        """Back to the state of a freshly constructed filter (initial pose, no landmarks, status cleared): the way out
        of a sticky device-side error (non-SPD innovation covariance, bad device-resident index, ...), usually followed
        by ``load_checkpoint``."""
        self.backend.reset(np.asarray(self._initial_pose, dtype=np.float64))
        self.landmarks = {}
        self.num_landmarks = 0
        self._pruned = False
        self._moved = False
        self.last_ignored = ()      # (the back-end's reset has unfrozen the map)
        if self._tentative is not None:
            self._tentative.clear()

    # -- resume (no reference counterpart: its map restore is the dead :249-272) -----
    def save_checkpoint(self, filename: str) -> None:
        """Full filter state for an exact resume: state vector, dense covariance (float64 copy of
        the device matrix) and the marker-id -> index table, as a plain ``.npz``."""
        ids = [k for k, _ in sorted(self.get_lm_estimates(), key=lambda kv: kv[1])]
        gate = self.backend.gate
        np.savez(filename, state=np.asarray(self.state, dtype=np.float64),
                 cov=np.asarray(self.uncertainty, dtype=np.float64),
                 marker_ids=np.asarray(ids, dtype=np.int64), filter=type(self).__name__,
                 gate=np.float64(np.inf if gate is None else gate), row_noise=np.bool_(self.backend.can_row_noise),
                 frame_scale=np.bool_(self.backend.can_frame_scale), pending_scale=np.float64(self.backend.pending_scale),
                 motion=np.bool_(self.backend.can_motion), map_frozen=np.bool_(self.backend.map_frozen))

    def load_checkpoint(self, filename: str) -> None:
        """Inverse of ``save_checkpoint`` on a filter of the same class; the device covariance
        is overwritten bit-for-bit when the stored values fit the covariance dtype.  The gate is part of the checkpoint: a
        filter built with ``gate=`` takes the stored one, so a checkpoint saved without a gate (stored as ``inf``) switches
        this filter's gate OFF -- call ``set_gate`` afterwards to keep your own; a stored finite gate needs a filter built
        with ``gate=`` (``ValueError`` otherwise).  Checkpoints from before the gate leave it as it is.  A checkpoint of a
        filter built with ``row_noise=True`` needs one built the same way (``ValueError`` otherwise), and so does one of a
        filter built with ``frame_scale=True``, whose pending scale is restored; a checkpoint without it leaves the pending
        scale 0.  Whether the map was frozen is part of the checkpoint; one from before that loads as not frozen."""
        with np.load(filename, allow_pickle=False) as ck:
            if str(ck["filter"]) != type(self).__name__:
                raise ValueError(f"checkpoint of {ck['filter']} loaded into {type(self).__name__}")
            state, cov, ids = ck["state"], ck["cov"], ck["marker_ids"]
            gate = float(ck["gate"]) if "gate" in ck.files else None      # (checkpoints from before the gate: as it is)
            row_noise = bool(ck["row_noise"]) if "row_noise" in ck.files else False
            frame_scale = bool(ck["frame_scale"]) if "frame_scale" in ck.files else False
            pending = float(ck["pending_scale"]) if "pending_scale" in ck.files else 0.0
            motion = bool(ck["motion"]) if "motion" in ck.files else False
            frozen = bool(ck["map_frozen"]) if "map_frozen" in ck.files else False      # (older checkpoints: not frozen)
        if motion and not self.backend.can_motion:
            raise ValueError("the checkpoint is of a filter with camera motions: build this one with motion=True")
        if frame_scale and not self.backend.can_frame_scale:
            raise ValueError("the checkpoint is of a filter with per-frame scales: build this one with frame_scale=True")
        if row_noise and not self.backend.can_row_noise:
            raise ValueError("the checkpoint is of a filter with per-detection noise: build this one with row_noise=True")
        if gate is not None and (np.isfinite(gate) or self.backend.can_gate):
            self.set_gate(gate)      # (a finite gate needs a filter built with gate=: ValueError otherwise)
        self.backend.set_map_frozen(frozen)
        if len(ids) == 0:
            if self.backend.can_frame_scale:
                self.backend.pending_scale = pending
            return
        self.backend.set_state_cov(state, cov)
        if self.backend.can_frame_scale:      # (set_state_cov has zeroed it)
            self.backend.pending_scale = pending
        self.landmarks = {int(k): i for i, k in enumerate(ids)}
        self.num_landmarks = len(ids)
        if self._tentative is not None:      # a checkpoint's landmarks are confirmed, like a map file's
            self._tentative.forget(list(self._tentative.tentative))
            self._tentative.confirm(self.landmarks)

    # -- abstract back-end API, base_filter.py:327-381 ------------------------
    def observe(self, ids, poses, noise=None, scale=None, motion=None) -> None:
        raise NotImplementedError(NOT_IMPLEMENTED_ERROR)

    def get_poses(self):
        raise NotImplementedError(NOT_IMPLEMENTED_ERROR)

    def get_lm_uncertainties(self, predicted=False):
        raise NotImplementedError(NOT_IMPLEMENTED_ERROR)

    def get_lm_estimates(self):
        raise NotImplementedError(NOT_IMPLEMENTED_ERROR)

    def get_cam_estimate(self, iteration: int):
        raise NotImplementedError(NOT_IMPLEMENTED_ERROR)
