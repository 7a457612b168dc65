"""``EKF``: drop-in for the reference filter of the same name
(/root/reference/filters/extended_kalman_filter.py:37-357) whose per-frame
``observe`` (predict + update, :58-156) runs as HIP kernels on an MI355X.

Same constructor, methods, attributes and error behaviour at the boundary
``BaseFilter`` drives.  The marker-id -> landmark-index
dictionary stays here on the host; state and covariance live in HBM.
"""
from __future__ import annotations

import functools

import numpy as np

from ..hip_backend import HipEkf
from .base_filter import BaseFilter, dictionary_size

MOVING_AVG_WINDOW = 10   # unused in the reference as well (:19)

INITIAL_CAMERA_UNCERTAINTY = 0.1
INITIAL_LANDMARK_UNCERTAINTY = 0.7
R_UNCERTAINTY = 0.9
Q_UNCERTAINTY_CAM = 0.3
Q_ERROR_UNCERTAINTY_CAM = 0.5
Q_UNCERTAINTY_LM = 0.01

CAM_DIMS = 10
XYZ_DIMS = slice(0, 3)
QUAT_DIMS = slice(3, 7)
ERROR_DIMS = slice(7, 10)
LM_DIMS = 3


def _cov_keyword(plain):
    """Gives ``smooth_detection_log`` its keyword-only option ``cov``: ``cov=True`` runs the same replay with
    the covariance pass behind it; without it the call is the plain method, positional arguments as they were."""
    @functools.wraps(plain)
    def call(self, *args, cov=False, **kw):
        return self._smooth_log("cov", *args, **kw) if cov else plain(self, *args, **kw)
    return call


class EKF(BaseFilter):
    """Object for tracking the positions of the camera and landmarks."""

    def __init__(self, initial_camera_pose, aruco_dict=None, *, max_landmarks: int | None = None,
                 max_visible: int | None = None, cov_dtype: str = "float64",
                 quat_update: str = "as_written", cov_kernel: str = "auto",
                 device: str = "cuda:0", map_file=None, lookahead: bool | None = None,
                 fused: bool = True, noise: dict | None = None, gate: float | None = None, confirm: tuple | None = None,
                 row_noise: bool = False, frame_scale: bool = False, motion: bool = False, localize: bool = False) -> None:
        """Positional arguments as the reference (:40-43).  Keyword-only extras:
        initial capacity (default: the number of ids of ``aruco_dict`` -- DICT_5X5_50
        has 50, base_filter.py:81-82; the buffers grow when more markers or more
        detections per frame show up, as the reference's arrays do, :274-290), covariance
        storage dtype, and the quaternion-injection convention
        (``"as_written"`` reproduces :138-149 exactly, ``"scalar_first"`` is the
        consistent one).  ``noise``: values that replace the module's noise constants, keyed by the
        ``ekf_config`` field names (``initial_camera_uncertainty``, ``initial_landmark_uncertainty``,
        ``r_uncertainty``, ``q_cam``, ``q_err``, ``q_lm``); None keeps the reference's constants.
        ``gate``: the chi-square gate on every detection's own Mahalanobis distance (``set_gate``; 3 degrees of
        freedom: 7.815 / 11.345 / 16.266 for 95 / 99 / 99.9 %); ``inf``: off, but the distances are reported
        (``last_mahal``); None: a filter without the gate.
        ``confirm``: ``(hits, window)`` = a new landmark must be used again in ``hits`` later frames within ``window``
        frames of its first sighting, or ``process_detections`` removes it again (``remove_markers``); None: off.
        ``row_noise``: the filter takes per-detection measurement noise (``observe(..., noise=)``).
        ``frame_scale``: frames may carry a process-noise scale (``observe(..., scale=)``, ``advance``): time between
        frames, in units of a nominal frame period, multiplies Q, and time without an update is kept for the next one.
        ``motion``: frames may carry the camera's motion since the previous frame (``observe(..., motion=)``, ``move``):
        odometry moves the prior instead of leaving the update to catch up with a camera the model holds still.
        ``localize``: with ``map_file``, run in the map made earlier without changing it: the same as loading the map and
        then calling ``freeze_map()`` (``ValueError`` without a ``map_file``)."""
        if localize and map_file is None:
            raise ValueError("localize=True needs a map_file: there is no map to localise in")
        super().__init__(initial_camera_pose, map_file, aruco_dict)
        self._initial_pose = np.array(initial_camera_pose)      # :46, dtype kept
        if self._initial_pose.shape != (CAM_DIMS,):
            raise ValueError("initial_camera_pose must have 10 entries")
        self.num_landmarks = 0
        self.landmarks = {}
        if max_landmarks is None:
            max_landmarks = dictionary_size(aruco_dict)
        if max_visible is None:
            max_visible = min(max_landmarks, 64)
        constants = {"initial_camera_uncertainty": INITIAL_CAMERA_UNCERTAINTY,
                     "initial_landmark_uncertainty": INITIAL_LANDMARK_UNCERTAINTY,
                     "r_uncertainty": R_UNCERTAINTY, "q_cam": Q_UNCERTAINTY_CAM,
                     "q_err": Q_ERROR_UNCERTAINTY_CAM, "q_lm": Q_UNCERTAINTY_LM}
        unknown = set(noise or {}) - set(constants)
        if unknown:
            raise ValueError(f"unknown noise constants {sorted(unknown)}; known: {sorted(constants)}")
        constants.update(noise or {})
        self._hip = HipEkf(max_landmarks, max_visible, cov_dtype=cov_dtype,
                           quat_mode=quat_update, cov_kernel=cov_kernel, device=device, lookahead=lookahead, fused=fused,
                           noise=constants, gate=gate, row_noise=row_noise, frame_scale=frame_scale,
                           motion=motion)
        self._hip.reset(self._initial_pose.astype(np.float64))
        self._load_initial_map()
        self._init_confirm(confirm)
        if localize:
            self.freeze_map()

    # -- attributes the base class / callers read (base_filter.py:293-304) ---
    @property
    def state(self) -> np.ndarray:
        if self.num_landmarks == 0 and not self._pruned and not self._moved:
            # the reference keeps the caller's (int64) array until the first
            # hstack (:46, :274): D7 in SURVEY appendix A
            return self._initial_pose
        return self._hip.get_state()

    @property
    def uncertainty(self) -> np.ndarray:
        return self._hip.get_cov()

    # -- :58-82 ----------------------------------------------------------------
    def observe(self, ids, poses, noise=None, scale=None, motion=None) -> None:
        """Add unseen markers, predict, update.  ``ids``: iterable of marker
        ids; ``poses``: (m, 6) ``[tvec | rvec]``, only ``pose[0:3]`` is used.  ``noise`` (a filter built with
        ``row_noise=True``): the frame's measurement noise, [m] (one variance per detection) or [m, 3] (x, y, z in the
        camera frame) instead of ``r_uncertainty``; anything else raises ``ValueError`` before the frame changes anything.
        ``scale`` (a filter built with ``frame_scale=True``): the frame's process-noise scale, a number >= 0; the frame
        runs with Q times (pending scale + scale).  ``motion`` (a filter built with ``motion=True``): six numbers
        ``(d, w)``, the camera's translation and rotation vector since the previous frame in its own frame; the same as
        ``move(d, w)`` followed by the call without it: the arguments are validated first, then the camera moves, then the frame runs -- an error the frame itself raises afterwards (capacity, a sticky device error) leaves the camera moved."""
        if isinstance(ids, np.ndarray) and ids.dtype.kind in "iu":
            ids = ids.reshape(-1).tolist()     # (what process_frame passes: ids.flatten(), base_filter.py:199)
        else:
            ids = [int(i) for i in ids]
        if not ids:
            raise ValueError("observe() needs at least one detection")
        poses = np.asarray(poses, dtype=np.float64).reshape(len(ids), -1)
        rows = self._frame_noise(noise, len(ids))
        scale = self._frame_scale(scale)
        motion = self._frame_motion(motion)
        self.last_ignored = ()
        if self.map_frozen:         # localisation: nothing is added, unknown ids are dropped
            return self._observe_frozen(ids, poses, rows, scale, motion)
        if motion is not None:      # the camera moves first: first sightings are placed from the moved camera
            self._move(motion)
        known = self.landmarks
        try:                                   # steady state: every marker of the frame is in the map already
            index = [known[i] for i in ids]
        except KeyError:
            fresh, new_xyz = [], []
            for idx, pose in zip(ids, poses):
                if idx in known or idx in fresh:
                    continue
                fresh.append(idx)
                new_xyz.append(pose[XYZ_DIMS])
            # every add_marker of a frame sees the same (pre-update) camera pose
            self._hip.add_markers(np.asarray(new_xyz))
            for idx in fresh:
                known[idx] = self.num_landmarks
                self.num_landmarks += 1
            index = [known[i] for i in ids]
            if self._hip.can_gate:      # the markers added just now are exempt from the gate (their z = h by construction)
                return self._observe_gated(index, poses[:, XYZ_DIMS], self._first_occurrences(ids, fresh), rows, scale)
        if self._hip.can_gate:
            return self._observe_gated(index, poses[:, XYZ_DIMS], None, rows, scale)
        self._hip.observe(index, poses[:, XYZ_DIMS], rows=rows, scale=scale)

    def _measurements(self, poses) -> np.ndarray:
        """z of the detections of a frame, [m, 3]: the marker positions in the camera frame."""
        return poses[:, XYZ_DIMS]

    # -- :239-290 --------------------------------------------------------------
    def add_marker(self, idx, pose, uncertainity=None) -> None:
        """(sic) ``uncertainity`` -- keyword spelled as in the reference."""
        self._hip.add_markers(np.asarray(pose, dtype=np.float64)[XYZ_DIMS][None, :], uncertainity)
        self.landmarks[idx] = self.num_landmarks
        self.num_landmarks += 1

    # -- :84-93, :355-357 --------------------------------------------------------
    def get_poses(self):
        state = self.state
        return state[:CAM_DIMS], state[CAM_DIMS:].reshape(-1, LM_DIMS)

    def get_lm_uncertainties(self, predicted: bool = False) -> np.ndarray:
        """diag(P) of the landmarks, [n, LM_DIMS]: P of the last stepped frame; ``predicted=True`` adds the process noise
        of the pending scale, fl(pending_scale q_lm), on the host."""
        return self._lm_variances(LM_DIMS, predicted)

    def get_lm_estimates(self):
        return self.landmarks.items()

    # -- offline smoothing (the reference's run_offline.py flow) ------
    @_cov_keyword
    def smooth_detection_log(self, ids, poses, offsets, has_detections=None, noise=None, scale=None, motion=None,
                             mahal=False):
        """``process_detection_log`` with a Rauch-Tung-Striebel backward pass behind it: the replay is recorded on the
        device, the pass runs over the records, and ``(filtered [F, 7], smoothed [F, 7])`` come back (plus ``d2 [D]`` with
        ``mahal=True``).  The log is planned, the buffers grow and everything is validated as in ``process_detection_log``,
        and the filter is left exactly where that call leaves it, bit for bit.  The smoothed log stays with the filter:
        ``get_cam_estimate(i)`` returns its row i.  Needs ``quat_update="scalar_first"`` and the float64 covariance; a
        frozen map is refused (``ValueError``, before anything runs).
        Keyword-only ``cov=True`` (default False): the pass forms the smoothed covariances as well and the
        call returns ``(filtered, smoothed, filtered_cov [F, 10, 10], smoothed_cov [F, 10, 10])`` (plus ``d2``): the camera
        blocks of P_r and of P^s_r of every frame's record, NaN for frames before the first record;
        ``get_cam_estimate_cov(i)`` returns row i."""
        return self._smooth_log(True, ids, poses, offsets, has_detections, noise, scale, motion, mahal)

    def _smooth_log(self, mode, ids, poses, offsets, has_detections=None, noise=None, scale=None, motion=None, mahal=False):
        """``smooth_detection_log``; mode True: poses only, "cov": with the covariances."""
        from ..hip_backend import EKF_COV_F64, EKF_QUAT_SCALAR_FIRST
        backend = self.backend
        if backend.cfg.quat_mode != EKF_QUAT_SCALAR_FIRST:
            raise ValueError('smoothing needs quat_update="scalar_first": the as-written injection has no inverse')
        if backend.cfg.cov_dtype != EKF_COV_F64:
            raise ValueError('smoothing needs cov_dtype="float64"')
        if self.map_frozen:
            raise ValueError("smoothing a frozen map is not supported: unfreeze_map() first")
        return self._replay_detection_log(ids, poses, offsets, has_detections, mahal, noise, scale, motion, mode)

    def get_cam_estimate(self, iteration: int):
        """Row ``iteration`` of the last smoothed log as ``process_detections(should_filter=False, iteration=i)`` expects
        it: ``[xyz, q, 0, 0, 0]``.  ``IndexError`` outside the log; ``NotImplementedError`` when nothing has been smoothed."""
        smoothed = getattr(self, "_smoothed", None)
        if smoothed is None:
            return super().get_cam_estimate(iteration)
        i = int(iteration)
        if not 0 <= i < smoothed.shape[0]:
            raise IndexError(f"frame {iteration} is outside the smoothed log of {smoothed.shape[0]} frames")
        return np.concatenate((smoothed[i], np.zeros(3)))

    def get_cam_estimate_cov(self, iteration: int):
        """Row ``iteration`` of the last smoothed covariance, [10, 10] (``smooth_detection_log(cov=True)``).  ``IndexError``
        outside the log; ``NotImplementedError`` when nothing has been smoothed with ``cov``."""
        cov = getattr(self, "_smoothed_cov", None)
        if cov is None:
            raise NotImplementedError("no smoothed covariance: call smooth_detection_log(..., cov=True) first")
        i = int(iteration)
        if not 0 <= i < cov.shape[0]:
            raise IndexError(f"frame {iteration} is outside the smoothed log of {cov.shape[0]} frames")
        return cov[i].copy()

    # -- extras: resident-detection batch entry, used by bench / replay --------
    @property
    def backend(self) -> HipEkf:
        return self._hip
