"""App loop: counterpart of the reference's ``main/run_slam.py``
(/root/reference/main/run_slam.py:82-173) for the filters this package ships.

    python -m aruco_slam_amd.main.run_slam --video input_video.mp4 --filter ekf
    python -m aruco_slam_amd.main.run_slam --detections tests/golden/c1_detections.npz
    python -m aruco_slam_amd.main.run_slam --detections tests/golden/c1_detections.npz --resident

Same CLI (``--video``, ``--filter``), same outputs (``outputs/trajectory.txt``
one line per frame, ``outputs/map.txt`` at exit).  The image has no OpenCV and
no video, so frames can also come from a detections replay file
(``--detections``): per frame a timestamp and the ``(ids, poses)`` the ArUco
front-end would have produced (``ids`` absent on frames without detections, in
which case the filter is not stepped -- base_filter.py:197-204).  With
``--resident`` the whole replay runs on the device in one call
(``process_detection_log``) and the outputs are written afterwards, byte for
byte what the frame-by-frame loop writes.  The 2-D/3-D viewers are GUI code
and are not part of this package.

    python -m aruco_slam_amd.main.run_slam --detections replay.npz --frame-period 33.3 --gate 7.815

``--frame-period MS`` makes the predict step time-aware: every frame's process noise is scaled by the time since the
previous frame in units of ``MS`` (a replay file's ``timestamps_ms``), and frames without an update leave their time
pending for the next one, so a gated filter finds its way back after a detection dropout.

    python -m aruco_slam_amd.main.run_slam --detections replay.npz --map outputs/map.txt --localize

``--map FILE`` starts from a map written earlier (the reference's ``LOAD_MAP`` / ``MAP_FILE``), with or without
``--resident``; ``--localize`` freezes it: the camera is tracked in the map as it is, markers the map does not hold are
ignored, and the ``map.txt`` written at exit is the one that was loaded.

    python -m aruco_slam_amd.main.run_slam --detections replay.npz --resident --smooth

``--smooth`` is the offline mode (the reference's ``main/run_offline.py``): the replay is recorded on the device, a backward
pass runs over it, and ``trajectory.txt`` carries for every frame the pose that the whole log supports.
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np

from ..filters.base_filter import BaseFilter, cv2
from ..filters.ekf_with_rotations import EKF_Rotations
from ..filters.extended_kalman_filter import EKF
from ..outputs.trajectory_writer import TrajectoryWriter

TRAJECTORY_TEXT_FILE = "outputs/trajectory.txt"     # run_slam.py:28
MAP_FILE = "outputs/map.txt"                        # run_slam.py:32
IMAGE_SIZE = 1920, 1080                             # run_slam.py:43


def init_tracker(filter_type: str, initial_pose: np.ndarray, **kwargs) -> BaseFilter:
    """run_slam.py:69-79.  The two EKF back-ends are accelerated; the factor graph is GTSAM."""
    if filter_type == "ekf":
        return EKF(initial_pose, **kwargs)
    if filter_type == "ekf_rotations":
        return EKF_Rotations(initial_pose, **kwargs)
    if filter_type == "factorgraph":
        raise NotImplementedError(
            f"filter '{filter_type}' is outside this package's scope (SURVEY section 8)")
    raise ValueError(f"Unknown filter type: {filter_type}")


def detection_frames(path: str):
    """Yield ``(timestamp_ms, ids | None, poses)`` from a replay ``.npz`` with
    arrays ids [sum m], poses [sum m, 6], offsets [F+1], timestamps_ms [F],
    has_detections [F]."""
    det = np.load(path, allow_pickle=False)
    offs = det["offsets"]
    for f in range(len(det["timestamps_ms"])):
        sl = slice(int(offs[f]), int(offs[f + 1]))
        ids = det["ids"][sl] if det["has_detections"][f] else None
        yield float(det["timestamps_ms"][f]), ids, det["poses"][sl]


def detection_noise(path: str):
    """The optional ``noise`` array of a replay file: per-detection measurement noise, [sum m] (one variance per detection)
    or [sum m, RD] (one per measurement row), aligned with ``ids``; None for a file without one."""
    det = np.load(path, allow_pickle=False)
    return np.asarray(det["noise"], dtype=np.float64) if "noise" in det.files else None


def detection_motion(path: str):
    """The optional ``motion`` array of a replay file: the camera's motion ``(d, w)`` before every frame, in the camera frame
    of the previous pose, [F, 6] with one row per frame (empty frames included); None for a file without one.  Another shape
    or an entry that is not finite raises ``ValueError``."""
    det = np.load(path, allow_pickle=False)
    if "motion" not in det.files:
        return None
    from ..hip_backend import motion_array
    return motion_array(det["motion"], len(det["timestamps_ms"]))


def frame_scales(path: str, frame_period_ms: float) -> np.ndarray:
    """The per-frame process-noise scales of a replay file for ``--frame-period``: ``(t_f - t_{f-1}) / frame_period_ms``
    from its ``timestamps_ms``, 1 for frame 0.  Timestamps that decrease, or a period that is not a finite number > 0,
    raise ``ValueError``."""
    period = float(frame_period_ms)
    if not (np.isfinite(period) and period > 0.0):
        raise ValueError(f"--frame-period must be > 0, got {frame_period_ms}")
    stamps = np.asarray(np.load(path, allow_pickle=False)["timestamps_ms"], dtype=np.float64)
    steps = np.diff(stamps)
    if not np.isfinite(stamps).all() or (steps < 0).any():
        raise ValueError("timestamps_ms must be finite and must not decrease")
    return np.concatenate((np.ones(min(1, stamps.shape[0])), steps / period))


def replay_resident(tracker: BaseFilter, path: str, cam_traj_writer: TrajectoryWriter, scales=None, motion=None,
                    smooth: bool = False, smooth_cov=None) -> None:
    """The whole replay file through ``process_detection_log``, then one trajectory line per frame.  Frames before the first
    stepped one carry the camera pose the filter had before the call (the integer initial pose of a fresh filter), as the
    frame-by-frame loop writes them; from the first frame with a motion on, the row is the (moved) pose of the device.
    ``smooth``: the replay goes through ``smooth_detection_log`` and the lines carry the smoothed poses; ``smooth_cov``: a
    file name, the pass forms the covariances too and ``smoothed_cov``, ``filtered_cov`` [F, 10, 10] are written there."""
    det = np.load(path, allow_pickle=False)
    offsets, has = det["offsets"], det["has_detections"].astype(bool)
    start_pose = tracker.get_poses()[0]
    noise = detection_noise(path)
    extra = {} if noise is None else {"noise": noise}
    if scales is not None:
        extra["scale"] = scales
    if motion is not None:
        extra["motion"] = motion
    if smooth and smooth_cov:
        _filtered, traj, filtered_cov, smoothed_cov = tracker.smooth_detection_log(det["ids"], det["poses"], offsets, has,
                                                                                   cov=True, **extra)
        np.savez(smooth_cov, smoothed_cov=smoothed_cov, filtered_cov=filtered_cov)
    elif smooth:
        _filtered, traj = tracker.smooth_detection_log(det["ids"], det["poses"], offsets, has, **extra)
    else:
        traj = tracker.process_detection_log(det["ids"], det["poses"], offsets, has, **extra)
    stepped = has & (np.diff(offsets) > 0)
    if motion is not None:
        stepped = stepped | motion.any(axis=1)
    first = int(np.argmax(stepped)) if stepped.any() else len(has)
    for f, timestamp in enumerate(det["timestamps_ms"]):
        cam_traj_writer.write(float(timestamp), start_pose if f < first else traj[f])


def main(cmdline_args: argparse.Namespace) -> None:
    initial_pose = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])     # run_slam.py:85-88 (int64)
    kwargs = dict(getattr(cmdline_args, "filter_kwargs", {}))
    map_file = getattr(cmdline_args, "map", None)
    if getattr(cmdline_args, "localize", False) and map_file is None:
        raise ValueError("--localize tracks the camera in an existing map: pass --map <map.txt>")
    smooth = getattr(cmdline_args, "smooth", False)
    smooth_cov = getattr(cmdline_args, "smooth_cov", None)
    if smooth_cov and not smooth:
        raise ValueError("--smooth-cov writes the covariances of the smoothed trajectory: pass --smooth")
    if smooth:
        if not (getattr(cmdline_args, "resident", False) and cmdline_args.detections):
            raise ValueError("--smooth runs a backward pass over a recorded replay: pass --detections <replay.npz> --resident")
        if getattr(cmdline_args, "localize", False):
            raise ValueError("--smooth does not go with --localize: a frozen map is not smoothed")
        if cmdline_args.filter != "ekf":
            raise ValueError("--smooth is implemented for --filter ekf")
        kwargs.setdefault("quat_update", "scalar_first")      # (the as-written injection has no inverse)
    if getattr(cmdline_args, "gate", None) is not None:
        kwargs["gate"] = cmdline_args.gate      # (acts in the frame loop and in the resident replay alike)
    if getattr(cmdline_args, "confirm", None) is not None:
        if getattr(cmdline_args, "resident", False):
            raise ValueError("--confirm prunes between frames: it does not go with --resident (one device call for the log)")
        kwargs["confirm"] = cmdline_args.confirm      # (with or without --gate)
    noise = detection_noise(cmdline_args.detections) if cmdline_args.detections else None
    if noise is not None:
        kwargs["row_noise"] = True      # (the file carries per-detection noise: frame loop and resident replay use it)
    scales = None
    if getattr(cmdline_args, "frame_period", None) is not None:
        if not cmdline_args.detections:
            raise ValueError("--frame-period reads the timestamps of a detections file: pass --detections <replay.npz>")
        scales = frame_scales(cmdline_args.detections, cmdline_args.frame_period)
        kwargs["frame_scale"] = True
    motion = detection_motion(cmdline_args.detections) if cmdline_args.detections else None
    if motion is not None:
        kwargs["motion"] = True      # (the file carries odometry: frame loop and resident replay move the camera first)
    tracker = init_tracker(cmdline_args.filter, initial_pose, **kwargs)
    if map_file is not None:
        tracker.load_map(map_file)
    if getattr(cmdline_args, "localize", False):
        tracker.freeze_map()
    out_dir = Path(getattr(cmdline_args, "output_dir", "outputs"))
    out_dir.mkdir(parents=True, exist_ok=True)

    resident = getattr(cmdline_args, "resident", False)
    if resident and not cmdline_args.detections:
        raise ValueError("--resident replays a detections file: pass --detections <replay.npz>")
    with TrajectoryWriter(str(out_dir / "trajectory.txt")) as cam_traj_writer:
        if resident:
            replay_resident(tracker, cmdline_args.detections, cam_traj_writer, scales, motion, smooth, smooth_cov)
        elif cmdline_args.detections:
            offs = np.load(cmdline_args.detections, allow_pickle=False)["offsets"]
            for f, (timestamp, ids, poses) in enumerate(detection_frames(cmdline_args.detections)):
                extra = {} if scales is None else {"scale": scales[f]}
                if noise is not None and ids is not None:
                    extra["noise"] = noise[int(offs[f]):int(offs[f + 1])]
                if motion is not None:
                    extra["motion"] = motion[f]
                _, camera_pose, _, _ = tracker.process_detections(ids, poses, **extra)
                cam_traj_writer.write(timestamp, camera_pose)
        else:
            if cv2 is None:
                raise RuntimeError("OpenCV (cv2) is not installed: pass --detections <replay.npz> "
                                   "instead of --video")
            cap = cv2.VideoCapture(cmdline_args.video)
            cap.set(cv2.CAP_PROP_BUFFERSIZE, 0)
            for _ in range(int(cap.get(cv2.CAP_PROP_FRAME_COUNT))):
                ret, frame = cap.read()
                if not ret:
                    break
                frame = cv2.resize(frame, IMAGE_SIZE)
                frame, camera_pose, _, _ = tracker.process_frame(frame)
                cam_traj_writer.write(cap.get(cv2.CAP_PROP_POS_MSEC), camera_pose)
            cap.release()
    tracker.save_map(str(out_dir / "map.txt"))


def confirm_pair(text: str):
    """``H,W`` of ``--confirm`` as a pair of integers."""
    try:
        hits, window = (int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--confirm takes H,W (two integers), got {text!r}") from None
    return hits, window


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Run the SLAM system")
    parser.add_argument("--video", type=str, help="Path to video file", default="input_video.mp4")
    parser.add_argument("--filter", type=str, help="Filter to use (ekf)", default="ekf")
    parser.add_argument("--detections", type=str, default=None,
                        help="replay file with pre-computed ArUco detections (.npz)")
    parser.add_argument("--output-dir", dest="output_dir", type=str, default="outputs")
    parser.add_argument("--resident", action="store_true",
                        help="with --detections: replay the whole file on the device in one call")
    parser.add_argument("--gate", type=float, default=None,
                        help="chi-square gate on every detection's own squared Mahalanobis distance: detections beyond "
                             "it are left out of their frame (ekf: 3 degrees of freedom, 11.345 = 99 %%; ekf_rotations: 7, "
                             "18.475)")
    parser.add_argument("--frame-period", dest="frame_period", type=float, default=None, metavar="MS",
                        help="with --detections: scale every frame's process noise by the time since the previous frame "
                             "in units of MS milliseconds (33.3 for a 30 fps video), from the file's timestamps_ms; frames "
                             "without an update leave their time pending for the next one (default: off)")
    parser.add_argument("--confirm", type=confirm_pair, default=None, metavar="H,W",
                        help="a new landmark must be used again in H later frames within W frames of its first sighting, "
                             "or it is removed from the map again (default: off)")
    parser.add_argument("--map", type=str, default=None, metavar="FILE",
                        help="start from a map written earlier (map.txt) instead of an empty one")
    parser.add_argument("--localize", action="store_true",
                        help="with --map: freeze the map and only track the camera in it; markers that are not in the map "
                             "are ignored and the map is written back unchanged")
    parser.add_argument("--smooth", action="store_true",
                        help="with --detections --resident: write the smoothed trajectory (a Rauch-Tung-Striebel backward "
                             "pass over the recorded replay: every pose uses the whole log; the filter runs with the "
                             "scalar-first quaternion update)")
    parser.add_argument("--smooth-cov", dest="smooth_cov", type=str, default=None, metavar="OUT.npz",
                        help="with --smooth: also form the smoothed covariances and write the camera blocks of every frame, "
                             "smoothed_cov and filtered_cov [F, 10, 10], to OUT.npz (NaN before the first update)")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
