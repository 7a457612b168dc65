"""Deterministic synthetic ArUco detections (no video / cv2 in this image).

Produces exactly what the vision front-end hands to the filter boundary
(reference ``BaseFilter.process_frame`` -> ``self.observe(ids, poses)``,
filters/base_filter.py:194-204): per frame a list of marker ids and an
``(m, 6)`` float64 array ``[tvec | rvec]`` in the camera frame.  Only
``pose[0:3]`` is used by the EKF (extended_kalman_filter.py:192,196,272).

Stream definition: landmarks ``U([-10,10]^2 x [5,25])``,
camera ``c(t) = (0.5 sin t, 0.2 sin 2t, 0.05 t)``,
``R(t) = Rz(0.05 t) Ry(0.15 sin 0.7t) Rx(0.1 sin t)``, ``t = frame / 30``;
bootstrap frames show ids ``j*m .. j*m+m-1``; steady-state frames show a sorted
random subset of m ids with ``z = R(t)^T (l - c(t)) + N(0, 0.01^2)``.
"""
from __future__ import annotations

import numpy as np


def camera_truth(frame: int):
    t = frame / 30.0
    c = np.array([0.5 * np.sin(t), 0.2 * np.sin(2.0 * t), 0.05 * t])
    ax, ay, az = 0.1 * np.sin(t), 0.15 * np.sin(0.7 * t), 0.05 * t
    cx, sx = np.cos(ax), np.sin(ax)
    cy, sy = np.cos(ay), np.sin(ay)
    cz, sz = np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return c, rz @ ry @ rx


class SyntheticStream:
    """n landmarks, m visible per frame, seeded."""

    def __init__(self, n: int, m: int, seed: int = 0, noise: float = 0.01, rvec_sigma: float = 0.0):
        if m > n:
            raise ValueError("m must be <= n")
        self.n, self.m, self.noise = n, m, noise
        self.rng = np.random.default_rng(seed)
        lm = np.empty((n, 3))
        lm[:, 0:2] = self.rng.uniform(-10.0, 10.0, size=(n, 2))
        lm[:, 2] = self.rng.uniform(5.0, 25.0, size=n)
        self.landmarks = lm
        self.rvec_sigma = rvec_sigma     # > 0: poses[:, 3:6] carry noisy marker orientations (EKF_Rotations)
        self.frame = 0

    @property
    def bootstrap_frames(self) -> int:
        return -(-self.n // self.m)

    def _observe(self, ids):
        c, rot = camera_truth(self.frame)
        z = (self.landmarks[ids] - c) @ rot          # rows = R^T (l - c)
        z = z + self.rng.normal(0.0, self.noise, size=z.shape)
        poses = np.zeros((len(ids), 6))
        poses[:, 0:3] = z
        if self.rvec_sigma > 0.0:
            poses[:, 3:6] = self.rng.normal(0.0, self.rvec_sigma, size=(len(ids), 3))
        self.frame += 1
        return np.asarray(ids, dtype=np.int32), poses

    def bootstrap(self):
        """Frames that introduce every landmark through ``observe()`` only."""
        for j in range(self.bootstrap_frames):
            lo = j * self.m
            ids = np.arange(lo, min(lo + self.m, self.n))
            yield self._observe(ids)

    def steady(self, frames: int):
        for _ in range(frames):
            ids = np.sort(self.rng.choice(self.n, self.m, replace=False))
            yield self._observe(ids)


def small_sequence(frames: int = 200, markers: int = 10, max_visible: int = 6,
                   seed: int = 0):
    """C1-sized replay: <=10 markers, 1..max_visible seen per frame, markers
    appear progressively, some frames empty, occasional duplicate ids
    (legal at the boundary: SURVEY 8(a) a2).  Returns a list of
    ``(timestamp_ms, ids, poses)``; ids is ``None`` for frames without
    detections (base_filter.py:197)."""
    rng = np.random.default_rng(seed)
    lm = np.empty((markers, 3))
    lm[:, 0:2] = rng.uniform(-2.0, 2.0, size=(markers, 2))
    lm[:, 2] = rng.uniform(3.0, 8.0, size=markers)
    marker_ids = rng.permutation(50)[:markers]       # DICT_5X5_50 id range
    out = []
    for f in range(frames):
        ts = (f + 1) * 1000.0 / 30.0
        if f in (0, 57, 58, 140):                     # frames with no detections
            out.append((ts, None, np.array([])))
            continue
        known = min(markers, 2 + f // 12)
        m = int(rng.integers(1, min(max_visible, known) + 1))
        pick = np.sort(rng.choice(known, m, replace=False))
        if f % 41 == 7 and m >= 2:                    # duplicate detection
            pick[-1] = pick[0]
        c, rot = camera_truth(f)
        z = (lm[pick] - c) @ rot + rng.normal(0.0, 0.01, size=(m, 3))
        poses = np.zeros((m, 6))
        poses[:, 0:3] = z
        poses[:, 3:6] = rng.normal(0.0, 0.05, size=(m, 3))
        out.append((ts, marker_ids[pick].astype(np.int32), poses))
    return out


def ragged_log(n: int, m_range, steady_frames: int, seed: int = 0, bootstrap_m: int | None = None, noise: float = 0.01,
               rvec_sigma: float = 0.0) -> dict:
    """A seeded ragged detection log in the layout of a replay file (``main/run_slam.py: detection_frames``): a bootstrap
    segment that first-sights all ``n`` landmarks, ``bootstrap_m`` per frame (default: the top of ``m_range``), then
    ``steady_frames`` frames that each see ``m ~ U[m_range]`` distinct landmarks.  Returns ids [D], poses [D,6],
    offsets [F+1], has_detections [F] and the number of bootstrap frames."""
    lo, hi = int(m_range[0]), int(m_range[1])
    stream = SyntheticStream(n, min(n, bootstrap_m or hi), seed=seed, noise=noise, rvec_sigma=rvec_sigma)
    frames = list(stream.bootstrap())
    boot = len(frames)
    for _ in range(steady_frames):
        m = int(stream.rng.integers(lo, hi + 1))
        frames.append(stream._observe(np.sort(stream.rng.choice(n, m, replace=False))))
    counts = np.array([len(ids) for ids, _ in frames], dtype=np.int64)
    return {"ids": np.concatenate([ids for ids, _ in frames]).astype(np.int32),
            "poses": np.concatenate([p for _, p in frames]),
            "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64),
            "has_detections": counts > 0, "bootstrap_frames": boot}


def _rodrigues(rvec: np.ndarray) -> np.ndarray:
    """Rotation matrix of an axis * angle vector."""
    theta = float(np.linalg.norm(rvec))
    if theta < 1e-12:
        return np.eye(3)
    a = rvec / theta
    ax = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(theta) * ax + (1.0 - np.cos(theta)) * (ax @ ax)


def _rotvec(rot: np.ndarray) -> np.ndarray:
    """Axis * angle (angle in [0, pi]) of a rotation matrix, through the unit quaternion: well conditioned near pi, where
    the markers that face the camera are."""
    q = np.empty(4)                       # (w, x, y, z), from the largest of the four candidates
    tr = np.trace(rot)
    cand = np.array([tr, rot[0, 0], rot[1, 1], rot[2, 2]])
    i = int(np.argmax(cand))
    if i == 0:
        q[:] = (1.0 + tr, rot[2, 1] - rot[1, 2], rot[0, 2] - rot[2, 0], rot[1, 0] - rot[0, 1])
    else:
        j, k = i % 3, (i + 1) % 3         # axes after i - 1 (cyclic)
        a = i - 1
        q[0] = rot[k, j] - rot[j, k]
        q[1 + a] = 1.0 + 2.0 * rot[a, a] - tr
        q[1 + j] = rot[j, a] + rot[a, j]
        q[1 + k] = rot[k, a] + rot[a, k]
    q /= np.linalg.norm(q)
    if q[0] < 0.0:
        q = -q
    s = float(np.linalg.norm(q[1:]))
    if s < 1e-12:
        return np.zeros(3)
    return q[1:] * (2.0 * np.arctan2(s, q[0]) / s)


def _project(points_cam: np.ndarray, camera_matrix, dist) -> np.ndarray:
    """Pinhole + Brown-Conrady (k1 k2 p1 p2 k3 k4 k5 k6, missing ones 0): camera-frame points [n,3] -> pixels [n,2]."""
    k = np.zeros(8)
    d = np.asarray([] if dist is None else dist, dtype=np.float64).reshape(-1)
    k[:d.size] = d
    cm = np.asarray(camera_matrix, dtype=np.float64)
    x, y = points_cam[:, 0] / points_cam[:, 2], points_cam[:, 1] / points_cam[:, 2]
    r2 = x * x + y * y
    cd = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = x * cd + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * cd + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    return np.stack([cm[0, 0] * xd + cm[0, 2], cm[1, 1] * yd + cm[1, 2]], axis=1)


def corner_camera(frame: int):
    """The gently moving camera of ``corner_log``: position and rotation (camera axes in the world) at ``frame``."""
    t = frame / 30.0
    c = np.array([0.06 * np.sin(t), 0.04 * np.sin(2.0 * t), 0.05 * np.sin(0.5 * t)])
    return c, _rodrigues(np.array([0.02 * np.sin(t), 0.03 * np.sin(0.7 * t), 0.02 * np.sin(1.3 * t)]))


def corner_log(n: int, m_range, steady_frames: int, seed: int, camera_matrix, dist, marker_size: float = 0.16,
               width: int = 1920, height: int = 1080) -> dict:
    """A seeded ragged log of marker CORNERS, what the detector hands to the pose front end: a static scene of ``n``
    oriented square markers at 1.5 to 4 m depth in front of the gently moving ``corner_camera`` (a different camera for
    each frame), facing it with tilts from 0 to about 65 degrees about random in-plane axes.  (``ragged_log``'s scene
    lies mostly outside any field of view and has no orientations.)  A marker is placed only where all four corners stay
    inside the ``width`` x ``height`` image in every frame of the log, so every listed detection is a full view.  As in
    ``ragged_log``, a bootstrap segment first-sights all ``n`` markers, the top of ``m_range`` per frame, then
    ``steady_frames`` frames each see ``m ~ U[m_range]`` distinct markers.  Returns ids [D], offsets [F+1],
    has_detections [F], bootstrap_frames, corners [D,4,2] in pixels (the detector's order: object points (-s/2, s/2),
    (s/2, s/2), (s/2, -s/2), (-s/2, -s/2)) and poses_clean [D,6], the ``[tvec | rvec]`` the corners were projected from."""
    lo, hi = int(m_range[0]), int(m_range[1])
    rng = np.random.default_rng(seed)
    cm = np.asarray(camera_matrix, dtype=np.float64)
    h = marker_size / 2.0
    obj = np.array([[-h, h, 0.0], [h, h, 0.0], [h, -h, 0.0], [-h, -h, 0.0]])
    boot_m = min(n, hi)
    boot = -(-n // boot_m)
    total = boot + int(steady_frames)
    cams = [corner_camera(f) for f in range(total)]

    def views(pos, rot):
        """corners [total,4,2] and poses [total,6] of one marker in every frame; None if a corner leaves the image"""
        px, poses = np.empty((total, 4, 2)), np.empty((total, 6))
        for f, (c, rc) in enumerate(cams):
            r_cam, t_cam = rc.T @ rot, rc.T @ (pos - c)
            px[f] = _project(obj @ r_cam.T + t_cam, cm, dist)
            poses[f, :3], poses[f, 3:] = t_cam, _rotvec(r_cam)
        if px[..., 0].min() < 0 or px[..., 0].max() > width or px[..., 1].min() < 0 or px[..., 1].max() > height:
            return None
        return px, poses

    flip = np.diag([1.0, -1.0, -1.0])           # Rx(pi): the marker faces the camera
    markers = []
    while len(markers) < n:
        z = rng.uniform(1.5, 4.0)
        u, v = rng.uniform(0.0, width), rng.uniform(0.0, height)
        pos = np.array([(u - cm[0, 2]) / cm[0, 0] * z, (v - cm[1, 2]) / cm[1, 1] * z, z])
        axis_angle, tilt = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(0.0, np.deg2rad(65.0))
        rot = _rodrigues(tilt * np.array([np.cos(axis_angle), np.sin(axis_angle), 0.0])) @ flip
        seen = views(pos, rot)
        if seen is not None:
            markers.append(seen)
    frames = [np.arange(j * boot_m, min((j + 1) * boot_m, n)) for j in range(boot)]
    for _ in range(int(steady_frames)):
        m = int(rng.integers(lo, hi + 1))
        frames.append(np.sort(rng.choice(n, m, replace=False)))
    counts = np.array([len(ids) for ids in frames], dtype=np.int64)
    corners = [markers[j][0][f] for f, ids in enumerate(frames) for j in ids]
    poses = [markers[j][1][f] for f, ids in enumerate(frames) for j in ids]
    return {"ids": np.concatenate(frames).astype(np.int32),
            "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64),
            "has_detections": counts > 0, "bootstrap_frames": boot,
            "corners": np.array(corners, dtype=np.float64).reshape(-1, 4, 2),
            "poses_clean": np.array(poses, dtype=np.float64).reshape(-1, 6)}
