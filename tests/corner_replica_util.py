"""NumPy mirror of the corner replicas of ``EKFBatch.replay_corner_replicas`` (``ekf_batch_replica_corners``, definition in
include/ekf_slam_hip.h): Philox4x32-10 with key (seed_lo, seed_hi) and counter (d_lo, d_hi, r, 4 + i), i = 0 .. 3, Box-Muller
as for the pose noise (``replica_util``), noisy corner = corner + sigma_px (g_u, g_v), the pose by the oracle's IPPE
(``oracle.ippe_numpy.ippe_square``) and flipped = trace(R_a R_clean^T) < trace(R_b R_clean^T)."""
import numpy as np
from scipy.spatial.transform import Rotation

import replica_util as ru
from oracle.ippe_numpy import ippe_square


def corner_normals(seed, replicas, detections):
    """g [R, D, 4, 2] = (g_u, g_v) of every corner for replica numbers ``replicas`` [R] and detection numbers
    ``detections`` [D]."""
    r = np.asarray(replicas, dtype=np.uint64).reshape(-1, 1)
    d = np.asarray(detections, dtype=np.uint64).reshape(1, -1)
    seed = int(seed)
    out = np.empty((r.shape[0], d.shape[1], 4, 2))
    for i in range(4):
        x = ru.philox4x32_10((d & ru.MASK, d >> ru.S32, r, np.uint64(4 + i)), (seed & 0xFFFFFFFF, seed >> 32))
        ua, ub = ru.unit_open(x[0], x[1]), ru.unit_open(x[2], x[3])
        rad, ang = np.sqrt(-2.0 * np.log(ua)), 2.0 * np.pi * ub
        out[:, :, i, 0] = rad * np.cos(ang)
        out[:, :, i, 1] = rad * np.sin(ang)
    return out


def replica_corners(corners, sigma_px, seed, replicas, first_replica=0):
    """The noisy corners [R, D, 4, 2] of replicas first_replica .. + R - 1; sigma_px a scalar or [R]."""
    corners = np.asarray(corners, dtype=np.float64)
    g = corner_normals(seed, np.arange(first_replica, first_replica + replicas), np.arange(corners.shape[0]))
    sigma = np.broadcast_to(np.asarray(sigma_px, dtype=np.float64), (replicas,))
    return corners[None] + sigma[:, None, None, None] * g


def _rot(rvec):
    return Rotation.from_rotvec(rvec).as_matrix()


def replica_corner_poses(corners, sigma_px, seed, replicas, camera_matrix, dist=None, marker_size=0.16, first_replica=0):
    """(poses [R, D, 6], candidates): ``candidates`` holds both IPPE solutions of every pair and what decides a flip:
    ``tvec`` / ``rvec`` / ``err`` [R, D, 2, ...] (returned candidate first), ``rvec_clean`` [D, 3], ``trace`` [R, D, 2] =
    trace(R_a R_clean^T), trace(R_b R_clean^T), and ``flipped`` [R, D] = trace[..., 0] < trace[..., 1]."""
    corners = np.asarray(corners, dtype=np.float64)
    noisy = replica_corners(corners, sigma_px, seed, replicas, first_replica)
    R, D = noisy.shape[:2]
    clean = np.stack([ippe_square(c, marker_size, camera_matrix, dist)[1] for c in corners]) if D else np.zeros((0, 3))
    rc = [_rot(v) for v in clean]
    poses = np.empty((R, D, 6))
    cand = {"tvec": np.empty((R, D, 2, 3)), "rvec": np.empty((R, D, 2, 3)), "err": np.empty((R, D, 2)),
            "trace": np.empty((R, D, 2)), "rvec_clean": clean}
    for r in range(R):
        for d in range(D):
            t, rv, sols = ippe_square(noisy[r, d], marker_size, camera_matrix, dist)
            poses[r, d, :3], poses[r, d, 3:] = t, rv
            for s, (ts, rs, es) in enumerate(sols):
                cand["tvec"][r, d, s], cand["rvec"][r, d, s], cand["err"][r, d, s] = ts, rs, es
                cand["trace"][r, d, s] = np.trace(_rot(rs) @ rc[d].T)
    cand["flipped"] = cand["trace"][..., 0] < cand["trace"][..., 1]
    return poses, cand
