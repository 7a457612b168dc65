"""NumPy mirror of the replica noise of ``EKFBatch.replay_replicas`` (``ekf_batch_replica_poses``, definition in
include/ekf_slam_hip.h): Philox4x32-10 with key (seed_lo, seed_hi) and counter (d_lo, d_hi, r, j), j = 0, 1, 2, and
Box-Muller on u = (((x0 << 32 | x1) >> 11) + 0.5) 2^-53 of each pair of words."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 of counter words (c0, c1, c2, c3) under key (k0, k1); every word an integer or an array (broadcast).
    Returns the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]          # (< 2^64: exact in uint64)
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def unit_open(hi, lo):
    """(0, 1] in the f64 operations of the device: (v + 0.5) 2^-53 with v the top 53 bits of (hi << 32 | lo)"""
    return ((((hi << S32) | lo) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, replicas, detections):
    """g [R, D, 6] for replica numbers ``replicas`` [R] and detection numbers ``detections`` [D]."""
    r = np.asarray(replicas, dtype=np.uint64).reshape(-1, 1)
    d = np.asarray(detections, dtype=np.uint64).reshape(1, -1)
    seed = int(seed)
    out = np.empty((r.shape[0], d.shape[1], 6))
    for j in range(3):
        x = philox4x32_10((d & MASK, d >> S32, r, np.uint64(j)), (seed & 0xFFFFFFFF, seed >> 32))
        ua, ub = unit_open(x[0], x[1]), unit_open(x[2], x[3])
        rad, ang = np.sqrt(-2.0 * np.log(ua)), 2.0 * np.pi * ub
        out[:, :, 2 * j] = rad * np.cos(ang)
        out[:, :, 2 * j + 1] = rad * np.sin(ang)
    return out


def replica_poses(poses, sigma, seed, replicas, first_replica=0):
    """The poses [R, D, 6] replicas first_replica .. + R - 1 consume: pose + sigma * g, sigma [R, 6] (or broadcastable)."""
    poses = np.asarray(poses, dtype=np.float64)
    g = normals(seed, np.arange(first_replica, first_replica + replicas), np.arange(poses.shape[0]))
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (replicas, 6))
    return poses[None] + sigma[:, None, :] * g
