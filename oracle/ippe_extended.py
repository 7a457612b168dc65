"""The detection -> pose step in extended precision  --  TEST INFRASTRUCTURE ONLY.

A sharper yardstick than ``ippe_numpy`` for ``ekf_ippe_square_kernel`` (csrc/ekf_pose_ippe.hip, ekf_ippe_device.h): the
kernel's published steps in ``np.longdouble`` (x87 80-bit, 64-bit significand on x86-64):

    1. pixel corners -> normalised image points: 5 fixed-point iterations of the 8-coefficient Brown-Conrady model (the
       kernel's own count: with distortion the reference is the 5-iteration algorithm, not the projected truth);
    2. the exact 4-point homography, by a linear solve (the kernel has a closed form);
    3. J, R_v (through the cross-product matrix; the kernel writes the entries out), A = B^-1 J, gamma (the 2 x 2 largest
       singular value from the two rotation-like parts of A; the kernel takes the eigenvalue of A^T A), both candidates;
    4. the translation of either by least squares (Householder QR; the kernel solves the normal equations);
    5. the reprojection error in the normalised plane, and the rotation vector through the unit quaternion
       (largest-of-four branch, 2 atan2(|v|, w)).

Rounding error ~2^-64 per operation, 2^-11 of an f64 computation's: the reference counts as exact in the bounds of
``tests/pose_sweep_util.py``.  Besides the candidates it returns what those bounds are conditioned on: ``b_min`` (the
smaller third-row entry of R~'s first two columns, the one square root of a cancelling quantity in the algorithm) and
``ell`` (the shortest side of the undistorted quadrilateral, normalised image units).
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:      # (no silent fall-back to a double-precision "reference")
    raise ImportError(f"oracle.ippe_extended needs an extended long double (64-bit significand); this platform has "
                      f"{np.finfo(LD).nmant + 1} bits")

U64 = 2.0 ** -53
TIE_REL = 1e3 * U64      # the reference's two reprojection errors tie: |e0 - e1| <= TIE_REL (e0 + e1) ...
TIE_ABS = 1e-25          # ... or both below TIE_ABS


def _ld(a):
    return np.asarray(a, dtype=LD)


def solve_ld(a, b):
    """a x = b by Gaussian elimination with partial pivoting, longdouble."""
    a, b = _ld(a).copy(), _ld(b).copy()
    n = a.shape[0]
    for c in range(n):
        piv = c + int(np.argmax(np.abs(a[c:, c])))
        if piv != c:
            a[[c, piv]] = a[[piv, c]]
            b[[c, piv]] = b[[piv, c]]
        for r in range(c + 1, n):
            m = a[r, c] / a[c, c]
            a[r, c:] -= m * a[c, c:]
            b[r] -= m * b[c]
    x = np.zeros(n, dtype=LD)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - a[r, r + 1:] @ x[r + 1:]) / a[r, r]
    return x


def lstsq_ld(a, b):
    """argmin |a x - b| by Householder QR, longdouble (a: [m, n], full column rank)."""
    a, b = _ld(a).copy(), _ld(b).copy()
    m, n = a.shape
    for c in range(n):
        v = a[c:, c].copy()
        alpha = -np.copysign(np.sqrt(v @ v), v[0])
        v[0] -= alpha
        vv = v @ v
        if vv == 0:
            continue
        a[c:, c:] -= np.outer(v, (2 / vv) * (v @ a[c:, c:]))
        b[c:] -= v * ((2 / vv) * (v @ b[c:]))
    x = np.zeros(n, dtype=LD)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - a[r, r + 1:n] @ x[r + 1:]) / a[r, r]
    return x


def dist8(dist):
    d = np.zeros(8, dtype=LD)
    v = _ld([] if dist is None else dist).reshape(-1)
    d[: v.size] = v
    return d


def undistort_ld(pixels, camera_matrix, dist=None, iterations=5):
    """pixels [n,2] -> normalised image points [n,2]: the kernel's fixed-point iteration, longdouble."""
    k = dist8(dist)
    cm = _ld(camera_matrix).reshape(3, 3)
    fx, fy, cx, cy = cm[0, 0], cm[1, 1], cm[0, 2], cm[1, 2]
    px = _ld(pixels)
    x0 = (px[:, 0] - cx) / fx
    y0 = (px[:, 1] - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        icd = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
        x = (x0 - dx) * icd
        y = (y0 - dy) * icd
    return np.stack([x, y], axis=1)


def project_ld(points_cam, camera_matrix, dist=None):
    """Forward camera model in longdouble, rounded to f64 pixels (what a detector hands over): [n,3] -> [n,2]."""
    k = dist8(dist)
    cm = _ld(camera_matrix).reshape(3, 3)
    p = _ld(points_cam)
    x, y = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    r2 = x * x + y * y
    cd = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = x * cd + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * cd + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
    return np.stack([cm[0, 0] * xd + cm[0, 2], cm[1, 1] * yd + cm[1, 2]], axis=1).astype(np.float64)


def quat_branch(rot):
    """Which of (trace, R00, R11, R22) is the largest: 0 .. 3, the first on ties (the kernel's rule restated)."""
    r = np.asarray(rot)
    tr = r[0, 0] + r[1, 1] + r[2, 2]
    if tr >= r[0, 0] and tr >= r[1, 1] and tr >= r[2, 2]:
        return 0
    if r[0, 0] >= r[1, 1] and r[0, 0] >= r[2, 2]:
        return 1
    return 2 if r[1, 1] >= r[2, 2] else 3


def quat_from_matrix_ld(rot):
    """Unit quaternion (w, x, y, z), w >= 0, of a rotation matrix: largest-of-four branch."""
    r = _ld(rot)
    br = quat_branch(r)
    if br == 0:
        q = [1 + r[0, 0] + r[1, 1] + r[2, 2], r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]]
    elif br == 1:
        q = [r[2, 1] - r[1, 2], 1 + r[0, 0] - r[1, 1] - r[2, 2], r[0, 1] + r[1, 0], r[0, 2] + r[2, 0]]
    elif br == 2:
        q = [r[0, 2] - r[2, 0], r[0, 1] + r[1, 0], 1 - r[0, 0] + r[1, 1] - r[2, 2], r[1, 2] + r[2, 1]]
    else:
        q = [r[1, 0] - r[0, 1], r[0, 2] + r[2, 0], r[1, 2] + r[2, 1], 1 - r[0, 0] - r[1, 1] + r[2, 2]]
    q = _ld(q)
    q = q / np.sqrt(q @ q)
    return -q if q[0] < 0 else q


def rotvec_from_matrix_ld(rot):
    q = quat_from_matrix_ld(rot)
    v = np.sqrt(q[1:] @ q[1:])
    if v == 0:
        return np.zeros(3, dtype=LD)
    return q[1:] * (2 * np.arctan2(v, q[0]) / v)


def matrix_from_rotvec_ld(rvec):
    """Rodrigues' formula in longdouble (the half-angle form: no cancellation in 1 - cos)."""
    r = _ld(rvec)
    th = np.sqrt(r @ r)
    k = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], dtype=LD)
    if th < LD(1e-12):
        return np.eye(3, dtype=LD) + k + LD(0.5) * (k @ k)
    s = np.sin(th / 2)
    return np.eye(3, dtype=LD) + (np.sin(th) / th) * k + (2 * s * s / (th * th)) * (k @ k)


def object_points_ld(marker_size):
    h = LD(marker_size) / 2
    return np.array([[-h, h, 0], [h, h, 0], [h, -h, 0], [-h, -h, 0]], dtype=LD)


def _translation_ld(rot, obj, img):
    pr = obj @ rot.T
    a, b = [], []
    for (X, Y, Z), (x, y) in zip(pr, img):
        a.append([1, 0, -x]); b.append(x * Z - X)
        a.append([0, 1, -y]); b.append(y * Z - Y)
    t = lstsq_ld(np.array(a, dtype=LD), np.array(b, dtype=LD))
    pc = pr + t
    d = pc[:, :2] / pc[:, 2:3] - img
    return t, np.sum(d * d)


def ippe_square_ld(corners_px, marker_size, camera_matrix, dist=None):
    """One marker.  Returns a dict: ``cands``: both candidates [(t, R, rvec, err), ...] in longdouble, best first;
    ``Rv``; ``b_min``; ``ell``; ``tie``: the two reprojection errors tie (``TIE_REL`` / ``TIE_ABS``)."""
    obj = object_points_ld(marker_size)
    img = undistort_ld(np.asarray(corners_px, dtype=np.float64).reshape(4, 2), camera_matrix, dist)
    a, b = [], []
    for (X, Y, _), (x, y) in zip(obj, img):
        a.append([X, Y, 1, 0, 0, 0, -x * X, -x * Y]); b.append(x)
        a.append([0, 0, 0, X, Y, 1, -y * X, -y * Y]); b.append(y)
    hm = np.append(solve_ld(np.array(a, dtype=LD), np.array(b, dtype=LD)), LD(1)).reshape(3, 3)
    p, q = hm[0, 2], hm[1, 2]
    jac = np.array([[hm[0, 0] - hm[2, 0] * p, hm[0, 1] - hm[2, 1] * p],
                    [hm[1, 0] - hm[2, 0] * q, hm[1, 1] - hm[2, 1] * q]], dtype=LD)
    d = np.array([p, q, 1], dtype=LD) / np.sqrt(p * p + q * q + 1)
    w = np.array([-d[1], d[0], 0], dtype=LD)                      # e_z x d
    wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=LD)
    rv = np.eye(3, dtype=LD) + wx + wx @ wx / (1 + d[2])
    bm = (np.array([[1, 0, -p], [0, 1, -q]], dtype=LD) @ rv)[:, :2]
    am = np.stack([solve_ld(bm, jac[:, 0]), solve_ld(bm, jac[:, 1])], axis=1)
    # largest singular value of a 2 x 2 matrix: half the sum of the moduli of its two "complex parts"
    e, f_, g, h = (am[0, 0] + am[1, 1]) / 2, (am[0, 0] - am[1, 1]) / 2, (am[1, 0] + am[0, 1]) / 2, (am[1, 0] - am[0, 1]) / 2
    gamma = np.sqrt(e * e + h * h) + np.sqrt(f_ * f_ + g * g)
    r22 = am / gamma
    b0 = np.sqrt(max(1 - r22[:, 0] @ r22[:, 0], LD(0)))
    b1 = np.sqrt(max(1 - r22[:, 1] @ r22[:, 1], LD(0)))
    if r22[:, 0] @ r22[:, 1] > 0:
        b1 = -b1
    cands = []
    for sgn in (1, -1):
        c0 = np.array([r22[0, 0], r22[1, 0], sgn * b0], dtype=LD)
        c1 = np.array([r22[0, 1], r22[1, 1], sgn * b1], dtype=LD)
        rot = rv @ np.stack([c0, c1, np.cross(c0, c1)], axis=1)
        t, err = _translation_ld(rot, obj, img)
        cands.append((t, rot, rotvec_from_matrix_ld(rot), err))
    if cands[1][3] < cands[0][3]:
        cands.reverse()
    e0, e1 = cands[0][3], cands[1][3]
    tie = bool(abs(e0 - e1) <= LD(TIE_REL) * (e0 + e1) or (e0 < TIE_ABS and e1 < TIE_ABS))
    sides = img - np.roll(img, -1, axis=0)
    ell = float(np.sqrt(np.sum(sides * sides, axis=1)).min())
    return {"cands": cands, "Rv": rv, "b_min": float(min(abs(b0), abs(b1))), "ell": ell, "tie": tie}
