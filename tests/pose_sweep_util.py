"""Helpers of the pose front end's sweep (``test_pose_sweep.py`` on the GPU, ``test_pose_sweep_cpu.py`` here): the case
table, the cameras, the extended-precision reference of every case (``oracle/ippe_extended.py``) and the conditioned bound.

Case table.  Views are R = Rodrigues(tilt (cos phi, sin phi, 0)) Rx(pi) Rz(roll) at position t: a marker that faces the
camera, tilted about an axis in the image plane and rolled in its own plane.  The structured part crosses (sparsely: every
value of every factor with an on-axis and an off-axis t)

    tilt   0, 1e-9, 1e-6, 1e-4, 1e-2, 0.3, 1.0, 1.4
    phi    0, pi/2, pi, -pi/2, 1.1 and pi/2 + {+-1e-6, +-8e-6, +-3e-5, +-1e-4}: a tilt about the camera's y axis is a rotation
           by exactly pi whatever the tilt, and the offsets straddle the |sin| < 1e-5 window cv::Rodrigues has there
    roll   0, pi/2, pi, -pi/2, 0.7, 1e-6, pi - 1e-6
    t      (0,0,1), (0,0,0.3), (0,0,30) on the optical axis (p = q = 0; 110 px, 750 px and 5 px wide), four off it

then come back-facing views (the pinhole projects them, IPPE recovers them: the small-angle end, the trace branch and the
R22 branch of the matrix -> quaternion step) and 40 generic views of ``conftest.synthetic_marker_views``.

Bound.  With u = 2^-53, ell the shortest side of the undistorted quadrilateral (normalised image units) and b_min the smaller
third-row entry of the first two columns of R~ (both from the reference):

    |R(rvec) - R_ref|_F / sqrt 2        <= c_R u / (ell max(b_min, sqrt u))
    |t - t_ref|_inf / |t_ref|_2         <= c_t u / (ell max(b_min, sqrt u))

The outputs are smooth functions of normalised corner coordinates that carry a relative error u on a figure of size ell,
hence u / ell; the one square root of a cancelling quantity is b_i = sqrt(1 - |c_i|^2), d b = d(|c|^2) / 2 b, which
saturates at sqrt u because of the fmax(., 0).  R(.) is evaluated in longdouble.  The reference is the extended
restatement's best candidate (with distortion: of the same 5 iterations, so the algorithm and not the projected truth is
the yardstick); where its two reprojection errors tie (``ippe_extended.TIE_REL`` / ``TIE_ABS``: on-axis with the marker's
normal within 1e-9 of the optical axis only, where the candidates are one pose to sqrt(u / ell); the CPU test holds that
cap) the nearer of its candidates counts.

The constants are the worst ratio ``ekf_ippe_square_kernel`` reached on an MI355X (profiles/pose_sweep/summary.json) with a
head-room of at most 8, and stay within 8 x the worst ratio of the f64 NumPy oracle (the CPU test asserts both).
"""
from __future__ import annotations

import functools
import subprocess
from pathlib import Path

import numpy as np

from oracle import ippe_extended as xt

REPO = Path(__file__).resolve().parent.parent
SUMMARY = REPO / "profiles" / "pose_sweep" / "summary.json"
MARKER = 0.16
WIDTH, HEIGHT = 1920, 1080
U = 2.0 ** -53
LD = xt.LD
# (c_R, c_t): see the module docstring
C_BOUNDS = {"c_R": 5.3, "c_t": 52.0}
HEADROOM_MAX = 8.0

TILTS = (0.0, 1e-9, 1e-6, 1e-4, 1e-2, 0.3, 1.0, 1.4)
PHI_OFFSETS = (1e-6, -1e-6, 8e-6, -8e-6, 3e-5, -3e-5, 1e-4, -1e-4)
PHIS = (0.0, np.pi / 2, np.pi, -np.pi / 2, 1.1) + tuple(np.pi / 2 + d for d in PHI_OFFSETS)
ROLLS = (0.0, np.pi / 2, np.pi, -np.pi / 2, 0.7, 1e-6, np.pi - 1e-6)
T_ON = ((0.0, 0.0, 1.0), (0.0, 0.0, 0.3), (0.0, 0.0, 30.0))
T_OFF = ((0.4, -0.2, 1.0), (1.2, 0.6, 3.0), (2.0, 1.0, 8.0), (-0.5, 0.3, 0.6))
BACK_FACING = ((0.0, 0.0, 0.0), (0.0, 0.0, 1e-7), (0.2, -0.1, 0.4),
               (0.0, 0.0, 3.0), (0.05, -0.02, 3.1))        # (the last two: R22 is the largest of the four)
GENERIC = 40
TIE_TILT_MAX = 1e-9
RATIONAL8 = (0.06, -0.30, 0.0005, 0.003, 0.44, 0.02, -0.05, 0.1)


def cameras():
    """name -> (camera matrix, distortion coefficients or None)."""
    cal = np.load(REPO / "tests" / "golden" / "calibration.npz", allow_pickle=False)
    k, d5 = cal["camera_matrix"], cal["dist_coeffs"].reshape(-1)
    return {"none": (k, None), "calib5": (k, d5.copy()), "calib4": (k, d5[:4].copy()), "rational8": (k, np.array(RATIONAL8))}


def _rz(roll):
    c, s = np.cos(LD(roll)), np.sin(LD(roll))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=LD)


def facing_view(tilt, phi, roll):
    """R = Rodrigues(tilt (cos phi, sin phi, 0)) Rx(pi) Rz(roll), longdouble."""
    axis = np.array([np.cos(LD(phi)), np.sin(LD(phi)), 0], dtype=LD)
    return xt.matrix_from_rotvec_ld(LD(tilt) * axis) @ np.diag(np.array([1, -1, -1], dtype=LD)) @ _rz(roll)


@functools.lru_cache(maxsize=None)
def views():
    """The table: a list of dicts ``R`` (longdouble [3,3]), ``t`` (f64 [3]), ``kind`` ('grid' / 'back' / 'generic'),
    ``tilt``, ``phi``, ``roll`` (None where they do not apply), ``on_axis``, ``normal_tilt``."""
    out = []

    def grid(tilt, phi, roll, t, on_axis):
        out.append({"R": facing_view(tilt, phi, roll), "t": np.array(t, dtype=np.float64), "kind": "grid", "tilt": tilt,
                    "phi": phi, "roll": roll, "on_axis": on_axis})

    # tilt x phi in full at roll 0, each on the axis and off it
    for i, tilt in enumerate(TILTS):
        for j, phi in enumerate(PHIS):
            grid(tilt, phi, 0.0, T_ON[(i + j) % 3], True)
            grid(tilt, phi, 0.0, T_OFF[(i + j) % 4], False)
    # roll x tilt, about the camera's y axis (rotation angle pi), x axis and a general one in turn
    for i, roll in enumerate(ROLLS[1:]):
        for j, tilt in enumerate(TILTS):
            phi = (np.pi / 2, 1.1, 0.0)[(i + j) % 3]
            grid(tilt, phi, roll, T_ON[(i + 2 * j) % 3], True)
            grid(tilt, phi, roll, T_OFF[(i + 3 * j) % 4], False)
    # every position with every roll
    for i, t in enumerate(T_ON + T_OFF):
        for j, roll in enumerate(ROLLS):
            grid(0.3, (1.1, np.pi / 2)[(i + j) % 2], roll, t, i < len(T_ON))
    for rv in BACK_FACING:
        for t, on_axis in ((T_ON[0], True), (T_OFF[0], False)):
            out.append({"R": xt.matrix_from_rotvec_ld(np.array(rv, dtype=LD)), "t": np.array(t, dtype=np.float64),
                        "kind": "back", "tilt": None, "phi": None, "roll": None, "on_axis": on_axis})
    from conftest import synthetic_marker_views
    _k, _d, _c, tvecs, rots = synthetic_marker_views(GENERIC, seed=2)
    for t, rot in zip(tvecs, rots):
        out.append({"R": rot.as_matrix().astype(LD), "t": np.array(t, dtype=np.float64), "kind": "generic", "tilt": None,
                    "phi": None, "roll": None, "on_axis": False})
    for v in out:      # the angle between the marker's normal and the optical axis (the grid's tilt; back-facing views have one too)
        v["normal_tilt"] = float(np.arctan2(np.sqrt(v["R"][0, 2] ** 2 + v["R"][1, 2] ** 2), abs(v["R"][2, 2])))
    return out


@functools.lru_cache(maxsize=None)
def table(camera):
    """The cases of one camera: dict ``index`` (into ``views()``: distorted cameras keep a view only if all four corners fall
    inside the image), ``corners`` [n,4,2] f64 pixels and the reference per case: ``t`` [n,2,3] and ``R`` [n,2,3,3]
    (longdouble, both candidates, best first), ``tie`` [n], ``b_min`` [n], ``ell`` [n], ``scale`` [n] = u / (ell max(b_min,
    sqrt u))."""
    k, dist = cameras()[camera]
    obj = xt.object_points_ld(MARKER)
    index, corners, ts, rs, tie, b_min, ell = [], [], [], [], [], [], []
    for i, v in enumerate(views()):
        px = xt.project_ld(obj @ v["R"].T + v["t"].astype(LD), k, dist)
        if dist is not None and (px[:, 0].min() < 0 or px[:, 0].max() > WIDTH or px[:, 1].min() < 0 or px[:, 1].max() > HEIGHT):
            continue
        ref = xt.ippe_square_ld(px, MARKER, k, dist)
        index.append(i)
        corners.append(px)
        ts.append(np.stack([c[0] for c in ref["cands"]]))
        rs.append(np.stack([c[1] for c in ref["cands"]]))
        tie.append(ref["tie"]); b_min.append(ref["b_min"]); ell.append(ref["ell"])
    b_min, ell = np.array(b_min), np.array(ell)
    return {"index": np.array(index), "corners": np.stack(corners), "t": np.stack(ts), "R": np.stack(rs),
            "tie": np.array(tie), "b_min": b_min, "ell": ell, "scale": U / (ell * np.maximum(b_min, np.sqrt(U)))}


def errors(rot, t, tab, j):
    """(rotation error, translation error) of one pose (``rot`` [3,3], ``t`` [3]) against case j's reference, in the
    bound's measures; where the reference ties, against the nearer of its candidates."""
    best = None
    for c in range(2 if tab["tie"][j] else 1):
        d = np.asarray(rot, dtype=LD) - tab["R"][j, c]
        e_r = float(np.sqrt(np.sum(d * d) / 2))
        tc = tab["t"][j, c]
        e_t = float(np.abs(np.asarray(t, dtype=LD) - tc).max() / np.sqrt(tc @ tc))
        if best is None or e_r < best[0]:
            best = (e_r, e_t)
    return best


def ratios(poses, tab):
    """(ratio_R [n], ratio_t [n]) of poses [n,6] = [tvec | rvec]: the errors in units of the bound's ``scale``.  A
    non-finite pose gives inf."""
    poses = np.asarray(poses, dtype=np.float64)
    r_r, r_t = np.full(len(poses), np.inf), np.full(len(poses), np.inf)
    for j, p in enumerate(poses):
        if np.isfinite(p).all():
            e_r, e_t = errors(xt.matrix_from_rotvec_ld(p[3:]), p[:3], tab, j)
            r_r[j], r_t[j] = e_r / tab["scale"][j], e_t / tab["scale"][j]
    return r_r, r_t


def describe(camera, j):
    v = views()[table(camera)["index"][j]]
    return {k: (v[k] if not isinstance(v[k], np.ndarray) else v[k].tolist()) for k in ("kind", "tilt", "phi", "roll", "t")}


def worst(camera, r_r, r_t):
    """What ``conftest.report`` and the summary take: both worst ratios and where they were reached."""
    jr, jt = int(np.argmax(r_r)), int(np.argmax(r_t))
    return {"camera": camera, "cases": int(len(r_r)), "ratio_R": float(r_r[jr]), "ratio_t": float(r_t[jt]),
            "worst_R_at": str(describe(camera, jr)), "worst_t_at": str(describe(camera, jt))}


# --------------------------------------------------------------------------------------------------------------------
# host build of the device code (tests/host/ippe_host_main.hip)
# --------------------------------------------------------------------------------------------------------------------
def run_host_program(exe, corners, camera_matrix, dist, marker_size=MARKER):
    """(poses [n,6], chosen candidate [n]) of the host build, as a child process."""
    k = np.asarray(camera_matrix, dtype=np.float64).reshape(3, 3)
    d = np.zeros(8)
    if dist is not None:
        d[: len(dist)] = dist
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 8)
    head = [k[0, 0], k[1, 1], k[0, 2], k[1, 2], *d, marker_size]
    text = " ".join(repr(float(x)) for x in head) + f" {len(c)}\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in c)
    done = subprocess.run([str(exe)], input=text + "\n", capture_output=True, text=True, check=True)
    rows = np.array([[float(x) for x in line.split()] for line in done.stdout.splitlines()]).reshape(-1, 7)
    assert len(rows) == len(c)
    return rows[:, :6], rows[:, 6].astype(int)


def degenerate_detections(corners):
    """Detections that span no quadrilateral or hold a non-finite coordinate, made from one valid marker's corners [4,2]:
    name -> [4,2].  ``ekf_estimate_poses`` answers each with a pose that is not finite."""
    c = np.asarray(corners, dtype=np.float64).reshape(4, 2)
    out = {"collinear": np.stack([c[0] + i * (c[1] - c[0]) for i in range(4)]), "identical": np.repeat(c[:1], 4, axis=0)}
    for i in range(4):
        two = c.copy()
        two[(i + 1) % 4] = two[i]
        out[f"coincident_{i}_{(i + 1) % 4}"] = two
    for name, val in (("nan", np.nan), ("inf", np.inf), ("minus_inf", -np.inf)):
        for i in range(8):
            bad = c.copy()
            bad.reshape(-1)[i] = val
            out[f"{name}_{i}"] = bad
    return out
