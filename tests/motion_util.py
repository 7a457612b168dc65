"""Helpers of the camera-motion tests (``test_motion_cpu.py`` here, ``test_motion.py`` on the GPU): the move of
``include/ekf_slam_hip.h`` ("Odometry input") restated in NumPy -- once in f64 as a wrapper that gives an oracle instance
``move(d, w)``, once in ``np.longdouble`` as the reference of the one-step bound -- and the scene of the tracking fixture.
``oracle/`` is not edited: the wrapper works on an oracle's ``state`` and ``uncertainty``.

The move, for u = (d, w) in the camera frame of the pose (c, q), q scalar-first:
    c' = c + R(q) d,   q' = q (x) delta (normalised; q itself when w = 0),   delta = (cos(|w|/2), sin(|w|/2) w/|w|),
    P' = F~ P F~^T,    F~ = diag(F, I),   F = [I G G E(q); 0 Rm(delta) 0; 0 0 I]  in the column order [c q e].

One-step bound (the issue's): |P'_dev - P'_ref|_ij <= 64 u64 (Fb |P| Fb^T)_ij (+ u32 |P'_ref|_ij for an f32 P), Fb = |F| with
4 |d| added to every entry of the G and G E blocks; state: 8 u64 (|c| + |d|) on c, 8 u64 on q.
"""
from __future__ import annotations

import numpy as np

import update_sweep_util as sw

LD = np.longdouble
U64, U32 = 2.0 ** -53, 2.0 ** -24
C_P, C_STATE = 64.0, 8.0


# --------------------------------------------------------------------------------------------------------------------
# the move, in any float type
# --------------------------------------------------------------------------------------------------------------------
def _skew(w, dt):
    z = dt(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=dt)


def rotmat(q, dt=np.float64):
    """R(q), normalised: camera to map (``oracle.ekf_numpy.rotmat_scalar_first``)."""
    q = np.asarray(q, dtype=dt)
    a, v = q[0], q[1:4]
    return ((a * a - v @ v) * np.eye(3, dtype=dt) + dt(2) * np.outer(v, v) + dt(2) * a * _skew(v, dt)) / (a * a + v @ v)


def delta_quat(w, dt=np.float64):
    w = np.asarray(w, dtype=dt)
    th = np.sqrt(w @ w)
    if th == 0:
        return np.array([1, 0, 0, 0], dtype=dt)
    return np.concatenate(([np.cos(th / 2)], np.sin(th / 2) / th * w)).astype(dt)


def _rmat(b, dt):
    w, x, y, z = b
    return np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]], dtype=dt)


def _emap(q, dt):
    a, v = q[0], q[1:4]
    out = np.empty((4, 3), dtype=dt)
    out[0] = -v
    out[1:4] = a * np.eye(3, dtype=dt) - _skew(v, dt)
    return out


def motion_parts(cam, u, dt=np.float64):
    """(F [10, 10], c', q') of the move u = (d, w) at the camera state cam[0:7]."""
    cam, u = np.asarray(cam, dtype=dt), np.asarray(u, dtype=dt)
    c, q, d, w = cam[0:3], cam[3:7], u[0:3], u[3:6]
    a, v = q[0], q[1:4]
    s = a * a + v @ v
    rd = rotmat(q, dt) @ d
    eye = np.eye(3, dtype=dt)
    g = np.empty((3, 4), dtype=dt)
    g[:, 0] = (2 * a * d + 2 * np.cross(v, d)) / s - 2 * a * rd / s
    g[:, 1:4] = (-2 * np.outer(d, v) + 2 * np.outer(v, d) + 2 * (v @ d) * eye - 2 * a * _skew(d, dt)) / s \
        - 2 * np.outer(rd, v) / s
    dl = delta_quat(w, dt)
    rm = _rmat(dl, dt)
    f = np.eye(10, dtype=dt)
    f[0:3, 3:7] = g
    f[0:3, 7:10] = g @ _emap(q, dt)
    f[3:7, 3:7] = rm
    q1 = rm @ q
    if (w != 0).any():
        q1 = q1 / np.sqrt(q1 @ q1)
    else:
        q1 = q.copy()
    return f, c + rd, q1


def state_map(x10, u):
    """(c, q, e) -> (c + R((1, e) (x) q) d, q (x) delta, e), the map F differentiates (f64; q (x) delta NOT normalised)."""
    from oracle.ekf_numpy import _qmul
    x10 = np.asarray(x10, dtype=np.float64)
    c, q, e = x10[0:3], x10[3:7], x10[7:10]
    qe = _qmul(np.concatenate(([1.0], e)), q)
    return np.concatenate((c + rotmat(qe) @ u[0:3], _qmul(q, delta_quat(u[3:6])), e))


def inverse_motion(u):
    """The motion that undoes u: w' = -w, d' = -R(delta)^T d."""
    u = np.asarray(u, dtype=np.float64)
    return np.concatenate((-rotmat(delta_quat(u[3:6])).T @ u[0:3], -u[3:6]))


def with_move(orc):
    """Gives the oracle instance ``move(d, w)`` by the formulas above, in NumPy f64 (P' made bitwise symmetric from its
    lower triangle, stored through the oracle's ``_store``; a zero motion does nothing).  Returns the instance."""
    def move(d, w):
        u = np.concatenate((np.asarray(d, dtype=np.float64), np.asarray(w, dtype=np.float64)))
        if not u.any():
            return
        state = np.array(orc.state, dtype=np.float64)
        f, c1, q1 = motion_parts(state[:10], u)
        p = np.array(orc.uncertainty, dtype=np.float64)
        ft = np.eye(p.shape[0])
        ft[:10, :10] = f
        p1 = ft @ p @ ft.T
        orc.uncertainty = orc._store(np.tril(p1) + np.tril(p1, -1).T)
        state[0:3], state[3:7] = c1, q1
        orc.state = state
    orc.move = move
    return orc


def extended_move(state, p, u):
    """The same step in ``np.longdouble`` from the f64 prior (state, P): {"x1", "P1" (rounded to f64), "P1_lo" (what the
    rounding dropped), "bound_P" = (Fb |P| Fb^T), "bound_c", "F"}."""
    state, p, u = np.asarray(state, dtype=np.float64), np.asarray(p, dtype=np.float64), np.asarray(u, dtype=np.float64)
    f, c1, q1 = motion_parts(state[:10], u, LD)
    fb = np.abs(f).astype(np.float64)
    fb[0:3, 3:10] += 4.0 * np.linalg.norm(u[0:3])

    def congruence(a, m):      # diag(m, I) a diag(m, I)^T for a symmetric a: only rows and columns 0 .. 9 change
        out = a.copy()
        out[:10, :] = m @ a[:10, :]
        out[:, :10] = out[:10, :].T
        out[:10, :10] = m @ a[:10, :10] @ m.T
        return out

    p1 = congruence(p.astype(LD), f)
    x1 = state.copy()
    x1[0:3], x1[3:7] = c1.astype(np.float64), q1.astype(np.float64)
    p1_64 = p1.astype(np.float64)
    return {"x1": x1, "x1_ld": np.concatenate((c1, q1)), "P1": p1_64, "P1_lo": (p1 - p1_64.astype(LD)).astype(np.float64),
            "bound_P": congruence(np.abs(p), fb), "bound_c": np.abs(state[0:3]) + np.linalg.norm(u[0:3]), "F": f.astype(np.float64)}


def step_ratios(ref, p_dev, x_dev, dtype):
    """(r_P, r_c, r_q): the worst error in units of the bounds of the module docstring (<= 1 passes)."""
    p_dev = np.asarray(p_dev, dtype=np.float64)
    tiny = np.finfo(np.float64).tiny
    bound = C_P * U64 * ref["bound_P"] + (U32 * np.abs(ref["P1"]) if dtype == "float32" else 0.0)
    r_p = (np.abs((p_dev - ref["P1"]) - ref["P1_lo"]) / np.maximum(bound, tiny)).max()
    err = np.abs(np.asarray(x_dev[:7], dtype=LD) - ref["x1_ld"]).astype(np.float64)
    r_c = (err[0:3] / np.maximum(C_STATE * U64 * ref["bound_c"], tiny)).max()
    r_q = err[3:7].max() / (C_STATE * U64)
    return float(r_p), float(r_c), float(r_q)


def run_host_program(exe, state, p, u, dtype):
    """(state[0:7], P') of the host build for one move, as a child process."""
    import subprocess
    n = p.shape[0]
    nums = [*np.asarray(u, dtype=np.float64), *np.asarray(state[:7], dtype=np.float64), *np.asarray(p, dtype=np.float64).ravel()]
    text = f"{n} {int(dtype == 'float32')}\n" + " ".join(repr(float(x)) for x in nums) + "\n"
    done = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True)
    vals = np.array(done.stdout.split(), dtype=np.float64)
    assert vals.shape[0] == 7 + n * n
    return vals[:7], vals[7:].reshape(n, n)


# the motions of the one-step test: general, pure translation, pure rotation of 2.5 rad, |w| = 1e-9
STEP_MOTIONS = {
    "general": np.array([0.3, -0.1, 0.2, 0.02, -0.05, 0.01]),
    "translation": np.array([0.3, -0.1, 0.2, 0.0, 0.0, 0.0]),
    "rotation": np.concatenate((np.zeros(3), 2.5 * np.array([2.0, -1.0, 2.0]) / 3.0)),
    "tiny_w": np.concatenate((np.array([0.3, -0.1, 0.2]), 1e-9 * np.array([2.0, -1.0, 2.0]) / 3.0)),
}
# First n whose N = lmd n + 10 crosses the motion kernel's workgroup boundary: the strip has N - 10 = lmd n columns, one per
# thread of a 256-thread workgroup (csrc/ekf_kernels.h: EKF_MOTION_THREADS), so 3 n > 256 at n = 86 and 10 n > 256 at n = 26.
MOTION_THREADS = 256
BOUNDARY_N = {"ekf": 86, "rot": 26}
STEP_SIZES = {"ekf": (0, 1, 40, 86), "rot": (0, 1, 26, 40)}


def step_prior(model, n, dtype):
    """(state, P, landmark ids) from ``update_sweep_util.dense_prior`` (n = 0: the camera block of the n = 1 prior)."""
    state, p, lm_ids, _ids, _poses = sw.dense_prior(model, max(n, 1), 1, 4200 + 13 * n + (7 if model == "rot" else 0), dtype)
    if n == 0:
        return state[:10].copy(), p[:10, :10].copy(), []
    return state, p, lm_ids


# --------------------------------------------------------------------------------------------------------------------
# the tracking fixture
# --------------------------------------------------------------------------------------------------------------------
TRACK_FRAMES, TRACK_LANDMARKS, TRACK_STEP = 40, 10, np.array([0.0, 0.0, 0.2, 0.0, 0.01, 0.0])
TRACK_SIGMA, TRACK_ODO_NOISE, TRACK_FROM = 0.01, 0.02, 5
TRACK_RATIO = 0.2      # the condition: mean position error with odometry <= 1/5 of the error without


def _euler_xyz_of(rot):
    """Angles a with ``rotmat_euler_xyz(a) == rot`` (R = Rz Ry Rx, |pitch| < pi/2)."""
    return np.array([np.arctan2(rot[2, 1], rot[2, 2]), -np.arcsin(rot[2, 0]), np.arctan2(rot[1, 0], rot[0, 0])])


def tracking_scene(model, seed=0, step=TRACK_STEP, frames=TRACK_FRAMES, plan=None, still=()):
    """The camera starts at the origin and moves by `step` = (d, w) per frame in its own frame.  10 landmarks lie 2.5 .. 5 m
    from the start.  Frame 0 sights all of them, every later frame 4 of the 6 nearest.  Detections carry N(0, 0.01^2) noise
    on the position (and 0.01 rad on the angles of EKF_Rotations, whose rvecs are the xyz Euler angles of the true relative
    orientation), the odometry 2 % multiplicative noise.  Returns {"ids", "poses" [D, 6], "offsets" [F + 1],
    "motion" [F, 6] (row t: the noisy motion between frame t - 1 and t; row 0 zero), "truth" [F, 3]}.
    plan (None: as above): per frame the landmarks it sights (an empty list: an empty frame), and then the camera also moves
    before frame 0; still: frames before which the camera does not move and the motion is exactly zero."""
    from oracle.ekf_numpy import quat_from_euler_xyz, rotmat_euler_xyz
    rng = np.random.default_rng(1234 + seed)
    dirs = rng.normal(size=(TRACK_LANDMARKS, 3))
    lms = dirs / np.linalg.norm(dirs, axis=1)[:, None] * rng.uniform(2.5, 5.0, TRACK_LANDMARKS)[:, None]
    lm_rot = [rotmat_euler_xyz(rng.uniform(-0.3, 0.3, 3)) for _ in range(TRACK_LANDMARKS)]
    c, q = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    ids, poses, offsets, motion, truth = [], [], [0], [], []
    for t in range(frames):
        if (t > 0 or plan is not None) and t not in still:
            _f, c, q = motion_parts(np.concatenate((c, q)), step)
            motion.append(step * (1.0 + TRACK_ODO_NOISE * rng.normal(size=6)))
        else:
            motion.append(np.zeros(6))
        truth.append(c.copy())
        rcm = rotmat(q)
        if plan is not None:
            seen = np.asarray(plan[t], dtype=np.int64)
        elif t == 0:
            seen = np.arange(TRACK_LANDMARKS)
        else:
            near = np.argsort(np.linalg.norm(lms - c, axis=1))[:6]
            seen = np.sort(rng.choice(near, 4, replace=False))
        for i in seen:
            xyz = rcm.T @ (lms[i] - c) + rng.normal(0.0, TRACK_SIGMA, 3)
            ang = _euler_xyz_of(rcm.T @ lm_rot[i]) + (rng.normal(0.0, TRACK_SIGMA, 3) if model == "rot" else 0.0)
            assert np.abs(ang).max() < 1.2 and quat_from_euler_xyz(ang)[0] > 0.5      # (far from the sign tie)
            ids.append(100 + int(i))
            poses.append(np.concatenate((xyz, ang)))
        offsets.append(len(ids))
    return {"ids": np.array(ids), "poses": np.array(poses), "offsets": np.array(offsets, dtype=np.int64),
            "motion": np.array(motion), "truth": np.array(truth)}


# 14 frames: a leading empty frame, first sightings after a motion (frames 1, 3 and 8), a run of three empty frames that
# carry motions (4 .. 6), two exact-zero motions (frames 2 and 9), 1 .. 5 detections per frame
RAGGED_PLAN = ([], [0, 1, 2, 3], [1, 3], [2, 4, 5, 0, 1], [], [], [], [5], [6, 7, 0], [3, 6], [], [1, 2, 4, 7], [0, 5, 6], [2, 7])
RAGGED_STILL = (2, 9)


def ragged_motion_log(model, seed=5, step=(0.05, -0.02, 0.15, 0.004, 0.012, -0.006)):
    """The ragged log of bit rule 6(c), from the world of the tracking scene: {"ids", "poses", "offsets", "has_detections",
    "motion" [14, 6]}.  Other seeds and steps: other worlds and other motions (the members of a batch)."""
    log = tracking_scene(model, seed=seed, step=np.asarray(step, dtype=np.float64), frames=len(RAGGED_PLAN),
                         plan=RAGGED_PLAN, still=RAGGED_STILL)
    log["has_detections"] = np.diff(log["offsets"]) > 0
    return log


def oracle_for(model):
    from oracle.ekf_numpy import OracleEKF, OracleEKFRotations
    return with_move(OracleEKFRotations(sw.INIT, mode="fast") if model == "rot"
                     else OracleEKF(sw.INIT, mode="fast", quat_mode="scalar_first"))


def oracle_track(model, scene, odometry):
    """Trajectory [F, 7] of the oracle wrapper over the scene, with or without its motions."""
    orc = oracle_for(model)
    offs, out = scene["offsets"], []
    for t in range(len(offs) - 1):
        if odometry:
            orc.move(scene["motion"][t, 0:3], scene["motion"][t, 3:6])
        sl = slice(int(offs[t]), int(offs[t + 1]))
        if sl.stop > sl.start:
            orc.observe(scene["ids"][sl].tolist(), scene["poses"][sl])
        out.append(np.asarray(orc.state[:7], dtype=np.float64).copy())
    return np.array(out), orc


def mean_position_error(traj, scene, first=TRACK_FROM):
    return float(np.linalg.norm(traj[first:, 0:3] - scene["truth"][first:], axis=1).mean())
