"""Expected values of the per-frame process-noise scale (``frame_scale=True``, ``scale=``; include/ekf_slam_hip.h, "Per-frame
process-noise scale") from the oracle, and the cases the frame-scale tests share (``test_frame_scale_cpu.py`` checks them on
the CPU, ``test_frame_scale.py`` / ``test_batch_frame_scale.py`` run them on the GPU).  ``oracle/`` knows the constant Q only,
so the scaled reference is built here from the oracle's own pieces: ``scaled`` wraps an oracle instance so that
``process_noise_diag()`` returns ``fl(s_eff q)`` (one f64 multiplication per entry), and everything that reads it
(``oracle.ekf_extended.extended_step``, ``row_noise_util.extended_step_rows``, ``predict``, the gate's S_d) sees Q_eff.

``oracle_scaled_replay`` replays a log with rules 3 and 4: a stepped frame runs with ``s_eff = p + s`` and leaves p = 0, a
frame that is not stepped (no detections, or none survived the gate) sets ``p = p + s``; a frame without a scale
(``scale=None``) is the frame as it ever was (stepped: ``p + 1``; not stepped: p stays).

The lock-out fixture (``lockout_log``): a camera that moves during a detection dropout.  LOCKOUT[model] = (G, J) were chosen
with the oracle (``test_frame_scale_cpu.py`` asserts the conditions they were chosen for)."""
from __future__ import annotations

import contextlib
import functools

import numpy as np

import gating_util as gu
import row_noise_util as rn
import update_sweep_util as sw

RD = gu.RD
# chi^2 95 % quantiles of 3 and 7 degrees of freedom: the gates of the lock-out fixture
LOCKOUT_GATES = {"ekf": 7.815, "ekf_rotations": 14.067}
FRAME_MS = 33.3
# (G empty frames, J metres the camera backs away along its optical axis meanwhile) per model, chosen with the oracle: without
# scales every detection after the gap has d^2 >= 2 gate (2.8 / 2.3 times the gate), with the scales of the timestamps the
# first frame after the gap has every d^2 <= gate / 2 (0.42 / 0.44 times the gate) and nothing is rejected afterwards
LOCKOUT = {"ekf": (36, 6.5), "ekf_rotations": (36, 7.5)}
# the run with the jump ends within this factor of the position error of the same log without the jump (the f64 oracle:
# 2.3 / 2.8; the device differs from it by rounding)
LOCKOUT_FACTOR = 4.0
LOCKOUT_BEFORE, LOCKOUT_AFTER = 20, 24

WIDE_SCALES = (0.25, 8.0)


@contextlib.contextmanager
def scaled(orc, s_eff):
    """``orc`` with ``process_noise_diag()`` returning fl(s_eff q) while the block runs."""
    base = type(orc).process_noise_diag
    s_eff = np.float64(s_eff)
    orc.process_noise_diag = lambda: s_eff * base(orc)
    try:
        yield orc
    finally:
        del orc.process_noise_diag


def scaled_constants(model, s_eff, base=None):
    """The ``noise=`` dict of a twin filter configured with the products (bit rule 5(b)): fl(s_eff q) for q_cam, q_err,
    q_lm of the model (``base``: constants that replace the model's)."""
    if model in ("rot", "ekf_rotations"):
        from aruco_slam_amd.filters import ekf_with_rotations as mod
        q = {"q_cam": mod.Q_UNCERTAINTY_CAM, "q_err": mod.Q_ERROR_UNCERTAINTY_CAM, "q_lm": mod.Q_UNCERTAINTY_LM_XYZ}
    else:
        from aruco_slam_amd.filters import extended_kalman_filter as mod
        q = {"q_cam": mod.Q_UNCERTAINTY_CAM, "q_err": mod.Q_ERROR_UNCERTAINTY_CAM, "q_lm": mod.Q_UNCERTAINTY_LM}
    q.update(base or {})
    return {k: float(np.float64(s_eff) * np.float64(v)) for k, v in q.items()}


# ---- one step ---------------------------------------------------------------------------------------------------------------
# (group, model, n, m, fused, max_visible, (lo, hi)) as row_noise_util.STEP_CASES, (lo, hi) the range of the case's scale.
# The smallest shapes on either side of every dispatch boundary; the ranges narrow where kappa(S) would pass 1e3.
def _cases():
    want = {("ekf_fused", m) for m in (1, 5, 6, 16, 33, 64)} | {("ekf_stage", m) for m in (1, 5, 6, 16, 33, 64)}
    want |= {("ekf_wide", 69), ("ekf_blocked", 129)}
    want |= {("rot_fused", 1), ("rot_fused", 9), ("rot_stage", 28), ("rot_wide", 51)}
    return [c[:6] + (SCALE_RANGE.get((c[0], c[3]), WIDE_SCALES),) for c in rn.STEP_CASES if (c[0], c[3]) in want]


SCALE_RANGE = {}
STEP_CASES = _cases()


def case_scale(key, lo, hi):
    """The scale of a case: log-uniform in [lo, hi], never 1."""
    rng = np.random.default_rng(sw.prior_seed(key) + 77)
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def extended_step_scaled(orc, ids, poses, s_eff, rows=None, factors=False):
    """The extended-precision step with Q_eff = fl(s_eff q): ``oracle.ekf_extended.extended_step`` (rows None) or
    ``row_noise_util.extended_step_rows`` on the wrapped oracle."""
    from oracle.ekf_extended import extended_step
    with scaled(orc, s_eff):
        if rows is None:
            return extended_step(orc, ids, poses, factors=factors)
        return rn.extended_step_rows(orc, ids, poses, rows, factors=factors)


def step_reference(case, dtype):
    """(prior, scale, extended-precision step with that scale) of a STEP_CASES entry."""
    key = rn.case_key(case, dtype)
    prior = sw.dense_prior(key.model, key.n, key.m, sw.prior_seed(key), key.dtype)
    state, p, lm_ids, ids, poses = prior
    s = case_scale(key, *case[6])
    ref = extended_step_scaled(sw.oracle_at(key.model, state, p, lm_ids, key.quat), ids, poses, s, factors=True)
    return prior, s, ref


def step_references(dtypes=sw.DTYPES):
    import os
    from concurrent.futures import ThreadPoolExecutor
    todo = [(case, dt) for dt in dtypes for case in STEP_CASES]
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    workers = max(1, min(16, cpus, int(os.environ.get("OMP_NUM_THREADS", cpus))))
    with ThreadPoolExecutor(workers) as pool:
        return dict(zip(todo, pool.map(lambda cd: step_reference(*cd), todo)))


def block_distances_scaled(model, orc, ids, poses, s_eff, rows=None):
    """d^2 and kappa(S_d) of every detection with S_d = H_d (P + Q_eff) H_d^T + R (model as in gating_util)."""
    with scaled(orc, s_eff):
        if rows is None:
            return gu.block_distances(model, orc, ids, poses)
        return rn.block_distances_rows(model, orc, ids, poses, rows)


# ---- logs ---------------------------------------------------------------------------------------------------------------------
def oracle_scaled_replay(model, log, scale, gate=np.inf, quat="scalar_first", pending=0.0):
    """The f64 oracle on ``log`` with the gate's semantics and rules 3 and 4 of the scale.  ``scale`` [F] or None (no frame
    carries one).  Returns a dict: d2 [D], rejected [D], stepped [F] bool, s_eff [F] (NaN: not stepped), trajectory [F, 7],
    pending (after the log), orc."""
    orc = gu._new_oracle(model, quat)
    offs = log["offsets"]
    frames = len(offs) - 1
    d2_all = np.zeros(len(log["ids"]))
    stepped, s_effs, traj = np.zeros(frames, dtype=bool), np.full(frames, np.nan), np.zeros((frames, 7))
    p = np.float64(pending)
    for t in range(frames):
        ids = [int(i) for i in log["ids"][offs[t]:offs[t + 1]]]
        poses = log["poses"][offs[t]:offs[t + 1]]
        s = None if scale is None else np.float64(scale[t])
        s_eff = p + (np.float64(1.0) if s is None else s)
        keep = np.zeros(0, dtype=bool)
        if ids:
            exempt = np.zeros(len(ids), dtype=bool)
            for j, (k, pose) in enumerate(zip(ids, poses)):
                if k not in orc.landmarks:
                    orc.add_marker(k, pose)
                    exempt[j] = True
            with scaled(orc, s_eff):
                d2, _kappa = gu.block_distances(model, orc, ids, poses)
                d2[exempt] = 0.0
                d2_all[offs[t]:offs[t + 1]] = d2
                keep = ~(d2 > gate)
                if keep.any():
                    orc.predict()
                    orc.update([k for k, kept in zip(ids, keep) if kept], poses[keep])
        if keep.any():
            stepped[t], s_effs[t], p = True, s_eff, np.float64(0.0)
        elif s is not None:
            p = s_eff
        traj[t] = np.asarray(orc.state, dtype=np.float64)[:7]
    return {"d2": d2_all, "rejected": d2_all > gate, "stepped": stepped, "s_eff": s_effs, "trajectory": traj,
            "pending": float(p), "orc": orc}


def fold_log(log, scale, stepped=None, pending=0.0):
    """Bit rule 5(c): ``log`` with its frames that are not stepped deleted (``stepped`` [F] bool; None: the frames with
    detections) and their scales folded into the next stepped frame by rule 3's addition, in log order.  Returns (log',
    scale' [F'], pending left behind the last stepped frame)."""
    offs = np.asarray(log["offsets"], dtype=np.int64)
    counts = np.diff(offs)
    stepped = counts > 0 if stepped is None else np.asarray(stepped, dtype=bool)
    out_scale, keep_det, new_counts = [], np.zeros(len(log["ids"]), dtype=bool), []
    p = np.float64(pending)
    for t in range(len(counts)):
        s_eff = p + np.float64(scale[t])
        if stepped[t]:
            out_scale.append(s_eff)
            keep_det[offs[t]:offs[t + 1]] = True
            new_counts.append(counts[t])
            p = np.float64(0.0)
        else:
            p = s_eff
    new_offs = np.concatenate(([0], np.cumsum(np.asarray(new_counts, dtype=np.int64)))).astype(np.int64)
    folded = {"ids": log["ids"][keep_det], "poses": log["poses"][keep_det], "offsets": new_offs,
              "has_detections": np.ones(len(new_counts), dtype=bool)}
    return folded, np.asarray(out_scale, dtype=np.float64), float(p)


def ragged_scaled_log(model, seed=3, n=12, m_range=(1, 5), steady=40, empty_every=7):
    """A ragged log (synthetic.ragged_log: first sightings in its bootstrap segment) with empty frames inserted -- single
    ones and a run of three, one of them in front of everything -- and a scale per frame, log-uniform in [0.25, 4] with a
    few exact 0 and exact 1."""
    from aruco_slam_amd.synthetic import ragged_log
    base = ragged_log(n, m_range, steady, seed=seed, bootstrap_m=4, rvec_sigma=0.05 if model == "ekf_rotations" else 0.0)
    offs = base["offsets"]
    counts = []
    ids, poses = [], []
    for t in range(len(offs) - 1):
        if t == 0 or t % empty_every == 3:
            counts.append(0)
        if t == 17:
            counts += [0, 0, 0]
        counts.append(int(offs[t + 1] - offs[t]))
        ids.append(base["ids"][offs[t]:offs[t + 1]])
        poses.append(base["poses"][offs[t]:offs[t + 1]])
    counts.append(0)      # (a trailing empty frame: its scale stays pending)
    counts = np.asarray(counts, dtype=np.int64)
    rng = np.random.default_rng(900 + seed)
    scale = np.exp(rng.uniform(np.log(0.25), np.log(4.0), len(counts)))
    scale[5], scale[11], scale[12] = 0.0, 1.0, 0.0
    log = {"ids": np.concatenate(ids).astype(np.int32), "poses": np.concatenate(poses) + 0.0,
           "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64), "has_detections": counts > 0}
    return log, scale


# ---- the lock-out fixture -------------------------------------------------------------------------------------------------
def _lockout_world():
    rng = np.random.default_rng(4242)
    lm = np.column_stack((rng.uniform(-1.0, 1.0, 10), rng.uniform(-1.0, 1.0, 10), rng.uniform(3.0, 6.0, 10)))
    rvec = rng.uniform(-0.3, 0.3, (10, 3))
    return lm, rvec


@functools.lru_cache(maxsize=None)
def lockout_log(model, gap=None, jump=None):
    """About 10 landmarks, 3-4 detections per frame: LOCKOUT_BEFORE normal frames from a camera at rest at the origin, ``gap``
    empty frames during which the true camera translates by ``jump`` metres along x, LOCKOUT_AFTER more frames from where it
    stopped; timestamps FRAME_MS apart.  ``jump=0`` is the same log without the jump.  Returns the log (with
    ``timestamps_ms``, ``scale`` from them as ``run_slam --frame-period FRAME_MS`` forms it, ``truth`` [F, 3] camera
    positions and ``first_after``, the first frame after the gap)."""
    g, j = LOCKOUT[model]
    gap = g if gap is None else gap
    jump = j if jump is None else jump
    lm, rvec = _lockout_world()
    rng = np.random.default_rng(77)
    counts, ids, poses, truth = [], [], [], []
    frames = LOCKOUT_BEFORE + gap + LOCKOUT_AFTER
    for t in range(frames):
        in_gap = LOCKOUT_BEFORE <= t < LOCKOUT_BEFORE + gap
        after = t >= LOCKOUT_BEFORE + gap
        cam = np.array([0.0, 0.0, -jump * (min(t - LOCKOUT_BEFORE + 1, gap) / gap if (in_gap or after) else 0.0)])
        truth.append(cam)
        if in_gap:
            counts.append(0)
            continue
        m = 3 + t % 2
        pick = [(3 * t + 3 * i) % 10 for i in range(m)]
        z = lm[pick] - cam + rng.normal(0.0, 0.01, (m, 3))
        r = rvec[pick] + (rng.normal(0.0, 0.005, (m, 3)) if model == "ekf_rotations" else 0.0)
        ids += [10 + 3 * q for q in pick]
        poses.append(np.hstack((z, r if model == "ekf_rotations" else np.zeros((m, 3)))))
        counts.append(m)
    counts = np.asarray(counts, dtype=np.int64)
    stamps = FRAME_MS * np.arange(1, frames + 1)
    scale = np.concatenate(([1.0], np.diff(stamps) / FRAME_MS))
    return {"ids": np.asarray(ids, dtype=np.int32), "poses": np.concatenate(poses),
            "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64), "has_detections": counts > 0,
            "timestamps_ms": stamps, "scale": scale, "truth": np.asarray(truth), "first_after": LOCKOUT_BEFORE + gap}


def position_error(replay, log):
    """|camera position - truth| at the end of a replay (``oracle_scaled_replay`` or a device trajectory [F, 7])."""
    traj = replay["trajectory"] if isinstance(replay, dict) else np.asarray(replay)
    return float(np.linalg.norm(traj[-1, :3] - log["truth"][-1]))
