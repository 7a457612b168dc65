"""Expected per-detection Mahalanobis distances and gate decisions of ``EKFBatch`` from the NumPy oracle, and the logs the
gating tests share (``test_batch_gating_cpu.py`` checks on the CPU that no expected distance lies near its threshold;
``test_batch_gating.py`` runs the same logs on the GPU).

Teacher-forced: ``update_sweep_util.oracle_at`` holds a frame's prior, ``measurement_blocks`` gives z and h and
``oracle.ekf_extended.extended_step(..., factors=True)["S"]`` the joint innovation covariance, whose diagonal RD x RD
blocks are the S_d of the gate.  Free-running (``oracle_gated_replay``): the f64 oracle replays a log with the gate's
semantics, S_d formed from the support block of P + Q."""
import numpy as np

import support as sp
from conftest import load_npz

INIT = sp.INIT
RD = {"ekf": 3, "ekf_rotations": 7}
LMD = {"ekf": 3, "ekf_rotations": 10}
# chi^2 99 % quantiles of 3 and 7 degrees of freedom: the gates of the teacher-forced and the free-running tests
GATES = {"ekf": 11.345, "ekf_rotations": 18.475}
# free-running logs: the device and the f64 oracle drift apart by rounding only (the project's replay agreement is 1e-9
# and better), so a distance this far, relatively, from the gate has the same decision on both
FREE_MARGIN = 1e-3
# (model, family): the batch's keyword arguments and (landmarks, detections per frame) of its logs; in the wide family the
# frames span several blocks of 16 / 8 detections.  The free-running EKF logs run with the scalar-first quaternion update:
# with the as-written one the filter is inconsistent on its own after a dozen frames and every gate rejects inliers
FAMILIES = {
    ("ekf", "column"): ({"max_landmarks": 24, "max_visible": 16, "quat_update": "scalar_first"}, 24, (2, 10)),
    ("ekf_rotations", "column"): ({"max_landmarks": 12, "max_visible": 8}, 12, (1, 5)),
    ("ekf", "large"): ({"max_landmarks": 24, "max_visible": 16, "large_maps": True, "quat_update": "scalar_first"}, 24, (2, 10)),
    ("ekf_rotations", "large"): ({"max_landmarks": 12, "max_visible": 8, "large_maps": True}, 12, (1, 5)),
    ("ekf", "wide"): ({"max_landmarks": 40, "max_visible": 48, "wide_frames": True, "quat_update": "scalar_first"}, 40, (14, 36)),
    ("ekf_rotations", "wide"): ({"max_landmarks": 20, "max_visible": 24, "wide_frames": True}, 20, (6, 18)),
}
STEADY = 70        # frames after the bootstrap: more than one window of 64 frames in every family


def tolerance(kappa):
    """The project's NIS tolerance form on the block: relative, max(1e-9, 100 kappa(S_d) 2^-52)."""
    return max(1e-9, 100.0 * kappa * 2.0 ** -52)


def clean_log(model, family, seed):
    from aruco_slam_amd.synthetic import ragged_log
    _kw, n, m_range = FAMILIES[(model, family)]
    log = ragged_log(n, m_range, STEADY, seed=seed, rvec_sigma=0.05 if model == "ekf_rotations" else 0.0)
    log["poses"] = log["poses"] + 0.0
    return log


def dirty_log(model, log, seed, every=3):
    """``log`` with outliers inserted after the bootstrap: in every ``every``-th frame one or two extra detections of
    landmarks the frame already sees, with a gross tvec offset (rotations: every other one with a flipped rvec as well),
    at random positions; in front of every 11th frame a frame of outliers only is inserted, and two empty frames.
    Returns the log and the bool mask [D] of the inserted detections (``extra_frames`` tells the inserted frames)."""
    rng = np.random.default_rng(1000 + seed)
    offs, boot = log["offsets"], int(log["bootstrap_frames"])
    ids, poses, counts, marks = [], [], [], []
    for t in range(len(offs) - 1):
        fi = [int(i) for i in log["ids"][offs[t]:offs[t + 1]]]
        fp = [p.copy() for p in log["poses"][offs[t]:offs[t + 1]]]
        fm = [False] * len(fi)
        steady = t - boot
        if steady >= 0 and steady % 11 == 10:          # a frame of outliers only in front of this one
            ids += fi
            poses += [_outlier(model, p, rng, j) for j, p in enumerate(fp)]
            marks += [True] * len(fi)
            counts.append(len(fi))
        if steady >= 0 and steady % every == 0:
            for j in range(1 + steady % 2):
                src = int(rng.integers(len(fi)))
                pos = int(rng.integers(len(fi) + 1))
                fi.insert(pos, fi[src])
                fp.insert(pos, _outlier(model, fp[src], rng, j))
                fm.insert(pos, True)
        if steady in (5, 40):                           # an empty frame in front of this one
            counts.append(0)
        ids += fi
        poses += fp
        marks += fm
        counts.append(len(fi))
    counts = np.asarray(counts, dtype=np.int64)
    out = {"ids": np.asarray(ids, np.int32), "poses": np.asarray(poses, np.float64).reshape(-1, 6),
           "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64), "has_detections": counts > 0,
           "bootstrap_frames": boot}
    return out, np.asarray(marks, dtype=bool)


def _outlier(model, pose, rng, j):
    p = np.array(pose, dtype=np.float64)
    p[:3] += rng.choice([-1.0, 1.0], 3) * rng.uniform(100.0, 200.0, 3)    # gross: with q_err = 0.5 per frame S_d is tens of m^2
    if model == "ekf_rotations" and j % 2 == 0:
        p[3:6] = -p[3:6] + np.array([np.pi / 2, 0.0, 0.0])                # a flipped orientation
    return p


def extra_frames(log, marks):
    """bool [F]: the frames of a dirty log that hold no detection of the clean log (empty, or outliers only)."""
    kept = np.concatenate(([0], np.cumsum(~np.asarray(marks, dtype=bool))))
    return np.diff(kept[log["offsets"]]) == 0


def delete(log, drop):
    """``log`` without the detections ``drop`` [D] (bool); frames stay, possibly empty."""
    drop = np.asarray(drop, dtype=bool)
    kept = np.concatenate(([0], np.cumsum(~drop)))
    offs = kept[log["offsets"]]
    return {"ids": log["ids"][~drop], "poses": log["poses"][~drop], "offsets": offs.astype(np.int64),
            "has_detections": np.diff(offs) > 0}


def _new_oracle(model, quat="as_written"):
    from oracle.ekf_numpy import OracleEKF, OracleEKFRotations
    if model == "ekf_rotations":
        return OracleEKFRotations(INIT, mode="fast")
    return OracleEKF(INIT, mode="fast", quat_mode=quat)


def block_distances(model, orc, ids, poses, s_joint=None):
    """d^2 and kappa(S_d) of every detection of a frame on the prior ``orc`` holds (all ids known).  S_d: the diagonal
    block of ``s_joint`` if given, else H_d (P+Q) H_d^T + R I from the support block."""
    from oracle.ekf_numpy import R_UNCERTAINTY
    rd, lmd = RD[model], LMD[model]
    z, h, jac, col = orc.measurement_blocks(ids, poses)
    r = z - h
    pq = np.array(orc.uncertainty, dtype=np.float64)
    pq[np.arange(pq.shape[0]), np.arange(pq.shape[0])] += orc.process_noise_diag()
    d2, kappa = np.empty(len(ids)), np.empty(len(ids))
    for j, c0 in enumerate(col):
        sl = slice(rd * j, rd * j + rd)
        if s_joint is not None:
            sd = s_joint[sl, sl]
        else:
            supp = np.concatenate((np.arange(10), np.arange(c0, c0 + lmd)))
            sd = jac[j] @ pq[np.ix_(supp, supp)] @ jac[j].T + R_UNCERTAINTY * np.eye(rd)
            sd = 0.5 * (sd + sd.T)
        ev = np.linalg.eigvalsh(sd)
        d2[j] = float(r[sl] @ np.linalg.solve(sd, r[sl]))
        kappa[j] = float(ev[-1] / ev[0])
    return d2, kappa


def teacher_distances(model, state, p, lm_ids, ids, poses):
    """Teacher-forced expected distances of one frame: (d^2 [m], kappa(S_d) [m])."""
    from oracle.ekf_extended import extended_step
    from update_sweep_util import oracle_at
    qm = "rot" if model == "ekf_rotations" else "ekf"
    ref = extended_step(oracle_at(qm, state, p, lm_ids), ids, poses, factors=True)
    return block_distances(model, oracle_at(qm, state, p, lm_ids), ids, poses, ref["S"])


def teacher_frames(case):
    """The stepped C1 frames (EKF) or the G5 frames (EKF_Rotations) whose detections are all of known landmarks, each with
    one outlier appended (a copy of its first detection, grossly off): (model, [(state, P, lm_ids, ids, poses)])."""
    model = "ekf" if case == "c1" else "ekf_rotations"
    frames = []
    if case == "c1":
        det = load_npz("c1_detections.npz")
        offs = det["offsets"]
        orc = _new_oracle(model)
        for f in range(len(offs) - 1):
            if not det["has_detections"][f]:
                continue
            ids, poses = [int(i) for i in det["ids"][offs[f]:offs[f + 1]]], det["poses"][offs[f]:offs[f + 1]]
            lm = [k for k, _ in sorted(orc.landmarks.items(), key=lambda kv: kv[1])]
            frames.append((np.array(orc.state, dtype=np.float64), np.array(orc.uncertainty, dtype=np.float64), lm, ids,
                           np.array(poses, dtype=np.float64)))
            orc.observe(ids, poses)
    else:
        g = load_npz("g5_rotations.npz")
        offs = g["offsets"]
        frames = [(g[f"f{f}_state0"], g[f"f{f}_P0"], [int(i) for i in g[f"f{f}_lm_ids"]],
                   [int(i) for i in g["ids"][offs[f]:offs[f + 1]]], np.array(g["poses"][offs[f]:offs[f + 1]]))
                  for f in g["frames"]]
    rng = np.random.default_rng(7)
    out = []
    for s0, p0, lm, ids, poses in frames:
        if not set(ids) <= set(lm):
            continue        # (first sightings: the oracle's prior does not hold the new landmark yet)
        ids = ids + [ids[0]]
        poses = np.vstack((poses, _outlier(model, poses[0], rng, len(out))))
        out.append((s0, p0, lm, ids, poses))
    return model, out


def oracle_gated_replay(model, log, gate):
    """The f64 oracle on ``log`` with the gate's semantics.  Returns (d^2 [D], rejected [D]); exempt first sightings have
    d^2 = 0."""
    orc = _new_oracle(model, "scalar_first")
    offs = log["offsets"]
    d2_all = np.zeros(len(log["ids"]))
    for t in range(len(offs) - 1):
        ids = [int(i) for i in log["ids"][offs[t]:offs[t + 1]]]
        poses = log["poses"][offs[t]:offs[t + 1]]
        if not ids:
            continue
        exempt = np.zeros(len(ids), dtype=bool)
        for j, (k, pose) in enumerate(zip(ids, poses)):
            if k not in orc.landmarks:
                orc.add_marker(k, pose)
                exempt[j] = True
        d2, _kappa = block_distances(model, orc, ids, poses)
        d2[exempt] = 0.0
        d2_all[offs[t]:offs[t + 1]] = d2
        keep = ~(d2 > gate)
        if keep.any():
            orc.predict()
            orc.update([k for k, s in zip(ids, keep) if s], poses[keep])
    return d2_all, d2_all > gate
