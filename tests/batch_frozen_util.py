"""Shared pieces of the frozen-map tests of ``EKFBatch`` (``test_batch_frozen.py`` on the GPU, ``test_batch_frozen_cpu.py``
here): the batches of the three window-kernel families, the 60-frame ragged logs of the "20 mapping frames, freeze, 40 frozen
frames" case, and the recorder of ``tests/golden/batch_frozen_parent.npz`` (what a batch that never freezes computed on the
commit before the batch got its localisation mode)."""
import numpy as np

import motion_util as mu
import update_sweep_util as sw

INIT = sw.INIT
MODELS = ("ekf", "ekf_rotations")
QM = {"ekf": "ekf", "ekf_rotations": "rot"}
LMD = {"ekf": 3, "ekf_rotations": 10}
FAMILY = {"column": {}, "large": {"large_maps": True}, "wide": {"wide_frames": True}}
MEMBERS = 4
CAM = 10
# small steps: 60 of them keep every relative angle of the scene far from the limits tracking_scene asserts
STEPS = ((0.02, -0.01, 0.04, 0.001, 0.003, -0.0015), (0.05, 0.0, 0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.004, -0.002, 0.005),
         (-0.03, 0.015, 0.03, -0.002, 0.004, 0.001))
MAP_FRAMES, FROZEN_FRAMES = 20, 40


def batch(model, family, n, m, members=MEMBERS, **kw):
    from aruco_slam_amd.batch import EKFBatch
    if model == "ekf":
        kw.setdefault("quat_update", "scalar_first")
    return EKFBatch(members, INIT, model=model, max_landmarks=n, max_visible=m, **FAMILY[family], **kw)


def raw_cov(b):
    """The whole device covariance [B, ld, ld], capacity padding included."""
    b.stream.synchronize()
    return b.cov_t.cpu().numpy()


def raw_state(b):
    b.stream.synchronize()
    return b.state_t.cpu().numpy()


def ragged_plan():
    """60 frames over landmarks 0 .. 7: the 14 frames of motion_util.RAGGED_PLAN (a leading empty frame, the empty frames
    4 .. 6) and six more map the eight landmarks; the 40 that follow (the frozen part) begin with an empty frame, hold a run
    of three empty frames (30 .. 32), one more (45) and a frame with a repeated landmark (25), 1 .. 5 detections each."""
    plan = [list(p) for p in mu.RAGGED_PLAN] + [[0, 3, 5], [1, 4], [2, 6, 7], [0, 1, 2, 3, 4], [5, 6], [7, 0]]
    rng = np.random.default_rng(77)
    for t in range(MAP_FRAMES, MAP_FRAMES + FROZEN_FRAMES):
        if t in (20, 30, 31, 32, 45):
            plan.append([])
        else:
            plan.append(sorted(int(i) for i in rng.choice(8, int(rng.integers(1, 6)), replace=False)))
    plan[25] = [4, 1, 4]
    assert len(plan) == MAP_FRAMES + FROZEN_FRAMES
    return plan


def ragged_logs(model):
    """One 60-frame log per member (its own world, its own motions): {"ids", "poses", "offsets", "has_detections",
    "motion" [60, 6]}."""
    plan = ragged_plan()
    logs = []
    for b in range(MEMBERS):
        log = mu.tracking_scene(QM[model], seed=11 + b, step=np.asarray(STEPS[b], dtype=np.float64), frames=len(plan),
                                plan=plan, still=mu.RAGGED_STILL)
        log.pop("truth")
        log["has_detections"] = np.diff(log["offsets"]) > 0
        logs.append(log)
    return logs


def part(log, t0, t1, motion=True):
    """Frames [t0, t1) of a log as a log of its own (without its motions: ``motion=False``)."""
    offs = np.asarray(log["offsets"], dtype=np.int64)
    sl = slice(int(offs[t0]), int(offs[t1]))
    out = {"ids": log["ids"][sl], "poses": log["poses"][sl].reshape(-1, 6), "offsets": offs[t0:t1 + 1] - offs[t0],
           "has_detections": log["has_detections"][t0:t1]}
    if motion and "motion" in log:
        out["motion"] = log["motion"][t0:t1]
    return out


def parent_key(model, moved, name):
    return f"{model}_{'moved' if moved else 'plain'}_{name}"


def never_frozen_run(model, family, moved):
    """A batch that never freezes over the whole ragged logs: {"traj" [B, 60, 7], "nis" [B, 60], "state" [B, N], "cov": P of
    member 0 [N, N]}."""
    logs = ragged_logs(model)
    if not moved:
        logs = [{k: v for k, v in log.items() if k != "motion"} for log in logs]
    b = batch(model, family, 8, 8, motion=moved)
    out = b.process_detection_logs(logs, nis=True)
    assert b.status() == [0] * MEMBERS
    return {"traj": np.array(out.trajectory), "nis": np.array(out.nis), "state": np.array([b.get_state(i) for i in range(MEMBERS)]),
            "cov": b.get_cov(0)}


def record_parent():
    """The arrays of tests/golden/batch_frozen_parent.npz: ``never_frozen_run`` for both models, with and without motions.
    The three kernel families give the same bits (asserted here, on the recording commit), so each array is stored once."""
    out = {}
    for model in MODELS:
        for moved in (False, True):
            runs = {family: never_frozen_run(model, family, moved) for family in FAMILY}
            for family in ("large", "wide"):
                for name, v in runs[family].items():
                    assert np.array_equal(v, runs["column"][name]), (model, moved, family, name)
            for name, v in runs["column"].items():
                out[parent_key(model, moved, name)] = v
    return out
