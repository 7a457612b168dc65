"""Camera motion in ``EKFBatch`` (``motion=True``; ``"motion"`` in a log, ``observe_indexed(motion=)``) on an MI355X, for the
three window kernels and both models: members with different motions, bit rule 6(d) of ``include/ekf_slam_hip.h`` ("Odometry
input"), a member against the per-frame calls, one move per kernel against the extended-precision step under the bound of
``motion_util``, an empty frame that moves the member and its trajectory row, a failed member, and the host checks."""
import numpy as np
import pytest

import motion_util as mu
import support as sp
import update_sweep_util as sw
from conftest import rel_err, report

pytestmark = pytest.mark.gpu

INIT = sw.INIT
MODELS = ["ekf", "ekf_rotations"]
QM = {"ekf": "ekf", "ekf_rotations": "rot"}
FAMILY = {"column": {}, "large": {"large_maps": True}, "wide": {"wide_frames": True}}
MEMBERS = 4
STEPS = ((0.05, -0.02, 0.15, 0.004, 0.012, -0.006), (0.2, 0.0, 0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.02, -0.01, 0.03),
         (-0.1, 0.05, 0.1, -0.01, 0.02, 0.005))


def _batch(model, family, n, m, **kw):
    from aruco_slam_amd.batch import EKFBatch
    kw.setdefault("motion", True)
    if model == "ekf":
        kw.setdefault("quat_update", "scalar_first")
    return EKFBatch(MEMBERS, INIT, model=model, max_landmarks=n, max_visible=m, **FAMILY[family], **kw)


def _logs(model):
    return [mu.ragged_motion_log(QM[model], seed=5 + b, step=STEPS[b]) for b in range(MEMBERS)]


# ---- members with different motions: the three kernels, the per-frame calls, the oracle ---------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_three_kernels_agree_bitwise_and_a_member_is_its_per_frame_calls(model):
    """Four members, each with its own ragged log (a leading empty frame, three empty frames in a row, first sightings after
    motions, two exact-zero motions) and its own motions.  Bit rule 6(d): the large-map and wide-frame kernels give the bits
    of the one-column kernel in every output, state and P.  A member is bit for bit the batch fed frame by frame (one call
    per frame: the folded observe_indexed loop).  An empty frame moves the member and its trajectory row.  The trajectories
    match the oracle wrapper's (1e-9, the per-frame parity tolerance)."""
    logs = _logs(model)
    n, m = 8, 8
    outs = {}
    for family in FAMILY:
        batch = _batch(model, family, n, m)
        outs[family] = (batch.process_detection_logs(logs, nis=True, cam_cov=True), sp.snap_batch(batch))
        assert batch.status() == [0] * MEMBERS
    want, want_snap = outs["column"]
    for family in ("large", "wide"):
        got, snap = outs[family]
        for name in ("trajectory", "nis", "cam_cov"):
            for b in range(MEMBERS):
                assert np.array_equal(getattr(got, name)[b], getattr(want, name)[b]), (family, name, b)
        sp.assert_same(snap, want_snap, family, equal_nan=True)
    # frame by frame
    loop = _batch(model, "column", n, m)
    frames = len(logs[0]["offsets"]) - 1
    rows = [[] for _ in range(MEMBERS)]
    for t in range(frames):
        one = []
        for log in logs:
            sl = slice(int(log["offsets"][t]), int(log["offsets"][t + 1]))
            one.append({"ids": log["ids"][sl], "poses": log["poses"][sl].reshape(-1, 6),
                        "offsets": np.array([0, sl.stop - sl.start], np.int64), "motion": log["motion"][t:t + 1]})
        for b, tr in enumerate(loop.process_detection_logs(one)):
            rows[b].append(tr[0])
    sp.assert_same(sp.snap_batch(loop), want_snap, "per-frame calls", equal_nan=True)
    for b, log in enumerate(logs):
        traj = want.trajectory[b]
        assert np.array_equal(np.array(rows[b]), traj), b
        assert not np.array_equal(traj[0], INIT[:7]) or not log["motion"][0].any()
        assert len({tuple(traj[t]) for t in (3, 4, 5, 6)}) == 4, b      # (the empty frames 4 .. 6 move the row)
        assert (want.nis[b][[0, 4, 5, 6, 10]] == 0).all()
        ref, _orc = mu.oracle_track(QM[model], log, True)
        assert rel_err(traj, ref) <= 1e-9, (b, rel_err(traj, ref))
    assert not np.array_equal(want.trajectory[0], want.trajectory[3])
    # the motions are not ignored, and a batch without them is the batch it was
    plain = _batch(model, "column", n, m)
    bare = _batch(model, "column", n, m, motion=False)
    stripped = [{k: v for k, v in log.items() if k != "motion"} for log in logs]
    zeros = [dict(log, motion=np.zeros((frames, 6))) for log in stripped]
    t_zero, t_bare = plain.process_detection_logs(zeros), bare.process_detection_logs(stripped)
    for b in range(MEMBERS):
        assert np.array_equal(t_zero[b], t_bare[b]) and not np.array_equal(t_zero[b], want.trajectory[b])
    sp.assert_same(sp.snap_batch(plain), sp.snap_batch(bare), "zero motions = no motions", equal_nan=True)


# ---- one move per kernel against the extended form ----------------------------------------------------------------------------
SIZES = {("ekf", "column"): ((6, 4), (24, 16)), ("ekf_rotations", "column"): ((6, 4), (24, 8)),
         ("ekf", "large"): ((90, 16),), ("ekf_rotations", "large"): ((90, 8),),
         ("ekf", "wide"): ((24, 20),), ("ekf_rotations", "wide"): ((20, 20),)}


@pytest.mark.parametrize("model,family", list(SIZES))
def test_one_move_per_kernel_against_the_extended_reference(model, family):
    """One-column n = 6 and 24, large maps n = 90, wide frames m = 20; four members, each from its own dense prior with its
    own motion (motion_util.STEP_MOTIONS).  An empty frame with a motion is the move alone: state and P against the
    longdouble step under the single filter's bound (64 u64 Fb |P| Fb^T; 8 u64 on the state), P bitwise symmetric, the
    landmarks untouched.  Then a frame of m detections with a motion is bit for bit the move followed by the frame."""
    worst = np.zeros(3)
    for n, m in SIZES[(model, family)]:
        batch, twin = _batch(model, family, n, m), _batch(model, family, n, m)
        priors, moves, frames = [], [], []
        for b, (name, u) in enumerate(mu.STEP_MOTIONS.items()):
            state, p, lm_ids, ids, poses = sw.dense_prior(QM[model], n, m, 9100 + 17 * n + b)
            for bt in (batch, twin):
                bt.set_member(b, state, p, lm_ids)
            priors.append((state, p, u))
            empty = {"ids": np.zeros(0, np.int32), "poses": np.zeros((0, 6)), "offsets": np.array([0, 0], np.int64)}
            moves.append(dict(empty, motion=u[None, :]))
            frames.append({"ids": np.asarray(ids, np.int32), "poses": poses, "offsets": np.array([0, m], np.int64)})
        traj = batch.process_detection_logs(moves)
        assert batch.status() == [0] * MEMBERS
        for b, (state, p, u) in enumerate(priors):
            x, got = batch.get_state(b), batch.get_cov(b)
            ref = mu.extended_move(state, p, u)
            worst = np.maximum(worst, mu.step_ratios(ref, got, x, "float64"))
            assert np.array_equal(got, got.T) and np.array_equal(got[10:, 10:], p[10:, 10:]) and np.array_equal(x[7:], state[7:])
            assert np.array_equal(traj[b][0], x[:7]) and not np.array_equal(x[:7], state[:7])
        # a moved frame = the move, then the frame
        batch.process_detection_logs(frames)
        twin.process_detection_logs([dict(f, motion=mv["motion"]) for f, mv in zip(frames, moves)])
        assert batch.status() == twin.status() == [0] * MEMBERS
        sp.assert_same(sp.snap_batch(batch), sp.snap_batch(twin), (n, m), equal_nan=True)
    report(f"motion_batch_step[{model},{family}]", ratio_P=worst[0], ratio_c=worst[1], ratio_q=worst[2], bound=1.0)
    assert worst.max() <= 1.0, worst


# ---- a failed member ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILY))
def test_a_failed_member_ignores_motions(family):
    from aruco_slam_amd.batch import EKF_ERR_NUMERIC
    n, m = 6, 4
    batch = _batch("ekf", family, n, m)
    state, p, lm_ids, ids, poses = sw.dense_prior("ekf", n, m, 9300)
    for b in range(MEMBERS):
        batch.set_member(b, state, -np.eye(len(state)) if b == 2 else p, lm_ids)
    u = mu.STEP_MOTIONS["general"]
    log = {"ids": np.asarray(ids + ids, np.int32), "poses": np.vstack((poses, poses)), "offsets": np.array([0, m, m, 2 * m], np.int64),
           "has_detections": np.array([True, False, True]), "motion": np.vstack((np.zeros(6), u, u))}
    traj = batch.process_detection_logs([log] * MEMBERS)
    assert batch.status() == [0, 0, EKF_ERR_NUMERIC, 0]
    assert np.isnan(traj[2]).all() and np.isfinite(traj[0]).all()
    assert np.array_equal(batch.get_state(2), state) and np.array_equal(batch.get_cov(2), -np.eye(len(state)))
    assert not np.array_equal(traj[0][1], traj[0][0])      # (the others moved on their empty frame)


# ---- host checks and interop ------------------------------------------------------------------------------------------------
def test_motion_arguments_of_the_batch_are_validated():
    logs = _logs("ekf")
    bare = _batch("ekf", "column", 8, 8, motion=False)
    with pytest.raises(ValueError, match="motion=True"):
        bare.process_detection_logs(logs)
    with pytest.raises(ValueError, match="motion=True"):
        bare.observe_indexed(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(MEMBERS + 1, np.int64), np.zeros((0, 6)),
                             motion=np.zeros((0, 6)))
    batch = _batch("ekf", "column", 8, 8)
    before = sp.snap_batch(batch)
    partial = [dict(log) for log in logs]
    del partial[1]["motion"]
    with pytest.raises(ValueError, match="every log"):
        batch.process_detection_logs(partial)
    for bad in (logs[0]["motion"][:-1], np.full_like(logs[0]["motion"], np.nan)):
        with pytest.raises(ValueError, match="motion"):
            batch.process_detection_logs([dict(logs[0], motion=bad)] + logs[1:])
    sp.assert_same(sp.snap_batch(batch), before, "nothing changed", equal_nan=True)
    assert all(len(lm) == 0 for lm in batch.landmarks)
    # to_filter / load_filter carry the capability
    batch.process_detection_logs(logs)
    flt = batch.to_filter(1)
    assert flt.backend.can_motion and not bare.to_filter(1).backend.can_motion
    flt.move([0.1, 0.0, 0.0], [0.0, 0.0, 0.02])
    with pytest.raises(ValueError, match="motion=True"):
        bare.load_filter(0, flt)
    batch.load_filter(0, flt)
    assert np.array_equal(batch.get_state(0), flt.backend.get_state()) and np.array_equal(batch.get_cov(0), flt.backend.get_cov())
