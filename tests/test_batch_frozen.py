"""Localisation mode of ``EKFBatch`` (``freeze_map`` / ``unfreeze_map`` / ``map_frozen``; "Localisation mode of a batch" in
``include/ekf_slam_hip.h``) on an MI355X, for the three window kernels and both models: one frozen frame per kernel bit for bit
against the mapping frame, frozen beside mapping members in one launch, the three kernels against each other, the per-frame
calls and the Schmidt oracle, the composition with gate, per-detection noise, frame scale and motion, replicas, unfreezing,
first sightings, a frozen member that fails, the golden arrays of batches that never freeze, and the interop with filters."""
import numpy as np
import pytest

import batch_frozen_util as bu
import frozen_util as fu
import gating_util as gu
import support as sp
import update_sweep_util as sw
from conftest import load_npz, rel_err, synthetic_marker_views

pytestmark = pytest.mark.gpu

MEMBERS, CAM = bu.MEMBERS, bu.CAM
QM = bu.QM
EMPTY = {"ids": np.zeros(0, np.int32), "poses": np.zeros((0, 6)), "offsets": np.array([0, 0], np.int64)}


def _frame(ids, poses):
    return {"ids": np.asarray(ids, np.int32), "poses": np.asarray(poses, np.float64).reshape(-1, 6),
            "offsets": np.array([0, len(ids)], np.int64)}


def _dense_members(model, n, m, seed, duplicate=True):
    """Per member (state, P, landmark ids) and one frame of m detections from its own dense prior; with ``duplicate`` the
    last detection is a second, differently noised sighting of the first one's landmark."""
    priors, frames = [], []
    for b in range(MEMBERS):
        state, p, lm_ids, ids, poses = sw.dense_prior(QM[model], n, m, seed + 31 * b)
        if duplicate and m >= 2:
            ids, poses = list(ids), poses.copy()
            ids[-1] = ids[0]
            poses[-1] = poses[0] + 0.01 * np.array([1.0, -2.0, 1.5, 0.3, -0.2, 0.1]) * (1.0 if model == "ekf_rotations" else
                                                                                       np.array([1, 1, 1, 0, 0, 0]))
        priors.append((state, p, lm_ids))
        frames.append(_frame(ids, poses))
    return priors, frames


def _restore(batch, priors):
    for b, (state, p, lm_ids) in enumerate(priors):
        batch.set_member(b, state, p, lm_ids)


def _assert_frozen_member(b, batch, twin_snap, prior, raw):
    state0, p0, _ = prior
    n = state0.shape[0]
    sf, pf = batch.get_state(b), batch.get_cov(b)
    sm, pm = twin_snap[b]
    assert np.array_equal(sf[:CAM], sm[:CAM]), ("camera state", b)
    assert np.array_equal(pf[:CAM, :], pm[:CAM, :]) and np.array_equal(pf[:, :CAM], pm[:, :CAM]), ("camera strip", b)
    assert np.array_equal(sf[CAM:], state0[CAM:]) and np.array_equal(pf[CAM:, CAM:], p0[CAM:, CAM:]), ("the map moved", b)
    assert np.array_equal(pf, pf.T), ("symmetry", b)
    assert np.array_equal(raw[b][:n, :n], pf) and not raw[b][n:, :].any() and not raw[b][:, n:].any(), ("padding", b)
    assert not np.array_equal(pm[CAM:, CAM:], p0[CAM:, CAM:]) and not np.array_equal(sm[:CAM], state0[:CAM])


# ---- 1. one frozen frame per kernel ---------------------------------------------------------------------------------------
SHAPES = [("column", "ekf", 1, 1), ("column", "ekf", 6, 4), ("column", "ekf", 24, 16), ("column", "ekf", 82, 16),
          ("column", "ekf_rotations", 1, 1), ("column", "ekf_rotations", 6, 4), ("column", "ekf_rotations", 24, 8),
          ("large", "ekf", 90, 16), ("large", "ekf_rotations", 30, 8),
          ("wide", "ekf", 24, 20), ("wide", "ekf", 24, 33), ("wide", "ekf_rotations", 20, 20)]


@pytest.mark.parametrize("family,model,n,m", SHAPES)
def test_one_frozen_frame_is_the_camera_strip_of_the_mapping_frame(family, model, n, m):
    """Two batches restored from the same dense priors (one per member); in one, members 0 and 2 are frozen.  One frame
    with a repeated landmark.  Members 0 and 2: camera state, P[0:10, :] and P[:, 0:10] are the twin's bits, state[10:] and
    P[10:, 10:] the prior's, the padding is zero and P is bitwise symmetric.  Members 1 and 3 -- mapping members inside
    the launch of the FROZEN instance -- are the twin in every bit."""
    priors, frames = _dense_members(model, n, m, 7000 + 13 * n + m)
    batch, twin = bu.batch(model, family, n, m), bu.batch(model, family, n, m)
    for bt in (batch, twin):
        _restore(bt, priors)
    batch.freeze_map(0)
    batch.freeze_map(2)
    assert batch.map_frozen.tolist() == [True, False, True, False] and not twin.map_frozen.any()
    got = batch.process_detection_logs(frames, nis=True, cam_cov=True)
    want = twin.process_detection_logs(frames, nis=True, cam_cov=True)
    assert batch.status() == twin.status() == [0] * MEMBERS
    assert batch.map_frozen.tolist() == [True, False, True, False]
    twin_snap, raw, raw_twin = sp.snap_batch(twin), bu.raw_cov(batch), bu.raw_cov(twin)
    for name in ("trajectory", "nis", "cam_cov"):      # (the per-frame outputs hold camera quantities only)
        for b in range(MEMBERS):
            assert np.array_equal(getattr(got, name)[b], getattr(want, name)[b]), (name, b)
    for b in (0, 2):
        _assert_frozen_member(b, batch, twin_snap, priors[b], raw)
    for b in (1, 3):
        assert np.array_equal(raw[b], raw_twin[b]) and np.array_equal(batch.get_state(b), twin_snap[b][0]), b
    assert np.array_equal(bu.raw_state(batch)[[1, 3]], bu.raw_state(twin)[[1, 3]])


# ---- 2. the three kernels, the per-frame calls, the oracle -------------------------------------------------------------------
def _plain(logs):
    return [{k: v for k, v in log.items() if k != "motion"} for log in logs]


@pytest.mark.parametrize("model", bu.MODELS)
def test_three_kernels_agree_and_a_member_is_its_per_frame_calls_and_the_oracle(model):
    """Ragged logs (a leading empty frame, runs of empty frames): 20 mapping frames, freeze_map(), 40 frozen frames; n = 8,
    m = 8.  The large-map and wide-frame kernels give the one-column kernel's bits in trajectory, NIS, cam_cov, state and P;
    the log call is the batch fed one frame per call; the map keeps the bits it had when it was frozen; the trajectory
    matches the Schmidt oracle (frozen_util.schmidt_step on the NumPy oracle, bootstrapped identically) within 1e-9, the
    project's per-frame parity tolerance."""
    logs = _plain(bu.ragged_logs(model))
    a = [bu.part(log, 0, bu.MAP_FRAMES) for log in logs]
    z = [bu.part(log, bu.MAP_FRAMES, bu.MAP_FRAMES + bu.FROZEN_FRAMES) for log in logs]
    outs = {}
    for family in bu.FAMILY:
        batch = bu.batch(model, family, 8, 8)
        first = batch.process_detection_logs(a)
        at_freeze = sp.snap_batch(batch)
        batch.freeze_map()
        out = batch.process_detection_logs(z, nis=True, cam_cov=True)
        assert batch.status() == [0] * MEMBERS and batch.last_ignored == [()] * MEMBERS
        outs[family] = (first, out, sp.snap_batch(batch))
        for (s0, p0), (s1, p1) in zip(at_freeze, outs[family][2]):
            assert np.array_equal(s1[CAM:], s0[CAM:]) and np.array_equal(p1[CAM:, CAM:], p0[CAM:, CAM:]), family
            assert not np.array_equal(p1[:CAM], p0[:CAM])
    first, want, want_snap = outs["column"]
    for family in ("large", "wide"):
        _f, got, snap = outs[family]
        for name in ("trajectory", "nis", "cam_cov"):
            for b in range(MEMBERS):
                assert np.array_equal(getattr(got, name)[b], getattr(want, name)[b]), (family, name, b)
        sp.assert_same(snap, want_snap, family, equal_nan=True)
    # one frame per call
    loop = bu.batch(model, "column", 8, 8)
    rows = [[] for _ in range(MEMBERS)]
    for t in range(bu.MAP_FRAMES + bu.FROZEN_FRAMES):
        if t == bu.MAP_FRAMES:
            loop.freeze_map()
        for b, tr in enumerate(loop.process_detection_logs([bu.part(log, t, t + 1) for log in logs])):
            rows[b].append(tr[0])
    sp.assert_same(sp.snap_batch(loop), want_snap, "per-frame calls", equal_nan=True)
    worst = 0.0
    for b, log in enumerate(logs):
        traj = np.concatenate((first[b], want.trajectory[b]))
        assert np.array_equal(np.array(rows[b]), traj), b
        assert (want.nis[b][[0, 10, 11, 12, 25]] == 0).all() and (want.nis[b][[1, 5]] > 0).all()
        orc = fu.new_oracle(model)
        ref = []
        for t in range(len(log["offsets"]) - 1):
            sl = slice(int(log["offsets"][t]), int(log["offsets"][t + 1]))
            if sl.stop > sl.start and t < bu.MAP_FRAMES:
                orc.observe(log["ids"][sl].tolist(), log["poses"][sl])
            elif sl.stop > sl.start:
                fu.schmidt_step(orc, log["ids"][sl].tolist(), log["poses"][sl])
            ref.append(np.asarray(orc.state[:7], dtype=np.float64).copy())
        worst = max(worst, rel_err(traj, np.array(ref)))
    print(f"frozen batch vs Schmidt oracle [{model}]: {worst:.2e}")
    assert worst <= 1e-9, worst


# ---- 3. composition ----------------------------------------------------------------------------------------------------------
SMALL = {("ekf", "column"): (6, 4), ("ekf_rotations", "column"): (6, 4), ("ekf", "large"): (6, 4),
         ("ekf_rotations", "large"): (6, 4), ("ekf", "wide"): (24, 20), ("ekf_rotations", "wide"): (20, 20)}


def _frozen_batch(model, family, n, m, priors, **kw):
    batch = bu.batch(model, family, n, m, **kw)
    _restore(batch, priors)
    batch.freeze_map()
    return batch


@pytest.mark.parametrize("model,family", list(SMALL))
def test_a_gated_frozen_frame_is_the_ungated_frozen_frame_on_the_survivors(model, family):
    """Every member's frame gets gross outliers in place of two detections (gating_util's); the oracle alone (its d^2 on
    the prior, far from the gate on either side) rejects them and keeps the rest.  The gated frozen frame is bit for bit the
    ungated frozen frame on the survivors, and a frame in which every detection is rejected is a frame that is not stepped."""
    n, m = SMALL[(model, family)]
    gate = gu.GATES[model]
    priors, frames = _dense_members(model, n, m, 8100, duplicate=False)
    rng = np.random.default_rng(5)
    dirty, kept, all_out = [], [], []
    for (state, p, lm_ids), fr in zip(priors, frames):
        poses = fr["poses"].copy()
        for j in (1, m - 1):
            poses[j] = gu._outlier(model, poses[j], rng, j)
        d2, _kappa = gu.block_distances(model, sw.oracle_at(QM[model], state, p, lm_ids), fr["ids"].tolist(), poses)
        rejected = d2 > gate
        assert rejected.sum() == 2 and (d2[rejected] > 10 * gate).all() and (d2[~rejected] < 0.5 * gate).all(), d2
        dirty.append(_frame(fr["ids"], poses))
        kept.append(_frame(fr["ids"][~rejected], poses[~rejected]))
        all_out.append(_frame(fr["ids"][rejected], poses[rejected]))
    gated = _frozen_batch(model, family, n, m, priors, gate=gate)
    plain = _frozen_batch(model, family, n, m, priors)
    got = gated.process_detection_logs(dirty, nis=True, cam_cov=True)
    want = plain.process_detection_logs(kept, nis=True, cam_cov=True)
    assert gated.status() == plain.status() == [0] * MEMBERS
    for b in range(MEMBERS):
        assert got.rejected[b].tolist() == [j in (1, m - 1) for j in range(m)], b
        assert got.dof[b][0] == gu.RD[model] * (m - 2)
        for name in ("trajectory", "nis", "cam_cov"):
            assert np.array_equal(getattr(got, name)[b], getattr(want, name)[b]), (name, b)
    sp.assert_same(sp.snap_batch(gated), sp.snap_batch(plain), "gated = ungated on the survivors", equal_nan=True)
    for b, (state, p, _ids) in enumerate(priors):      # (and the map did not move)
        assert np.array_equal(gated.get_cov(b)[CAM:, CAM:], p[CAM:, CAM:])
    # every detection rejected: not stepped
    before = sp.snap_batch(gated)
    out = gated.process_detection_logs(all_out, nis=True)
    sp.assert_same(sp.snap_batch(gated), before, "a frame of outliers only", equal_nan=True)
    for b in range(MEMBERS):
        assert out.rejected[b].all() and out.nis[b][0] == 0 and np.array_equal(out.trajectory[b][0], before[b][0][:7])


@pytest.mark.parametrize("model,family", list(SMALL))
def test_frozen_frames_compose_with_noise_rows_scale_and_motion(model, family):
    """noise rows all equal to c are r_uncertainty = c; an unstepped frozen frame leaves its scale pending and the next
    stepped one uses the sum; a frozen moved frame is the move followed by the frozen frame (the MOVED + FROZEN instance of
    the family's kernel).  Bit for bit, and the map keeps its bits."""
    import motion_util as mu
    n, m = SMALL[(model, family)]
    priors, frames = _dense_members(model, n, m, 8300)
    # per-detection noise
    c = 0.37
    rows = _frozen_batch(model, family, n, m, priors, row_noise=True)
    const = _frozen_batch(model, family, n, m, priors, noise={"r_uncertainty": c})
    rows.process_detection_logs([dict(f, noise=np.full(m, c)) for f in frames])
    const.process_detection_logs(frames)
    assert rows.status() == const.status() == [0] * MEMBERS
    sp.assert_same(sp.snap_batch(rows), sp.snap_batch(const), "noise rows", equal_nan=True)
    # frame scale
    s1, s2 = 1.75, 0.6
    scaled = _frozen_batch(model, family, n, m, priors, frame_scale=True)
    summed = _frozen_batch(model, family, n, m, priors, frame_scale=True)
    scaled.process_detection_logs([dict(EMPTY, scale=np.array([s1]))] * MEMBERS)
    assert scaled.pending_scale.tolist() == [s1] * MEMBERS and scaled.map_frozen.all()
    sp.assert_same(sp.snap_batch(scaled), [(s, p) for s, p, _ in priors], "an unstepped frozen frame", equal_nan=True)
    scaled.process_detection_logs([dict(f, scale=np.array([s2])) for f in frames])
    summed.process_detection_logs([dict(f, scale=np.array([s1 + s2])) for f in frames])
    assert scaled.pending_scale.tolist() == [0.0] * MEMBERS and scaled.status() == summed.status() == [0] * MEMBERS
    sp.assert_same(sp.snap_batch(scaled), sp.snap_batch(summed), "pending scale", equal_nan=True)
    assert not np.array_equal(scaled.get_cov(0)[:CAM], const.get_cov(0)[:CAM])
    # motion
    moves = [dict(EMPTY, motion=u[None, :]) for u in mu.STEP_MOTIONS.values()]
    steps = _frozen_batch(model, family, n, m, priors, motion=True)
    fused = _frozen_batch(model, family, n, m, priors, motion=True)
    traj = steps.process_detection_logs(moves)
    for b, (state, p, _ids) in enumerate(priors):      # (an unstepped frozen frame is still moved)
        assert np.array_equal(traj[b][0], steps.get_state(b)[:7]) and not np.array_equal(traj[b][0], state[:7])
    steps.process_detection_logs(frames)      # (no motions: the FROZEN instance without the stage)
    fused.process_detection_logs([dict(f, motion=mv["motion"]) for f, mv in zip(frames, moves)])
    assert steps.status() == fused.status() == [0] * MEMBERS
    sp.assert_same(sp.snap_batch(steps), sp.snap_batch(fused), "moved frozen frame", equal_nan=True)
    for batch in (rows, scaled, fused):
        for b, (state, p, _ids) in enumerate(priors):
            assert np.array_equal(batch.get_state(b)[CAM:], state[CAM:]) and np.array_equal(batch.get_cov(b)[CAM:, CAM:], p[CAM:, CAM:])
            assert np.array_equal(batch.get_cov(b), batch.get_cov(b).T)


# ---- 4. replicas ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", bu.MODELS)
def test_frozen_replicas_are_frozen_logs_of_the_poses_they_consumed(model):
    """All members frozen on the same restored map: replay_replicas equals process_detection_logs fed replica_poses(...) on
    a frozen twin, bit for bit; an id the map does not hold is dropped and reported; every member's map keeps its bits.
    Mixed flags raise ValueError and nothing changes."""
    from aruco_slam_amd.batch import replica_poses
    n, m = 6, 4
    state, p, lm_ids, ids, poses = sw.dense_prior(QM[model], n, m, 8500)
    ids2 = [ids[1], 77, ids[0], ids[3]]
    log = {"ids": np.array(ids + ids2, np.int64), "poses": np.vstack((poses, poses[[1, 2, 0, 3]] + 0.004)),
           "offsets": np.array([0, m, m, 2 * m], np.int64), "has_detections": np.array([True, False, True])}
    keep = log["ids"] != 77
    sigma = np.array([0.01, 0.01, 0.01, 0.002, 0.002, 0.002])
    batch, twin = bu.batch(model, "column", n, m), bu.batch(model, "column", n, m)
    for bt in (batch, twin):
        _restore(bt, [(state, p, lm_ids)] * MEMBERS)
    batch.freeze_map(1)
    before = sp.snap_batch(batch)
    with pytest.raises(ValueError, match="frozen"):
        batch.replay_replicas(log, sigma, 3)
    sp.assert_same(sp.snap_batch(batch), before, "mixed flags", equal_nan=True)
    for bt in (batch, twin):
        bt.freeze_map()
    got = batch.replay_replicas(log, sigma, 3, nis=True, cam_cov=True)
    assert batch.last_ignored == [(77,)] * MEMBERS and batch.status() == [0] * MEMBERS
    noisy = replica_poses(log["poses"][keep], sigma, 3, replicas=MEMBERS)
    kept_log = {"ids": log["ids"][keep], "offsets": np.array([0, m, m, 2 * m - 1], np.int64), "has_detections": log["has_detections"]}
    want = twin.process_detection_logs([dict(kept_log, poses=noisy[b]) for b in range(MEMBERS)], nis=True, cam_cov=True)
    for b in range(MEMBERS):
        assert np.array_equal(got.trajectory[b], want.trajectory[b]) and np.array_equal(got.nis[b], want.nis[b])
        assert np.array_equal(got.cam_cov[b], want.cam_cov[b])
        assert np.array_equal(batch.get_state(b)[CAM:], state[CAM:]) and np.array_equal(batch.get_cov(b)[CAM:, CAM:], p[CAM:, CAM:])
    sp.assert_same(sp.snap_batch(batch), sp.snap_batch(twin), "replicas", equal_nan=True)
    assert not np.array_equal(got.trajectory[0], got.trajectory[1])


def test_frozen_corner_replicas_are_frozen_logs_of_the_poses_they_consumed():
    from aruco_slam_amd.batch import replica_corner_poses
    from aruco_slam_amd.synthetic import corner_log
    k, dist, _c, _t, _r = synthetic_marker_views(1, seed=0)
    full = corner_log(12, (1, 4), 8, 5, k, dist, 0.16)
    boot = int(full["bootstrap_frames"])
    offs = full["offsets"]
    d = int(offs[boot])
    mapper = bu.batch("ekf", "column", 12, 16, members=1)
    mapper.process_detection_logs([{"ids": full["ids"][:d], "poses": full["poses_clean"][:d] + 0.0, "offsets": offs[:boot + 1],
                                    "has_detections": full["has_detections"][:boot]}])
    state, p = mapper.get_state(0), mapper.get_cov(0)
    lm_ids = [i for i, _ in sorted(mapper.landmarks[0].items(), key=lambda kv: kv[1])]
    log = {"ids": full["ids"][d:], "corners": full["corners"][d:], "offsets": offs[boot:] - d, "has_detections": full["has_detections"][boot:]}
    batch, twin = bu.batch("ekf", "column", 12, 16), bu.batch("ekf", "column", 12, 16)
    for bt in (batch, twin):
        _restore(bt, [(state, p, lm_ids)] * MEMBERS)
        bt.set_camera(k, dist, 0.16)
    batch.freeze_map(3)
    with pytest.raises(ValueError, match="frozen"):
        batch.replay_corner_replicas(log, 0.5, 9)
    for bt in (batch, twin):
        bt.freeze_map()
    got = batch.replay_corner_replicas(log, 0.5, 9, nis=True)
    poses = replica_corner_poses(log["corners"], 0.5, 9, k, dist, 0.16, replicas=MEMBERS)
    want = twin.process_detection_logs([{"ids": log["ids"], "poses": poses[b], "offsets": log["offsets"],
                                         "has_detections": log["has_detections"]} for b in range(MEMBERS)], nis=True)
    assert batch.status() == twin.status() == [0] * MEMBERS
    for b in range(MEMBERS):
        assert np.array_equal(got.trajectory[b], want.trajectory[b]) and np.array_equal(got.nis[b], want.nis[b])
        assert np.array_equal(batch.get_state(b)[CAM:], state[CAM:]) and np.array_equal(batch.get_cov(b)[CAM:, CAM:], p[CAM:, CAM:])
    sp.assert_same(sp.snap_batch(batch), sp.snap_batch(twin), "corner replicas", equal_nan=True)


# ---- 5. freeze -> unfreeze ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(bu.FAMILY))
def test_unfreezing_continues_like_a_restored_member(family):
    """After frozen frames and unfreeze_map(), a mapping log (with first sightings) gives the bits of a batch that set_member
    restores from the arrays read at that moment."""
    model = "ekf"
    logs = _plain(bu.ragged_logs(model))
    batch = bu.batch(model, family, 8, 8)
    batch.process_detection_logs([bu.part(log, 0, 3) for log in logs])      # (landmarks 0 .. 3 only)
    batch.freeze_map()
    batch.process_detection_logs([bu.part(log, 3, 12) for log in logs])     # (unknown ids are dropped)
    assert all(len(ig) > 0 for ig in batch.last_ignored) and batch.num_landmarks == [4] * MEMBERS
    batch.unfreeze_map()
    assert not batch.map_frozen.any()
    twin = bu.batch(model, family, 8, 8)
    for b, (s, p) in enumerate(sp.snap_batch(batch)):
        twin.set_member(b, s, p, [i for i, _ in sorted(batch.landmarks[b].items(), key=lambda kv: kv[1])])
    rest = [bu.part(log, 12, 30) for log in logs]
    got, want = batch.process_detection_logs(rest), twin.process_detection_logs(rest)
    assert batch.num_landmarks == twin.num_landmarks == [8] * MEMBERS and batch.status() == [0] * MEMBERS
    for b in range(MEMBERS):
        assert np.array_equal(got[b], want[b]), b
    sp.assert_same(sp.snap_batch(batch), sp.snap_batch(twin), "unfrozen", equal_nan=True)


# ---- 6. first sightings -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(bu.FAMILY))
def test_a_frozen_member_refuses_first_sightings(family):
    from aruco_slam_amd.batch import EkfError
    n, m = 6, 4
    priors, frames = _dense_members("ekf", n - 1, m, 8700)      # (5 landmarks: index 5 would be a first sighting)
    batch = bu.batch("ekf", family, n, m)
    _restore(batch, priors)
    batch.freeze_map(2)
    before, counts = sp.snap_batch(batch), batch._num_landmarks_device().tolist()
    idx = np.concatenate([f["ids"] for f in frames]).astype(np.int32)
    poses = np.vstack([f["poses"] for f in frames])
    fo, mf = np.arange(MEMBERS + 1) * m, np.arange(MEMBERS + 1)
    bad = idx.copy()
    bad[2 * m + 1] = 5
    with pytest.raises(EkfError) as err:
        batch.observe_indexed(bad, fo, mf, poses)
    assert err.value.code == -4 and "frozen" in str(err.value)      # EKF_ERR_STATE
    sp.assert_same(sp.snap_batch(batch), before, "refused call", equal_nan=True)
    assert batch._num_landmarks_device().tolist() == counts and batch.status() == [0] * MEMBERS
    assert batch.map_frozen.tolist() == [False, False, True, False]
    bad = idx.copy()
    bad[m + 1] = 5      # (a mapping member may sight it)
    batch.observe_indexed(bad, fo, mf, poses)
    assert batch._num_landmarks_device().tolist() == [5, 6, 5, 5]
    # process_detection_logs drops an unknown id, reports it, and is the log without that row
    batch, twin = bu.batch("ekf", family, n, m), bu.batch("ekf", family, n, m)
    for bt in (batch, twin):
        _restore(bt, priors)
        bt.freeze_map()
    with_unknown = [dict(f, ids=np.where(np.arange(m) == b % m, 900 + b, f["ids"])) for b, f in enumerate(frames)]
    out = batch.process_detection_logs(with_unknown, mahal=True)
    twin.process_detection_logs([_frame(np.delete(f["ids"], b % m), np.delete(f["poses"], b % m, axis=0))
                                 for b, f in enumerate(frames)])
    assert batch.last_ignored == [(900 + b,) for b in range(MEMBERS)] and batch.num_landmarks == [5] * MEMBERS
    for b in range(MEMBERS):
        assert np.isnan(out.mahal[b][b % m]) and np.isfinite(np.delete(out.mahal[b], b % m)).all() and not out.rejected[b].any()
    sp.assert_same(sp.snap_batch(batch), sp.snap_batch(twin), "dropped row", equal_nan=True)


# ---- 7. a frozen member that fails -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(bu.FAMILY))
def test_a_frozen_member_that_fails_keeps_state_and_covariance(family):
    from aruco_slam_amd.batch import EKF_ERR_NUMERIC
    n, m = 6, 4
    priors, frames = _dense_members("ekf", n, m, 8900)
    state, _p, lm_ids = priors[2]
    priors[2] = (state, -np.eye(len(state)), lm_ids)      # (S cannot be positive definite)
    batch = _frozen_batch("ekf", family, n, m, priors)
    twin = _frozen_batch("ekf", family, n, m, priors)
    out = batch.process_detection_logs(frames, nis=True, cam_cov=True)
    assert batch.status() == [0, 0, EKF_ERR_NUMERIC, 0]
    assert np.isnan(out.trajectory[2]).all() and np.isnan(out.nis[2]).all() and np.isnan(out.cam_cov[2]).all()
    assert np.array_equal(batch.get_state(2), state) and np.array_equal(batch.get_cov(2), -np.eye(len(state)))
    twin.set_member(2, *priors[0])      # (a healthy member in its place: the others do not notice)
    twin.process_detection_logs(frames)
    for b in (0, 1, 3):
        assert np.isfinite(out.trajectory[b]).all()
        assert np.array_equal(batch.get_state(b), twin.get_state(b)) and np.array_equal(batch.get_cov(b), twin.get_cov(b))


# ---- 8. batches that never freeze ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("family", list(bu.FAMILY))
@pytest.mark.parametrize("model", bu.MODELS)
def test_a_batch_that_never_freezes_has_the_parents_bits(model, family, moved):
    """tests/golden/batch_frozen_parent.npz: trajectory, NIS, state and P (member 0's) the commit before the batch's
    localisation mode computed over the 60-frame ragged logs (batch_frozen_util.record_parent; there the three families
    gave the same bits, so each array is stored once)."""
    golden = load_npz("batch_frozen_parent.npz")
    run = bu.never_frozen_run(model, family, moved)
    for name, v in run.items():
        want = golden[bu.parent_key(model, moved, name)]
        assert v.shape == want.shape and np.array_equal(v, want), (name, float(np.abs(v - want).max()))


# ---- 9. filters ------------------------------------------------------------------------------------------------------------------
def test_load_filter_and_to_filter_carry_the_flag():
    n, m = 6, 4
    priors, frames = _dense_members("ekf", n, m, 9100)
    batch = bu.batch("ekf", "column", n, m)
    _restore(batch, priors)
    batch.freeze_map(1)
    frozen, mapping = batch.to_filter(1), batch.to_filter(0)
    assert frozen.map_frozen and not mapping.map_frozen
    batch.load_filter(2, frozen)
    batch.load_filter(1, mapping)
    assert batch.map_frozen.tolist() == [False, False, True, False]
    assert np.array_equal(batch.get_state(2), priors[1][0]) and np.array_equal(batch.get_cov(2), priors[1][1])
    # the frozen filter and the frozen member step alike: camera moves, the map does not
    fr = frames[1]
    frozen.observe(fr["ids"].tolist(), fr["poses"])
    batch.process_detection_logs([None, None, fr, None])
    s, p = batch.get_state(2), batch.get_cov(2)
    assert np.array_equal(s[CAM:], priors[1][0][CAM:]) and np.array_equal(p[CAM:, CAM:], priors[1][1][CAM:, CAM:])
    assert rel_err(s, np.asarray(frozen.state)) <= 1e-9 and rel_err(p, np.asarray(frozen.uncertainty)) <= 1e-9
    batch.reset(2)
    assert not batch.map_frozen.any()
