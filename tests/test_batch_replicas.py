"""Monte-Carlo replicas of one log (``EKFBatch.replay_replicas``, ``replica_poses``) and the per-frame NIS / camera
covariance outputs of every batch window kernel, on an MI355X: the same bits with and without the outputs, replicas equal
to explicit logs of the poses they consumed, replica identity across batch sizes and calls, the device noise against the
NumPy mirror and its statistics, NIS and P[0:10, 0:10] against the oracle, and the edges (empty frames, failing members,
bad arguments)."""
import numpy as np
import pytest

import replica_util as ru
import support as sp
from conftest import load_npz, rel_err_elem, report

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
# (model, family): the batch's keyword arguments and the log shape that exercises it
FAMILIES = {
    ("ekf", "column"): ({"max_landmarks": 24, "max_visible": 16}, 24, (1, 12)),
    ("ekf_rotations", "column"): ({"max_landmarks": 12, "max_visible": 8}, 12, (1, 6)),
    ("ekf", "large"): ({"max_landmarks": 24, "max_visible": 16, "large_maps": True}, 24, (1, 12)),
    ("ekf_rotations", "large"): ({"max_landmarks": 12, "max_visible": 8, "large_maps": True}, 12, (1, 6)),
    ("ekf", "wide"): ({"max_landmarks": 40, "max_visible": 40, "wide_frames": True}, 40, (10, 36)),
    ("ekf_rotations", "wide"): ({"max_landmarks": 20, "max_visible": 20, "wide_frames": True}, 20, (4, 18)),
}


def _batch(members, model="ekf", **kw):
    from aruco_slam_amd.batch import EKFBatch
    return EKFBatch(members, INIT, model=model, **kw)


def _ragged(model, n, m_range, steady, seed):
    from aruco_slam_amd.synthetic import ragged_log
    log = ragged_log(n, m_range, steady, seed=seed, rvec_sigma=0.05 if model == "ekf_rotations" else 0.0)
    log["poses"] = log["poses"] + 0.0        # (no -0.0 entries: -0.0 + 0 * g is +0.0)
    return log


def _family(model, family, members, steady=30, seed=0):
    kw, n, m_range = FAMILIES[(model, family)]
    return _batch(members, model, **kw), _ragged(model, n, m_range, steady, seed)


@pytest.mark.parametrize("model,family", list(FAMILIES))
def test_outputs_do_not_change_the_bits(model, family):
    kw, n, m_range = FAMILIES[(model, family)]
    logs = [_ragged(model, n, m_range, 25, seed=s) for s in range(5)] + [None]
    plain, diag = _batch(6, model, **kw), _batch(6, model, **kw)
    t_plain = plain.process_detection_logs(logs)
    out = diag.process_detection_logs(logs, nis=True, cam_cov=True)
    assert plain.status() == diag.status() == [0] * 6
    for a, b in zip(t_plain, out.trajectory):
        assert np.array_equal(a, b)
    sp.assert_same(sp.snap_batch(plain), sp.snap_batch(diag), "state / P", equal_nan=True)
    for b in range(5):
        # (a bootstrap frame only first-sights its landmarks: each is placed at its detection, so z - h = 0 and NIS = 0)
        boot = logs[b]["bootstrap_frames"]
        assert np.isfinite(out.nis[b]).all() and (out.nis[b] >= 0).all() and (out.nis[b][boot:] > 0).all()
        assert np.array_equal(out.dof[b], (3 if model == "ekf" else 7) * np.diff(logs[b]["offsets"]))


@pytest.mark.parametrize("model,family", list(FAMILIES))
def test_replicas_equal_explicit_logs_of_their_poses(model, family):
    from aruco_slam_amd.batch import replica_poses
    B, seed, r0 = 6, 0x5EED_0000_0000_0042, 3
    batch, log = _family(model, family, B, seed=7)
    sigma = np.random.default_rng(1).uniform(0.002, 0.02, (B, 6))
    got = batch.replay_replicas(log, sigma, seed, first_replica=r0, nis=True, cam_cov=True)
    poses = replica_poses(log["poses"], sigma, seed, first_replica=r0)
    assert poses.shape == (B, log["poses"].shape[0], 6)
    mirror = ru.replica_poses(log["poses"], sigma, seed, B, r0)
    assert np.abs(poses - mirror).max() <= 1e-13
    explicit, _ = _family(model, family, B)
    want = explicit.process_detection_logs([dict(log, poses=poses[b]) for b in range(B)], nis=True, cam_cov=True)
    assert batch.status() == explicit.status() == [0] * B
    assert np.array_equal(got.trajectory, np.stack(want.trajectory))
    assert np.array_equal(got.nis, np.stack(want.nis))
    assert np.array_equal(got.cam_cov, np.stack(want.cam_cov))
    assert np.array_equal(got.dof, want.dof[0])
    sp.assert_same(sp.snap_batch(batch), sp.snap_batch(explicit), "state / P", equal_nan=True)
    assert batch.landmarks == explicit.landmarks
    # replicas differ from each other (sigma > 0)
    assert not np.array_equal(got.trajectory[0], got.trajectory[1])


@pytest.mark.parametrize("model", ["ekf", "ekf_rotations"])
def test_zero_sigma_is_the_plain_log_replay(model):
    B = 4
    batch, log = _family(model, "column", B, seed=3)
    plain, _ = _family(model, "column", B)
    got = batch.replay_replicas(log, 0.0, 99, nis=True, cam_cov=True)
    want = plain.process_detection_logs([log] * B, nis=True, cam_cov=True)
    assert np.array_equal(got.trajectory, np.stack(want.trajectory))
    assert np.array_equal(got.nis, np.stack(want.nis)) and np.array_equal(got.cam_cov, np.stack(want.cam_cov))
    sp.assert_same(sp.snap_batch(batch), sp.snap_batch(plain), "state / P", equal_nan=True)


def test_replica_identity_across_batch_sizes_and_calls():
    seed = 2024
    sigma = np.random.default_rng(5).uniform(0.0, 0.02, (16, 6))
    big, log = _family("ekf", "column", 16, seed=11)
    whole = big.replay_replicas(log, sigma, seed, nis=True, cam_cov=True)
    parts, snaps = [], []
    for r0 in (0, 8, 4):
        part, _ = _family("ekf", "column", 8)
        parts.append(part.replay_replicas(log, sigma[r0:r0 + 8], seed, first_replica=r0, nis=True, cam_cov=True))
        snaps.append(sp.snap_batch(part))
    big_snap = sp.snap_batch(big)
    for (r0, part, snap) in zip((0, 8, 4), parts, snaps):
        sl = slice(r0, r0 + 8)
        assert np.array_equal(part.trajectory, whole.trajectory[sl])
        assert np.array_equal(part.nis, whole.nis[sl]) and np.array_equal(part.cam_cov, whole.cam_cov[sl])
        sp.assert_same(snap, big_snap[sl], f"members {r0}..{r0 + 7}", equal_nan=True)


def test_device_normals_match_the_mirror_and_are_standard_normal():
    from aruco_slam_amd.batch import replica_poses
    R, D = 128, 1400                    # 1,075,200 samples
    seed, r0 = 0x1234_5678_9ABC_DEF0, 2 ** 32 - R      # (both key words and the top replica numbers in use)
    g = replica_poses(np.zeros((D, 6)), 1.0, seed, replicas=R, first_replica=r0)
    want = ru.normals(seed, np.arange(r0, r0 + R), np.arange(D))
    err = float(np.abs(g - want).max())
    n = g.size
    mean, var = float(g.mean()), float(g.var())
    comp = np.corrcoef(g[..., :5].reshape(-1), g[..., 1:].reshape(-1))[0, 1]
    adj = np.corrcoef(g[:-1].reshape(-1), g[1:].reshape(-1))[0, 1]
    det = np.corrcoef(g[:, :-1].reshape(-1), g[:, 1:].reshape(-1))[0, 1]
    report("replica_normals", samples=n, max_abs_vs_mirror=err, mean=mean, var=var, corr_components=comp,
           corr_adjacent_replicas=adj, corr_adjacent_detections=det)
    assert err <= 4e-15, err      # (measured on an MI355X: 6.7e-16 over 1,075,200 samples)
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n)
    for c in range(6):
        gc = g[..., c].reshape(-1)
        assert abs(gc.mean()) <= 5 / np.sqrt(gc.size) and abs(gc.var() - 1) <= 5 * np.sqrt(2 / gc.size), c
    assert abs(comp) <= 5 / np.sqrt(g[..., :5].size)
    assert abs(adj) <= 5 / np.sqrt(g[:-1].size) and abs(det) <= 5 / np.sqrt(g[:, :-1].size)


def _oracle_chain_c1():
    """(prior state, prior P, prior marker ids, frame ids, frame poses, posterior P) of every stepped C1 frame."""
    from oracle.ekf_numpy import OracleEKF
    det = load_npz("c1_detections.npz")
    offs = det["offsets"]
    orc = OracleEKF(INIT, mode="fast")
    out = []
    for f in range(len(offs) - 1):
        if not det["has_detections"][f]:
            continue
        sl = slice(offs[f], offs[f + 1])
        ids, poses = list(det["ids"][sl]), det["poses"][sl]
        lm_ids = [k for k, _ in sorted(orc.landmarks.items(), key=lambda kv: kv[1])]
        prior = (np.asarray(orc.state, dtype=np.float64).copy(), np.array(orc.uncertainty, dtype=np.float64), lm_ids)
        orc.observe(ids, poses)
        out.append(prior + (ids, poses, np.array(orc.uncertainty)))
    return out


def _g5_frames():
    g = load_npz("g5_rotations.npz")
    offs = g["offsets"]
    return [(g[f"f{f}_state0"], g[f"f{f}_P0"], list(g[f"f{f}_lm_ids"]), list(g["ids"][offs[f]:offs[f + 1]]),
             g["poses"][offs[f]:offs[f + 1]], g[f"f{f}_P1"]) for f in g["frames"]]


@pytest.mark.parametrize("case", ["c1", "g5"])
def test_nis_and_cam_cov_against_the_oracle_teacher_forced(case):
    from oracle.ekf_extended import extended_step
    from update_sweep_util import oracle_at
    frames = _oracle_chain_c1() if case == "c1" else _g5_frames()
    model = "ekf" if case == "c1" else "ekf_rotations"
    batch = _batch(len(frames), model, max_landmarks=16 if case == "c1" else 8, max_visible=8)
    for b, (s0, p0, lm, *_rest) in enumerate(frames):
        batch.set_member(b, s0, p0, lm)
    logs = [{"ids": np.asarray(f[3], np.int32), "poses": np.asarray(f[4], np.float64),
             "offsets": np.array([0, len(f[3])], np.int64)} for f in frames]
    out = batch.process_detection_logs(logs, nis=True, cam_cov=True)
    assert batch.status() == [0] * len(frames)
    worst_nis, worst_cov, checked = 0.0, 0.0, 0
    for b, (s0, p0, lm, ids, poses, p1) in enumerate(frames):
        worst_cov = max(worst_cov, rel_err_elem(out.cam_cov[b][0], p1[:10, :10]))
        assert out.dof[b][0] == (3 if model == "ekf" else 7) * len(ids)
        if not set(int(i) for i in ids) <= set(int(i) for i in lm):
            continue        # (first sightings: the oracle's prior does not hold the new landmark yet)
        qm = "rot" if model == "ekf_rotations" else "ekf"
        ref = extended_step(oracle_at(qm, s0, p0, lm), ids, poses, factors=True)
        z, h, _j, _c = oracle_at(qm, s0, p0, lm).measurement_blocks(ids, poses)
        r = z - h
        want = float(r @ np.linalg.solve(ref["S"], r))
        rel = abs(out.nis[b][0] - want) / abs(want)
        tol = max(1e-9, 100 * ref["kappa"] * 2.0 ** -52)
        assert rel <= tol, (b, rel, tol)
        worst_nis = max(worst_nis, rel / tol)
        checked += 1
    report(f"replica_nis_cam_cov_{case}", members=len(frames), nis_checked=checked, nis_worst_over_tol=worst_nis,
           cam_cov_elem=worst_cov)
    assert checked >= 3, checked
    assert worst_cov <= 1e-9, worst_cov


def test_nis_is_bitwise_equal_across_kernels():
    log = _ragged("ekf", 24, (1, 12), 40, seed=17)
    outs = []
    for extra in ({}, {"large_maps": True}, {"wide_frames": True}):
        batch = _batch(2, "ekf", max_landmarks=24, max_visible=16, **extra)
        outs.append(batch.process_detection_logs([log, None], nis=True, cam_cov=True))
    ref = outs[0]
    for other in outs[1:]:
        same = (ref.trajectory[0] == other.trajectory[0]).all(axis=1)
        report("replica_nis_across_kernels", frames=len(same), agreeing=int(same.sum()))
        assert same.any()
        assert np.array_equal(ref.nis[0][same], other.nis[0][same])
        assert np.array_equal(ref.cam_cov[0][same], other.cam_cov[0][same])


@pytest.mark.parametrize("model,family", [("ekf", "column"), ("ekf_rotations", "wide")])
def test_cam_cov_is_the_covariance_after_each_frame(model, family):
    kw, n, m_range = FAMILIES[(model, family)]
    log = _ragged(model, n, m_range, 8, seed=23)
    F = len(log["offsets"]) - 1
    whole = _batch(1, model, **kw).process_detection_logs([log], cam_cov=True)
    step = _batch(1, model, **kw)
    for t in range(F):
        step.process_detection_logs([sp.sub_log(log, t, t + 1)])
        assert np.array_equal(whole.cam_cov[0][t], step.get_cov(0)[:10, :10]), t


def test_empty_frames_and_failing_members():
    from aruco_slam_amd.batch import EKF_ERR_NUMERIC
    logs = [_ragged("ekf", 20, (1, 8), 30, seed=s) for s in range(4)]
    boot = [sp.sub_log(lg, 0, 10) for lg in logs]
    rest = [sp.sub_log(lg, 10, len(lg["offsets"]) - 1) for lg in logs]
    # empty frames: a leading one, and two in the middle
    lg = rest[0]
    offs = lg["offsets"]
    rest[0] = {"ids": lg["ids"], "poses": lg["poses"],
               "offsets": np.concatenate(([0], offs[:4], offs[3:5], offs[4:])),
               "has_detections": np.concatenate(([False], lg["has_detections"][:3], [False], lg["has_detections"][3:4],
                                                 [False], lg["has_detections"][4:]))}
    ref, bad = _batch(4, max_landmarks=20, max_visible=16), _batch(4, max_landmarks=20, max_visible=16)
    for batch in (ref, bad):
        batch.process_detection_logs(boot)
    cov0 = ref.get_cov(0)[:10, :10]
    ids = [k for k, _ in sorted(bad.landmarks[2].items(), key=lambda kv: kv[1])]
    s0 = bad.get_state(2)
    bad.set_member(2, s0, -np.eye(s0.shape[0]), ids)       # (S cannot be positive definite)
    want = ref.process_detection_logs([rest[0], rest[1], None, rest[3]], nis=True, cam_cov=True)
    got = bad.process_detection_logs(rest, nis=True, cam_cov=True)
    assert bad.status() == [0, 0, EKF_ERR_NUMERIC, 0]
    empty = np.nonzero(np.diff(rest[0]["offsets"]) == 0)[0]
    assert list(empty) == [0, 4, 6]
    nis, dof, cc = want.nis[0], want.dof[0], want.cam_cov[0]
    assert (nis[empty] == 0).all() and (dof[empty] == 0).all() and (nis[dof > 0] > 0).all()
    assert np.array_equal(cc[0], cov0)
    for t in empty[1:]:
        assert np.array_equal(cc[t], cc[t - 1])
    assert np.isnan(got.nis[2]).all() and np.isnan(got.cam_cov[2]).all() and np.isnan(got.trajectory[2]).all()
    for b in (0, 1, 3):
        assert np.array_equal(got.nis[b], want.nis[b]) and np.array_equal(got.cam_cov[b], want.cam_cov[b])
        assert np.array_equal(got.trajectory[b], want.trajectory[b])


def test_bad_replica_arguments_raise_before_anything_runs():
    from aruco_slam_amd.hip_backend import EkfError
    batch, log = _family("ekf", "column", 3, steady=5, seed=2)
    batch.replay_replicas(sp.sub_log(log, 0, 4), 0.01, 1)
    before, tables = sp.snap_batch(batch), [dict(t) for t in batch.landmarks]
    wide = _ragged("ekf", 40, (20, 30), 2, seed=4)
    cases = [
        ("negative", lambda: batch.replay_replicas(log, -0.1, 1), ValueError),
        ("nan", lambda: batch.replay_replicas(log, np.full(6, np.nan), 1), ValueError),
        ("shape", lambda: batch.replay_replicas(log, np.ones((2, 6)), 1), ValueError),
        ("first_replica", lambda: batch.replay_replicas(log, 0.01, 1, first_replica=2 ** 32 - 2), ValueError),
        ("capacity", lambda: batch.replay_replicas(wide, 0.01, 1), EkfError),
    ]
    for name, call, exc in cases:
        with pytest.raises(exc) as info:
            call()
        if exc is EkfError:
            assert info.value.code == -2, name
        assert batch.landmarks == tables, name
        sp.assert_same(before, sp.snap_batch(batch), name, equal_nan=True)
        assert batch.status() == [0, 0, 0]
    batch.reset(1)
    with pytest.raises(ValueError, match="landmark table"):
        batch.replay_replicas(log, 0.01, 1)
    assert batch.landmarks[0] == tables[0] and batch.num_landmarks[1] == 0
    sp.assert_same(before[::2], sp.snap_batch(batch)[::2], "unequal tables", equal_nan=True)
