"""Batch of independent EKF_Rotations filters (``EKFBatch(model="ekf_rotations")``, kernel ekf_batch_rot.hip) on an MI355X:
teacher-forced steps and a free run against the reference's G5 fixtures, the extended-precision step, the single-filter path,
composition and window independence, the covariance and quaternion invariants, failure isolation, host validation and
interop with ``EKF_Rotations``."""
import numpy as np
import pytest

import support as sp
import update_sweep_util as sw
from conftest import load_npz, rel_err, rel_err_elem, report

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
STEP_TOL, ELEM_TOL = 1e-10, 1e-9       # f64, as test_hip_parity.py
# (c_P, c_x) of the rotations batch against the extended-precision step: 4x the worst ratio measured on an MI355X (0.78 at
# n = 24, m = 2; 1.88 at n = 12, m = 1).  c_x is looser than the EKF batch's 2.8: DESIGN section 4.7.1 says why.
C_ROT_BATCH = (3.2, 7.6)


def _batch(members, **kw):
    from aruco_slam_amd.batch import EKFBatch
    kw.setdefault("max_landmarks", 24)
    kw.setdefault("max_visible", 8)
    return EKFBatch(members, INIT, model="ekf_rotations", **kw)


def _frame_log(ids, poses):
    ids = np.asarray(ids, dtype=np.int32)
    return {"ids": ids, "poses": np.asarray(poses, dtype=np.float64), "offsets": np.array([0, len(ids)], dtype=np.int64)}


def _ragged(n, m_range, steady, seed):
    from aruco_slam_amd.synthetic import ragged_log
    return ragged_log(n, m_range, steady, seed=seed, rvec_sigma=0.05)


def _g5_log():
    g = load_npz("g5_detections.npz")
    return {k: g[k] for k in ("ids", "poses", "offsets", "has_detections")}


def _snapshot(batch, b):
    return batch.get_state(b), batch.get_cov(b)


def _worst(batch, want):
    worst = np.zeros(4)
    for b, (s1, p1) in enumerate(want):
        s, p = _snapshot(batch, b)
        assert s.shape == s1.shape and p.shape == p1.shape
        worst = np.maximum(worst, [rel_err(s, s1), rel_err(p, p1), rel_err_elem(s, s1), rel_err_elem(p, p1)])
    return worst


def test_g5_teacher_forced_every_frame_as_a_member_in_one_call():
    g = load_npz("g5_rotations.npz")
    frames, offs = list(g["frames"]), g["offsets"]
    batch = _batch(len(frames), max_landmarks=8)
    for b, f in enumerate(frames):
        batch.set_member(b, g[f"f{f}_state0"], g[f"f{f}_P0"], g[f"f{f}_lm_ids"])
    batch.process_detection_logs([_frame_log(g["ids"][offs[f]:offs[f + 1]], g["poses"][offs[f]:offs[f + 1]])
                                  for f in frames])
    assert batch.status() == [0] * len(frames)
    worst = _worst(batch, [(g[f"f{f}_state1"], g[f"f{f}_P1"]) for f in frames])
    report("batch_rot_g5_teacher_forced", members=len(frames), state_norm=worst[0], cov_norm=worst[1],
           state_elem=worst[2], cov_elem=worst[3])
    assert worst[0] <= STEP_TOL and worst[1] <= STEP_TOL, worst
    assert worst[2] <= ELEM_TOL and worst[3] <= ELEM_TOL, worst


def test_g5_free_run_in_one_member_of_a_larger_batch():
    g = load_npz("g5_rotations.npz")
    logs = [_ragged(n, (1, min(n, 8)), 40, seed=s) for s, n in enumerate((3, 24, 8, 17, 12, 24, 5, 20))]
    logs[5] = _g5_log()
    batch = _batch(8)
    cams = batch.process_detection_logs(logs)[5]
    assert batch.status() == [0] * 8
    errs = {"cam": rel_err(cams, g["cam"]), "state": rel_err(batch.get_state(5), g["final_state"]),
            "cov": rel_err(batch.get_cov(5), g["final_P"]),
            "lm_unc": rel_err(batch.get_lm_uncertainties(5), np.diagonal(g["final_P"])[10:].reshape(-1, 10))}
    report("batch_rot_g5_free_run", **errs)
    assert max(errs.values()) <= 1e-9, errs
    assert list(batch.landmarks[5].keys()) == list(g["lm_ids"])
    cam, lms = batch.get_poses(5)
    assert cam.shape == (10,) and lms.shape == (len(g["lm_ids"]), 10)


def test_batch_members_against_the_extended_reference():
    """One call, 16 members: member j sees m = 1..8 detections from its own dense prior, at n = 1, 12 and 24."""
    keys = [sw.RefKey("rot", (1, 12, 24)[j % 3], (j - 1) % 8 + 1, "float64", "scalar_first") for j in range(1, 17)]
    got = sw.references(keys)
    batch = _batch(len(keys))
    logs = []
    for b, key in enumerate(keys):
        state, p, lm_ids, ids, poses = got[key][0]
        batch.set_member(b, state, p, lm_ids)
        logs.append(_frame_log(ids, poses))
    batch.process_detection_logs(logs)
    assert batch.status() == [0] * len(keys)
    worst, at = np.zeros(2), [None, None]
    for b, key in enumerate(keys):
        ref = got[key][1]
        assert ref["kappa"] <= sw.KAPPA_MAX
        p = batch.get_cov(b)
        assert np.array_equal(p, p.T)
        r = sw.ratios(ref, p, batch.get_state(b), "float64")
        for i in range(2):
            if r[i] > worst[i]:
                worst[i], at[i] = r[i], f"n={key.n},m={key.m}"
    c_p, c_x = C_ROT_BATCH
    report("update_sweep[batch_rot,float64]", members=len(keys), ratio_P=worst[0], ratio_x=worst[1], worst_P_at=at[0],
           worst_x_at=at[1], c_P=c_p, c_x=c_x)
    assert worst[0] <= c_p and worst[1] <= c_x, worst


def _horizon(a, b, envelope=1e-8):
    d = np.abs(a - b).max(axis=1)
    bad = np.nonzero(d > envelope)[0]
    return int(bad[0]) - 1 if len(bad) else len(d) - 1


def test_against_the_single_filter_path():
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    log = _ragged(24, (1, 8), 200, seed=31)

    def single(poses):
        flt = EKF_Rotations(INIT, max_landmarks=24, max_visible=8, cov_dtype="float64")
        return flt.process_detection_log(log["ids"], poses, log["offsets"], log["has_detections"]), flt.landmarks

    want, table = single(log["poses"])
    rng = np.random.default_rng(31)
    pert, _ = single(log["poses"] * (1.0 + 1e-15 * rng.standard_normal(log["poses"].shape)))
    hz = _horizon(want, pert)
    batch = _batch(3)
    got = batch.process_detection_logs([None, log, _ragged(10, (1, 8), 30, seed=2)])[1]
    err = float(np.abs(got[:hz + 1] - want[:hz + 1]).max())
    report("batch_rot_vs_single[n=24,m=(1,8)]", horizon=hz, frames=len(want), max_abs=err)
    assert hz >= 50, hz
    assert err <= 1e-6, err
    assert batch.landmarks[1] == table


def test_composition_independence_bitwise():
    log = _ragged(24, (1, 8), 80, seed=3)
    others = [_ragged(n, (1, min(n, 8)), 30, seed=s) for s, n in enumerate((6, 24, 13, 1))] + [None]
    runs = []
    for B, slots in ((1, (0,)), (7, (3,)), (300, (5, 299))):
        logs = [others[i % len(others)] for i in range(B)]
        for s in slots:
            logs[s] = log
        batch = _batch(B)
        traj = batch.process_detection_logs(logs)
        for s in slots:
            runs.append((traj[s], *_snapshot(batch, s)))
        del batch
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b)


def test_continuation_across_calls_and_windows_is_bitwise():
    log = _ragged(24, (1, 8), 200, seed=5)
    frames = len(log["offsets"]) - 1
    assert frames > 3 * 64
    one = _batch(2)
    t_one = one.process_detection_logs([log, None])[0]
    two = _batch(2)
    cut = 100                                     # inside the second window
    t_a = two.process_detection_logs([sp.sub_log(log, 0, cut), None])[0]
    t_b = two.process_detection_logs([sp.sub_log(log, cut, frames), None])[0]
    assert np.array_equal(t_one, np.concatenate([t_a, t_b]))
    for a, b in zip(_snapshot(one, 0), _snapshot(two, 0)):
        assert np.array_equal(a, b)
    assert one.landmarks[0] == two.landmarks[0]


def test_covariance_symmetric_padding_zero_and_landmark_quaternions():
    logs = [_ragged(n, (1, min(n, 8)), 60, seed=n) for n in (1, 5, 13, 24)]
    batch = _batch(4)
    batch.process_detection_logs(logs)
    assert batch.status() == [0] * 4
    P = batch.cov_t.cpu().numpy()
    S = batch.state_t.cpu().numpy()
    assert P.shape[1] == 256
    for b in range(4):
        n = batch.num_landmarks[b]
        N = 10 * n + 10
        assert np.array_equal(P[b], P[b].T)
        assert not P[b, N:, :].any() and not P[b, :, N:].any() and not S[b, N:].any()
        assert np.isfinite(P[b, :N, :N]).all()
        cam, lms = batch.get_poses(b)
        assert lms.shape == (n, 10)
        assert not lms[:, 7:10].any()                     # the landmarks' error states are never written
        assert not cam[7:10].any()                        # the camera's is reset every update
        assert np.abs(np.linalg.norm(lms[:, 3:7], axis=1) - 1.0).max() <= 1e-12
        assert batch.get_lm_uncertainties(b).shape == (n, 10)


def test_non_finite_pose_stops_only_its_member():
    from aruco_slam_amd.batch import EKF_ERR_NUMERIC
    logs = [_ragged(16, (1, 8), 40, seed=s) for s in range(4)]
    bad_log = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in logs[2].items()}
    t_bad_frame = 1                                   # a bootstrap frame: its detections are first sightings
    bad_log["poses"][int(bad_log["offsets"][t_bad_frame]), 0] = np.nan
    ref = _batch(4)
    bad = _batch(4)
    t_ref = ref.process_detection_logs([logs[0], logs[1], None, logs[3]])
    t_bad = bad.process_detection_logs([logs[0], logs[1], bad_log, logs[3]])
    assert bad.status() == [0, 0, EKF_ERR_NUMERIC, 0]
    assert np.isfinite(t_bad[2][:t_bad_frame]).all()
    assert np.isnan(t_bad[2][t_bad_frame:]).all() and t_bad[2].shape[0] == len(bad_log["offsets"]) - 1
    for b in (0, 1, 3):
        assert np.array_equal(t_ref[b], t_bad[b])
        for a, c in zip(_snapshot(ref, b), _snapshot(bad, b)):
            assert np.array_equal(a, c)
    bad.reset(2)
    assert bad.status() == [0, 0, 0, 0] and bad.num_landmarks[2] == 0


def test_bad_logs_raise_before_anything_runs():
    from aruco_slam_amd.hip_backend import EkfError
    logs = [_ragged(12, (1, 8), 10, seed=s) for s in range(3)]
    batch = _batch(3)
    batch.process_detection_logs(logs)
    before = [_snapshot(batch, b) for b in range(3)]
    tables = [dict(t) for t in batch.landmarks]
    step = _ragged(12, (1, 8), 3, seed=9)
    cases = [
        ("malformed_log", lambda: batch.process_detection_logs([None, dict(step, offsets=step["offsets"][::-1]), None]),
         ValueError),
        ("bad_poses", lambda: batch.process_detection_logs([None, dict(step, poses=step["poses"][:, :3]), None]),
         ValueError),
        ("too_wide", lambda: batch.process_detection_logs([None, _frame_log(np.arange(9) % 5, np.ones((9, 6))), None]),
         EkfError),
        ("too_many_landmarks", lambda: batch.process_detection_logs([_ragged(25, (1, 8), 2, seed=1), None, None]),
         EkfError),
    ]
    for name, call, exc in cases:
        with pytest.raises(exc) as info:
            call()
        if exc is EkfError:
            assert info.value.code == -2, name
        assert batch.landmarks == tables, name
        for b in range(3):
            for a, c in zip(before[b], _snapshot(batch, b)):
                assert np.array_equal(a, c), name
        assert batch.status() == [0, 0, 0]


def test_interop_with_ekf_rotations():
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations, Q_UNCERTAINTY_CAM
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    noise = {"r_uncertainty": np.array([0.9, 0.5]), "q_lm": np.array([0.01, 0.02])}
    batch = _batch(2, max_landmarks=12, noise=noise)
    assert batch.noise[0, 3] == Q_UNCERTAINTY_CAM == 0.2 and batch.quat_update == "scalar_first"
    log = _ragged(12, (1, 8), 20, seed=21)
    batch.process_detection_logs([log, log])
    with pytest.raises(ValueError, match="EKF"):
        batch.load_filter(0, EKF(INIT, max_landmarks=12, max_visible=8, quat_update="scalar_first"))
    # to_filter: the member as an ordinary EKF_Rotations with its noise constants, bit for bit
    flt = batch.to_filter(1)
    assert isinstance(flt, EKF_Rotations)
    assert (flt.backend.cfg.r_uncertainty, flt.backend.cfg.q_lm, flt.backend.cfg.q_cam) == (0.5, 0.02, 0.2)
    assert np.array_equal(np.asarray(flt.state), batch.get_state(1)) and np.array_equal(flt.uncertainty, batch.get_cov(1))
    assert flt.landmarks == batch.landmarks[1] and flt.num_landmarks == batch.num_landmarks[1]
    # one more frame, in the filter and in the batch
    nxt = sp.sub_log(_ragged(12, (1, 8), 3, seed=22), 3, 4)
    flt.observe(nxt["ids"], nxt["poses"])
    got = batch.process_detection_logs([None, nxt])[1][-1]
    assert rel_err(got, np.asarray(flt.state)[:7]) <= 1e-10
    assert rel_err(batch.get_state(1), np.asarray(flt.state)) <= 1e-10
    assert rel_err(batch.get_cov(1), flt.uncertainty) <= 1e-10
    # load_filter round trip
    batch.load_filter(0, flt)
    assert np.array_equal(batch.get_state(0), np.asarray(flt.state)) and np.array_equal(batch.get_cov(0), flt.uncertainty)
    assert batch.landmarks[0] == flt.landmarks
    back = batch.to_filter(0)
    assert np.array_equal(np.asarray(back.state), np.asarray(flt.state)) and np.array_equal(back.uncertainty, flt.uncertainty)
    assert back.backend.cfg.r_uncertainty == 0.9            # member 0 keeps its own constants
