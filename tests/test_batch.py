"""Batch of independent filters (``aruco_slam_amd.batch.EKFBatch``, ekf_batch_* C ABI) on an MI355X: teacher-forced steps
against the NumPy oracle and the reference goldens, a free run, the single-filter path, composition and window
independence, the covariance invariants, failure isolation, host validation and interop with ``EKF``."""
import numpy as np
import pytest

import support as sp
from conftest import chaos_horizon, load_npz, rel_err, rel_err_elem, report

pytestmark = pytest.mark.gpu

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
STEP_TOL, ELEM_TOL = 1e-10, 1e-9       # f64, as test_hip_parity.py


def _batch(members, **kw):
    from aruco_slam_amd.batch import EKFBatch
    return EKFBatch(members, INIT, **kw)


def _c1():
    det = load_npz("c1_detections.npz")
    return {k: det[k] for k in ("ids", "poses", "offsets", "has_detections")}


def _frame_log(ids, poses):
    ids = np.asarray(ids, dtype=np.int32)
    return {"ids": ids, "poses": np.asarray(poses, dtype=np.float64), "offsets": np.array([0, len(ids)], dtype=np.int64)}


def _ragged(n, m_range, steady, seed):
    from aruco_slam_amd.synthetic import ragged_log
    return ragged_log(n, m_range, steady, seed=seed)


def _oracle_chain_c1():
    """(prior state, prior P, prior marker ids, frame ids, frame poses, posterior state, posterior P) of every stepped C1
    frame, the oracle stepping its own chain."""
    from oracle.ekf_numpy import OracleEKF
    det = _c1()
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
        out.append(prior + (ids, poses, np.asarray(orc.state, dtype=np.float64).copy(), np.array(orc.uncertainty)))
    return out


def _worst(batch, members, want):
    worst = np.zeros(4)
    for b, (s1, p1) in zip(members, want):
        s, p = batch.get_state(b), batch.get_cov(b)
        assert s.shape == s1.shape and p.shape == p1.shape
        worst = np.maximum(worst, [rel_err(s, s1), rel_err(p, p1), rel_err_elem(s, s1), rel_err_elem(p, p1)])
    return worst


def test_c1_teacher_forced_every_frame_as_a_member_in_one_call():
    chain = _oracle_chain_c1()
    batch = _batch(len(chain), max_landmarks=16, max_visible=8)
    for b, (s0, p0, lm, *_rest) in enumerate(chain):
        batch.set_member(b, s0, p0, lm)
    batch.process_detection_logs([_frame_log(c[3], c[4]) for c in chain])
    assert batch.status() == [0] * len(chain)
    worst = _worst(batch, range(len(chain)), [(c[5], c[6]) for c in chain])
    report("batch_c1_teacher_forced", members=len(chain), state_norm=worst[0], cov_norm=worst[1], state_elem=worst[2],
           cov_elem=worst[3])
    assert worst[0] <= STEP_TOL and worst[1] <= STEP_TOL, worst
    assert worst[2] <= ELEM_TOL and worst[3] <= ELEM_TOL, worst


def test_per_member_noise_constants(monkeypatch):
    from oracle import ekf_numpy
    chain = _oracle_chain_c1()[::16]
    rng = np.random.default_rng(7)
    B = len(chain)
    noise = {"initial_camera_uncertainty": rng.uniform(0.05, 0.5, B), "initial_landmark_uncertainty": rng.uniform(0.2, 2.0, B),
             "r_uncertainty": rng.uniform(0.3, 2.0, B), "q_cam": rng.uniform(0.05, 0.6, B), "q_err": rng.uniform(0.1, 1.0, B),
             "q_lm": rng.uniform(0.001, 0.05, B)}
    batch = _batch(B, max_landmarks=16, max_visible=8, noise=noise)
    want = []
    for b, (s0, p0, lm, ids, poses, _s1, _p1) in enumerate(chain):
        batch.set_member(b, s0, p0, lm)
        for name, key in (("INITIAL_LANDMARK_UNCERTAINTY", "initial_landmark_uncertainty"), ("R_UNCERTAINTY", "r_uncertainty"),
                          ("Q_UNCERTAINTY_CAM", "q_cam"), ("Q_ERROR_UNCERTAINTY_CAM", "q_err"), ("Q_UNCERTAINTY_LM", "q_lm")):
            monkeypatch.setattr(ekf_numpy, name, float(noise[key][b]))
        orc = ekf_numpy.OracleEKF(INIT, mode="fast")
        orc.state, orc.uncertainty = s0.copy(), p0.copy()
        orc.landmarks = {int(k): i for i, k in enumerate(lm)}
        orc.num_landmarks = len(lm)
        orc.observe(ids, poses)
        want.append((np.asarray(orc.state, dtype=np.float64), np.asarray(orc.uncertainty)))
    batch.process_detection_logs([_frame_log(c[3], c[4]) for c in chain])
    worst = _worst(batch, range(B), want)
    report("batch_per_member_noise", members=B, state_norm=worst[0], cov_norm=worst[1], state_elem=worst[2], cov_elem=worst[3])
    assert worst[0] <= STEP_TOL and worst[1] <= STEP_TOL, worst
    assert worst[2] <= ELEM_TOL and worst[3] <= ELEM_TOL, worst
    batch.reset()
    for b in range(B):      # the member's own initial camera uncertainty
        assert np.array_equal(batch.get_cov(b), np.eye(10) * noise["initial_camera_uncertainty"][b])


def test_g2_teacher_forced_vs_reference_golden():
    g = load_npz("g2_teacher_forced.npz")
    frames = list(g["frames"])
    batch = _batch(len(frames), max_landmarks=16, max_visible=8)
    for b, f in enumerate(frames):
        batch.set_member(b, g[f"f{f}_state0"], g[f"f{f}_P0"], g[f"f{f}_lm_ids"])
    batch.process_detection_logs([_frame_log(g[f"f{f}_ids"], g[f"f{f}_poses"]) for f in frames])
    worst = _worst(batch, range(len(frames)), [(g[f"f{f}_state1"], g[f"f{f}_P1"]) for f in frames])
    report("batch_g2_teacher_forced", state_norm=worst[0], cov_norm=worst[1], state_elem=worst[2], cov_elem=worst[3])
    assert worst[0] <= STEP_TOL and worst[1] <= STEP_TOL, worst
    assert worst[2] <= ELEM_TOL and worst[3] <= ELEM_TOL, worst


def test_g3_free_run_in_one_member_of_a_larger_batch_inside_chaos_horizon():
    g = load_npz("g3_free_run.npz")
    logs = [_ragged(12, (1, 6), 40, seed=s) for s in range(5)]
    logs[2] = _c1()
    logs[4] = None
    batch = _batch(5, max_landmarks=16, max_visible=8)
    cams = batch.process_detection_logs(logs)[2]
    hz = chaos_horizon(g)
    assert hz >= 120
    err = rel_err(cams[:hz + 1], g["cam"][:hz + 1])
    report("batch_g3_free_run", horizon=hz, rel_err=err)
    assert err <= 1e-4
    assert list(batch.landmarks[2].keys()) == list(g["lm_ids"])


def _horizon(a, b, envelope=1e-8):
    d = np.abs(a - b).max(axis=1)
    bad = np.nonzero(d > envelope)[0]
    return int(bad[0]) - 1 if len(bad) else len(d) - 1


@pytest.mark.parametrize("quat", ["as_written", "scalar_first"])
@pytest.mark.parametrize("n,m_range,seed", [(50, (1, 10), 11), (82, (8, 16), 12)])
def test_against_the_single_filter_path(quat, n, m_range, seed):
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    log = _ragged(n, m_range, 150, seed=seed)

    def single(poses):
        flt = EKF(INIT, max_landmarks=n, max_visible=16, cov_dtype="float64", quat_update=quat)
        return flt.process_detection_log(log["ids"], poses, log["offsets"], log["has_detections"]), flt.landmarks

    want, table = single(log["poses"])
    rng = np.random.default_rng(seed)
    pert, _ = single(log["poses"] * (1.0 + 1e-15 * rng.standard_normal(log["poses"].shape)))
    hz = _horizon(want, pert)
    batch = _batch(3, max_landmarks=n, max_visible=16, quat_update=quat)
    got = batch.process_detection_logs([None, log, None])[1]
    err = float(np.abs(got[:hz + 1] - want[:hz + 1]).max())
    report(f"batch_vs_single[{quat},n={n},m={m_range}]", horizon=hz, frames=len(want), max_abs=err)
    assert hz >= 50, hz
    assert err <= 1e-6, err
    assert batch.landmarks[1] == table


def _snapshot(batch, b):
    return batch.get_state(b), batch.get_cov(b)


def test_composition_independence_bitwise():
    log = _ragged(50, (1, 10), 80, seed=3)
    others = [_ragged(20, (1, 16), 30, seed=s) for s in range(4)] + [None, _ragged(50, (12, 16), 20, seed=9)]
    runs = []
    for B, slots in ((1, (0,)), (7, (3,)), (300, (5, 299))):
        logs = [others[i % len(others)] for i in range(B)]
        for s in slots:
            logs[s] = log
        batch = _batch(B, max_landmarks=50, max_visible=16)
        traj = batch.process_detection_logs(logs)
        for s in slots:
            runs.append((traj[s], *_snapshot(batch, s)))
        del batch
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert np.array_equal(a, b)


def test_continuation_across_calls_and_windows_is_bitwise():
    log = _ragged(40, (1, 10), 200, seed=5)
    frames = len(log["offsets"]) - 1
    assert frames > 3 * 64
    one = _batch(2, max_landmarks=40, max_visible=16)
    t_one = one.process_detection_logs([log, None])[0]
    two = _batch(2, max_landmarks=40, max_visible=16)
    cut = 100                                     # inside the second window
    t_a = two.process_detection_logs([sp.sub_log(log, 0, cut), None])[0]
    t_b = two.process_detection_logs([sp.sub_log(log, cut, frames), None])[0]
    assert np.array_equal(t_one, np.concatenate([t_a, t_b]))
    for a, b in zip(_snapshot(one, 0), _snapshot(two, 0)):
        assert np.array_equal(a, b)
    assert one.landmarks[0] == two.landmarks[0]


def test_covariance_bitwise_symmetric_and_padding_zero():
    logs = [_ragged(n, (1, min(n, 16)), 60, seed=n) for n in (5, 30, 50, 82)]
    batch = _batch(4, max_landmarks=82, max_visible=16)
    batch.process_detection_logs(logs)
    P = batch.cov_t.cpu().numpy()
    S = batch.state_t.cpu().numpy()
    for b in range(4):
        N = 3 * batch.num_landmarks[b] + 10
        assert np.array_equal(P[b], P[b].T)
        assert not P[b, N:, :].any() and not P[b, :, N:].any() and not S[b, N:].any()
        assert np.isfinite(P[b, :N, :N]).all()


def test_failure_stays_inside_its_member():
    from aruco_slam_amd.batch import EKF_ERR_NUMERIC
    logs = [_ragged(20, (1, 8), 40, seed=s) for s in range(4)]
    boot = [sp.sub_log(lg, 0, 10) for lg in logs]        # every landmark is sighted in the first 10 frames
    rest = [sp.sub_log(lg, 10, len(lg["offsets"]) - 1) for lg in logs]
    ref = _batch(4, max_landmarks=20, max_visible=16)
    bad = _batch(4, max_landmarks=20, max_visible=16)
    for batch in (ref, bad):
        batch.process_detection_logs(boot)
        assert all(batch.num_landmarks[b] == 20 for b in range(4))
    ids = [k for k, _ in sorted(bad.landmarks[2].items(), key=lambda kv: kv[1])]
    s0 = bad.get_state(2)
    bad.set_member(2, s0, -np.eye(s0.shape[0]), ids)     # S = H (Q - I) H^T + R I cannot be positive definite
    t_ref = ref.process_detection_logs([rest[0], rest[1], None, rest[3]])
    t_bad = bad.process_detection_logs(rest)
    assert bad.status() == [0, 0, EKF_ERR_NUMERIC, 0]
    assert np.isnan(t_bad[2]).all() and t_bad[2].shape[0] == len(rest[2]["offsets"]) - 1
    assert np.array_equal(bad.get_state(2), s0) and np.array_equal(bad.get_cov(2), -np.eye(s0.shape[0]))
    for b in (0, 1, 3):
        assert np.array_equal(t_ref[b], t_bad[b])
        for a, c in zip(_snapshot(ref, b), _snapshot(bad, b)):
            assert np.array_equal(a, c)
    t_again = bad.process_detection_logs([None, None, rest[2], None])[2]    # stopped until reset / set_member
    assert np.isnan(t_again).all() and bad.status()[2] == EKF_ERR_NUMERIC
    bad.reset(2)
    assert bad.status() == [0, 0, 0, 0] and bad.num_landmarks[2] == 0


def test_bad_logs_raise_before_anything_runs():
    from aruco_slam_amd.hip_backend import EkfError
    logs = [_ragged(20, (1, 8), 10, seed=s) for s in range(3)]
    batch = _batch(3, max_landmarks=30, max_visible=16)
    batch.process_detection_logs(logs)
    before = [_snapshot(batch, b) for b in range(3)]
    tables = [dict(t) for t in batch.landmarks]
    step = _ragged(20, (1, 8), 3, seed=9)
    frames = np.array([0, 0, 0, 3], dtype=np.int64)
    fo = np.array([0, 2, 4, 6], dtype=np.int64)
    poses = np.zeros((6, 6))
    poses[:, 2] = 5.0
    cases = [
        ("out_of_range", lambda: batch.observe_indexed(np.array([0, 1, 2, 22, 3, 4], np.int32), fo, frames, poses), EkfError),
        ("negative", lambda: batch.observe_indexed(np.array([0, 1, 2, -1, 3, 4], np.int32), fo, frames, poses), EkfError),
        ("misnumbered", lambda: batch.observe_indexed(np.array([0, 21, 20, 1, 3, 4], np.int32), fo, frames, poses), EkfError),
        ("offsets", lambda: batch.observe_indexed(np.arange(6, dtype=np.int32), np.array([0, 4, 2, 6]), frames, poses),
         EkfError),
        ("offsets_end", lambda: batch.observe_indexed(np.arange(6, dtype=np.int32), np.array([0, 2, 4, 7]), frames, poses),
         ValueError),
        ("member_frames", lambda: batch.observe_indexed(np.arange(6, dtype=np.int32), fo, np.array([0, 2, 1, 3]), poses),
         ValueError),
        ("malformed_log", lambda: batch.process_detection_logs([None, dict(step, offsets=step["offsets"][::-1]), None]),
         ValueError),
        ("too_wide", lambda: batch.process_detection_logs([None, _frame_log(np.arange(17) % 5, np.ones((17, 6))), None]),
         EkfError),
        ("too_many_landmarks", lambda: batch.process_detection_logs([_ragged(40, (1, 8), 2, seed=1), None, None]), EkfError),
    ]
    for name, call, exc in cases:
        with pytest.raises(exc) as info:
            call()
        if name in ("too_wide", "too_many_landmarks"):
            assert info.value.code == -2, name
        elif exc is EkfError:
            assert info.value.code == -1, name
        assert batch.landmarks == tables, name
        for b in range(3):
            for a, c in zip(before[b], _snapshot(batch, b)):
                assert np.array_equal(a, c), name
        assert batch.status() == [0, 0, 0]


def test_interop_with_ekf_and_empty_logs():
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    log = _ragged(20, (1, 8), 30, seed=21)
    frames = len(log["offsets"]) - 1
    empty = {"ids": np.zeros(0, np.int32), "poses": np.zeros((0, 6)), "offsets": np.zeros(4, np.int64),
             "has_detections": np.zeros(3, bool)}
    lead = {"ids": log["ids"], "poses": log["poses"], "offsets": np.concatenate(([0, 0], log["offsets"])),
            "has_detections": np.concatenate(([False, False], log["has_detections"]))}
    batch = _batch(4, max_landmarks=20, max_visible=16)
    trajs = batch.process_detection_logs([log, None, empty, lead])
    assert trajs[1].shape == (0, 7) and batch.num_landmarks[1] == 0
    assert np.array_equal(trajs[2], np.tile(INIT[:7].astype(np.float64), (3, 1)))
    assert np.array_equal(trajs[3][:2], np.tile(INIT[:7].astype(np.float64), (2, 1)))
    assert np.array_equal(trajs[3][2:], trajs[0])
    single = EKF(INIT, max_landmarks=20, max_visible=16, cov_dtype="float64")
    want = single.process_detection_log(lead["ids"], lead["poses"], lead["offsets"], lead["has_detections"])
    assert np.abs(trajs[3][:12] - want[:12]).max() <= 1e-9
    assert batch.landmarks[0] == single.landmarks
    # to_filter: the member as an ordinary EKF, bit for bit, which keeps stepping
    ekf = batch.to_filter(0)
    assert np.array_equal(np.asarray(ekf.state), batch.get_state(0)) and np.array_equal(ekf.uncertainty, batch.get_cov(0))
    assert ekf.landmarks == batch.landmarks[0] and ekf.num_landmarks == batch.num_landmarks[0]
    more = _ragged(20, (1, 8), 5, seed=22)
    nxt = sp.sub_log(more, len(more["offsets"]) - 4, len(more["offsets"]) - 1)
    for t in range(3):
        sl = slice(int(nxt["offsets"][t]), int(nxt["offsets"][t + 1]))
        ekf.observe(nxt["ids"][sl], nxt["poses"][sl])
    got = batch.process_detection_logs([nxt, None, None, None])[0][-1]
    assert rel_err(got, np.asarray(ekf.state)[:7]) <= 1e-9
    # load_filter round trip
    batch.load_filter(1, ekf)
    assert np.array_equal(batch.get_state(1), np.asarray(ekf.state)) and np.array_equal(batch.get_cov(1), ekf.uncertainty)
    assert batch.landmarks[1] == ekf.landmarks
    back = batch.to_filter(1)
    assert np.array_equal(np.asarray(back.state), np.asarray(ekf.state)) and np.array_equal(back.uncertainty, ekf.uncertainty)
    assert frames > 0


def test_load_filter_checks_the_filter_and_to_filter_keeps_the_member_noise():
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    noise = {"r_uncertainty": np.array([0.9, 0.4]), "q_lm": np.array([0.01, 0.03])}
    batch = _batch(2, max_landmarks=16, max_visible=8, noise=noise)
    log = _ragged(12, (1, 6), 10, seed=4)
    batch.process_detection_logs([log, log])
    with pytest.raises(ValueError, match="quaternion"):
        batch.load_filter(0, EKF(INIT, max_landmarks=16, max_visible=8, quat_update="scalar_first"))
    with pytest.raises(ValueError, match="EKF_Rotations"):
        batch.load_filter(0, EKF_Rotations(INIT, max_landmarks=4, max_visible=4))
    ekf = batch.to_filter(1)
    assert (ekf.backend.cfg.r_uncertainty, ekf.backend.cfg.q_lm) == (0.4, 0.03)
    assert np.array_equal(np.asarray(ekf.state), batch.get_state(1)) and np.array_equal(ekf.uncertainty, batch.get_cov(1))
    # the filter steps with the member's constants: one more frame, in the batch and in the filter
    nxt = sp.sub_log(_ragged(12, (1, 6), 3, seed=5), 2, 3)
    ekf.observe(nxt["ids"], nxt["poses"])
    got = batch.process_detection_logs([None, nxt])[1][-1]
    assert rel_err(got, np.asarray(ekf.state)[:7]) <= 1e-10
    assert rel_err(batch.get_cov(1), ekf.uncertainty) <= 1e-10
