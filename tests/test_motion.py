"""Camera motion (``motion=True``, ``move``, ``observe(..., motion=)``) of the single filter on an MI355X: one move against
the extended-precision step, the invariants of P, the bit rules of ``include/ekf_slam_hip.h`` ("Odometry input"), and the
tracking fixture.  Cases and expected values: ``motion_util.py`` (``test_motion_cpu.py`` checks them without a GPU)."""
import numpy as np
import pytest

import gating_util as gu
import motion_util as mu
import row_noise_util as rn
import support as sp
import update_sweep_util as sw
from conftest import rel_err, report

pytestmark = pytest.mark.gpu

INIT = sw.INIT
DTYPES = ["float64", "float32"]
GU = {"ekf": "ekf", "rot": "ekf_rotations"}
U = mu.STEP_MOTIONS["general"]


def _filter(model, n, m, dtype="float64", **kw):
    kw.setdefault("motion", True)
    if model == "rot":
        from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
        kw.pop("quat_update", None)
        return EKF_Rotations(INIT, max_landmarks=max(n, 1), max_visible=max(m, 1), cov_dtype=dtype, **kw)
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    kw.setdefault("quat_update", "scalar_first")
    return EKF(INIT, max_landmarks=max(n, 1), max_visible=max(m, 1), cov_dtype=dtype, **kw)


# ---- 1. one move against the extended form, and the invariants ------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["ekf", "rot"])
def test_one_move_against_the_extended_reference(model, dtype):
    """n = 0, 1, 40 and the first n whose strip needs a second workgroup (motion_util.BOUNDARY_N: 86 / 26: N - 10 = lmd n
    columns, 256 per workgroup), four motions each.  |P' - P'_ref| <= 64 u64 (Fb |P| Fb^T) (+ u32 |P'_ref|, f32) and the
    state within 8 u64 (|c| + |d|) / 8 u64.  P' bitwise symmetric, the padding exactly zero, the landmarks untouched."""
    import torch
    worst, failures = [0.0, 0.0, 0.0], []
    for n in mu.STEP_SIZES[model]:
        flt = _filter(model, n, 4, dtype)
        prior = mu.step_prior(model, n, dtype)
        dims = len(prior[0])
        for name, u in mu.STEP_MOTIONS.items():
            sp.restore(flt, prior)
            flt.move(u[0:3], u[3:6])
            x, p = sp.snap_backend(flt.backend)
            ref = mu.extended_move(prior[0], prior[1], u)
            r = mu.step_ratios(ref, p, x, dtype)
            worst = [max(a, b) for a, b in zip(worst, r)]
            if max(r) > 1.0:
                failures.append((n, name, r))
            assert np.array_equal(p, p.T), (n, name)
            assert np.array_equal(x[7:], prior[0][7:]) and np.array_equal(p[10:, 10:], prior[1][10:, 10:]), (n, name)
            flt.backend.sync()
            torch.cuda.synchronize()
            full = flt.backend.cov_t.cpu().numpy()
            assert not full[dims:, :].any() and not full[:, dims:].any(), (n, name)
            assert np.array_equal(full[:dims, :dims].astype(np.float64), p)
            assert not flt.backend.state_t.cpu().numpy()[dims:].any()
    report(f"motion_step[{model},{dtype}]", ratio_P=worst[0], ratio_c=worst[1], ratio_q=worst[2], bound=1.0)
    assert not failures, failures


def test_a_large_map_moves_with_many_workgroups():
    """n = 1000 (N = 3010: 12 workgroups; the state is stored by the second launch) against the extended step, and a getter
    straight after the move returns the moved pose."""
    n = 1000
    flt = _filter("ekf", n, 4, "float32")
    rng = np.random.default_rng(3)
    state = np.concatenate((mu.step_prior("ekf", 1, "float32")[0][:10], rng.uniform(-3, 3, 3 * n)))
    f = rng.normal(size=(10 + 3 * n, 3))
    p = (0.05 * (f @ f.T) + np.diag(rng.uniform(0.5, 1.0, 10 + 3 * n))).astype(np.float32).astype(np.float64)
    p = np.tril(p) + np.tril(p, -1).T
    sp.restore(flt, (state, p, list(range(n))))
    flt.move(U[0:3], U[3:6])
    cam = flt.get_poses()[0]
    ref = mu.extended_move(state, p, U)
    x, got = sp.snap_backend(flt.backend)
    assert np.array_equal(cam[:7], x[:7]) and not np.array_equal(x[:7], state[:7])
    r = mu.step_ratios(ref, got, x, "float32")
    assert max(r) <= 1.0, r
    assert np.array_equal(got, got.T) and np.array_equal(got[10:, 10:], p[10:, 10:]) and np.array_equal(x[7:], state[7:])


# ---- 2. bit rules 6(a), 6(b), 6(e) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gate"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stage"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["ekf", "rot"])
def test_zero_motion_is_no_motion_and_a_moved_frame_is_move_then_observe(model, dtype, fused, gated):
    """n = 40, m = 1, 16, 17 and one wide frame (66 / 52): (a) motion = None and six exact zeros against a filter built
    without the flag; (b) observe(..., motion=u) against move(u) and then observe(...), with and without a scale; (e) a pure
    translation leaves the quaternion and its rows and columns of P as they were.  State, P and, gated, d^2."""
    from aruco_slam_amd.filters.ekf_with_rotations import euler_xyz_to_quat
    n = 40
    wide_m = 52 if model == "rot" else 66
    gate = float("inf") if gated else None
    flt = _filter(model, n, wide_m, dtype, fused=fused, gate=gate, frame_scale=True)
    two = _filter(model, n, wide_m, dtype, fused=fused, gate=gate, frame_scale=True)
    bare = _filter(model, n, wide_m, dtype, fused=fused, gate=gate, frame_scale=True, motion=False)
    for m in (1, 16, 17, wide_m):
        prior = sw.dense_prior(model, n, m, 700 + m, dtype)
        # (a)
        sp.restore(bare, prior)
        bare.observe(prior[3], prior[4])
        want = sp.snap_backend(bare.backend)
        for u in (None, np.zeros(6), np.array([0.0, -0.0, 0.0, 0.0, 0.0, -0.0])):
            sp.restore(flt, prior)
            flt.observe(prior[3], prior[4], motion=u)
            sp.assert_same(sp.snap_backend(flt.backend), want, ("6a", m, u))
            if gated:
                assert np.array_equal(flt.last_mahal, bare.last_mahal)
        # (b), without and with a scale
        for scale in (None, 2.5):
            kw = {} if scale is None else {"scale": scale}
            sp.restore(flt, prior)
            sp.restore(two, prior)
            if scale is None:
                flt.observe(prior[3], prior[4], motion=U)
            else:      # ekf_observe_moved itself, under the filter layer (whose motion= is move() and then the frame)
                pz = np.asarray(prior[4], dtype=np.float64)
                z = pz[:, :3] if model == "ekf" else np.hstack((pz[:, :3], euler_xyz_to_quat(pz[:, 3:6])))
                d2 = flt.backend.observe(prior[3], z, mahal=gated, scale=scale, motion=U)
                if gated:
                    flt.last_mahal = d2
            two.move(U[0:3], U[3:6])
            two.observe(prior[3], prior[4], **kw)
            sp.assert_same(sp.snap_backend(flt.backend), sp.snap_backend(two.backend), ("6b", m, scale))
            assert not np.array_equal(flt.backend.get_cov(), want[1])      # (the motion is not ignored)
            if gated:
                assert np.array_equal(flt.last_mahal, two.last_mahal) and (flt.last_mahal > 0).all()
    # (e)
    prior = sw.dense_prior(model, n, 1, 701, dtype)
    t = mu.STEP_MOTIONS["translation"]
    sp.restore(flt, prior)
    x0, p0 = sp.snap_backend(flt.backend)
    flt.move(t[0:3], t[3:6])
    x, p = sp.snap_backend(flt.backend)
    assert np.array_equal(x[3:], x0[3:]) and not np.array_equal(x[0:3], x0[0:3])
    assert np.array_equal(p[3:10, 3:], p0[3:10, 3:]) and np.array_equal(p[3:, 3:10], p0[3:, 3:10])
    assert not np.array_equal(p[0:3], p0[0:3])


# ---- 3. bit rule 6(c): log replay, per-frame loop and sequence call ---------------------------------------------------------
def _loop(flt, log, motion, scale=None, rows=None):
    offs = log["offsets"]
    traj = []
    for t in range(len(offs) - 1):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        kw = {} if motion is None else {"motion": motion[t]}
        if scale is not None:
            kw["scale"] = scale[t]
        if rows is not None and offs[t + 1] > offs[t]:
            kw["noise"] = rows[sl]
        _, cam, _, _ = flt.process_detections(log["ids"][sl] if offs[t + 1] > offs[t] else None, log["poses"][sl], **kw)
        traj.append(np.asarray(cam, dtype=np.float64)[:7])
    return np.array(traj)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["ekf", "rot"])
def test_a_log_replay_with_motions_is_the_per_frame_loop(model, dtype):
    """The ragged 14-frame log (a leading empty frame, three empty frames in a row that carry motions, first sightings after
    motions, two exact-zero motions): process_detection_log against the per-frame loop, every trajectory row included -- an
    empty frame's row is the moved pose.  The call runs in serial order; the same log without motions still pipelines.
    EKF: bit for bit.  EKF_Rotations: the replay forms z on the device, the loop on the host, so the two agree as the replay
    and the loop agree without motions (1e-9; covariance 1e-5 for f32)."""
    log = mu.ragged_motion_log(model)
    n, m = 8, 5
    loop, rep, still = _filter(model, n, m, dtype, lookahead=True), _filter(model, n, m, dtype, lookahead=True), \
        _filter(model, n, m, dtype, lookahead=True)
    want_traj = _loop(loop, log, log["motion"])
    traj = rep.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"], motion=log["motion"])
    stats = rep.backend.last_log_stats()
    assert stats["frames_pipelined"] == 0 and stats["frames_stepped"] == int(log["has_detections"].sum()), stats
    assert rep.backend.last_sequence_mode() == "serial"
    # rows of empty frames: the moved pose, not a repeat
    assert not np.array_equal(traj[0], INIT[:7]) and len({tuple(traj[t]) for t in (3, 4, 5, 6)}) == 4
    if model == "ekf":
        assert np.array_equal(traj, want_traj)
        sp.assert_same(sp.snap_backend(rep.backend), sp.snap_backend(loop.backend), "log = loop")
    else:
        a, b = sp.snap_backend(rep.backend), sp.snap_backend(loop.backend)
        assert np.abs(traj - want_traj).max() <= 1e-9 and np.abs(a[0] - b[0]).max() <= 1e-9
        assert np.abs(a[1] - b[1]).max() <= (1e-9 if dtype == "float64" else 1e-5)
    # the oracle wrapper agrees (the tolerance of the per-frame parity tests)
    ref, _orc = mu.oracle_track(model, log, True)
    assert rel_err(want_traj, ref) <= {"float64": 1e-9, "float32": 1e-4}[dtype]
    # without the motion array the log is replayed as ever
    plain = still.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"])
    assert still.backend.last_log_stats()["frames_pipelined"] > 0 and not np.array_equal(plain, traj)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["ekf", "rot"])
def test_a_sequence_call_with_motions_is_the_per_frame_loop(model, dtype):
    """Frames 1 .. 12 of the tracking scene (m = 4, every landmark known after frame 0) as one sequence call with their
    motions (one exact zero) against the loop: bit for bit, in serial order; without the array the call pipelines."""
    import torch
    from aruco_slam_amd.filters.ekf_with_rotations import euler_xyz_to_quat
    scene = mu.tracking_scene(model)
    offs = scene["offsets"]
    motion = scene["motion"][1:13].copy()
    motion[4] = 0.0

    def booted():
        flt = _filter(model, 10, 10, dtype, lookahead=True)
        flt.observe(scene["ids"][:offs[1]], scene["poses"][:offs[1]])
        return flt

    loop = booted()
    want_traj = []
    for t in range(1, 13):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        loop.observe(scene["ids"][sl], scene["poses"][sl], motion=motion[t - 1])
        want_traj.append(np.asarray(loop.get_poses()[0], dtype=np.float64)[:7])
    sl = slice(int(offs[1]), int(offs[13]))
    idx = np.array([loop.landmarks[int(i)] for i in scene["ids"][sl]], dtype=np.int32).reshape(12, 4)
    poses = scene["poses"][sl]
    z = poses[:, :3] if model == "ekf" else np.hstack((poses[:, :3], euler_xyz_to_quat(poses[:, 3:6])))
    z = z.reshape(12, 4, -1)
    for with_motion in (True, False):
        seq = booted()
        dev = seq.backend.device
        traj_t = torch.empty((12, 7), dtype=torch.float64, device=dev)
        seq.backend.observe_sequence(torch.tensor(idx, device=dev), torch.tensor(z, dtype=torch.float64, device=dev), traj_t,
                                     motion=motion if with_motion else None)
        if with_motion:
            assert seq.backend.last_sequence_mode() == "serial"
            sp.assert_same(sp.snap_backend(seq.backend), sp.snap_backend(loop.backend), "sequence = loop")
            assert np.array_equal(traj_t.cpu().numpy(), np.array(want_traj))
        else:
            assert seq.backend.last_sequence_mode() == "pipelined"
            assert not np.array_equal(seq.backend.get_cov(), loop.backend.get_cov())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["ekf", "rot"])
def test_an_all_zero_motion_array_is_the_pipelined_call_without_it(model, dtype):
    """Bit rule 6(a), pipelined runs included: frames 1 .. 12 of the tracking scene as a log and as a sequence call.  Given
    an all-zero motion array the call runs in serial order; without the array it pipelines; state, P and trajectory agree
    bit for bit (both replays form z on the device, so this holds for EKF_Rotations as well)."""
    import torch
    from aruco_slam_amd.filters.ekf_with_rotations import euler_xyz_to_quat
    scene = mu.tracking_scene(model)
    offs = scene["offsets"]
    d0, d1 = int(offs[1]), int(offs[13])
    seg = (scene["ids"][d0:d1], scene["poses"][d0:d1], offs[1:14] - d0)
    runs = {}
    for zero in (True, False):
        flt = _filter(model, 10, 10, dtype, lookahead=True)
        flt.observe(scene["ids"][:d0], scene["poses"][:d0])
        traj = flt.process_detection_log(*seg, motion=np.zeros((12, 6)) if zero else None)
        stats = flt.backend.last_log_stats()
        assert (stats["frames_pipelined"] == 0) if zero else (stats["frames_pipelined"] > 0), stats
        runs[zero] = (traj, sp.snap_backend(flt.backend))
        seq = _filter(model, 10, 10, dtype, lookahead=True)
        seq.observe(scene["ids"][:d0], scene["poses"][:d0])
        idx = np.array([seq.landmarks[int(i)] for i in seg[0]], dtype=np.int32).reshape(12, 4)
        z = seg[1][:, :3] if model == "ekf" else np.hstack((seg[1][:, :3], euler_xyz_to_quat(seg[1][:, 3:6])))
        dev = seq.backend.device
        traj_t = torch.empty((12, 7), dtype=torch.float64, device=dev)
        seq.backend.observe_sequence(torch.tensor(idx, device=dev), torch.tensor(z.reshape(12, 4, -1), dtype=torch.float64, device=dev),
                                     traj_t, motion=np.zeros((12, 6)) if zero else None)
        assert seq.backend.last_sequence_mode() == ("serial" if zero else "pipelined")
        snap = sp.snap_backend(seq.backend)      # (the getters wait for the call; the trajectory tensor is complete behind them)
        runs[("seq", zero)] = (traj_t.cpu().numpy(), snap)
    for a, b in ((True, False), (("seq", True), ("seq", False))):
        assert np.array_equal(runs[a][0], runs[b][0]), a
        sp.assert_same(runs[a][1], runs[b][1], a)


# ---- 4. bit rule 6(f): gate, rows and scales compose -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["ekf", "rot"])
def test_gate_rows_scales_and_motions_compose(model, dtype):
    """gating_util's dirty log (outliers, frames of outliers only, empty frames) with rows, a scale and a small motion per
    frame.  The gated run is bit for bit the ungated run with the same motions on the log without the rejected detections,
    per frame and as a log; a frame whose detections are all rejected ends on the moved pose with p + s pending."""
    gmodel = GU[model]
    clean = gu.clean_log(gmodel, "column", seed=0)
    dirty, marks = gu.dirty_log(gmodel, clean, seed=0)
    rows = rn.log_rows(gmodel, dirty, 0)
    kw, n, _range = gu.FAMILIES[(gmodel, "column")]
    m, gate = kw["max_visible"], gu.GATES[gmodel]
    frames = len(dirty["offsets"]) - 1
    rng = np.random.default_rng(77)
    scale = np.exp(rng.uniform(np.log(0.5), np.log(2.0), frames))
    motion = rng.normal(0.0, 1e-3, (frames, 6))      # (small: the camera of the log stands still, the decisions stay)
    motion[3] = 0.0
    offs = dirty["offsets"]
    flt = _filter(model, n, m, dtype, gate=gate, row_noise=True, frame_scale=True)
    traj, rej = [], np.zeros(len(dirty["ids"]), dtype=bool)
    extra = gu.extra_frames(dirty, marks)
    checked = 0
    for t in range(frames):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        before, pend = flt.backend.get_state()[:7].copy(), flt.pending_scale
        if offs[t + 1] > offs[t]:
            flt.observe(dirty["ids"][sl], dirty["poses"][sl], noise=rows[sl], scale=scale[t], motion=motion[t])
            rej[sl] = flt.last_rejected
        else:
            flt.process_detections(None, None, scale=scale[t], motion=motion[t])
        traj.append(flt.backend.get_state()[:7].copy())
        if extra[t] and offs[t + 1] > offs[t]:      # every detection rejected: moved, not stepped
            _f, c1, q1 = mu.motion_parts(before, motion[t])
            assert np.abs(traj[-1] - np.concatenate((c1, q1))).max() <= 1e-14 and not np.array_equal(traj[-1], before)
            assert flt.pending_scale == pend + scale[t]
            checked += 1
    assert np.array_equal(rej, marks) and marks.any() and checked >= 1
    cut, cut_rows = gu.delete(dirty, rej), rows[~rej]
    plain = _filter(model, n, m, dtype, row_noise=True, frame_scale=True)
    traj_p = _loop(plain, cut, motion, scale, cut_rows)
    assert np.array_equal(np.array(traj), traj_p)
    sp.assert_same(sp.snap_backend(flt.backend), sp.snap_backend(plain.backend), "gated loop = loop without the rejected")
    glog = _filter(model, n, m, dtype, gate=gate, row_noise=True, frame_scale=True)
    g_traj, g_d2 = glog.process_detection_log(dirty["ids"], dirty["poses"], dirty["offsets"], mahal=True, noise=rows,
                                              scale=scale, motion=motion)
    assert np.array_equal(g_d2 > gate, marks)
    plog = _filter(model, n, m, dtype, row_noise=True, frame_scale=True)
    p_traj = plog.process_detection_log(cut["ids"], cut["poses"], cut["offsets"], noise=cut_rows, scale=scale, motion=motion)
    assert np.array_equal(g_traj, p_traj)
    sp.assert_same(sp.snap_backend(glog.backend), sp.snap_backend(plog.backend), "gated log = log without the rejected")
    assert glog.pending_scale == plog.pending_scale == flt.pending_scale
    if model == "ekf":
        sp.assert_same(sp.snap_backend(glog.backend), sp.snap_backend(flt.backend), "log = loop")
        assert np.array_equal(g_traj, np.array(traj))


def test_a_scaled_moved_frame_is_the_plain_moved_frame_with_the_products():
    """Rule 5(b) of the frame scale on a moved frame: s_eff = 2.5 against a twin configured with fl(2.5 q)."""
    import frame_scale_util as fs
    prior = sw.dense_prior("ekf", 40, 16, 716)
    flt = _filter("ekf", 40, 16, frame_scale=True, quat_update="as_written")
    twin = _filter("ekf", 40, 16, noise=fs.scaled_constants("ekf", 2.5), quat_update="as_written")
    sp.restore(flt, prior)
    sp.restore(twin, prior)
    flt.observe(prior[3], prior[4], scale=2.5, motion=U)
    twin.observe(prior[3], prior[4], motion=U)
    sp.assert_same(sp.snap_backend(flt.backend), sp.snap_backend(twin.backend), "5(b) on a moved frame")


# ---- 5. the tracking fixture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["ekf", "rot"])
def test_tracking_fixture_on_the_device(model, dtype):
    """The device replays the fixture's log with and without its motions: the trajectories match the oracle wrapper's under
    the tolerance of the per-frame parity tests of the model and dtype (tests/test_hip_parity.py: 1e-9; f32 1e-4 for EKF,
    2e-5 for EKF_Rotations), and the device's two mean position errors reproduce the 1/5 condition."""
    scene = mu.tracking_scene(model)
    tol = {"float64": 1e-9, "float32": 1e-4 if model == "ekf" else 2e-5}[dtype]
    errs = {}
    for odo in (True, False):
        flt = _filter(model, 10, 10, dtype)
        traj = flt.process_detection_log(scene["ids"], scene["poses"], scene["offsets"],
                                         motion=scene["motion"] if odo else None)
        ref, _orc = mu.oracle_track(model, scene, odo)
        assert rel_err(traj, ref) <= tol, (odo, rel_err(traj, ref))
        errs[odo] = mu.mean_position_error(traj, scene)
    report(f"motion_tracking[{model},{dtype}]", with_odometry_m=errs[True], without_odometry_m=errs[False],
           ratio=errs[True] / errs[False])
    assert errs[True] <= mu.TRACK_RATIO * errs[False], errs


# ---- 6. validation and the capability ----------------------------------------------------------------------------------------
def test_motions_are_validated_before_anything_changes(tmp_path):
    from aruco_slam_amd.hip_backend import EkfError, _dptr
    prior = sw.dense_prior("ekf", 12, 4, 91)
    flt = _filter("ekf", 12, 4)
    sp.restore(flt, prior)
    before = sp.snap_backend(flt.backend)
    for bad in (np.full(6, np.nan), [0, 0, 0, np.inf, 0, 0], np.zeros(5), np.zeros((2, 6))):
        with pytest.raises(ValueError, match="motion"):
            flt.observe(prior[3], prior[4], motion=bad)
        with pytest.raises(ValueError, match="motion"):
            flt.process_detections(None, None, motion=bad)
    with pytest.raises(ValueError, match="motion"):
        flt.process_detection_log(prior[3], prior[4], [0, 4], motion=np.zeros((2, 6)))
    # the C ABI itself: NaN -> EKF_ERR_INVALID, a handle without the flag -> EKF_ERR_STATE, nothing enqueued
    lib, h = flt.backend.lib, flt.backend.h
    nan = np.array([0.1, 0, 0, 0, np.nan, 0])
    assert lib.ekf_move(h, _dptr(nan)) == -1
    bare = _filter("ekf", 12, 4, motion=False)
    sp.restore(bare, prior)
    assert lib.ekf_move(bare.backend.h, _dptr(U.copy())) == -4
    with pytest.raises(ValueError, match="motion=True"):
        bare.move(U[0:3], U[3:6])
    with pytest.raises(ValueError, match="motion=True"):
        bare.observe(prior[3], prior[4], motion=U)
    sp.assert_same(sp.snap_backend(flt.backend), before, "nothing changed")
    sp.assert_same(sp.snap_backend(bare.backend), before, "nothing changed")
    # grow, remove_markers and checkpoints keep the capability
    flt.backend.grow(24)
    flt.remove_markers([prior[2][0]])
    flt.move(U[0:3], U[3:6])
    assert not np.array_equal(flt.backend.get_state()[:7], before[0][:7])
    flt.save_checkpoint(str(tmp_path / "ck.npz"))
    with pytest.raises(ValueError, match="motion=True"):
        bare.load_checkpoint(str(tmp_path / "ck.npz"))
    again = _filter("ekf", 12, 4)
    again.load_checkpoint(str(tmp_path / "ck.npz"))
    sp.assert_same(sp.snap_backend(again.backend), sp.snap_backend(flt.backend), "checkpoint")
    assert isinstance(EkfError(-1, "x"), RuntimeError)


def test_a_failed_filter_ignores_motions():
    """A device-resident index out of range raises the sticky status word; a motion after it changes nothing."""
    import torch
    prior = sw.dense_prior("ekf", 12, 4, 92)
    flt = _filter("ekf", 12, 4)
    sp.restore(flt, prior)
    dev = flt.backend.device
    idx = torch.tensor([[0, 1, 2, 99]], dtype=torch.int32, device=dev)
    z = torch.tensor(np.asarray(prior[4])[None, :, :3], dtype=torch.float64, device=dev)
    flt.backend.observe_sequence(idx, z)
    with pytest.raises(Exception):
        flt.backend.sync()
    torch.cuda.synchronize()
    state0, cov0 = flt.backend.state_t.cpu().numpy().copy(), flt.backend.cov_t.cpu().numpy().copy()
    flt.backend.move(U)
    torch.cuda.synchronize()
    assert np.array_equal(flt.backend.state_t.cpu().numpy(), state0) and np.array_equal(flt.backend.cov_t.cpu().numpy(), cov0)


def test_run_slam_moves_the_camera_with_the_files_motion(tmp_path):
    """A replay file with a ``motion`` array: the frame loop and --resident agree (EKF: bit for bit on the trajectory text),
    and both differ from the run on the file without it."""
    import argparse
    from aruco_slam_amd.main import run_slam
    scene = mu.tracking_scene("ekf")
    frames = len(scene["offsets"]) - 1
    base = dict(ids=scene["ids"], poses=scene["poses"], offsets=scene["offsets"], timestamps_ms=33.3 * np.arange(frames),
                has_detections=np.ones(frames, dtype=bool))
    np.savez(tmp_path / "odo.npz", motion=scene["motion"], **base)
    np.savez(tmp_path / "plain.npz", **base)
    texts = {}
    for name, file, resident in (("loop", "odo.npz", False), ("resident", "odo.npz", True), ("plain", "plain.npz", True)):
        out = tmp_path / name
        run_slam.main(argparse.Namespace(filter="ekf", detections=str(tmp_path / file), video=None, resident=resident,
                                         output_dir=str(out), filter_kwargs={"quat_update": "scalar_first"}))
        texts[name] = (out / "trajectory.txt").read_text()
    assert texts["loop"] == texts["resident"] and texts["plain"] != texts["resident"]
