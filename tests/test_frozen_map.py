"""Localisation mode on an MI355X: a frozen map and the Schmidt-Kalman camera-strip update (include/ekf_slam_hip.h,
"Localisation mode"; csrc/ekf_cov_strip.hip).  A frozen frame is compared bit for bit with the mapping frame of a second
filter restored from the same arrays (camera rows and columns), with the prior (landmarks, P[10:, 10:]) and, free-running,
with the NumPy oracle's Schmidt step (``frozen_util.schmidt_step``)."""
import argparse
import functools

import numpy as np
import pytest

import frozen_util as fu
from conftest import load_npz, rel_err, rel_err_elem, report

pytestmark = pytest.mark.gpu

CAM = fu.CAM


@functools.lru_cache(maxsize=None)
def _prior(model, n, dtype, quat):
    return fu.prior(model, n, seed=17 + n, dtype=dtype, quat=quat)


def _pair(model, n, m, dtype, quat, fused, **kw):
    """Two filters with room for ``m`` detections per frame, restored from the same prior; the first one frozen."""
    state0, p0, ids = _prior(model, n, dtype, quat)
    pair = []
    for _ in range(2):
        flt = fu.make(model, n, m, dtype=dtype, quat=quat, fused=fused, **kw)
        fu.restore(flt, state0, p0, ids)
        pair.append(flt)
    pair[0].freeze_map()
    assert pair[0].map_frozen and not pair[1].map_frozen
    return pair[0], pair[1], state0, p0


# ---- 1. one frame, bitwise, against the mapping frame ------------------------------------------------------------------------
# N = 13, 73, 139 and 259 (past one 256-thread workgroup of the strip kernel); k = 3 (padded to 16), 18 (padded rows), 99; a
# duplicated id; wide frames by duplicates on n = 43: m = 66 (the wide front, stage factorisation) and m = 130 (k = 390:
# beyond 384 rows, two row chunks)
EKF_SHAPES = [(1, 1, False), (1, 6, True), (21, 1, False), (21, 6, False), (21, 6, True), (43, 33, False), (83, 6, False),
              (83, 33, False)]
EKF_WIDE = [(43, 66), (43, 130)]
# N = 20 and 140; k = 7, 56, and 357 / 392 (stage kernels; beyond 384 rows)
ROT_SHAPES = [(1, 1, False), (1, 8, True), (13, 1, False), (13, 8, False)]
ROT_WIDE = [(13, 51), (13, 56)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stage"])
@pytest.mark.parametrize("quat", ["as_written", "scalar_first"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m,dup", EKF_SHAPES)
def test_ekf_frozen_frame_is_bitwise_the_mapping_frame_on_the_camera(n, m, dup, dtype, quat, fused):
    frozen, mapping, state0, p0 = _pair("ekf", n, m, dtype, quat, fused)
    ids, poses = fu.frame("ekf", n, m, seed=5 + m, duplicate=dup)
    for flt in (frozen, mapping):
        flt.observe(ids, poses)
    fu.assert_frozen_frame(frozen, mapping, state0, p0)
    assert frozen.last_ignored == ()


@pytest.mark.parametrize("quat", ["as_written", "scalar_first"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m", EKF_WIDE)
def test_ekf_frozen_wide_frame_is_bitwise_the_mapping_frame_on_the_camera(n, m, dtype, quat):
    frozen, mapping, state0, p0 = _pair("ekf", n, m, dtype, quat, True)
    ids, poses = fu.frame("ekf", n, m, seed=5 + m)
    for flt in (frozen, mapping):
        flt.observe(ids, poses)
    fu.assert_frozen_frame(frozen, mapping, state0, p0)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stage"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m,dup", ROT_SHAPES)
def test_rotations_frozen_frame_is_bitwise_the_mapping_frame_on_the_camera(n, m, dup, dtype, fused):
    frozen, mapping, state0, p0 = _pair("ekf_rotations", n, m, dtype, None, fused)
    ids, poses = fu.frame("ekf_rotations", n, m, seed=5 + m, duplicate=dup)
    for flt in (frozen, mapping):
        flt.observe(ids, poses)
    fu.assert_frozen_frame(frozen, mapping, state0, p0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m", ROT_WIDE)
def test_rotations_frozen_wide_frame_is_bitwise_the_mapping_frame_on_the_camera(n, m, dtype):
    frozen, mapping, state0, p0 = _pair("ekf_rotations", n, m, dtype, None, True)
    ids, poses = fu.frame("ekf_rotations", n, m, seed=5 + m)
    for flt in (frozen, mapping):
        flt.observe(ids, poses)
    fu.assert_frozen_frame(frozen, mapping, state0, p0)


# ---- 2. chains ---------------------------------------------------------------------------------------------------------------
def _log(model, n, m_range, steady, seed):
    from aruco_slam_amd.synthetic import ragged_log
    return ragged_log(n, m_range, steady, seed=seed, rvec_sigma=0.05 if model == "ekf_rotations" else 0.0)


def _frames(log, t0, t1):
    offs = log["offsets"]
    return [(log["ids"][int(offs[t]):int(offs[t + 1])], log["poses"][int(offs[t]):int(offs[t + 1])]) for t in range(t0, t1)]


def _sub(log, t0, t1):
    offs = log["offsets"]
    d0, d1 = int(offs[t0]), int(offs[t1])
    return log["ids"][d0:d1], log["poses"][d0:d1], offs[t0:t1 + 1] - d0, log["has_detections"][t0:t1]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_chain_of_frozen_frames_every_frame_against_a_mapping_frame_from_the_same_prior(dtype):
    log = _log("ekf", 12, (2, 8), 40, seed=3)
    boot = int(log["bootstrap_frames"])
    frozen = fu.ekf(12, 8, dtype=dtype)
    for ids, poses in _frames(log, 0, boot):
        frozen.observe(ids, poses)
    frozen.freeze_map()
    mapping = fu.ekf(12, 8, dtype=dtype)
    table = [k for k, _ in sorted(frozen.landmarks.items(), key=lambda kv: kv[1])]
    for ids, poses in _frames(log, boot, boot + 40):
        state0, p0 = fu.arrays(frozen)
        fu.restore(mapping, state0, p0, table)
        frozen.observe(ids, poses)
        mapping.observe(ids, poses)
        fu.assert_frozen_frame(frozen, mapping, state0, p0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_frozen_log_replay_is_bitwise_the_per_frame_frozen_loop(dtype):
    log = _log("ekf", 12, (2, 8), 40, seed=4)
    boot, frames = int(log["bootstrap_frames"]), len(log["has_detections"])
    loop, replay = fu.ekf(12, 8, dtype=dtype), fu.ekf(12, 8, dtype=dtype)
    for flt in (loop, replay):
        for ids, poses in _frames(log, 0, boot):
            flt.observe(ids, poses)
        flt.freeze_map()
    rows = []
    for ids, poses in _frames(log, boot, frames):
        _, cam, _, _ = loop.process_detections(ids, poses)
        rows.append(np.asarray(cam, dtype=np.float64)[:7])
    traj = replay.process_detection_log(*_sub(log, boot, frames))
    assert np.array_equal(traj, np.array(rows))
    for a, b in zip(fu.arrays(loop), fu.arrays(replay)):
        assert np.array_equal(a, b)
    stats = replay.backend.last_log_stats()
    assert stats["frames_stepped"] == frames - boot and stats["frames_pipelined"] == 0 and stats["markers_added"] == 0
    assert replay.map_frozen and replay.last_ignored == ()


# ---- 3. against the Schmidt oracle (f64 covariance, scalar-first quaternion rule) --------------------------------------------
@pytest.mark.parametrize("model,n,m_range", [("ekf", 24, (2, 10)), ("ekf_rotations", 12, (1, 5))])
def test_frozen_replay_against_the_schmidt_oracle(model, n, m_range):
    """Bootstrap + 20 mapping + 60 frozen frames; the bounds of a mapping replay against the oracle
    (tests/test_log_replay.py: 1e-9 norm-wise, 1e-6 element-wise on trajectory, map and variances)."""
    log = _log(model, n, m_range, 80, seed=21)
    boot = int(log["bootstrap_frames"])
    flt = fu.make(model, n, m_range[1], quat="scalar_first")
    orc = fu.new_oracle(model)
    want, got = [], []
    for t, (ids, poses) in enumerate(_frames(log, 0, boot + 80)):
        if t == boot + 20:
            flt.freeze_map()
        if t < boot + 20:
            orc.observe([int(i) for i in ids], poses)
        else:
            fu.schmidt_step(orc, ids, poses)
        _, cam, _, _ = flt.process_detections(ids, poses)
        got.append(np.asarray(cam, dtype=np.float64)[:7])
        want.append(np.asarray(orc.state, dtype=np.float64)[:7])
    got, want = np.array(got), np.array(want)
    lm_got, lm_want = flt.get_poses()[1], np.asarray(orc.state, dtype=np.float64)[CAM:].reshape(-1, fu.LMD[model])
    unc_got, unc_want = np.diagonal(flt.uncertainty), np.diagonal(np.asarray(orc.uncertainty))
    errs = dict(traj_norm=rel_err(got, want), traj_elem=rel_err_elem(got, want), map_norm=rel_err(lm_got, lm_want),
                map_elem=rel_err_elem(lm_got, lm_want), unc_norm=rel_err(unc_got, unc_want),
                unc_elem=rel_err_elem(unc_got, unc_want), cov_norm=rel_err(flt.uncertainty, orc.uncertainty))
    report(f"frozen_oracle_{model}", **errs)
    assert max(errs["traj_norm"], errs["map_norm"], errs["unc_norm"], errs["cov_norm"]) <= 1e-9, errs
    assert max(errs["traj_elem"], errs["map_elem"], errs["unc_elem"]) <= 1e-6, errs
    assert np.linalg.eigvalsh(flt.uncertainty)[0] > 0.0


# ---- 4. composition ----------------------------------------------------------------------------------------------------------
def _frozen(n=21, m=8, dtype="float64", **kw):
    """A frozen EKF restored from the n = 21 prior, and the prior."""
    state0, p0, ids = _prior("ekf", n, dtype, "scalar_first")
    flt = fu.ekf(n, m, dtype=dtype, quat="scalar_first", **kw)
    fu.restore(flt, state0, p0, ids)
    flt.freeze_map()
    return flt, state0, p0


def _equal(a, b):
    for x, y in zip(fu.arrays(a), fu.arrays(b)):
        assert np.array_equal(x, y), float(np.abs(x - y).max())


def test_gated_frozen_frame_is_the_frozen_frame_on_the_survivors():
    from gating_util import _outlier
    # the frame is seen from two frames back on the track, and the prior is young: on the oracle the inliers' d^2 reach 49
    # and the outlier's is 1.7e4 -- a gate of 1000 is a factor 17 away from either
    ids, poses = fu.frame("ekf", 21, 6, seed=31)
    bad = _outlier("ekf", poses[2], np.random.default_rng(1), 0)
    ids_d, poses_d = np.insert(ids, 3, ids[2]), np.insert(poses, 3, bad, axis=0)
    gated, _, _ = _frozen(gate=1000.0)
    plain, state0, p0 = _frozen()
    gated.observe(ids_d, poses_d)
    plain.observe(ids, poses)
    _equal(gated, plain)
    assert gated.last_rejected.tolist() == [False, False, False, True, False, False, False]
    assert gated.last_mahal[3] > 3000.0 and np.delete(gated.last_mahal, 3).max() < 300.0
    assert np.array_equal(fu.arrays(gated)[0][CAM:], state0[CAM:])


def test_rows_all_equal_to_c_are_r_uncertainty_c_on_a_frozen_map():
    ids, poses = fu.frame("ekf", 21, 6, seed=32)
    rows, _, _ = _frozen(row_noise=True)
    const, _, _ = _frozen(noise={"r_uncertainty": 0.37})
    rows.observe(ids, poses, noise=np.full(len(ids), 0.37))
    const.observe(ids, poses)
    _equal(rows, const)


def test_scaled_frozen_frame_is_the_plain_frame_with_the_products():
    from aruco_slam_amd.filters import extended_kalman_filter as mod
    ids, poses = fu.frame("ekf", 21, 6, seed=33)
    s = 2.75
    scaled, _, _ = _frozen(frame_scale=True)
    plain, _, _ = _frozen(noise={"q_cam": s * mod.Q_UNCERTAINTY_CAM, "q_err": s * mod.Q_ERROR_UNCERTAINTY_CAM,
                                 "q_lm": s * mod.Q_UNCERTAINTY_LM})
    scaled.observe(ids, poses, scale=s)
    plain.observe(ids, poses)
    _equal(scaled, plain)


def test_moved_frozen_frame_is_move_then_the_frozen_frame():
    ids, poses = fu.frame("ekf", 21, 6, seed=34)
    u = np.array([0.02, -0.01, 0.03, 0.004, -0.002, 0.006])
    a, _, _ = _frozen(motion=True)
    b, _, _ = _frozen(motion=True)
    a.observe(ids, poses, motion=u)
    b.move(u[:3], u[3:])
    b.observe(ids, poses)
    _equal(a, b)


def test_unstepped_frozen_frame_is_moved_and_leaves_its_scale_pending():
    flt, state0, p0 = _frozen(frame_scale=True, motion=True)
    moved, _, _ = _frozen(frame_scale=True, motion=True)
    u = np.array([0.02, -0.01, 0.03, 0.004, -0.002, 0.006])
    flt.observe([900, 901], np.ones((2, 6)), scale=1.5, motion=u)       # ids the map does not hold
    moved.move(u[:3], u[3:])
    assert flt.last_ignored == (900, 901) and flt.num_landmarks == 21 and 900 not in flt.landmarks
    assert flt.pending_scale == 1.5 and moved.pending_scale == 0.0
    _equal(flt, moved)
    state, p = fu.arrays(flt)
    assert np.array_equal(state[CAM:], state0[CAM:]) and np.array_equal(p[CAM:, CAM:], p0[CAM:, CAM:])
    # without a motion nothing changes at all; a mixed frame keeps the known detections
    still, _, _ = _frozen()
    still.observe([900], np.ones((1, 6)))
    assert np.array_equal(fu.arrays(still)[0], state0) and np.array_equal(fu.arrays(still)[1], p0)
    ids, poses = fu.frame("ekf", 21, 4, seed=35)
    mixed, _, _ = _frozen()
    mixed.observe(np.insert(ids, 1, 900), np.insert(poses, 1, np.ones(6), axis=0))
    still.observe(ids, poses)
    assert mixed.last_ignored == (900,)
    _equal(mixed, still)


# ---- 5. freeze -> unfreeze ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_unfrozen_filter_maps_on_like_one_restored_from_its_arrays(dtype):
    flt, _, _ = _frozen(dtype=dtype)
    s = fu.stream("ekf", 21, 6, seed=41)
    frames = list(s.steady(11))
    for ids, poses in frames[:10]:
        flt.observe(ids, poses)
    state, p = fu.arrays(flt)
    other = fu.ekf(21, 8, dtype=dtype, quat="scalar_first")
    fu.restore(other, state, p, [k for k, _ in sorted(flt.landmarks.items(), key=lambda kv: kv[1])])
    flt.unfreeze_map()
    assert not flt.map_frozen
    for f in (flt, other):
        f.observe(*frames[10])
    _equal(flt, other)
    assert not np.array_equal(fu.arrays(flt)[0][CAM:], state[CAM:])      # (mapping again)


def test_freeze_flag_survives_reset_only_as_off_and_travels_in_checkpoints(tmp_path):
    flt, _, _ = _frozen()
    flt.save_checkpoint(str(tmp_path / "frozen.npz"))
    other = fu.ekf(24, 8, quat="scalar_first")
    other.load_checkpoint(str(tmp_path / "frozen.npz"))
    assert other.map_frozen
    _equal(flt, other)
    flt.reset()
    assert not flt.map_frozen and flt.last_ignored == ()
    # C ABI: a log call that would add landmarks while frozen is refused before anything is enqueued
    import torch
    be = other.backend
    state, p = fu.arrays(other)
    idx = np.array([0, 21], dtype=np.int32)           # 21: a first sighting
    with pytest.raises(Exception) as err:
        be.observe_log(idx, np.array([0, 2]), np.ones((2, 6)), torch.empty((1, 7), dtype=torch.float64, device=be.device))
    assert err.value.code == -4 and "frozen" in str(err.value)      # EKF_ERR_STATE
    assert other.map_frozen and be.num_landmarks == 21
    for a, b in zip(fu.arrays(other), (state, p)):
        assert np.array_equal(a, b)
    assert other.backend.lib.ekf_get_map_frozen(None) == -1 and other.backend.lib.ekf_set_map_frozen(None, 1) == -1


def test_a_filter_that_was_never_frozen_computes_what_it_computed_before():
    """c1_detections through the per-frame call and the log call, either dtype: bit for bit the arrays the commit before
    the localisation mode produced (tests/golden/frozen_c1_parent.npz, recorded with tests/frozen_util.py:
    ``record_c1``), and so is a sequence call over 64 frames, which still reports the pipelined mode and is bit for bit the
    per-frame loop."""
    want = load_npz("frozen_c1_parent.npz")
    got = fu.record_c1()
    assert sorted(got) == sorted(want.files)
    for key in want.files:
        assert np.array_equal(got[key], want[key]), key
    # the sequence call on a mapping filter still pipelines
    seq, frames, idx_t, z_t = fu.sequence_run("float32")
    be = seq.backend
    assert be.last_sequence_mode() == "pipelined"
    assert np.array_equal(fu.arrays(seq)[1], want["seq_cov_float32"])
    loop = fu.ekf(32, 4, dtype="float32")
    for ids, poses in list(fu.stream("ekf", 32, 4, seed=9).bootstrap()) + frames:
        loop.observe(ids, poses)
    _equal(seq, loop)
    # ... and the same call on a frozen map runs in serial order
    seq.freeze_map()
    loop.freeze_map()
    be.observe_sequence(idx_t, z_t)
    be.sync()
    assert be.last_sequence_mode() == "serial"
    for ids, poses in frames:
        loop.observe(ids, poses)
    _equal(seq, loop)


# ---- the app loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True], ids=["per_frame", "resident"])
def test_run_slam_localize_writes_back_the_map_it_loaded(tmp_path, golden_dir, resident):
    from aruco_slam_amd.main import run_slam
    log = str(golden_dir / "c1_detections.npz")
    kw = {"max_landmarks": 16, "max_visible": 8}
    base = dict(video="input_video.mp4", filter="ekf", detections=log, filter_kwargs=kw)
    run_slam.main(argparse.Namespace(output_dir=str(tmp_path / "mapping"), resident=False, **base))
    made = tmp_path / "mapping" / "map.txt"
    run_slam.main(argparse.Namespace(output_dir=str(tmp_path / "loc"), resident=resident, map=str(made), localize=True, **base))
    assert (tmp_path / "loc" / "map.txt").read_bytes() == made.read_bytes()
    lines = (tmp_path / "loc" / "trajectory.txt").read_text().splitlines()
    assert len(lines) == 200
    assert np.isfinite(np.array([[float(v) for v in ln.split()] for ln in lines])).all()


# ---- state getters behind a frozen frame -----------------------------------------------------------------------------------
# A frozen frame writes the camera only, so the getter that follows it must not take the landmarks from a host mirror that
# the frames before it (a map file, a log, an add_marker, a wide frame) never filled.  No getter runs between the step that
# changes the device's landmarks and the frozen frame.
def _device_state(flt):
    flt.backend.sync()
    return flt.backend.state_t[:flt.backend.dims].cpu().numpy()


def _map_file(tmp_path, n=12):
    """A map.txt of ``n`` landmarks written by a mapping filter, and that filter's landmark state."""
    flt = fu.ekf(n, 8)
    s = fu.stream("ekf", n, 8, seed=51)
    for ids, poses in list(s.bootstrap()) + list(s.steady(3)):
        flt.observe(ids, poses)
    path = tmp_path / "made.txt"
    flt.save_map(str(path))
    return path, fu.arrays(flt)[0][CAM:]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stage"])
def test_getter_behind_the_first_frozen_frame_of_a_localising_filter(tmp_path, fused):
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    path, landmarks = _map_file(tmp_path)
    flt = EKF(fu.INIT, max_landmarks=12, max_visible=8, map_file=str(path), localize=True, fused=fused)
    assert flt.map_frozen and flt.num_landmarks == 12
    ids, poses = fu.frame("ekf", 12, 5, seed=52)
    flt.observe(ids, poses)                    # the first call after the constructor
    state = np.array(flt.state, dtype=np.float64)
    assert np.array_equal(state[CAM:], landmarks)      # (the map as the file holds it: written with repr precision)
    assert np.array_equal(state, _device_state(flt))
    assert not np.array_equal(state[:3], fu.INIT[:3])
    flt.save_map(str(tmp_path / "back.txt"))
    assert (tmp_path / "back.txt").read_bytes() == path.read_bytes()


def test_getter_behind_a_frozen_frame_after_a_mapping_log():
    log = _log("ekf", 12, (2, 8), 20, seed=53)
    flt, twin = fu.ekf(12, 8), fu.ekf(12, 8)
    for f in (flt, twin):
        f.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"])
    landmarks = fu.arrays(twin)[0][CAM:]       # (a full read back on the twin only)
    flt.freeze_map()
    ids, poses = fu.frame("ekf", 12, 5, seed=54)
    flt.observe(ids, poses)
    state = np.array(flt.state, dtype=np.float64)
    assert np.array_equal(state[CAM:], landmarks) and landmarks.any()
    assert np.array_equal(state, _device_state(flt))


def test_getter_behind_a_frozen_frame_after_add_marker_and_after_a_wide_frame():
    state0, p0, table = _prior("ekf", 21, "float64", "scalar_first")
    flt = fu.ekf(24, 8, quat="scalar_first")    # (room for one more: the buffers do not grow)
    fu.restore(flt, state0, p0, table)
    fu.arrays(flt)                              # a full read back: the mirror holds the 21 landmarks and is trusted
    flt.freeze_map()
    flt.add_marker(777, np.array([0.5, -0.25, 9.0]), np.array([0.3, 0.3, 0.3]))
    ids, poses = fu.frame("ekf", 21, 5, seed=55)
    flt.observe(ids, poses)
    state = np.array(flt.state, dtype=np.float64)
    assert state.shape == (CAM + 3 * 22,) and flt.landmarks[777] == 21 and state[-3:].any()
    assert np.array_equal(state, _device_state(flt))
    # a wide mapping frame (not mirrored) moves the landmarks; then freeze, a small frozen frame, the getter
    wide = fu.ekf(43, 66)
    state0, p0, table = _prior("ekf", 43, "float64", "as_written")
    fu.restore(wide, state0, p0, table)
    fu.arrays(wide)                             # a full read back: the mirror is trusted
    wide.observe(*fu.frame("ekf", 43, 6, seed=56))      # a mirrored mapping frame
    wide.observe(*fu.frame("ekf", 43, 66, seed=57))
    wide.freeze_map()
    wide.observe(*fu.frame("ekf", 43, 6, seed=58))
    state = np.array(wide.state, dtype=np.float64)
    assert np.array_equal(state, _device_state(wide))


# ---- the VALU reference kernel's chain step --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m", [(21, 6), (83, 33), (43, 130)])
def test_frozen_frame_is_bitwise_the_valu_mapping_frame_on_the_camera(n, m, dtype):
    frozen, mapping, state0, p0 = _pair("ekf", n, m, dtype, "scalar_first", True, cov_kernel="valu")
    ids, poses = fu.frame("ekf", n, m, seed=5 + m)
    for flt in (frozen, mapping):
        flt.observe(ids, poses)
    fu.assert_frozen_frame(frozen, mapping, state0, p0)
