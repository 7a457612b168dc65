"""Camera motion without a GPU: the restatement of ``motion_util`` against finite differences and against the measurement
model it must be consistent with, the tracking fixture's condition on the oracle, the host side of ``motion=`` / ``move``, the
replay file handling of ``run_slam``, and the header.  ``test_motion.py`` runs the device against the same helpers."""
import json
import re

import numpy as np
import pytest

import motion_util as mu
import support as sp
import update_sweep_util as sw
from support import lib

NEW_SYMBOLS = ("ekf_move", "ekf_observe_moved", "ekf_observe_sequence_device_moved", "ekf_observe_log_moved",
               "ekf_batch_observe_logs_moved")
MODELS = ["ekf", "rot"]


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mu.STEP_MOTIONS))
def test_f_is_the_jacobian_of_the_state_map(name):
    """F of the wrapper against central differences of (c, q, e) -> (c + R((1, e) (x) q) d, q (x) delta, e), 1e-6 relative."""
    u = mu.STEP_MOTIONS[name]
    state, _p, _ids = mu.step_prior("ekf", 5, "float64")
    f, _c1, _q1 = mu.motion_parts(state[:10], u)
    num, h = np.zeros((10, 10)), 1e-6
    for k in range(10):
        xp, xm = state[:10].copy(), state[:10].copy()
        xp[k] += h
        xm[k] -= h
        num[:, k] = (mu.state_map(xp, u) - mu.state_map(xm, u)) / (2 * h)
    assert np.abs(f - num).max() <= 1e-6 * np.abs(num).max()
    # ... and the longdouble form is the same F
    assert np.abs(mu.extended_move(state[:10], np.eye(10), u)["F"] - f).max() <= 1e-15 * np.abs(f).max()


def test_f_is_the_identity_for_a_zero_motion():
    state, p, _ids = mu.step_prior("rot", 3, "float64")
    f, c1, q1 = mu.motion_parts(state[:10], np.zeros(6))
    assert np.array_equal(f, np.eye(10)) and np.array_equal(c1, state[0:3]) and np.array_equal(q1, state[3:7])
    orc = mu.with_move(sw.oracle_at("rot", state, p, [0, 1, 2]))
    orc.move(np.zeros(3), np.zeros(3))
    assert np.array_equal(orc.state, state) and np.array_equal(orc.uncertainty, p)
    # w = 0: the quaternion and its rows of F are untouched (bit rule 6(e))
    f, _c1, q1 = mu.motion_parts(state[:10], mu.STEP_MOTIONS["translation"])
    assert np.array_equal(f[3:10], np.eye(10)[3:10]) and np.array_equal(q1, state[3:7])


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", list(mu.STEP_MOTIONS))
def test_a_move_and_its_inverse_return_state_and_covariance(model, name):
    u = mu.STEP_MOTIONS[name]
    state, p, lm_ids = mu.step_prior(model, 6, "float64")
    orc = mu.with_move(sw.oracle_at(model, state, p, lm_ids))
    orc.move(u[0:3], u[3:6])
    assert not np.array_equal(orc.state, state) and not np.array_equal(orc.uncertainty, p)
    assert np.array_equal(orc.uncertainty, orc.uncertainty.T) and np.array_equal(orc.state[10:], state[10:])
    assert np.array_equal(orc.uncertainty[10:, 10:], p[10:, 10:]) and np.array_equal(orc.state[7:10], state[7:10])
    back = mu.inverse_motion(u)
    orc.move(back[0:3], back[3:6])
    assert np.abs(orc.state - state).max() <= 1e-12 * np.abs(state).max()
    assert np.abs(orc.uncertainty - p).max() <= 1e-12 * np.abs(p).max()


@pytest.mark.parametrize("name", list(mu.STEP_MOTIONS))
def test_predicted_measurements_move_with_the_camera(name):
    """h of every landmark changes under a motion exactly as R(delta)^T (h - d)."""
    from oracle.ekf_numpy import h_closed
    u = mu.STEP_MOTIONS[name]
    state, p, lm_ids = mu.step_prior("ekf", 12, "float64")
    orc = mu.with_move(sw.oracle_at("ekf", state, p, lm_ids))
    before = np.array([h_closed(np.concatenate((state[:10], state[10 + 3 * i:13 + 3 * i]))) for i in range(12)])
    orc.move(u[0:3], u[3:6])
    after = np.array([h_closed(np.concatenate((orc.state[:10], orc.state[10 + 3 * i:13 + 3 * i]))) for i in range(12)])
    want = (before - u[0:3]) @ mu.rotmat(mu.delta_quat(u[3:6]))      # rows: R(delta)^T (h - d)
    assert np.abs(after - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_step_sizes_name_the_workgroup_boundary():
    text = (sw.CSRC / "ekf_kernels.h").read_text()
    assert int(re.search(r"#define EKF_MOTION_THREADS (\d+)", text).group(1)) == mu.MOTION_THREADS
    for model, lmd in (("ekf", 3), ("rot", 10)):
        n = mu.BOUNDARY_N[model]
        assert lmd * (n - 1) <= mu.MOTION_THREADS < lmd * n and n in mu.STEP_SIZES[model]
        assert {0, 1, 40} <= set(mu.STEP_SIZES[model])
    assert np.isclose(np.linalg.norm(mu.STEP_MOTIONS["rotation"][3:]), 2.5)
    assert np.isclose(np.linalg.norm(mu.STEP_MOTIONS["tiny_w"][3:]), 1e-9) and not mu.STEP_MOTIONS["translation"][3:].any()


# ---- the stage functions, compiled for the host ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return sp.build_host_program("motion_host_main", tmp_path_factory.mktemp("motion_host"))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_host_build_of_the_stage_functions_is_inside_the_bound(host_program, model, dtype):
    """csrc/ekf_motion_device.h as the kernel calls it (tests/host/motion_host_main.hip) against the longdouble step, under
    the bound of the GPU test; P' bitwise symmetric, landmark block untouched, bit rule 6(e) for a pure translation."""
    for n in (0, 1, 7):
        state, p, _ids = mu.step_prior(model, n, dtype)
        for name, u in mu.STEP_MOTIONS.items():
            x1, p1 = mu.run_host_program(host_program, state, p, u, dtype)
            ref = mu.extended_move(state, p, u)
            r_p, r_c, r_q = mu.step_ratios(ref, p1, x1, dtype)
            assert max(r_p, r_c, r_q) <= 1.0, (model, dtype, n, name, r_p, r_c, r_q)
            assert np.array_equal(p1, p1.T) and np.array_equal(p1[10:, 10:], p[10:, 10:])
            if name == "translation":
                assert np.array_equal(x1[3:7], state[3:7])
                assert np.array_equal(p1[3:10, 3:], p[3:10, 3:]) and np.array_equal(p1[3:, 3:10], p[3:, 3:10])


# ---- the tracking fixture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_tracking_fixture_condition_on_the_oracle(model):
    """Mean position error over frames 5 .. 39 with odometry <= 1/5 of the error without, on the oracle alone.  The two
    numbers are recorded in profiles/motion/fixture.json."""
    scene = mu.tracking_scene(model)
    counts = np.diff(scene["offsets"])
    assert len(counts) == 40 and counts[0] == 10 and (counts[1:] == 4).all() and not scene["motion"][0].any()
    assert np.allclose(np.linalg.norm(np.diff(scene["truth"], axis=0), axis=1), 0.2, atol=1e-12)
    without, _ = mu.oracle_track(model, scene, False)
    with_odo, _ = mu.oracle_track(model, scene, True)
    e0, e1 = mu.mean_position_error(without, scene), mu.mean_position_error(with_odo, scene)
    assert e1 <= mu.TRACK_RATIO * e0, (e1, e0)
    recorded = json.loads((sw.REPO / "profiles" / "motion" / "fixture.json").read_text())[model]
    assert np.isclose(recorded["without_odometry_m"], e0, rtol=1e-6) and np.isclose(recorded["with_odometry_m"], e1, rtol=1e-6)


# ---- the host side --------------------------------------------------------------------------------------------------------
def test_motion_arrays_are_validated_on_the_host():
    from aruco_slam_amd.hip_backend import motion_array
    got = motion_array([1, 2, 3, 4, 5, 6])
    assert got.dtype == np.float64 and got.flags["C_CONTIGUOUS"] and got.tolist() == [1, 2, 3, 4, 5, 6]
    assert motion_array(np.zeros((4, 6), dtype=np.float32), 4).shape == (4, 6)
    for bad in ([1.0] * 5, np.zeros((1, 6)), 1.0, None, ["a"] * 6, [0, 0, 0, 0, 0, np.nan], [np.inf, 0, 0, 0, 0, 0]):
        with pytest.raises(ValueError, match="motion"):
            motion_array(bad)
    for bad in (np.zeros(6), np.zeros((3, 6)), np.zeros((4, 5)), np.full((4, 6), np.nan)):
        with pytest.raises(ValueError, match="motion"):
            motion_array(bad, 4)


class _Backend:
    def __init__(self, can):
        self.can_motion = can
        self.moved = []

    def move(self, u):
        self.moved.append(u)


def test_motion_on_a_filter_built_without_it_is_a_value_error_before_anything_changes():
    from aruco_slam_amd.filters.base_filter import BaseFilter
    flt = BaseFilter.__new__(BaseFilter)
    flt.backend = _Backend(False)
    assert flt._frame_motion(None) is None
    with pytest.raises(ValueError, match="motion=True"):
        flt._frame_motion(np.zeros(6))
    with pytest.raises(ValueError, match="motion=True"):
        flt.move([0.1, 0, 0], [0, 0, 0])
    flt.backend = _Backend(True)
    for d, w in (([0.1, 0], [0, 0, 0]), ([0.1, 0, 0], [0, 0, np.nan]), ([np.inf, 0, 0], [0, 0, 0]), (0.1, [0, 0, 0])):
        with pytest.raises(ValueError, match="motion"):
            flt.move(d, w)
    assert flt.backend.moved == [] and not flt._moved
    flt.move([0.1, 0, 0], [0, 0, 0.2])
    assert flt._moved and np.array_equal(flt.backend.moved[0], [0.1, 0, 0, 0, 0, 0.2])


def test_new_symbols_and_the_flag_are_declared_and_exported(lib):
    from aruco_slam_amd import hip_backend
    sp.assert_abi(lib, NEW_SYMBOLS)
    header = sp.HEADER.read_text()
    assert re.search(r"EKF_FLAG_MOTION = 512\b", header) and hip_backend.EKF_FLAG_MOTION == 512
    # no handle: EKF_ERR_INVALID, nothing touched
    u = np.zeros(6)
    up = u.ctypes.data_as(hip_backend.C.POINTER(hip_backend.C.c_double))
    assert lib.ekf_move(None, up) == -1
    assert lib.ekf_observe_moved(None, None, None, None, 1, None, None, None, 1.0, up) == -1
    assert lib.ekf_observe_sequence_device_moved(None, None, None, None, None, up, 1, 1, None) == -1
    assert lib.ekf_observe_log_moved(None, None, None, 0, None, None, None, up, None, 0, None, None) == -1
    assert lib.ekf_batch_observe_logs_moved(None, None, None, None, None, None, None, None, None, 0, None, None, None, None) == -1


def test_the_flag_changes_no_size(lib):
    from aruco_slam_amd.hip_backend import EKF_FLAG_MOTION
    for (model, n, mv, dtype, flags), want in sp.PARENT_SIZES:
        assert sp.sizes(lib, model, n, mv, dtype, flags | EKF_FLAG_MOTION) == want


def test_python_layer_takes_motion():
    import inspect
    from aruco_slam_amd import hip_backend
    from aruco_slam_amd.filters.base_filter import BaseFilter
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    for cls in (EKF, EKF_Rotations):
        assert inspect.signature(cls.__init__).parameters["motion"].default is False
        assert inspect.signature(cls.observe).parameters["motion"].default is None
    for fn in (BaseFilter.process_detections, BaseFilter.process_detection_log, hip_backend.HipEkf.observe,
               hip_backend.HipEkf.observe_sequence, hip_backend.HipEkf.observe_log):
        assert inspect.signature(fn).parameters["motion"].default is None
    assert list(inspect.signature(BaseFilter.move).parameters) == ["self", "d", "w"]
    from aruco_slam_amd import batch
    assert inspect.signature(batch.EKFBatch.__init__).parameters["motion"].default is False
    assert inspect.signature(batch.EKFBatch.observe_indexed).parameters["motion"].default is None


def test_run_slam_reads_the_motion_array_of_a_replay_file(tmp_path):
    from aruco_slam_amd.main import run_slam
    base = dict(ids=np.array([3, 4]), poses=np.zeros((2, 6)), offsets=np.array([0, 1, 1, 2]),
                timestamps_ms=np.array([0.0, 33.3, 66.6]), has_detections=np.array([True, False, True]))
    np.savez(tmp_path / "plain.npz", **base)
    assert run_slam.detection_motion(str(tmp_path / "plain.npz")) is None
    motion = np.arange(18.0).reshape(3, 6)
    np.savez(tmp_path / "odo.npz", motion=motion, **base)
    got = run_slam.detection_motion(str(tmp_path / "odo.npz"))
    assert np.array_equal(got, motion) and got.dtype == np.float64
    np.savez(tmp_path / "short.npz", motion=motion[:2], **base)
    with pytest.raises(ValueError, match="motion"):
        run_slam.detection_motion(str(tmp_path / "short.npz"))
    bad = motion.copy()
    bad[1, 2] = np.nan
    np.savez(tmp_path / "nan.npz", motion=bad, **base)
    with pytest.raises(ValueError, match="motion"):
        run_slam.detection_motion(str(tmp_path / "nan.npz"))
