"""Per-detection measurement noise without a GPU: the restated extended step is the oracle's when the rows are the
constant, the GPU cases of ``test_row_noise.py`` keep kappa(S) under the limit the componentwise bounds assume, their gate
cases are clear of the gate, the host side validates ``noise=`` / ``rows=``, and the header declares the entry points."""
import re

import numpy as np
import pytest

import gating_util as gu
import row_noise_util as rn
import support as sp
import update_sweep_util as sw
from support import lib

NEW_SYMBOLS = ("ekf_observe_rows", "ekf_observe_sequence_device_rows", "ekf_observe_log_rows", "ekf_batch_observe_logs_rows")
LOG_SEED = 0


@pytest.mark.parametrize("model,n,m", [("ekf", 20, 7), ("rot", 9, 4)])
def test_rows_equal_to_the_constant_give_the_extended_step_bit_for_bit(model, n, m):
    from oracle.ekf_extended import extended_step
    state, p, lm_ids, ids, poses = sw.dense_prior(model, n, m, 11)
    want = extended_step(sw.oracle_at(model, state, p, lm_ids), ids, poses, factors=True)
    got = rn.extended_step_rows(sw.oracle_at(model, state, p, lm_ids), ids, poses, np.full((m, rn.RD[model]), 0.9),
                                factors=True)
    assert set(got) == set(want)
    for key, v in want.items():
        assert np.array_equal(np.asarray(got[key]), np.asarray(v)), key
    # ... and other rows move it
    other = rn.extended_step_rows(sw.oracle_at(model, state, p, lm_ids), ids, poses, np.full((m, rn.RD[model]), 0.5))
    assert not np.array_equal(other["P1"], want["P1"])


def test_every_gpu_step_case_has_kappa_below_the_limit_of_the_bounds():
    """kappa(S) <= KAPPA_MAX for every case of test_row_noise.py's step test, both dtypes (an f32 filter starts from its own
    f32-rounded prior, another draw).  m = 200 is not a case: its kappa passes 1e3 even with rows in [0.6, 1.35]."""
    refs = rn.step_references()
    assert len(refs) == 2 * len(rn.STEP_CASES)
    for (case, dt), (_prior, rows, ref) in refs.items():
        lo, hi = case[6]
        assert rows.shape == (case[3], rn.RD[case[1]]) and (rows >= lo).all() and (rows <= hi).all()
        assert ref["kappa"] <= sw.KAPPA_MAX, (case, dt, ref["kappa"])
    # the boundaries of the dispatch (update_sweep_util.instances_of) are what the case list says they are
    groups = {(c[0], c[3]) for c in rn.STEP_CASES}
    assert {("ekf_fused", 64), ("ekf_wide", 69), ("ekf_wide", 128), ("ekf_blocked", 129), ("rot_fused", 27), ("rot_stage", 28),
            ("rot_stage", 50), ("rot_wide", 51), ("rot_blocked", 55)} <= groups
    for group, model, n, m, fused, mv, _r in rn.STEP_CASES:
        inst = sw.instances_of(sw.Case(group, model, "float64", n, m, "auto", fused, "as_written", mv))
        front = any(i[0] == "front" for i in inst)
        stage = any(i[0] == "solve" for i in inst)
        assert front == group.endswith("fused") and stage == (group.endswith("stage") or group.endswith("wide")), (group, m)


@pytest.mark.parametrize("model", ["ekf", "ekf_rotations"])
def test_gate_cases_are_clear_of_the_gate(model):
    """The dirty log of the GPU gate test with its rows: the oracle rejects exactly the inserted detections, and every
    tested distance is outside [0.5, 2] gate."""
    clean = gu.clean_log(model, "column", seed=LOG_SEED)
    dirty, marks = gu.dirty_log(model, clean, seed=LOG_SEED)
    rows = rn.log_rows(model, dirty, LOG_SEED)
    gate = gu.GATES[model]
    d2, rejected, _kappa = rn.oracle_gated_replay_rows(model, dirty, rows, gate)
    assert np.array_equal(rejected, marks) and marks.any()
    tested = d2 > 0
    ratio = d2[tested] / gate
    assert ((ratio < 0.5) | (ratio > 2.0)).all(), (ratio.min(), ratio.max())


@pytest.mark.parametrize("model", ["ekf", "ekf_rotations"])
def test_the_two_sided_gate_frame_decides_by_the_rows(model):
    """The frame of test_row_noise.py that shows rows reach the gate: under the constant detection 0 is rejected and
    detection 1 kept, under the rows (a large one for 0, a small one for 1) the other way round, each distance at least
    5 % of the gate away from it (the device and the oracle differ by rounding, gating_util.tolerance)."""
    frame = rn_two_sided(model)
    gate = gu.GATES[model]
    for d2, want in ((frame["d2_const"], [True, False]), (frame["d2_rows"], [False, True])):
        assert (d2[:2] > gate).tolist() == want and not (d2[2:] > gate).any()
        assert (np.abs(d2 - gate) / gate > 0.05).all(), d2 / gate


def rn_two_sided(model):
    return rn.two_sided_frame(model)


def test_noise_arguments_are_validated_on_the_host():
    from aruco_slam_amd.hip_backend import row_noise_array
    assert np.array_equal(row_noise_array([0.5, 2.0], 2, 3), [[0.5] * 3, [2.0] * 3])
    full = np.arange(1.0, 15.0).reshape(2, 7)
    got = row_noise_array(full, 2, 7)
    assert np.array_equal(got, full) and got.flags["C_CONTIGUOUS"] and got.dtype == np.float64
    for bad in ([0.5], [[0.5, 0.5], [1.0, 1.0]], np.ones((2, 3, 1)), 0.9, [0.5, np.nan], [0.5, np.inf], [0.5, 0.0],
                [0.5, -1.0], ["a", "b"], None):
        with pytest.raises(ValueError, match="noise"):
            row_noise_array(bad, 2, 3)
    with pytest.raises(ValueError, match="rows"):
        row_noise_array([1.0], 2, 3, "rows")


class _Backend:
    rows_per_detection = 3

    def __init__(self, can):
        self.can_row_noise = can


def test_noise_on_a_filter_built_without_row_noise_is_a_value_error():
    from aruco_slam_amd.filters.base_filter import BaseFilter
    flt = BaseFilter.__new__(BaseFilter)
    flt.backend = _Backend(False)
    assert flt._frame_noise(None, 4) is None
    with pytest.raises(ValueError, match="row_noise=True"):
        flt._frame_noise([0.9] * 4, 4)
    flt.backend = _Backend(True)
    assert flt._frame_noise([0.9] * 4, 4).shape == (4, 3)
    with pytest.raises(ValueError, match="noise"):
        flt._frame_noise([0.9] * 3, 4)


def test_new_symbols_and_the_flag_are_declared_and_exported(lib):
    from aruco_slam_amd import hip_backend
    sp.assert_abi(lib, NEW_SYMBOLS)
    header = sp.HEADER.read_text()
    assert re.search(r"EKF_FLAG_ROW_NOISE = 128\b", header) and hip_backend.EKF_FLAG_ROW_NOISE == 128
    # no handle: EKF_ERR_INVALID, nothing touched
    assert lib.ekf_observe_rows(None, None, None, None, 1, None, None, None) == -1
    assert lib.ekf_observe_sequence_device_rows(None, None, None, None, 1, 1, None) == -1
    assert lib.ekf_observe_log_rows(None, None, None, 0, None, None, None, 0, None, None) == -1
    assert lib.ekf_batch_observe_logs_rows(None, None, None, None, None, None, None, 0, None, None, None, None) == -1


def test_sizes_without_the_flag_are_the_parents_and_the_flag_adds_the_survivors_rows(lib):
    """Bit rule 2, the sizes: a configuration without EKF_FLAG_ROW_NOISE has the workspace it had before the flag existed
    (support.PARENT_SIZES).  The flag alone adds nothing to the device workspace (host rows are staged in
    the pinned slot, device rows are read where they are); with the gate it adds the survivors' rows, 8 RD max_visible
    bytes padded to 256."""
    from aruco_slam_amd.hip_backend import EKF_FLAG_GATE, EKF_FLAG_ROW_NOISE

    def pad(v):
        return -(-v // 256) * 256

    for (model, n, mv, dtype, flags), want in sp.PARENT_SIZES:
        rd = 7 if model == 1 else 3
        assert sp.sizes(lib, model, n, mv, dtype, flags) == want
        assert sp.sizes(lib, model, n, mv, dtype, flags | EKF_FLAG_ROW_NOISE) == want
        gated = sp.sizes(lib, model, n, mv, dtype, flags | EKF_FLAG_GATE)
        both = sp.sizes(lib, model, n, mv, dtype, flags | EKF_FLAG_GATE | EKF_FLAG_ROW_NOISE)
        assert both[:3] == gated[:3] and both[3] == gated[3] + pad(8 * rd * mv)


def test_batch_and_tools_take_row_noise():
    import inspect
    from aruco_slam_amd import batch
    assert "row_noise" in inspect.signature(batch.EKFBatch.__init__).parameters
    assert "noise" in inspect.signature(batch.EKFBatch.observe_indexed).parameters
    assert list(inspect.signature(batch.corner_row_noise).parameters)[:8] == [
        "log", "sigma_px", "seed", "replicas", "camera_matrix", "dist_coeffs", "marker_size", "model"]
    z = batch.replica_z(np.array([[[1.0, 2.0, 3.0, 0.0, 0.0, 0.0]]]), "ekf_rotations")
    assert z.shape == (1, 1, 7) and np.array_equal(z[0, 0], [1, 2, 3, 1, 0, 0, 0])
    assert np.array_equal(batch.replica_z(np.arange(6.0)[None], "ekf"), [[0, 1, 2]])
