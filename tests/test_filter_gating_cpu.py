"""The per-detection chi-square gate of the single filter (``EKF`` / ``EKF_Rotations``) without a GPU: the new C ABI is
declared and exported and validates what it can without a handle (a handle needs a device: the checks that need one --
a bad gate on a handle, ``ekf_set_gate`` without the flag -- are in ``test_filter_gating.py``), the workspace of a
configuration without ``EKF_FLAG_GATE`` is the size it was before the flag existed, the gate kernel's resources, the host
side of ``gate=`` / ``set_gate``, and the fixtures of ``test_filter_gating.py``: no expected distance lies within the
comparison margin of its gate."""
import ctypes as C
import re

import numpy as np
import pytest

import gating_util as gu
import support as sp
from support import lib

NEW_SYMBOLS = ("ekf_set_gate", "ekf_observe_gated", "ekf_observe_log_gated", "ekf_last_gate_stats")
# the seed of the free-running logs of test_filter_gating.py (gating_util.clean_log / dirty_log, family "column")
LOG_SEED = 0


def test_new_symbols_are_declared_and_exported(lib):
    from aruco_slam_amd import hip_backend
    sp.assert_abi(lib, NEW_SYMBOLS)
    header = sp.HEADER.read_text()
    assert re.search(r"EKF_FLAG_GATE = 64\b", header) and hip_backend.EKF_FLAG_GATE == 64
    # no handle: EKF_ERR_INVALID, nothing touched
    assert lib.ekf_set_gate(None, 11.345) == -1
    assert lib.ekf_last_gate_stats(None, (C.c_int64 * 2)()) == -1
    assert lib.ekf_observe_gated(None, None, None, 1, None, None, None) == -1
    assert lib.ekf_observe_log_gated(None, None, None, 0, None, None, 0, None, None) == -1


def test_sizes_without_the_flag_are_the_parents_and_the_flag_adds_the_gate_scratch(lib):
    from aruco_slam_amd.hip_backend import EKF_FLAG_GATE

    def pad(v):
        return -(-v // 256) * 256

    for (model, n, mv, dtype, flags), want in sp.PARENT_SIZES:
        assert sp.sizes(lib, model, n, mv, dtype, flags) == want, (model, n, mv, dtype, flags)
        ld, cb, sb, wb = sp.sizes(lib, model, n, mv, dtype, flags | EKF_FLAG_GATE)
        # survivors' indices and z (7 doubles per detection, as the staging of z) and the distances
        assert (ld, cb, sb) == want[:3] and wb == want[3] + pad(4 * mv) + pad(56 * mv) + pad(8 * mv)


def test_gate_kernel_uses_no_scratch_and_no_spill_and_its_own_lds_only():
    """Four instances (f32 / f64 covariance x two models): no scratch, no VGPR spill; the static LDS is what ekf_gate.hip
    declares: CHUNK detections of 90 (EKF, 64 per chunk) / 336 (EKF_Rotations, 16 per chunk) doubles and CHUNK ints."""
    found = sp.kernel_resources("ekf_gate.hip", r"ekf_frame_gate_kernel")
    assert len(found) == 4, found
    lds = {"Li0E": 64 * 90 * 8 + 64 * 4, "Li1E": 16 * 336 * 8 + 16 * 4}
    for name, res in found.items():
        want = next(v for k, v in lds.items() if k in name)
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, res)
        assert res["group_segment_fixed_size"] == want, (name, res)
    csrc = sp.REPO / "aruco_slam_amd" / "csrc"
    # (the kernel's measurement stage is the shared core's, and that one's model is ekf_device.h's, not a copy)
    assert "ekf_gate_measure<MODEL>" in (csrc / "ekf_gate.hip").read_text()
    assert "ekf_measure_model<MODEL>" in (csrc / "ekf_gate_device.h").read_text()


def test_gate_values_are_checked_on_the_host():
    from aruco_slam_amd.hip_backend import check_gate
    assert check_gate(None) is None and check_gate(7.815) == 7.815 and check_gate(np.inf) == np.inf
    for bad in (np.nan, 0.0, -1.0, -np.inf):
        with pytest.raises(ValueError, match="gate"):
            check_gate(bad)


def test_first_occurrences_marks_each_new_marker_once():
    from aruco_slam_amd.filters.base_filter import BaseFilter
    got = BaseFilter._first_occurrences([7, 3, 7, 9, 3, 9, 9], [3, 9])
    assert got.tolist() == [False, True, False, True, False, False, False]


def test_run_slam_and_replay_bench_take_a_gate():
    from aruco_slam_amd.main import run_slam
    assert run_slam.build_parser().parse_args([]).gate is None
    assert run_slam.build_parser().parse_args(["--gate", "11.345"]).gate == 11.345
    assert "--gate" in (sp.REPO / "tools" / "replay_bench.py").read_text()


@pytest.mark.parametrize("model", ["ekf", "ekf_rotations"])
def test_free_running_logs_are_clear_of_the_gate(model):
    """The dirty log the GPU tests replay: the f64 oracle rejects exactly the inserted detections, and no tested distance is
    within FREE_MARGIN (relative) of the gate."""
    clean = gu.clean_log(model, "column", seed=LOG_SEED)
    dirty, marks = gu.dirty_log(model, clean, seed=LOG_SEED)
    gate = gu.GATES[model]
    d2, rejected = gu.oracle_gated_replay(model, dirty, gate)
    assert np.array_equal(rejected, marks) and marks.any()
    tested = d2 > 0
    assert (np.abs(d2[tested] - gate) / d2[tested] > gu.FREE_MARGIN).all()
    offs = dirty["offsets"]
    assert any(marks[offs[t]:offs[t + 1]].all() for t in range(len(offs) - 1) if offs[t + 1] > offs[t])
