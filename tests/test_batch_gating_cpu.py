"""The per-detection chi-square gate of EKFBatch without a GPU: the new C ABI is declared and exported, every batch
translation unit still compiles without scratch, VGPR spills or static LDS, the host side of ``gate`` / ``mahal``, and the
fixtures of ``test_batch_gating.py``: no expected distance lies within the comparison margin of its threshold."""
import numpy as np
import pytest

import gating_util as gu
import support as sp
from support import lib

NEW_SYMBOLS = ("ekf_batch_set_gate", "ekf_batch_observe_logs_gated", "ekf_batch_observe_replicas_gated")


def test_new_symbols_are_declared_and_exported(lib):
    sp.assert_abi(lib, NEW_SYMBOLS)
    assert lib.ekf_batch_set_gate(None, None) == -1          # (no handle: EKF_ERR_INVALID, nothing touched)


@pytest.mark.parametrize("src,pattern,count", [
    ("ekf_batch.hip", r"ekf_batch_window_kernel", 1),
    ("ekf_batch_rot.hip", r"ekf_batch_rot_window_kernel", 1),
    ("ekf_batch_wide.hip", r"ekf_batch_wide_(rot_)?window_kernel", 2),
    ("ekf_batch_wide.hip", r"ekf_batch_one_block_(rot_)?window_kernel", 2),
])
def test_gated_kernels_use_no_scratch_no_spill_no_static_lds(src, pattern, count):
    text = (sp.REPO / "aruco_slam_amd" / "csrc" / "ekf_batch_impl.h").read_text()
    assert "ekf_batch_gate" in text          # (the kernels compiled here hold the gate stage)
    found = sp.kernel_resources(src, pattern)
    assert len(found) == count, found
    for name, res in found.items():
        assert [res[k] for k in sp.BUDGET_FIELDS] == [0, 0, 0], (name, res)


def test_gate_array_shapes_and_values():
    from aruco_slam_amd.batch import gate_array
    assert gate_array(None, 3) is None
    assert np.array_equal(gate_array(7.815, 3), np.full(3, 7.815))
    assert np.array_equal(gate_array([1.0, np.inf, 3.0], 3), [1.0, np.inf, 3.0])
    for bad in (np.nan, 0.0, -1.0, -np.inf, [1.0, 2.0], [1.0, np.nan, 2.0], np.ones((3, 1))):
        with pytest.raises(ValueError, match="gate"):
            gate_array(bad, 3)


def test_process_detection_logs_returns_the_gated_type_only_when_asked():
    from aruco_slam_amd.batch import BatchReplay, GatedBatchReplay
    batch = sp.host_batch(2, "ekf")
    assert batch.gate is None          # (the class default: a batch has no gate until set_gate)
    plain = batch.observe_indexed

    def observe_indexed(index, fo, mf, poses, nis=False, cam_cov=False, mahal=False):
        if not mahal:
            return plain(index, fo, mf, poses, nis=nis, cam_cov=cam_cov)
        f = int(mf[-1])
        return np.zeros((f, 7)), None, None, np.arange(len(index), dtype=np.float64)

    batch.observe_indexed = observe_indexed
    log = {"ids": np.array([4, 4, 9, 7, 9], np.int32), "poses": np.zeros((5, 6)), "offsets": np.array([0, 2, 3, 5]),
           "has_detections": np.array([True, False, True])}
    assert isinstance(batch.process_detection_logs([log, None]), list)
    assert isinstance(batch.process_detection_logs([log, None], nis=True), BatchReplay)
    out = batch.process_detection_logs([log, log], mahal=True)
    assert isinstance(out, GatedBatchReplay) and not out.rejected[0].any()
    # the planner drops the detection of the frame without detections: NaN, and the device's values around it
    assert np.array_equal(out.mahal[0], [0, 1, np.nan, 2, 3], equal_nan=True)
    assert np.array_equal(out.mahal[1], [4, 5, np.nan, 6, 7], equal_nan=True)
    assert [list(d) for d in out.dof] == [[6, 0, 6], [6, 0, 6]]
    batch.gate = np.array([2.5, np.inf])
    out = batch.process_detection_logs([log, log])
    assert isinstance(out, GatedBatchReplay)
    assert list(out.rejected[0]) == [False, False, False, False, True] and not out.rejected[1].any()
    assert [list(d) for d in out.dof] == [[6, 0, 3], [6, 0, 6]]          # (survivors only)


@pytest.mark.parametrize("case", ["c1", "g5"])
def test_teacher_forced_distances_are_clear_of_the_gate(case):
    """Every expected d^2 of the C1 / G5 frames is outside the comparison tolerance of the gate, so the GPU test compares
    every decision; both decisions occur."""
    model, frames = gu.teacher_frames(case)
    gate, worst, rejected, total = gu.GATES[model], np.inf, 0, 0
    assert len(frames) >= 3
    for s0, p0, lm, ids, poses in frames:
        d2, kappa = gu.teacher_distances(model, s0, p0, lm, ids, poses)
        assert np.isfinite(d2).all() and (d2 > 0).all()
        for d, k in zip(d2, kappa):
            worst = min(worst, abs(d - gate) / d / gu.tolerance(k))
        rejected += int((d2 > gate).sum())
        total += len(d2)
        assert d2[-1] > gate          # (the appended outlier)
    assert worst > 10.0, worst
    assert 0 < rejected < total


@pytest.mark.parametrize("model,family", list(gu.FAMILIES))
def test_free_running_logs_are_clear_of_the_gate(model, family):
    """On the dirty log of every family the oracle rejects exactly the inserted detections, and no distance is within
    FREE_MARGIN of the gate."""
    clean = gu.clean_log(model, family, seed=0)
    dirty, marks = gu.dirty_log(model, clean, seed=0)
    offs = dirty["offsets"]
    assert marks.any() and (np.diff(offs) == 0).sum() == 2 and len(offs) - 1 > 64
    assert gu.extra_frames(dirty, marks).sum() == 2 + gu.STEADY // 11
    assert any(marks[offs[t]:offs[t + 1]].all() for t in range(len(offs) - 1) if offs[t + 1] > offs[t])
    gate = gu.GATES[model]
    d2, rejected = gu.oracle_gated_replay(model, dirty, gate)
    assert np.array_equal(rejected, marks)
    tested = d2 > 0
    assert (np.abs(d2[tested] - gate) / d2[tested] > gu.FREE_MARGIN).all()
    undone = gu.delete(dirty, marks)
    assert np.array_equal(undone["ids"], clean["ids"]) and np.array_equal(undone["poses"], clean["poses"])
    assert np.array_equal(undone["offsets"][1:][~gu.extra_frames(dirty, marks)], clean["offsets"][1:])
