"""Log replay (ekf_observe_log / BaseFilter.process_detection_log) without a GPU: the host-side planning of a ragged log
against the per-frame ``observe`` rules, rejection of malformed logs, the register budget of the new kernels and the
exported C ABI."""
import types

import numpy as np
import pytest

import support as sp
from aruco_slam_amd.filters.base_filter import BaseFilter, plan_detection_log


def _per_frame_indices(landmarks, ids, offsets, has):
    """What EKF.observe does frame by frame (extended_kalman_filter.py: the id -> index dict): a frame's unseen ids are
    added in order of first occurrence, then every detection is looked up.  Returns (indices, landmarks after)."""
    known = dict(landmarks)
    out = []
    for t in range(len(offsets) - 1):
        if not has[t]:
            continue
        frame = [int(i) for i in ids[offsets[t]:offsets[t + 1]]]
        fresh = []
        for i in frame:
            if i not in known and i not in fresh:
                fresh.append(i)
        for i in fresh:
            known[i] = len(known)
        out.extend(known[i] for i in frame)
    return np.asarray(out, dtype=np.int32), known


def _ragged_log(seed, frames=60, pool=40):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 9, size=frames)
    counts[5] = 0                                          # empty frames
    ids = [rng.integers(0, pool, size=c) for c in counts]
    ids[3] = np.array([31, 31, 7, 31, 7])                  # duplicates inside a frame with first sightings
    counts[3] = 5
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    return np.concatenate(ids).astype(np.int32), offsets, counts > 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_plan_matches_per_frame_observe(seed):
    ids, offsets, has = _ragged_log(seed)
    plan = plan_detection_log({}, 0, ids, offsets, has)
    want, known = _per_frame_indices({}, ids, offsets, has)
    np.testing.assert_array_equal(plan.index, want)
    assert plan.new_landmarks == known and list(plan.new_landmarks) == list(known)      # order of first occurrence
    assert plan.num_landmarks == len(known)
    np.testing.assert_array_equal(plan.offsets, offsets)
    assert plan.widest == int(np.diff(offsets).max())


def test_plan_after_map_restore_and_has_detections_false():
    """Landmarks restored before the log (map_file= / add_marker) keep their indices; new ids continue after them.  A frame
    whose has_detections is False is not replayed, whatever rows it has."""
    restored = {11: 0, 4: 1, 30: 2}
    ids = np.array([4, 99, 11, 99, 5, 5, 30, 6, 7], dtype=np.int32)
    offsets = np.array([0, 3, 4, 4, 6, 9], dtype=np.int64)
    has = np.array([True, True, False, True, False])
    plan = plan_detection_log(restored, 3, ids, offsets, has)
    want, known = _per_frame_indices(restored, ids, offsets, has)
    np.testing.assert_array_equal(plan.index, want)
    assert plan.new_landmarks == {99: 3, 5: 4}
    assert restored == {11: 0, 4: 1, 30: 2}                # (not modified)
    np.testing.assert_array_equal(plan.offsets, [0, 3, 4, 4, 6, 6])
    np.testing.assert_array_equal(plan.keep, [True] * 6 + [False] * 3)


def test_plan_split_into_two_calls():
    ids, offsets, has = _ragged_log(7)
    whole = plan_detection_log({}, 0, ids, offsets, has)
    cut = 30
    a = plan_detection_log({}, 0, ids[:offsets[cut]], offsets[:cut + 1], has[:cut])
    b = plan_detection_log(dict(a.new_landmarks), a.num_landmarks, ids[offsets[cut]:], offsets[cut:] - offsets[cut], has[cut:])
    np.testing.assert_array_equal(np.concatenate((a.index, b.index)), whole.index)
    assert {**a.new_landmarks, **b.new_landmarks} == whole.new_landmarks
    assert b.num_landmarks == whole.num_landmarks


class _HostOnly(BaseFilter):
    """A filter with a landmark table and a backend stub: enough for everything that runs before the device."""

    def __init__(self):
        super().__init__(np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0]))
        import torch
        self.landmarks = {3: 0, 8: 1}
        self.num_landmarks = 2
        self.backend = types.SimpleNamespace(device=torch.device("cuda:0"), max_landmarks=2, max_visible=2)


@pytest.mark.parametrize("case", ["non_monotonic", "offsets_end", "poses_shape", "poses_device", "empty_with_detections",
                                  "offsets_start"])
def test_malformed_logs_are_rejected_before_anything_runs(case):
    import torch
    ids = np.array([3, 8, 5, 8, 9], dtype=np.int32)
    offsets = np.array([0, 2, 3, 5], dtype=np.int64)
    poses = np.zeros((5, 6))
    has = np.ones(3, dtype=bool)
    if case == "non_monotonic":
        offsets = np.array([0, 3, 2, 5])
    elif case == "offsets_end":
        offsets = np.array([0, 2, 3, 4])
    elif case == "offsets_start":
        offsets = np.array([1, 2, 3, 5])
    elif case == "poses_shape":
        poses = np.zeros((5, 3))
    elif case == "poses_device":
        poses = torch.zeros((5, 6), dtype=torch.float64)       # a host tensor
    elif case == "empty_with_detections":
        offsets = np.array([0, 2, 2, 5])
    flt = _HostOnly()
    with pytest.raises(ValueError):
        flt.process_detection_log(ids, poses, offsets, has)
    assert flt.landmarks == {3: 0, 8: 1} and flt.num_landmarks == 2


def test_log_kernels_do_not_spill():
    """No scratch memory and no spills in the kernels of the log replay (ekf_log.hip)."""
    found = sp.kernel_resources("ekf_log.hip", r"ekf_log_")
    for kind in ("prepare", "add_markers", "fill_rows"):
        assert any(kind in n for n in found), kind
    assert len(found) >= 6, sorted(found)
    for name, res in found.items():
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (name, res)


def test_log_entry_points_are_exported():
    from aruco_slam_amd import hip_backend
    lib = sp.load_lib()
    for name in ("ekf_observe_log", "ekf_log_workspace_bytes", "ekf_last_log_stats"):
        assert name in hip_backend.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    header = sp.HEADER.read_text()
    for name in ("ekf_observe_log(", "ekf_log_workspace_bytes(", "ekf_last_log_stats("):
        assert name in header
