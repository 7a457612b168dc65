"""Landmark removal (``ekf_remove_markers`` / ``ekf_batch_remove_markers``) without a GPU: the four new symbols are declared
and exported and validate what they can without a handle, ``ekf_query_sizes`` is what it was, the gather kernel's build
resources, the ``TentativeLandmarks`` policy on hand-written sequences and the id-table renumbering against ``np.delete``."""
import ctypes as C
import re

import numpy as np
import pytest

import support as sp
from support import lib

NEW_SYMBOLS = ("ekf_remove_workspace_bytes", "ekf_remove_markers", "ekf_batch_remove_workspace_bytes",
               "ekf_batch_remove_markers")


def test_new_symbols_are_declared_and_exported(lib):
    from aruco_slam_amd import hip_backend
    declared = set(re.findall(r"^(?:int|const char \*)\s*(ekf_\w+)\(", sp.HEADER.read_text(), re.M))
    assert declared == set(hip_backend.EXPORTED_SYMBOLS)
    sp.assert_abi(lib, NEW_SYMBOLS)
    # no handle: EKF_ERR_INVALID, nothing touched
    nbytes = C.c_size_t(77)
    assert lib.ekf_remove_workspace_bytes(None, 1, C.byref(nbytes)) == -1
    assert lib.ekf_batch_remove_workspace_bytes(None, 1, C.byref(nbytes)) == -1
    assert lib.ekf_remove_markers(None, None, 0, None, 0, None, None, 0) == -1
    assert lib.ekf_batch_remove_markers(None, None, None, None, 0, None, None, 0) == -1
    assert nbytes.value == 77


def test_query_sizes_are_what_they_were(lib):
    """A pin, not a test of the feature: it passes before the removal calls exist as well, and keeps passing only while the
    removal needs nothing from the workspace."""
    for (model, n, mv, dtype, flags), want in sp.PARENT_SIZES:
        assert sp.sizes(lib, model, n, mv, dtype, flags) == want, (model, n, mv, dtype, flags)


def test_gather_kernel_uses_no_scratch_and_no_spill():
    """Two instances (f32 / f64 covariance): no scratch, no VGPR spill, no LDS; the register counts are printed."""
    found = sp.kernel_resources("ekf_remove.hip", r"ekf_remove_gather_kernel")
    assert len(found) == 2, found
    for name, res in found.items():
        print(f"{name}: {res['vgpr_count']} VGPRs, {res['sgpr_count']} SGPRs")
        assert res["private_segment_fixed_size"] == 0 and res["vgpr_spill_count"] == 0, (name, res)
        assert res["sgpr_spill_count"] == 0 and res["group_segment_fixed_size"] == 0, (name, res)
        assert res["vgpr_count"] <= 128, (name, res)      # (at least four waves per SIMD: the kernel hides latency by occupancy)


# ---- the policy ----------------------------------------------------------------------------------------------------------
def _policy(hits, window):
    from aruco_slam_amd.filters.map_management import TentativeLandmarks
    return TentativeLandmarks(hits, window)


def test_policy_confirms_exactly_at_h_hits():
    p = _policy(2, 5)
    assert p.end_frame([7]) == []                   # t0 = 0: the first sighting is no hit
    assert p.end_frame([7]) == [] and 7 in p.tentative and p.tentative[7][1] == 1
    assert p.end_frame([7, 7]) == []                # second hit (two detections of one frame count once)
    assert 7 in p.confirmed and 7 not in p.tentative
    for _ in range(10):                             # confirmed for good
        assert p.end_frame([]) == []
    # two detections in the first-sighting frame are no hit either
    q = _policy(1, 3)
    assert q.end_frame([4, 4]) == [] and q.tentative[4] == [0, 0]
    assert q.end_frame([4]) == [] and 4 in q.confirmed


def test_policy_removes_exactly_at_the_window():
    p = _policy(2, 5)
    assert p.end_frame([1, 9]) == []                # t0 = 0 for both
    assert p.end_frame([1]) == []
    assert p.end_frame([1]) == []                   # 1 confirmed at t = 2
    assert p.end_frame([]) == []                    # t = 3: 3 - 0 + 1 = 4 < 5
    assert p.end_frame([]) == [9]                   # t = 4: 4 - 0 + 1 = 5 >= 5
    assert 9 not in p.tentative and 9 not in p.confirmed and 1 in p.confirmed
    # a landmark confirmed in the very frame its window closes stays
    q = _policy(2, 3)
    assert q.end_frame([5]) == [] and q.end_frame([5]) == [] and q.end_frame([5]) == []
    assert 5 in q.confirmed
    # returned in order of first sighting
    r = _policy(1, 2)
    assert r.end_frame([8, 3]) == [] and r.end_frame([]) == [8, 3]


def test_policy_does_not_count_frames_the_gate_rejected():
    p = _policy(1, 4)
    assert p.end_frame([2]) == []
    assert p.end_frame([2], [False]) == []          # rejected: no hit
    assert p.end_frame([2, 2], [False, False]) == []
    assert 2 in p.tentative and p.tentative[2][1] == 0
    assert p.end_frame([2], [False]) == [2]         # t = 3: the window closes
    q = _policy(1, 4)
    assert q.end_frame([2]) == []
    assert q.end_frame([2, 2], [False, True]) == []      # one used detection is enough
    assert 2 in q.confirmed
    with pytest.raises(ValueError):
        q.end_frame([1, 2], [True])


def test_policy_restarts_a_removed_id_and_keeps_map_file_landmarks():
    p = _policy(2, 3)
    p.confirm([40, 41])                             # restored from a map file
    assert p.end_frame([40, 6]) == []
    assert p.end_frame([]) == [] and p.end_frame([]) == [6]
    assert p.end_frame([6]) == []                   # seen again: t0 = 3, no hits carried over
    assert p.tentative[6] == [3, 0]
    assert p.end_frame([6]) == [] and p.end_frame([6]) == []
    assert 6 in p.confirmed
    for _ in range(8):
        assert p.end_frame([]) == []                # 40, 41 never come back
    assert {40, 41} <= p.confirmed
    p.forget([40])                                  # removed by hand: a first sighting when it is seen again
    assert p.end_frame([40]) == [] and p.tentative[40][1] == 0
    for bad in ((0, 5), (1, 1)):
        with pytest.raises(ValueError):
            _policy(*bad)


# ---- the id table --------------------------------------------------------------------------------------------------------
def test_renumbering_is_np_delete_on_the_index_array():
    from aruco_slam_amd.filters.map_management import renumber_landmarks
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 40):
        markers = rng.permutation(1000)[:n]         # marker id of landmark i
        table = {int(k): i for i, k in enumerate(markers)}
        for count in sorted({0, 1, n // 2, n}):
            removed = rng.permutation(n)[:count]    # unsorted
            got = renumber_landmarks(table, removed)
            kept = np.delete(markers, removed)      # marker ids in the new index order
            assert got == {int(k): i for i, k in enumerate(kept)}
            assert table == {int(k): i for i, k in enumerate(markers)}      # (not modified)
    with pytest.raises(ValueError):
        renumber_landmarks({5: 0, 6: 1}, [1, 1])
    with pytest.raises(ValueError):
        renumber_landmarks({5: 0, 6: 1}, [2])


def test_run_slam_takes_confirm():
    from aruco_slam_amd.main import run_slam
    assert run_slam.build_parser().parse_args([]).confirm is None
    assert run_slam.build_parser().parse_args(["--confirm", "2,5"]).confirm == (2, 5)
    assert run_slam.build_parser().parse_args(["--confirm", "2,5", "--gate", "11.345"]).gate == 11.345
    with pytest.raises(SystemExit):
        run_slam.build_parser().parse_args(["--confirm", "2"])
