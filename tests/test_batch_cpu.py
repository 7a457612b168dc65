"""Batch of independent filters without a GPU: the host-side planning and validation of batch logs (what runs before the
library), construction without a device, and the register / LDS budget of the batch kernel."""
import re

import numpy as np
import pytest

import support as sp
from aruco_slam_amd.filters.base_filter import plan_detection_log


def _host_batch(members=3):
    """An EKFBatch without device state: observe_indexed records what would reach the library."""
    from aruco_slam_amd.batch import EKFBatch
    batch = object.__new__(EKFBatch)
    batch.members = members
    batch.landmarks = [{7: 0, 9: 1}, {}, {4: 0}]
    batch.num_landmarks = [2, 0, 1]
    batch.calls = []

    def observe_indexed(index, frame_offsets, member_frames, poses):
        batch.calls.append((index, frame_offsets, member_frames, poses))
        return np.zeros((int(member_frames[-1]), 7))

    batch.observe_indexed = observe_indexed
    batch._num_landmarks_device = lambda: np.array([4, 0, 2], dtype=np.int32)
    return batch


def _log(ids, counts, has=None):
    ids = np.asarray(ids, dtype=np.int32)
    poses = np.arange(6 * len(ids), dtype=np.float64).reshape(-1, 6)
    out = {"ids": ids, "poses": poses, "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64)}
    if has is not None:
        out["has_detections"] = np.asarray(has, dtype=bool)
    return out


def test_logs_are_planned_per_member_and_concatenated():
    batch = _host_batch()
    logs = [_log([9, 3, 3, 7, 5], [3, 0, 2]), None, _log([4, 8, 4], [2, 1], has=[True, False])]
    trajs = batch.process_detection_logs(logs)
    (index, fo, mf, poses), = batch.calls
    p0 = plan_detection_log({7: 0, 9: 1}, 2, logs[0]["ids"], logs[0]["offsets"])
    p2 = plan_detection_log({4: 0}, 1, logs[2]["ids"], logs[2]["offsets"], [True, False])
    assert list(index) == list(p0.index) + list(p2.index) == [1, 2, 2, 0, 3, 0, 1]
    assert list(fo) == [0, 3, 3, 5, 7, 7]              # member 2's second frame is not replayed (has_detections False)
    assert list(mf) == [0, 3, 3, 5]
    assert np.array_equal(poses, np.concatenate([logs[0]["poses"], logs[2]["poses"][:2]]))
    assert [t.shape for t in trajs] == [(3, 7), (0, 7), (2, 7)]
    # landmark tables follow the device's counts (all of member 0's new ids: 4 landmarks)
    assert batch.landmarks == [{7: 0, 9: 1, 3: 2, 5: 3}, {}, {4: 0, 8: 1}]
    assert batch.num_landmarks == [4, 0, 2]
    # a member that stopped early (fewer landmarks on the device than planned) keeps only those it added
    batch._num_landmarks_device = lambda: np.array([5, 0, 2], dtype=np.int32)
    batch.process_detection_logs([_log([11, 12], [2]), None, None])
    assert batch.landmarks[0] == {7: 0, 9: 1, 3: 2, 5: 3, 11: 4} and batch.num_landmarks[0] == 5


@pytest.mark.parametrize("case", ["count", "offsets", "ids_end", "poses", "has"])
def test_malformed_batch_logs_raise_before_the_library(case):
    batch = _host_batch()
    good = _log([9, 3], [1, 1])
    logs = [good, None, good]
    if case == "count":
        logs = [good, None]
    elif case == "offsets":
        logs[2] = dict(good, offsets=np.array([0, 2, 1]))
    elif case == "ids_end":
        logs[0] = dict(good, offsets=np.array([0, 1, 3]))
    elif case == "poses":
        logs[0] = dict(good, poses=np.zeros((2, 3)))
    elif case == "has":
        logs[2] = dict(good, has_detections=np.array([True]))
    with pytest.raises(ValueError):
        batch.process_detection_logs(logs)
    assert batch.calls == []
    assert batch.landmarks == [{7: 0, 9: 1}, {}, {4: 0}] and batch.num_landmarks == [2, 0, 1]


def test_no_batch_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from aruco_slam_amd import _build
    from aruco_slam_amd.batch import EKFBatch
    _build.build()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EKFBatch(4, np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0]))


def test_bad_arguments_raise_value_errors():
    from aruco_slam_amd.batch import EKFBatch
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    init = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="as_written"):
        EKFBatch(4, init, quat_update="scalar_last")
    with pytest.raises(ValueError, match="r_unc"):
        EKFBatch(4, init, noise={"r_unc": 0.5})
    with pytest.raises(ValueError, match="r_unc"):
        EKF(init, noise={"r_unc": 0.5})


def test_batch_config_limits_are_checked():
    import ctypes
    lib = sp.load_lib()
    cfg = sp.config(lib, max_visible=16)
    ld = ctypes.c_int64()
    assert lib.ekf_batch_query_sizes(ctypes.byref(cfg), 8, ctypes.byref(ld), None, None, None) == 0
    assert ld.value % 32 == 0 and 160 <= ld.value < 192          # N = 3 * 50 + 10
    for field, value in (("max_landmarks", 83), ("max_visible", 17), ("model", 1), ("cov_dtype", 1)):
        bad = sp.config(lib, **{"max_visible": 16, field: value})
        assert lib.ekf_batch_query_sizes(ctypes.byref(bad), 8, None, None, None, None) == -1, field
        if field in ("max_landmarks", "max_visible"):      # (batch errors reach the library's one error slot)
            assert field.encode() in lib.ekf_last_error_string(), field
    assert lib.ekf_batch_query_sizes(ctypes.byref(cfg), 0, None, None, None, None) == -1


def test_batch_kernel_uses_no_scratch_and_fits_the_lds():
    """No scratch memory, no spills, no static LDS; and the dynamic LDS the library requests for the largest batch (k = 3
    EKF_BATCH_MAX_VISIBLE rows, A/W rows of round_up(3 EKF_BATCH_MAX_LANDMARKS + 10 + 1, 4)) fits the 160 KiB of a CU."""
    import ctypes
    from aruco_slam_amd import _build
    found = sp.kernel_resources("ekf_batch.hip", r"ekf_batch_window_kernel")
    assert len(found) == 1, found
    for field in ("private_segment_fixed_size", "vgpr_spill_count"):
        assert [res[field] for res in found.values()] == [0], (field, found)
    static = [res["group_segment_fixed_size"] for res in sp.kernel_resources("ekf_batch.hip").values()]
    assert static == [0], static      # (the file's only kernel)
    header = (_build.CSRC / "ekf_kernels.h").read_text()
    max_lm = int(re.search(r"#define EKF_BATCH_MAX_LANDMARKS (\d+)", header).group(1))
    max_vis = int(re.search(r"#define EKF_BATCH_MAX_VISIBLE (\d+)", header).group(1))
    lib = sp.load_lib()
    lds_bytes = lib.ekf_batch_lds_bytes
    lds_bytes.argtypes, lds_bytes.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_size_t
    kmax, lda = 3 * max_vis, -(-(3 * max_lm + 11) // 4) * 4
    assert (kmax, lda) == (48, 260)
    need = 8 * (kmax * lda + kmax * kmax)              # at least A/W and L
    assert need < lds_bytes(kmax, lda) <= 160 * 1024
    assert lds_bytes(kmax, lda - 4) < lds_bytes(kmax, lda) and lds_bytes(kmax - 3, lda) < lds_bytes(kmax, lda)
