"""Batch smoothing without a GPU: the exported symbols, the size of a batch history, the table the backward pass gets from
the words a recorded call leaves (``ekf_batch_history_table``: no handle, no device), the resources of the recording kernels,
and the fixtures the GPU tests judge the device by -- the growing scene under the bound, the replica condition on the oracle.
``test_batch_smooth.py`` runs the device against the same helpers."""
import numpy as np

import batch_smooth_util as bu
import motion_util as mu
import smooth_util as su
import support as sp
from support import lib

NEW_SYMBOLS = ("ekf_batch_history_bytes", "ekf_batch_observe_logs_recorded", "ekf_batch_history_info",
               "ekf_batch_history_record", "ekf_batch_history_table", "ekf_batch_smooth_workspace_bytes",
               "ekf_batch_smooth_history")


def test_new_symbols_are_declared_exported_and_refuse_a_null_handle(lib):
    from aruco_slam_amd import _build, hip_backend
    sp.assert_abi(lib, NEW_SYMBOLS)
    header = sp.HEADER.read_text()
    assert "ekf_batch_recorded.hip" in _build.SOURCES and "ekf_batch_smooth_host.h" in _build.HEADERS
    block = header[header.index("Batch smoothing: recorded replays"):]
    for word in ("EKF_MODEL_ROTATIONS", "EKF_QUAT_AS_WRITTEN", "EKF_FLAG_BATCH_LARGE_MAPS", "EKF_FLAG_BATCH_WIDE_FRAMES",
                 "frozen member", "past 50", "EKF_ERR_CAPACITY", "ekf_batch_reset", "ekf_batch_set_member",
                 "ekf_batch_remove_markers", "blocked tier", "smoothed covariances", "smoothed landmark outputs"):
        assert word in block, word
    # the single filter's section no longer lists the batch as missing
    single = header[header.index("Offline smoothing"):header.index("Batch smoothing: recorded replays")]
    assert "smoothed covariances, ekf_batch." not in single
    C = hip_backend.C
    n = C.c_size_t()
    assert lib.ekf_batch_history_bytes(None, None, None, None, 0, C.byref(n)) == -1
    assert lib.ekf_batch_observe_logs_recorded(None, None, None, None, None, None, None, None, None, 0, None, None, None,
                                               None, None, 0) == -1
    assert lib.ekf_batch_history_info(None, 0, None, 0, None, None, None, None, None, None) == -1
    assert lib.ekf_batch_history_record(None, None, 0, 0, None, None, 10) == -1
    assert lib.ekf_batch_smooth_workspace_bytes(None, C.byref(n)) == -1
    assert lib.ekf_batch_smooth_history(None, None, 0, None, 0, None, None) == -1
    assert lib.ekf_batch_history_table(0, None, None, None, None, None, None, None, 0, None, None, None, None, None, None) == -1


def test_history_bytes_restatement_equals_the_hand_count():
    """Two members: 3 frames that add 2, 0 and 1 markers (N = 16, 16, 19), and 1 frame that adds 1 (N = 13).  Regions:
    256 + 1280 + 1280 + 1792 and 256 + 1024; the call's words for 2 members and 4 frames: four pieces of 256 bytes, and a
    fifth for the motions.  An empty frame has a slot only in a call with motions (test_batch_smooth.py compares
    ekf_batch_history_bytes on a handle with the same counts)."""
    assert bu.record_bytes(16) == 1280 and bu.record_bytes(19) == 1792 and bu.record_bytes(13) == (13 + 91) * 8 + 192 == 1024
    assert bu.record_bytes(160) == (160 + 12880) * 8 + 128
    members = [[(16, True), (16, True), (19, True)], [(13, True)]]
    assert bu.history_bytes(members, False) == 4608 + 1280 + 4 * 256 == 6912
    assert bu.history_bytes(members, True) == 6912 + 256
    holes = [[(16, True), (16, False), (19, True)], []]
    assert bu.history_bytes(holes, False) == (256 + 1280 + 1792) + 256 + 4 * 256
    assert bu.history_bytes(holes, True) == (256 + 1280 + 1280 + 1792) + 256 + 5 * 256
    assert bu.history_bytes([[(160, True)] * 300], False) == 256 + 300 * 104448 + 256 + 2560 + 1280 + 2560


def test_table_from_the_flags_of_a_call(lib):
    """Three members over 5, 4 and 0 frames.  Member 0: an empty frame, a stepped one, one that was only moved, an unstepped
    one, a stepped one.  Member 1: a stepped frame, then it fails at its third frame.  Member 2 has no log."""
    mf = [0, 5, 9, 9]
    flag = [0, 1, 2, 0, 1, 1, 0, -1, -1]
    s_eff = [0.0, 1.5, 0.0, 0.0, 2.0, 1.0, 0.0, 0.0, 0.0]
    dims = [10, 16, 16, 16, 19, 13, 13, 13, 13]
    slot = [32, 128, 288, 448, 608, 1000, 1100, 1200, 1300]
    motion = np.zeros((9, 6))
    motion[2] = [0.1, 0, 0, 0, 0, 0.01]
    motion[4, 1] = -0.2
    noise = np.array([[1e2, 1e3, 1e-4, 0.3, 0.5, 0.01], [1e2, 1e3, 1e-4, 0.1, 0.7, 0.02], [1e2, 1e3, 1e-4, 0.3, 0.5, 0.01]])
    rows, member, rec_rows, q, moved = bu.table_from_flags(lib, mf, slot, dims, flag, s_eff, motion, noise)
    # (records, first row, end of the lead rows, first NaN row, end row)
    assert rows.tolist() == [[3, 0, 1, 5, 5], [1, 5, 5, 7, 9], [0, 9, 9, 9, 9]]
    assert member.tolist() == [0, 0, 0, 1]
    assert rec_rows.tolist() == [[1, 2], [2, 4], [4, 5], [5, 7]]      # every record's rows end where the next one's begin
    assert moved.tolist() == [0, 1, 1, 0]
    want = [1.5 * noise[0, 3:6], 0.0 * noise[0, 3:6], 2.0 * noise[0, 3:6], 1.0 * noise[1, 3:6]]      # fl(s_eff q), the member's q
    assert np.array_equal(q, np.array(want))
    # without motions nothing is moved; a member that has failed before the call has NaN rows only
    rows, member, rec_rows, q, moved = bu.table_from_flags(lib, [0, 2, 4], [0, 0, 0, 0], [10] * 4, [-1, -1, 0, 1], [0, 0, 0, 1.0],
                                                           None, noise[:2])
    assert rows.tolist() == [[0, 0, 0, 0, 2], [1, 2, 3, 4, 4]] and moved.tolist() == [0] and rec_rows.tolist() == [[3, 4]]


def test_recording_kernels_use_no_scratch_and_no_vgpr_spill():
    """The two RECORDED instances, like the instances they are built from: no scratch memory, no VGPR spill, no static LDS."""
    found = sp.kernel_resources("ekf_batch_recorded.hip", r"ekf_batch_recorded_(moved_)?window_kernel")
    assert len(found) == 2, found
    for name, res in found.items():
        assert [res[k] for k in sp.BUDGET_FIELDS] == [0, 0, 0], (name, res)


def test_growing_scene_reaches_the_resident_limit_with_room_under_the_bound():
    """growing_scene(16, 34, tail=2): 37 frames, the widest frame has 16 detections (the batch's max_visible), N grows by 3 per
    frame up to 160 inside the pass; the rule in plain f64 stays below 1/8 of the bound."""
    log = bu.scene_log("growing")
    assert len(log["offsets"]) - 1 == 37 and int(np.diff(log["offsets"]).max()) == 16
    records, filtered, start = su.oracle_records(log)
    assert [r["dims"] for r in records] == [58] + [61 + 3 * t for t in range(34)] + [160, 160]
    ref = su.smooth_records(records, 37, start)
    f64 = su.smooth_records(records, 37, start, np.float64)
    ratio = su.worst_ratio(f64["smoothed"], ref, records)
    print(f"growing scene, plain f64: worst error / bound = {ratio:.4f}, kappa <= {ref['kappa'].max():.1f}")
    assert ratio <= 0.125
    assert np.array_equal(f64["smoothed"][36:], filtered[36:])


def test_member_noise_reaches_the_oracle():
    """The oracle with a member's own q differs from the one with the default constants, and the patch is undone."""
    log = bu.scene_log("tracking")
    records, _filtered, start = su.oracle_records(log)
    base = su.smooth_records(records, 40, start)["smoothed"]
    other = bu.member_oracle(records, 40, start, [0, 0, 0, 0.1, 0.5, 0.02])["smoothed"]
    assert (su.Q_CAM, su.Q_ERR, su.Q_LM) == (0.3, 0.5, 0.01)
    assert np.abs((other - base).astype(np.float64)).max() > 1e-6
    assert np.array_equal(bu.member_oracle(records, 40, start, [0, 0, 0, 0.3, 0.5, 0.01])["smoothed"], base)


def test_replica_condition_holds_on_the_oracle():
    """Every replica of the tracking log that smooth_replicas(log, REPLICA_SIGMA, REPLICA_SEED) draws: on the oracle filter
    the smoothed mean position error is at most TRACK_SMOOTH_RATIO times the filtered one.  The device is judged by the same
    condition in test_batch_smooth.py."""
    log, replicas = bu.replica_logs()
    for r, rep in enumerate(replicas):
        assert not np.array_equal(rep["poses"][:, :3], log["poses"][:, :3])
        records, filtered, start = su.oracle_records(rep)
        ref = su.smooth_records(records, 40, start)
        e0 = mu.mean_position_error(filtered, log)
        e1 = mu.mean_position_error(ref["smoothed"].astype(np.float64), log)
        print(f"replica {r}: filtered {e0:.4f} m, smoothed {e1:.4f} m, ratio {e1 / e0:.3f}")
        assert e1 <= su.TRACK_SMOOTH_RATIO * e0, (r, e1, e0)
