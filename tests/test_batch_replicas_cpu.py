"""Replicas of one log and per-frame NIS / camera covariance in EKFBatch, without a GPU: the NumPy mirror of the replica
noise against the Philox4x32-10 known answers, the new C ABI (declared, exported, validated before any device work), the
register / LDS budget of the noise kernel and of the window kernels that write the new outputs, and the host side of
``replay_replicas`` / ``process_detection_logs(..., nis=, cam_cov=)``."""
import ctypes

import numpy as np
import pytest

import replica_util as ru
import support as sp
from support import lib

NEW_SYMBOLS = ("ekf_batch_observe_logs_diag", "ekf_batch_replica_poses", "ekf_batch_replica_workspace_bytes",
               "ekf_batch_observe_replicas")


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_mirror_reproduces_the_philox_known_answers(counter, key, want):
    assert tuple(int(x) for x in ru.philox4x32_10(counter, key)) == want


def test_mirror_noise_is_per_replica_and_detection():
    g = ru.normals(11, np.arange(16), np.arange(40))
    assert g.shape == (16, 40, 6) and np.isfinite(g).all()
    assert np.array_equal(ru.normals(11, np.arange(4, 12), np.arange(40)), g[4:12])      # (not a function of R)
    assert np.array_equal(ru.normals(11, [7], [33]), g[7:8, 33:34])
    assert not np.array_equal(ru.normals(12, np.arange(16), np.arange(40)), g)
    assert np.array_equal(ru.replica_poses(np.ones((40, 6)), 0.0, 11, 16), np.ones((16, 40, 6)))


def test_new_symbols_are_declared_and_exported(lib):
    sp.assert_abi(lib, NEW_SYMBOLS)


def test_replica_poses_validates_before_any_device_work(lib):
    """Bad sigma or replica range: EKF_ERR_INVALID before anything touches a device (no buffers are needed to find out)."""
    sig = np.full((3, 6), 0.01)
    fake = ctypes.c_void_p(256)        # (never dereferenced: validation fails first)
    dp = ctypes.POINTER(ctypes.c_double)

    def call(sigma, replicas=3, first=0):
        return lib.ekf_batch_replica_poses(fake, 10, np.ascontiguousarray(sigma).ctypes.data_as(dp), replicas, 5, first,
                                           fake, None)

    for bad in (-1.0, np.nan, np.inf):
        s = sig.copy()
        s[2, 4] = bad
        assert call(s) == -1, bad
        assert b"sigma" in lib.ekf_last_error_string()
    assert call(sig, 3, 2 ** 32 - 2) == -1
    assert b"2^32" in lib.ekf_last_error_string()
    assert call(sig, 0, 2 ** 32 - 1) == 0          # (nothing to do)
    assert lib.ekf_batch_replica_workspace_bytes(None, 1, 1, ctypes.byref(ctypes.c_size_t())) == -1


@pytest.mark.parametrize("src,pattern,count", [
    ("ekf_batch_replicas.hip", r"ekf_replica_poses_kernel", 1),
    ("ekf_batch.hip", r"ekf_batch_window_kernel", 1),
    ("ekf_batch_rot.hip", r"ekf_batch_rot_window_kernel", 1),
    ("ekf_batch_wide.hip", r"ekf_batch_wide_(rot_)?window_kernel", 2),
    ("ekf_batch_wide.hip", r"ekf_batch_one_block_(rot_)?window_kernel", 2),
])
def test_kernels_use_no_scratch_no_spill_no_static_lds(src, pattern, count):
    """No scratch memory, no VGPR spills (SGPR spills go to VGPR lanes, as before these outputs), no static LDS."""
    found = sp.kernel_resources(src, pattern)
    assert len(found) == count, found
    for name, res in found.items():
        assert [res[k] for k in sp.BUDGET_FIELDS] == [0, 0, 0], (name, res)


def test_window_kernels_dynamic_lds_is_unchanged(lib):
    """The new outputs live in HBM only: the LDS of every window kernel is what the layouts documented before them give
    (ekf_batch_impl.h; ekf_batch_wide.hip: R | L | 1 / L_jj | J of a block of at most 48 / 56 rows, y [kmax] and 64 + 4 /
    50 + 4 ints: with one block, as in a large-map call, 122,768 bytes at the EKF's kmax = 48 and 149,848 at the rotations'
    kmax = 56; 123,920 at the EKF's kmax = 192 and 152,200 at the rotations' kmax = 350)."""
    f = {}
    for name, args in (("ekf_batch_lds_bytes", [ctypes.c_int, ctypes.c_int]),
                       ("ekf_batch_rot_lds_bytes", [ctypes.c_int, ctypes.c_int]),
                       ("ekf_batch_wide_lds_bytes", [ctypes.c_int, ctypes.c_int])):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, ctypes.c_size_t
        f[name] = fn
    assert f["ekf_batch_lds_bytes"](48, 260) == 8 * (48 * 260 + 48 * 48 + 48 + 48 * 13 + 260) + 4 * (16 + 4)
    assert f["ekf_batch_rot_lds_bytes"](56, 260) == 8 * (56 * 260 + 56 * 56 + 56 + 56 * 20 + 260) + 4 * (8 + 4)
    assert f["ekf_batch_wide_lds_bytes"](0, 48) == 8 * (256 * 48 + 48 * 48 + 48 + 48 * 13 + 48) + 4 * (64 + 4) == 122768
    assert f["ekf_batch_wide_lds_bytes"](1, 56) == 8 * (256 * 56 + 56 * 56 + 56 + 56 * 20 + 56) + 4 * (50 + 4) == 149848
    assert f["ekf_batch_wide_lds_bytes"](0, 192) == 123920
    assert f["ekf_batch_wide_lds_bytes"](1, 350) == 8 * (256 * 56 + 56 * 56 + 56 + 56 * 20 + 350) + 4 * (50 + 4) == 152200


def test_sigma_shapes_and_values():
    from aruco_slam_amd.batch import replica_sigma
    assert np.array_equal(replica_sigma(0.5, 3), np.full((3, 6), 0.5))
    row = np.arange(6.0)
    assert np.array_equal(replica_sigma(row, 2), np.stack([row, row]))
    assert replica_sigma(np.ones((4, 6)), 4).flags.c_contiguous
    for bad in (-0.1, np.nan, np.inf, np.ones(5), np.ones((3, 6)), np.ones((4, 3))):
        with pytest.raises(ValueError, match="sigma"):
            replica_sigma(bad, 4)


@pytest.mark.parametrize("model,rd", [("ekf", 3), ("ekf_rotations", 7)])
def test_process_detection_logs_returns_per_member_statistics(model, rd):
    from aruco_slam_amd.batch import BatchReplay
    batch = sp.host_batch(3, model)
    log = {"ids": np.array([4, 4, 9, 9], np.int32), "poses": np.zeros((4, 6)), "offsets": np.array([0, 2, 2, 4]),
           "has_detections": np.array([True, False, True])}
    plain = batch.process_detection_logs([log, None, log])
    assert isinstance(plain, list) and [t.shape for t in plain] == [(3, 7), (0, 7), (3, 7)]
    out = batch.process_detection_logs([log, None, log], nis=True)
    assert isinstance(out, BatchReplay) and out.cam_cov is None
    assert [list(d) for d in out.dof] == [[2 * rd, 0, 2 * rd], [], [2 * rd, 0, 2 * rd]]      # duplicates count
    assert [list(v) for v in out.nis] == [[0, 1, 2], [], [3, 4, 5]]
    out = batch.process_detection_logs([None, log, None], cam_cov=True)
    assert out.nis is None and [c.shape for c in out.cam_cov] == [(0, 10, 10), (3, 10, 10), (0, 10, 10)]
    assert [c[4:] for c in batch.calls] == [(False, False), (True, False), (False, True)]


def test_replay_replicas_checks_before_the_library():
    batch = sp.host_batch(3)
    log = {"ids": np.array([1, 2], np.int32), "poses": np.zeros((2, 6)), "offsets": np.array([0, 1, 2])}
    batch.landmarks[1] = {5: 0}
    batch.num_landmarks[1] = 1
    with pytest.raises(ValueError, match="landmark table"):
        batch.replay_replicas(log, 0.01, 1)
    batch.landmarks[1], batch.num_landmarks[1] = {}, 0
    for kw in ({"sigma": -1.0}, {"sigma": np.ones((2, 6))}, {"sigma": np.nan}, {"first_replica": -1},
               {"first_replica": 2 ** 32 - 2}, {"seed": -3}):
        args = {"sigma": 0.01, "seed": 1, **kw}
        with pytest.raises(ValueError):
            batch.replay_replicas(log, args.pop("sigma"), args.pop("seed"), **args)
    with pytest.raises(ValueError):
        batch.replay_replicas(dict(log, offsets=np.array([0, 2, 1])), 0.01, 1)
    assert batch.calls == [] and batch.landmarks == [{}, {}, {}]
