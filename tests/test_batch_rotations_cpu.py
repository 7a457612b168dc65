"""Batch of EKF_Rotations filters without a GPU: the capacity and convention checks of the batch C ABI for model 1, the
Python argument checks of ``EKFBatch(model="ekf_rotations")`` and the register / LDS budget of the rotations window
kernel."""
import ctypes
import re

import pytest

import support as sp

INIT = sp.INIT


def _lib():
    from aruco_slam_amd import hip_backend
    return hip_backend, sp.load_lib()


def _rot_config(hb, lib, **fields):
    return sp.config(lib, **{"model": 1, "quat_mode": hb.EKF_QUAT_SCALAR_FIRST, "max_landmarks": 24, "max_visible": 8,
                             **fields})


def test_rotations_batch_config_limits_are_checked():
    hb, lib = _lib()
    ld = ctypes.c_int64()
    cov, state = ctypes.c_size_t(), ctypes.c_size_t()
    cfg = _rot_config(hb, lib)
    assert lib.ekf_batch_query_sizes(ctypes.byref(cfg), 8, ctypes.byref(ld), ctypes.byref(cov), ctypes.byref(state),
                                     None) == 0
    assert ld.value == 256                                       # N = 10 * 24 + 10 = 250
    assert cov.value == 8 * 256 * 256 * 8 and state.value == 8 * 256 * 8
    for field, value in (("max_landmarks", 25), ("max_visible", 9), ("quat_mode", hb.EKF_QUAT_AS_WRITTEN),
                         ("cov_dtype", hb.EKF_COV_F32), ("max_landmarks", 0), ("max_visible", 0)):
        bad = _rot_config(hb, lib, **{field: value})
        assert lib.ekf_batch_query_sizes(ctypes.byref(bad), 8, None, None, None, None) == -1, field
        assert field.encode() in lib.ekf_last_error_string(), (field, lib.ekf_last_error_string())
        handle = ctypes.c_void_p()
        assert lib.ekf_batch_create(ctypes.byref(bad), 8, ctypes.byref(handle)) == -1 and not handle.value, field
    # the EKF model keeps its own limits: 82 / 16 pass there and are beyond the rotations model's
    ekf = _rot_config(hb, lib, model=0, quat_mode=hb.EKF_QUAT_AS_WRITTEN, max_landmarks=82, max_visible=16)
    assert lib.ekf_batch_query_sizes(ctypes.byref(ekf), 8, ctypes.byref(ld), None, None, None) == 0
    assert ld.value == 256                                       # N = 3 * 82 + 10 = 256
    bad = _rot_config(hb, lib, model=2)
    assert lib.ekf_batch_query_sizes(ctypes.byref(bad), 8, None, None, None, None) == -1


def test_rotations_batch_bad_arguments_raise_value_errors():
    from aruco_slam_amd.batch import EKFBatch
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    with pytest.raises(ValueError, match="model"):
        EKFBatch(4, INIT, model="rotations")
    with pytest.raises(ValueError, match="scalar_first"):
        EKFBatch(4, INIT, model="ekf_rotations", quat_update="as_written")
    with pytest.raises(ValueError, match="quat_update"):
        EKFBatch(4, INIT, model="ekf_rotations", quat_update="scalar_last")
    with pytest.raises(ValueError, match="r_unc"):
        EKFBatch(4, INIT, model="ekf_rotations", noise={"r_unc": 0.5})
    with pytest.raises(ValueError, match="r_unc"):
        EKF_Rotations(INIT, noise={"r_unc": 0.5})


def test_rotations_batch_kernel_uses_no_scratch_and_fits_the_lds():
    """The rotations window kernel, compiled alone: no scratch memory, no spills, no static LDS.  The dynamic LDS the library
    requests for the largest rotations batch (k = 7 * 8 rows, A/W rows of round_up(10 * 24 + 10 + 1, 4)) fits the 160 KiB
    of a CU and grows with both arguments."""
    from aruco_slam_amd import _build
    found = sp.kernel_resources("ekf_batch_rot.hip")
    names = list(found)
    assert len(names) == 1 and "ekf_batch_rot_window_kernel" in names[0], names
    assert [found[names[0]][k] for k in sp.BUDGET_FIELDS] == [0, 0, 0], found
    header = (_build.CSRC / "ekf_kernels.h").read_text()
    max_lm = int(re.search(r"#define EKF_BATCH_ROT_MAX_LANDMARKS (\d+)", header).group(1))
    max_vis = int(re.search(r"#define EKF_BATCH_ROT_MAX_VISIBLE (\d+)", header).group(1))
    _, lib = _lib()
    lds_bytes = lib.ekf_batch_rot_lds_bytes
    lds_bytes.argtypes, lds_bytes.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_size_t
    kmax, lda = 7 * max_vis, -(-(10 * max_lm + 11) // 4) * 4
    assert (kmax, lda) == (56, 252)
    need = 8 * (kmax * lda + kmax * kmax + kmax * 20)           # at least A/W, L and the 20-column Jacobian rows
    assert need < lds_bytes(kmax, lda) <= 160 * 1024
    assert lds_bytes(kmax, lda - 4) < lds_bytes(kmax, lda) and lds_bytes(kmax - 7, lda) < lds_bytes(kmax, lda)
    # the EKF kernel's size is its own
    ekf_bytes = lib.ekf_batch_lds_bytes
    ekf_bytes.argtypes, ekf_bytes.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_size_t
    assert ekf_bytes(kmax, lda) < lds_bytes(kmax, lda)
