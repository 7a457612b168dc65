"""Dictionary-sized batch maps (``EKF_FLAG_BATCH_LARGE_MAPS``) without a GPU: the limits the flag opens in the batch C ABI,
the workspace it adds, the LDS budget of a large-map call and the Python choice of the flag."""
import ctypes
import re

import pytest

import support as sp


def _lib():
    from aruco_slam_amd import hip_backend
    return hip_backend, sp.load_lib()


def _config(hb, lib, model, large=True, **fields):
    cfg = sp.config(lib)
    if model == 1:
        cfg.model, cfg.quat_mode, cfg.max_landmarks, cfg.max_visible = 1, hb.EKF_QUAT_SCALAR_FIRST, 101, 8
    else:
        cfg.model, cfg.max_landmarks, cfg.max_visible = 0, 338, 16
    if large:
        cfg.flags |= hb.EKF_FLAG_BATCH_LARGE_MAPS
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg


def test_flag_value():
    from aruco_slam_amd import hip_backend
    assert hip_backend.EKF_FLAG_BATCH_LARGE_MAPS == 16
    header = sp.HEADER.read_text()
    assert re.search(r"EKF_FLAG_BATCH_LARGE_MAPS = 16\b", header)


@pytest.mark.parametrize("model", [0, 1])
def test_large_map_limits_are_checked(model):
    hb, lib = _lib()
    rc, ld, cov, state, _ = sp.batch_query_sizes(lib, _config(hb, lib, model))
    assert rc == 0, lib.ekf_last_error_string()
    assert ld == 1024                       # EKF: N = 3 * 338 + 10 = 1024; EKF_Rotations: N = 10 * 101 + 10 = 1020
    assert cov == 4 * 1024 * 1024 * 8 and state == 4 * 1024 * 8
    bad_cases = [("max_landmarks", 339 if model == 0 else 102), ("max_landmarks", 0),
                 ("max_visible", 17 if model == 0 else 9), ("max_visible", 0), ("cov_dtype", hb.EKF_COV_F32)]
    if model == 1:
        bad_cases.append(("quat_mode", hb.EKF_QUAT_AS_WRITTEN))
    for field, value in bad_cases:
        bad = _config(hb, lib, model, **{field: value})
        assert lib.ekf_batch_query_sizes(ctypes.byref(bad), 4, None, None, None, None) == -1, field
        msg = lib.ekf_last_error_string()
        assert field.encode() in msg or (field == "cov_dtype" and b"EKF_COV_F64" in msg), (field, msg)
        handle = ctypes.c_void_p()
        assert lib.ekf_batch_create(ctypes.byref(bad), 4, ctypes.byref(handle)) == -1 and not handle.value, field
    # a map that the one-column kernel holds passes with the flag too, at that kernel's ld
    small = _config(hb, lib, model, max_landmarks=82 if model == 0 else 24)
    assert sp.batch_query_sizes(lib, small)[:2] == (0, 256)


@pytest.mark.parametrize("model", [0, 1])
def test_without_the_flag_nothing_changes(model):
    hb, lib = _lib()
    over = 83 if model == 0 else 25
    bad = _config(hb, lib, model, large=False, max_landmarks=over)
    assert lib.ekf_batch_query_sizes(ctypes.byref(bad), 4, None, None, None, None) == -1
    msg = lib.ekf_last_error_string()
    assert b"max_landmarks" in msg and (b"1..82" in msg if model == 0 else b"1..24" in msg), msg
    # workspace_bytes grows with the flag only: by members * rd * max_visible * ld * 8 (and its alignment)
    for lm in ((10, 82) if model == 0 else (3, 24)):
        plain = sp.batch_query_sizes(lib, _config(hb, lib, model, large=False, max_landmarks=lm))
        large = sp.batch_query_sizes(lib, _config(hb, lib, model, max_landmarks=lm))
        assert plain[0] == large[0] == 0 and plain[1:4] == large[1:4]
        rd, vis, ld = (3, 16, plain[1]) if model == 0 else (7, 8, plain[1])
        w = 4 * rd * vis * ld * 8
        assert w <= large[4] - plain[4] < w + 256, (plain, large)
    # at the largest map: at most about 450 KiB of A / W per member
    big = sp.batch_query_sizes(lib, _config(hb, lib, model), members=1)
    assert big[4] <= 460 * 1024 + 4096


def test_large_map_kernels_use_no_scratch_and_fit_the_lds():
    """A large-map batch runs the one-block instances of the kernels of ekf_batch_wide.hip (no scratch memory, no spills, no
    static LDS: test_batch_wide_frames_cpu.py); ekf_batch_large.hip is gone.  The dynamic LDS such a call gets at the
    largest kmax of each model fits the 160 KiB of a CU and does not depend on the map."""
    from aruco_slam_amd import _build
    assert "ekf_batch_large.hip" not in _build.SOURCES and not (_build.CSRC / "ekf_batch_large.hip").exists()
    assert "ekf_batch_wide.hip" in _build.SOURCES
    _, lib = _lib()
    lds = lib.ekf_batch_wide_lds_bytes
    lds.argtypes, lds.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_size_t
    for model, kmax, jc in ((0, 3 * 16, 13), (1, 7 * 8, 20)):
        need = 8 * (256 * kmax + kmax * kmax + kmax * jc)       # at least the column / panel region, L and J
        assert need < lds(model, kmax) <= 160 * 1024, (model, lds(model, kmax))
        assert lds(model, kmax - 4) < lds(model, kmax)
    assert lds(0, 48) < lds(1, 48)                              # (J has 20 columns in the rotations model)


@pytest.mark.parametrize("model,limit,top", [("ekf", 82, 338), ("ekf_rotations", 24, 101)])
def test_python_flag_choice(model, limit, top):
    from aruco_slam_amd import batch
    assert batch.COLUMN_MAX_LANDMARKS[model] == limit and batch.LARGE_MAX_LANDMARKS[model] == top
    for n, want_none in ((1, False), (limit, False), (limit + 1, True), (top, True)):
        assert batch.use_large_maps(model, n, None) is want_none, n
        assert batch.use_large_maps(model, n, True) is True, n
        assert batch.use_large_maps(model, n, False) is False, n
