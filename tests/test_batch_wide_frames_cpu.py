"""Wide batch frames (``EKF_FLAG_BATCH_WIDE_FRAMES``) without a GPU: the limits the flag opens in the batch C ABI, the
workspace it adds, the register / LDS budget of the wide-frame kernels and the Python choice of the flag."""
import ctypes
import re

import pytest

import support as sp

TOP = {0: (338, 64, 3), 1: (101, 50, 7)}      # model: (max_landmarks, max_visible, rows per detection) with the flag


def _lib():
    from aruco_slam_amd import hip_backend
    return hip_backend, sp.load_lib()


def _config(hb, lib, model, wide=True, large=False, **fields):
    cfg = sp.config(lib, model=model, max_landmarks=TOP[model][0], max_visible=TOP[model][1])
    if model == 1:
        cfg.quat_mode = hb.EKF_QUAT_SCALAR_FIRST
    if wide:
        cfg.flags |= hb.EKF_FLAG_BATCH_WIDE_FRAMES
    if large:
        cfg.flags |= hb.EKF_FLAG_BATCH_LARGE_MAPS
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg


def test_flag_value():
    from aruco_slam_amd import hip_backend
    assert hip_backend.EKF_FLAG_BATCH_WIDE_FRAMES == 32
    header = sp.HEADER.read_text()
    assert re.search(r"EKF_FLAG_BATCH_WIDE_FRAMES = 32\b", header)


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("large", [False, True])
def test_wide_frame_limits_are_checked(model, large):
    hb, lib = _lib()
    rc, ld, cov, state, _ = sp.batch_query_sizes(lib, _config(hb, lib, model, large=large))
    assert rc == 0, lib.ekf_last_error_string()
    assert ld == 1024 and cov == 4 * 1024 * 1024 * 8 and state == 4 * 1024 * 8
    lm, vis, _ = TOP[model]
    bad_cases = [("max_visible", vis + 1), ("max_visible", 0), ("max_landmarks", lm + 1), ("max_landmarks", 0),
                 ("cov_dtype", hb.EKF_COV_F32)]
    if model == 1:
        bad_cases.append(("quat_mode", hb.EKF_QUAT_AS_WRITTEN))
    else:
        bad_cases.append(("quat_mode", 7))
    for field, value in bad_cases:
        bad = _config(hb, lib, model, large=large, **{field: value})
        assert lib.ekf_batch_query_sizes(ctypes.byref(bad), 4, None, None, None, None) == -1, field
        msg = lib.ekf_last_error_string()
        assert field.encode() in msg or (field == "cov_dtype" and b"EKF_COV_F64" in msg), (field, msg)
        if field == "max_visible":
            assert b"EKF_FLAG_BATCH_WIDE_FRAMES" in msg and f"1..{vis}".encode() in msg, msg
        handle = ctypes.c_void_p()
        assert lib.ekf_batch_create(ctypes.byref(bad), 4, ctypes.byref(handle)) == -1 and not handle.value, field


@pytest.mark.parametrize("model", [0, 1])
def test_without_the_flag_nothing_changes(model):
    hb, lib = _lib()
    vis = 16 if model == 0 else 8
    for large in (False, True):
        bad = _config(hb, lib, model, wide=False, large=large, max_landmarks=10, max_visible=vis + 1)
        assert lib.ekf_batch_query_sizes(ctypes.byref(bad), 4, None, None, None, None) == -1
        msg = lib.ekf_last_error_string()
        assert b"max_visible" in msg and f"1..{vis}".encode() in msg and b"WIDE" not in msg, msg
    # sizes without the flag: as the one-column and the large-map kernels define them
    for large, lm in ((False, 10), (True, 10), (True, TOP[model][0])):
        rc, ld, cov, state, ws = sp.batch_query_sizes(lib, _config(hb, lib, model, wide=False, large=large, max_landmarks=lm,
                                                      max_visible=vis))
        assert rc == 0
        lmd, rd = (3, 3) if model == 0 else (10, 7)
        assert ld == -(-(lmd * lm + 10) // 32) * 32
        fixed = 4 * (6 * 8 + 4 + 4)
        w = 4 * rd * vis * ld * 8 if large else 0
        assert fixed + w <= ws < fixed + w + 3 * 256, (large, lm, ws)


@pytest.mark.parametrize("model", [0, 1])
def test_workspace_growth_follows_the_formula(model):
    """members * rd * max_visible * ld * 8 bytes beyond the flagless workspace, with or without bit 4 beside bit 5."""
    hb, lib = _lib()
    _, top_vis, rd = TOP[model]
    for lm in (1, 30, TOP[model][0]):
        for vis in (1, 17, top_vis):
            for members in (1, 5):
                plain = sp.batch_query_sizes(lib, _config(hb, lib, model, wide=False, large=True, max_landmarks=lm,
                                                          max_visible=1), members)
                assert plain[0] == 0
                w_plain = members * rd * 1 * plain[1] * 8
                for large in (False, True):
                    wide = sp.batch_query_sizes(lib, _config(hb, lib, model, large=large, max_landmarks=lm, max_visible=vis),
                                                members)
                    assert wide[0] == 0 and wide[1:4] == plain[1:4]
                    w = members * rd * vis * wide[1] * 8
                    assert w <= wide[4] - (plain[4] - w_plain) < w + 256, (lm, vis, members, large)


def test_wide_frame_kernels_use_no_scratch_and_fit_the_lds():
    """ekf_batch_wide.hip compiled alone: two kernels and their two one-block instances (the ones a large-map batch
    runs), no scratch memory, no spills, no static LDS.  The dynamic LDS of the largest kmax of each model fits the
    160 KiB of a CU."""
    from aruco_slam_amd import _build
    assert "ekf_batch_wide.hip" in _build.SOURCES
    resources = sp.kernel_resources("ekf_batch_wide.hip")
    names = list(resources)
    kernels = ("ekf_batch_wide_window_kernel", "ekf_batch_wide_rot_window_kernel", "ekf_batch_one_block_window_kernel",
               "ekf_batch_one_block_rot_window_kernel")
    assert len(names) == 4, names
    for kernel in kernels:
        assert any(kernel in n for n in names), kernel
    for kernel in kernels:
        found = sp.kernel_resources("ekf_batch_wide.hip", kernel)
        assert len(found) == 1, (kernel, found)
        for field in ("private_segment_fixed_size", "vgpr_spill_count"):
            assert [res[field] for res in found.values()] == [0], (kernel, field, found)
    assert [res["group_segment_fixed_size"] for res in resources.values()] == [0] * 4
    _, lib = _lib()
    lds = lib.ekf_batch_wide_lds_bytes
    lds.argtypes, lds.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_size_t
    for model, kw, jc in ((0, 48, 13), (1, 56, 20)):
        _, vis, rd = TOP[model]
        kmax = rd * vis
        need = 8 * (256 * kw + kw * kw + kw * jc + kmax)       # at least the column / panel region, L, J and y
        assert need < lds(model, kmax) <= 160 * 1024, (model, lds(model, kmax))
        assert lds(model, kmax - rd) < lds(model, kmax)
        # up to one block, as in a large-map call, the budget is the layout's regions and nothing more: R [256][kw] |
        # L [kw][kw] | 1 / L_jj [kw] | J [kw][jc] | y [kw] doubles and one first column per detection + 4 ints
        assert lds(model, kw) <= 8 * (256 * kw + kw * kw + kw + kw * jc + kw) + 4 * (vis + 4)


@pytest.mark.parametrize("model,plain,top", [("ekf", 16, 64), ("ekf_rotations", 8, 50)])
def test_python_flag_choice(model, plain, top):
    from aruco_slam_amd import batch
    assert batch.COLUMN_MAX_VISIBLE[model] == plain and batch.WIDE_MAX_VISIBLE[model] == top
    for m, want_none in ((1, False), (plain, False), (plain + 1, True), (top, True)):
        assert batch.use_wide_frames(model, m, None) is want_none, m
        assert batch.use_wide_frames(model, m, True) is True, m
        assert batch.use_wide_frames(model, m, False) is False, m
