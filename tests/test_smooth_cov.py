"""Smoothed covariances on the device: ``ekf_smooth_history_cov`` against the longdouble oracle of ``smooth_cov_util`` under
its bound (the oracle is fed the device's own records), the bit rules, the refusals, and the way up through
``EKF.smooth_detection_log(cov=True)``, ``get_cam_estimate_cov`` and ``run_slam --smooth-cov``.  One recorded replay and
one pass per scene (``smooth_cov_util.device_case``) serve every test that reads them."""
import numpy as np
import pytest

import motion_util as mu
import smooth_cov_util as sc
import smooth_util as su

pytestmark = pytest.mark.gpu


# ---- 1. against the oracle under the bound ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.GPU_SCENES)
def test_covariances_against_the_oracle_under_the_bound(name):
    """cam_cov on every frame and first_cov on all entries: n18 (N = 64, one block), n19 (N = 67, ragged second block), the
    growing log (dims 61, 64, 67, 70: npad 64 -> 128 inside the pass, P^s_{r+1} cut to N_r), ragged (motions, moved-only
    records with s_eff = 0, scales), tracking (40 steps), n49_52 (three blocks), n82 (N = 256: four blocks, no padding row)
    and g81_2 (dims 253, 256, 259, 259: npad 256 -> 320 inside the pass).  Measured worst error / bound on one MI355X
    (cam_cov / first_cov): 0.0032 / 0.0050, 0.0041 / 0.0065, 0.0016 / 0.0053, 0.0080 / 0.0000, 0.0061 / 0.0006,
    0.0017 / 0.0043, 0.0018 / 0.0078, 0.0015 / 0.0078.  (NaN rows before the first record and frames that share a
    record: the next test.)"""
    case = sc.device_case(name)
    out, records, ref, frames = case["out"], case["records"], case["ref"], case["frames"]
    cam, fb, rec_of = sc.frame_rows(ref, records, frames)
    lead = rec_of < 0
    assert np.isnan(out["cam_cov"][lead]).all() and np.isnan(out["filt_cam_cov"][lead]).all()
    assert np.isfinite(out["cam_cov"][~lead]).all()
    err = np.abs(out["cam_cov"][~lead].astype(sc.LD) - cam[~lead]).astype(np.float64).max(axis=(1, 2))
    r_cam = float((err / fb[~lead]).max())
    n0 = records[0]["dims"]
    assert out["first_cov"].shape == (n0, n0)
    r_first = float(np.abs(out["first_cov"].astype(sc.LD) - ref["Ps"][0]).max()) / sc.record_bound(ref, records)[0]
    print(f"{name}: worst error / bound: cam_cov {r_cam:.4f}, first_cov {r_first:.4f}")
    assert r_cam <= 1.0 and r_first <= 1.0
    if name == "ragged":      # (frame 0 is moved, so it is a record: the next test has the NaN rows and the shared records)
        assert lead.sum() == 0 and sum(not r["stepped"] for r in records) == 5 and any(r["u"].any() for r in records)
    if name == sc.GROWING:
        assert [r["dims"] for r in records][:4] == [61, 64, 67, 70]
        filt0 = records[0]["P"][:10, :10]      # returning the filtered covariance would miss by orders of magnitude
        assert np.abs(out["cam_cov"][records[0]["frame"]] - filt0).max() >= 1e6 * fb[records[0]["frame"]]


def test_frames_before_the_first_record_and_frames_that_share_a_record():
    """A log whose first two frames are empty and whose frame 4 is empty: NaN covariance rows before the first record, the
    start pose in `smoothed`, and frame 4 repeats the rows of frame 3."""
    base = su.growing_scene(5, 2, tail=2)
    offs = base["offsets"]
    counts = np.diff(offs)
    new_counts = np.concatenate(([0, 0], counts[:2], [0], counts[2:]))
    log = {"ids": base["ids"], "poses": base["poses"], "offsets": np.concatenate(([0], np.cumsum(new_counts))).astype(np.int64)}
    flt = sc.new_filter()
    traj, history = sc.recorded_replay(flt, log)
    frames = traj.shape[0]
    out = {k: v.cpu().numpy() for k, v in flt.backend.smooth_history_cov(history, frames).items()}
    records, info = su.device_records(flt.backend, history)
    assert info["frame_record"].tolist()[:5] == [-1, -1, 0, 1, 1]
    assert np.isnan(out["cam_cov"][:2]).all() and np.isnan(out["filt_cam_cov"][:2]).all()
    assert np.array_equal(out["smoothed"][:2], np.tile(sc.INIT[:7], (2, 1)))
    assert np.array_equal(out["cam_cov"][4], out["cam_cov"][3]) and np.array_equal(out["filt_cam_cov"][4], out["filt_cam_cov"][3])
    ref = sc.smooth_cov_records(records)
    cam, fb, rec_of = sc.frame_rows(ref, records, frames)
    ok = rec_of >= 0
    err = np.abs(out["cam_cov"][ok].astype(sc.LD) - cam[ok]).astype(np.float64).max(axis=(1, 2))
    assert (err <= fb[ok]).all()


# ---- 2. bit rules ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", sc.GROWING, "g81_2"])
def test_bit_rules(name):
    case = sc.device_case(name)
    out, records, frames, flt, history = case["out"], case["records"], case["frames"], case["flt"], case["history"]
    b = flt.backend
    # the state half keeps the bits of the forced-blocked state pass
    assert np.array_equal(out["smoothed"], case["blocked"])
    # filtered rows are the records' own camera blocks; the last record's smoothed rows are its filtered ones
    _cam, _fb, rec_of = sc.frame_rows(case["ref"], records, frames)
    for t in range(frames):
        if rec_of[t] >= 0:
            assert np.array_equal(out["filt_cam_cov"][t], records[rec_of[t]]["P"][:10, :10]), t
    last = records[-1]["frame"]
    assert np.array_equal(out["cam_cov"][last:], out["filt_cam_cov"][last:])
    # bitwise symmetric
    assert np.array_equal(out["first_cov"], out["first_cov"].T)
    ok = rec_of >= 0
    assert np.array_equal(out["cam_cov"][ok], out["cam_cov"][ok].transpose(0, 2, 1))
    # repeatable, and read-only: state and P of the filter are where the replay left them
    again = {k: v.cpu().numpy() for k, v in b.smooth_history_cov(history, frames).items()}
    for key in ("smoothed", "cam_cov", "filt_cam_cov", "first_cov"):
        assert np.array_equal(out[key], again[key], equal_nan=True), key
    assert np.array_equal(b.get_state(), case["state"]) and np.array_equal(b.get_cov(), case["P"])
    # a plain ekf_smooth_history afterwards returns its own bits, in both tiers
    assert np.array_equal(b.smooth_history(history, frames, blocked=True).cpu().numpy(), case["blocked"])
    plain = b.smooth_history(history, frames).cpu().numpy()
    assert np.array_equal(plain, b.smooth_history(history, frames).cpu().numpy())
    assert np.abs(plain - case["blocked"]).max() <= 1e-9


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------
def _direct_call(b, history, ws_bytes=None):
    """ekf_smooth_history_cov through the library itself, with outputs that show whether anything was written."""
    import torch
    ws = torch.zeros((1 << 20,), dtype=torch.uint8, device=b.device)
    outs = [torch.full((14 * n,), 7.0, dtype=torch.float64, device=b.device) for n in (7, 100, 100)]
    rc = b.lib.ekf_smooth_history_cov(b.h, history.data_ptr(), history.numel(), ws.data_ptr(),
                                      ws.numel() if ws_bytes is None else ws_bytes, 0, outs[0].data_ptr(), outs[1].data_ptr(),
                                      outs[2].data_ptr(), None)
    b.sync()
    torch.cuda.synchronize(b.device)
    assert all(bool((o == 7.0).all()) for o in outs)      # nothing was enqueued
    return rc


@pytest.mark.parametrize("kw", [{"quat_update": "as_written"}, {"cov_dtype": "float32"}])
def test_configurations_that_are_not_supported_are_refused(kw):
    import torch
    flt = sc.new_filter(motion=True, **kw)
    b = flt.backend
    history = torch.zeros((4096,), dtype=torch.uint8, device=b.device)
    before = (b.get_state(), b.get_cov())
    assert _direct_call(b, history) == -4      # EKF_ERR_STATE
    assert np.array_equal(before[0], b.get_state()) and np.array_equal(before[1], b.get_cov())


def test_a_stale_history_and_a_short_workspace_are_refused():
    from aruco_slam_amd import hip_backend
    from aruco_slam_amd.hip_backend import EkfError
    log, motion, scale = sc.scene("ragged")
    flt = sc.new_filter(motion=True, frame_scale=True)
    _traj, history = sc.recorded_replay(flt, log, motion, scale)
    b = flt.backend
    need = hip_backend.C.c_size_t()
    assert b.lib.ekf_smooth_cov_workspace_bytes(b.h, hip_backend.C.byref(need)) == 0
    assert 0 < need.value < (1 << 20)
    assert _direct_call(b, history, need.value - 1) == -1      # EKF_ERR_INVALID: one byte short
    with pytest.raises(EkfError) as err:
        b.smooth_history_cov(history, 14, ws_bytes=need.value - 1)
    assert err.value.code == -1
    assert b.smooth_history_cov(history, 14, ws_bytes=need.value)["cam_cov"].shape == (14, 10, 10)
    # after a second recorded call the first buffer is refused
    sl = slice(int(log["offsets"][-2]), int(log["offsets"][-1]))
    tail = {"ids": log["ids"][sl], "poses": log["poses"][sl], "offsets": np.array([0, sl.stop - sl.start]),
            "has_detections": np.array([True])}
    _t, second = sc.recorded_replay(flt, tail, np.zeros((1, 6)), np.ones(1))
    assert _direct_call(b, history) == -4
    with pytest.raises(EkfError) as err:
        b.smooth_history_cov(history, 14)
    assert err.value.code == -4
    out = b.smooth_history_cov(second, 1)      # one record: P^s_0 = P_0
    _x, p0 = b.history_record(second, 0, int(b.history_info()["dims"][0]))
    assert np.array_equal(out["first_cov"].cpu().numpy(), p0)


# ---- 4. top level ----------------------------------------------------------------------------------------------------------
def test_smooth_detection_log_with_cov_and_run_slam(tmp_path):
    from aruco_slam_amd.main import run_slam
    scene = mu.tracking_scene("ekf")
    case = sc.device_case("tracking")
    flt, twin = sc.new_filter(n=10, m=10), sc.new_filter(n=10, m=10)
    filtered, smoothed, filtered_cov, smoothed_cov = flt.smooth_detection_log(scene["ids"], scene["poses"], scene["offsets"],
                                                                             cov=True)
    plain = twin.smooth_detection_log(scene["ids"], scene["poses"], scene["offsets"])
    assert len(plain) == 2 and np.array_equal(filtered, plain[0])
    assert np.abs(smoothed - plain[1]).max() <= 2 * su.bound(su.smooth_records(case["records"], 40, sc.INIT), case["records"]).max()
    assert filtered_cov.shape == smoothed_cov.shape == (40, 10, 10)
    assert np.array_equal(smoothed_cov, case["out"]["cam_cov"]) and np.array_equal(filtered_cov, case["out"]["filt_cam_cov"])
    # smoothing never adds uncertainty: position block of P^s below the filtered one, eigenvalues with the bound as slack
    _cam, fb, _rec_of = sc.frame_rows(case["ref"], case["records"], 40)
    ratios = []
    for t in range(40):
        gap = np.linalg.eigvalsh(filtered_cov[t, :3, :3] - smoothed_cov[t, :3, :3]).min()
        assert gap >= -3 * fb[t], (t, gap)
        ratios.append(np.trace(smoothed_cov[t, :3, :3]) / np.trace(filtered_cov[t, :3, :3]))
    print(f"tracking scene: smoothed / filtered position variance {min(ratios):.3f} ... {max(ratios):.3f}")
    assert min(ratios) < 0.9 and max(ratios) <= 1.0
    # get_cam_estimate_cov
    assert np.array_equal(flt.get_cam_estimate_cov(7), smoothed_cov[7])
    with pytest.raises(IndexError):
        flt.get_cam_estimate_cov(40)
    with pytest.raises(NotImplementedError):
        twin.get_cam_estimate_cov(0)
    d2_out = sc.new_filter(n=10, m=10, gate=1e300).smooth_detection_log(scene["ids"], scene["poses"], scene["offsets"],
                                                                       mahal=True, cov=True)
    assert len(d2_out) == 5 and d2_out[4].shape == (len(scene["ids"]),) and d2_out[3].shape == (40, 10, 10)
    # run_slam --smooth --smooth-cov writes the same arrays
    stamps = 33.3 * np.arange(40)
    np.savez(tmp_path / "log.npz", ids=scene["ids"], poses=scene["poses"], offsets=scene["offsets"], timestamps_ms=stamps,
             has_detections=np.ones(40, dtype=bool))
    run_slam.main(run_slam.build_parser().parse_args(["--detections", str(tmp_path / "log.npz"), "--resident", "--smooth",
                                                      "--smooth-cov", str(tmp_path / "cov.npz"),
                                                      "--output-dir", str(tmp_path / "out")]))
    written = np.load(tmp_path / "cov.npz")
    assert np.array_equal(written["smoothed_cov"], smoothed_cov) and np.array_equal(written["filtered_cov"], filtered_cov)
