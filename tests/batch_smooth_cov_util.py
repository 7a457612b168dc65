"""Helpers of the batch smoothed-covariance tests (``test_batch_smooth_cov_cpu.py`` here, ``test_batch_smooth_cov.py`` on
the GPU): the scenes as batch logs, the covariance oracle of ``smooth_cov_util`` with a member's own noise constants, one
recorded call and its passes per scene (shared by the GPU tests, read and never changed), and the pass through the library
itself.

The batch kernels that record take frames of at most 16 detections (``batch.COLUMN_MAX_VISIBLE``), and the first frame of
``n18``, ``n19`` and ``g17_3`` sights 18, 19 and 17 markers.  ``scene_log`` gives those scenes with that frame cut in two --
its first 16 detections, then the rest as a frame of their own, the camera where it was -- so the markers, the measurements
and every N of the scene are what they were, behind one more record of 58 dims."""
from __future__ import annotations

import functools

import numpy as np

import batch_smooth_util as bu
import smooth_cov_util as scu
import smooth_util as su
import support as sp

LD = su.LD
WIDTH = 16                                            # batch.COLUMN_MAX_VISIBLE["ekf"]
CUT_SCENES = ("n18", "n19", scu.GROWING)
GPU_SCENES = ("tracking", "ragged", "n18", "n19", scu.GROWING, "growing")
SCENE_NOISE = {"q_cam": [0.3, 0.1, 0.5], "q_lm": [0.01, 0.02, 0.005]}      # the three members of a scene's batch
EXPECTED_DIMS = {"tracking": [40], "ragged": [10, 22, 28, 34], "n18": [58, 64], "n19": [58, 67],
                 scu.GROWING: [58, 61, 64, 67, 70], "growing": [58] + [61 + 3 * t for t in range(34)]}


def cut_first_frame(log, width=WIDTH):
    """The log with its first frame cut in two at ``width`` detections (see the module docstring)."""
    offs = np.asarray(log["offsets"], dtype=np.int64)
    assert offs[1] > width
    return {**log, "offsets": np.concatenate(([0, width], offs[1:]))}


def scene_log(name):
    """The named scene as a log dict of ``process_detection_logs`` (``batch_smooth_util.scene_log`` for the scenes it knows)."""
    if name not in CUT_SCENES:
        return bu.scene_log(name)
    log = cut_first_frame(scu.scene(name)[0])
    return {"ids": log["ids"], "poses": log["poses"], "offsets": log["offsets"], "has_detections": np.diff(log["offsets"]) > 0}


def member_cov_oracle(records, noise_row, dt=LD, form="direct"):
    """``smooth_cov_util.smooth_cov_records`` for one member; noise_row: its constants in ``batch.NOISE_KEYS`` order."""
    with bu.member_noise(noise_row[3], noise_row[4], noise_row[5]):
        return scu.smooth_cov_records(records, dt, form)


def oracle_noise_row(q_cam=su.Q_CAM, q_err=su.Q_ERR, q_lm=su.Q_LM):
    return [0.0, 0.0, 0.0, q_cam, q_err, q_lm]


def worst_ratios(cam_cov, first_cov, ref, records, frames):
    """(worst error / bound of cam_cov over the frames behind the first record, the same of first_cov over all entries)."""
    cam, fb, rec_of = scu.frame_rows(ref, records, frames)
    live = rec_of >= 0
    err = np.abs(np.asarray(cam_cov, dtype=LD)[live] - cam[live]).astype(np.float64).max(axis=(1, 2))
    first = np.abs(np.asarray(first_cov, dtype=LD) - ref["Ps"][0]).astype(np.float64).max() / scu.record_bound(ref, records)[0]
    return float((err / fb[live]).max()), float(first)


def run_batch(logs, order=None, **kw):
    """A batch over ``logs`` (in ``order``: members permuted with their poses and noise) recorded, then: the state pass, the
    covariance pass with first_cov, the state pass again and the covariance pass again.  Returns {"batch", "order", "before",
    "after" (snapshots around the passes), "status" (of the replay, around the passes), "filtered", "state0", "state1",
    "cov0", "cov1" (each (smoothed, cam_cov, filt_cam_cov, first_cov)), "smooth_status"}; lists are indexed by SLOT."""
    members = len(logs)
    order = list(range(members)) if order is None else list(order)
    poses = bu.initial_poses(members)[order]
    noise = {k: np.asarray(v, dtype=np.float64)[order] for k, v in kw.pop("noise", {}).items()}
    batch = bu.new_batch(len(order), poses=poses, noise=noise, **kw)
    filtered = batch.process_detection_logs([logs[i] for i in order], record=True)
    before, status0 = sp.snap_batch(batch, tables=True), batch.status()
    state0 = batch.smooth_history()
    cov0 = batch.smooth_history_cov(first=True)
    smooth_status = batch.last_smooth_status.copy()
    state1 = batch.smooth_history()
    cov1 = batch.smooth_history_cov(first=True)
    return {"batch": batch, "order": order, "poses": poses, "before": before, "after": sp.snap_batch(batch, tables=True),
            "status": (status0, batch.status()), "filtered": filtered, "state0": state0, "state1": state1, "cov0": cov0,
            "cov1": cov1, "smooth_status": smooth_status}


@functools.lru_cache(maxsize=None)
def device_case(name):
    """``run_batch`` of the named scene as a 3-member batch (initial poses of ``batch_smooth_util``, SCENE_NOISE), with
    "records" [3] and "frames"."""
    log = scene_log(name)
    kw = {"motion": "motion" in log, "frame_scale": "scale" in log}
    case = run_batch([log] * 3, noise=SCENE_NOISE, **kw)
    case["records"] = [case["batch"].history_records(b) for b in range(3)]
    case["frames"] = len(log["offsets"]) - 1
    return case


@functools.lru_cache(maxsize=None)
def mixed_case():
    """``run_batch`` of ``batch_smooth_util.mixed_logs()`` under MIXED_NOISE with motion and frame scale."""
    logs = bu.mixed_logs()
    case = run_batch(logs, noise=bu.MIXED_NOISE, motion=True, frame_scale=True)
    case["records"] = [case["batch"].history_records(b) for b in range(4)]
    case["logs"] = logs
    return case


def direct_batch_smooth_cov(batch, poison=False, first_ld=None, ws_bytes=None, flags=0, handle=True):
    """``ekf_batch_smooth_history_cov`` through the library itself: a workspace of exactly
    ``ekf_batch_smooth_cov_workspace_bytes`` (zeros, or with ``poison`` 0xFF bytes: every double a NaN) and outputs pre-filled
    with ``smooth_util.SENTINEL``.  Returns (rc, {"smoothed", "cam_cov", "filt_cam_cov" [Ftot, ...], "first_cov" [B, ld, ld]},
    status [B])."""
    import ctypes as C

    import torch
    from aruco_slam_amd.batch import _iptr
    need = C.c_size_t()
    assert batch.lib.ekf_batch_smooth_cov_workspace_bytes(batch.h, C.byref(need)) == 0
    mf, history = batch._history_frames, batch.last_history
    frames = int(mf[-1])
    if first_ld is None:
        first_ld = max([r[0]["dims"] for r in (batch.history_records(b) for b in range(batch.members)) if r] or [1])
    size = need.value if ws_bytes is None else ws_bytes
    ws = torch.full((max(size, 256),), 0xFF if poison else 0, dtype=torch.uint8, device=batch.device)
    out = {key: torch.full(shape, su.SENTINEL, dtype=torch.float64, device=batch.device)
           for key, shape in (("smoothed", (frames, 7)), ("cam_cov", (frames, 10, 10)), ("filt_cam_cov", (frames, 10, 10)),
                              ("first_cov", (batch.members, max(first_ld, 1), max(first_ld, 1))))}
    status = np.full(batch.members, 99, dtype=np.int32)
    torch.cuda.synchronize(batch.device)
    rc = batch.lib.ekf_batch_smooth_history_cov(batch.h if handle else None, history.data_ptr(), history.numel(), ws.data_ptr(),
                                                size, flags, out["smoothed"].data_ptr(), out["cam_cov"].data_ptr(),
                                                out["filt_cam_cov"].data_ptr(), out["first_cov"].data_ptr(), first_ld,
                                                _iptr(status))
    batch.stream.synchronize()
    torch.cuda.synchronize(batch.device)
    return rc, {key: v.cpu().numpy() for key, v in out.items()}, status
