"""Helpers of the smoothed-covariance tests (``test_smooth_cov_cpu.py`` here, ``test_smooth_cov.py`` on the GPU): the
covariance rule of ``include/ekf_slam_hip.h`` ("Smoothed covariances") restated in NumPy for any float type, on the records
and transitions of ``smooth_util`` -- ``np.longdouble`` is the oracle, ``np.float64`` the plain run that shows the bound has
room -- in its two forms, with an own Cholesky and substitutions for many right-hand sides, and the bound.

    direct      P^s_r = P_r + G (P^s_{r+1}[0:N, 0:N] - P_p) G^T,  G^T = P_p^-1 (F~ P_r)
    products    P^s_r = P_r - W^T W + Z^T (P^s_{r+1}[0:N, 0:N] Z),  L L^T = P_p, W = L^-1 F~ P_r, Z = L^-T W

Bound for every entry of P^s_r (the protocol of the state: the forward error of a Cholesky solve, constant 1, summed over
the steps because the smoother gain contracts), u = 2^-53, kappa and the maxima from the oracle's own run:
    |dev - ref| <= u sum_{s >= r} N_s kappa_2(P_p,s) max|P_s| + 4 u max|P^s_r|
"""
from __future__ import annotations

import functools

import numpy as np

import motion_util as mu
import smooth_util as su
import update_sweep_util as sw

LD = su.LD
U = su.U
INIT = sw.INIT
GROWING = "g17_3"      # growing_scene(17, 3, tail=2): dims 61, 64, 67, 70 -- npad changes 64 -> 128 inside the pass
CPU_SCENES = su.SCENES + (GROWING,)      # (with n82 and g81_2: four blocks without a padding row, and 4 -> 5 blocks)
GPU_SCENES = ("n18", "n19", GROWING, "ragged", "tracking", "n49_52", "n82", "g81_2")


def scene(name):
    if name == GROWING:
        return su.growing_scene(17, 3, tail=2), None, None
    return su.scene(name)


# --------------------------------------------------------------------------------------------------------------------
# the rule, in any float type
# --------------------------------------------------------------------------------------------------------------------
def cholesky_factor(a):
    """Lower L with L L^T = a, by an own right-looking Cholesky in the dtype of a."""
    a = a.copy()
    n = a.shape[0]
    for j in range(n):
        if not a[j, j] > 0:
            raise np.linalg.LinAlgError("not positive definite")
        a[j, j] = np.sqrt(a[j, j])
        a[j + 1:, j] /= a[j, j]
        a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j + 1:, j])
    return np.tril(a)


def forward(l, b):
    """L^-1 b for a matrix b."""
    y = b.copy()
    for j in range(l.shape[0]):
        y[j] /= l[j, j]
        y[j + 1:] -= np.outer(l[j + 1:, j], y[j])
    return y


def backward(l, b):
    """L^-T b for a matrix b."""
    y = b.copy()
    for j in range(l.shape[0] - 1, -1, -1):
        y[j] /= l[j, j]
        y[:j] -= np.outer(l[j, :j], y[j])
    return y


def transition(rec, nxt, dt):
    """(F~, P_p) of the step rec -> nxt in dt: the transition of ``smooth_util.smooth_records``."""
    n = rec["dims"]
    xr, pr = np.asarray(rec["x"], dtype=dt), np.asarray(rec["P"], dtype=dt)
    u = np.asarray(nxt["u"], dtype=np.float64)
    ft = np.eye(n, dtype=dt)
    if u.any():
        f, _c1, _q1 = mu.motion_parts(xr[:10], u, dt)
        ft[:10, :10] = f
    s_eff = np.float64(nxt["s_eff"])
    qd = np.full(n, s_eff * np.float64(su.Q_LM))
    qd[0:3], qd[3:7], qd[7:10] = s_eff * np.float64(su.Q_CAM), 0.0, s_eff * np.float64(su.Q_ERR)
    return ft, ft @ pr @ ft.T + np.diag(qd.astype(dt))


def smooth_cov_records(records, dt=LD, form="direct"):
    """The covariance recursion over the records: {"Ps": [R] matrices in dt, "kappa" [R-1], "pmax" [R-1] (max|P_s|)}."""
    count = len(records)
    ps = [None] * count
    kappa, pmax = np.zeros(max(count - 1, 0)), np.zeros(max(count - 1, 0))
    if count == 0:
        return {"Ps": ps, "kappa": kappa, "pmax": pmax}
    ps[-1] = np.asarray(records[-1]["P"], dtype=dt)
    for r in range(count - 2, -1, -1):
        rec, nxt = records[r], records[r + 1]
        n = rec["dims"]
        pr = np.asarray(rec["P"], dtype=dt)
        ft, pp = transition(rec, nxt, dt)
        l = cholesky_factor(pp)
        w = forward(l, ft @ pr)
        z = backward(l, w)                         # = G^T
        nxt_s = ps[r + 1][:n, :n]
        if form == "direct":
            out = pr + z.T @ (nxt_s - pp) @ z
        else:
            out = pr - w.T @ w + z.T @ (nxt_s @ z)
        ps[r] = np.tril(out) + np.tril(out, -1).T      # the lower triangle, mirrored
        kappa[r] = np.linalg.cond(pp.astype(np.float64))
        pmax[r] = float(np.abs(np.asarray(rec["P"], dtype=np.float64)).max())
    return {"Ps": ps, "kappa": kappa, "pmax": pmax}


def record_bound(ref, records):
    """[R]: the bound of the module docstring for the entries of P^s_r."""
    dims = np.array([rec["dims"] for rec in records[:-1]], dtype=np.float64)
    term = dims * ref["kappa"] * ref["pmax"]
    tail = np.concatenate((np.cumsum(term[::-1])[::-1], [0.0]))
    top = np.array([float(np.abs(p.astype(np.float64)).max()) for p in ref["Ps"]])
    return U * tail + 4.0 * U * top


def worst_record_ratio(got, ref, records):
    """max over records and entries of |got_r - ref_r| / bound_r for a list of full matrices ``got``."""
    b = record_bound(ref, records)
    return max(float(np.abs(np.asarray(g, dtype=LD) - p).max()) / b[r] for r, (g, p) in enumerate(zip(got, ref["Ps"])))


def frame_rows(ref, records, frames):
    """(cam [F, 10, 10] in longdouble with NaN before the first record, bound [F], record of every frame [F])."""
    rec_of = np.full(frames, -1, dtype=np.int64)
    for r, rec in enumerate(records):
        rec_of[rec["frame"]:] = r
    b = record_bound(ref, records)
    cam = np.full((frames, 10, 10), np.nan, dtype=LD)
    fb = np.full(frames, np.nan)
    for t in range(frames):
        if rec_of[t] >= 0:
            cam[t] = ref["Ps"][rec_of[t]][:10, :10]
            fb[t] = b[rec_of[t]]
    return cam, fb, rec_of


# --------------------------------------------------------------------------------------------------------------------
# the device: one recorded replay and one covariance pass per scene, shared by the GPU tests (read, never changed)
# --------------------------------------------------------------------------------------------------------------------
def new_filter(n=8, m=8, **kw):
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    kw.setdefault("quat_update", "scalar_first")
    return EKF(INIT, max_landmarks=n, max_visible=m, **kw)


def recorded_replay(flt, log, motion=None, scale=None, record=True, mahal=False, poison=False):
    """One log call on the back end; returns (trajectory, history | None), with ``mahal`` (trajectory, history | None, d2
    [D]).  ``poison``: the history holds 0xFF bytes (every double a NaN) before the call."""
    import torch
    from aruco_slam_amd.filters.base_filter import plan_detection_log
    b = flt.backend
    plan = plan_detection_log(flt.landmarks, flt.num_landmarks, log["ids"], log["offsets"], log.get("has_detections"))
    if plan.num_landmarks > b.max_landmarks:
        b.grow(plan.num_landmarks)
    if plan.widest > b.max_visible:
        b.grow(new_max_visible=plan.widest)
    frames = len(plan.offsets) - 1
    traj = torch.empty((frames, 7), dtype=torch.float64, device=b.device)
    d2 = torch.empty((len(plan.index),), dtype=torch.float64, device=b.device) if mahal else None
    history = b.new_history(plan.index, plan.offsets) if record else None
    if poison:
        history.fill_(0xFF)
        torch.cuda.synchronize(b.device)
    b.observe_log(plan.index, plan.offsets, log["poses"], traj, d2, None, scale, motion, **({"history": history} if record else {}))
    b.sync()
    flt.landmarks.update(plan.new_landmarks)
    flt.num_landmarks = plan.num_landmarks
    if mahal:
        return traj.cpu().numpy(), history, d2.cpu().numpy()
    return traj.cpu().numpy(), history


def direct_smooth_cov(b, history, frames, n0, poison=False):
    """``ekf_smooth_history_cov`` through the library itself: a workspace of exactly ``ekf_smooth_cov_workspace_bytes``
    (zeros, or with ``poison`` 0xFF bytes: every double a NaN) and outputs pre-filled with ``smooth_util.SENTINEL``.
    Returns (rc, {"smoothed", "cam_cov", "filt_cam_cov", "first_cov" [n0, n0]} as arrays)."""
    import ctypes as C

    import torch
    need = C.c_size_t()
    assert b.lib.ekf_smooth_cov_workspace_bytes(b.h, C.byref(need)) == 0
    ws = torch.full((need.value,), 0xFF if poison else 0, dtype=torch.uint8, device=b.device)
    out = {key: torch.full(shape, su.SENTINEL, dtype=torch.float64, device=b.device)
           for key, shape in (("smoothed", (frames, 7)), ("cam_cov", (frames, 10, 10)), ("filt_cam_cov", (frames, 10, 10)),
                              ("first_cov", (n0, n0)))}
    torch.cuda.synchronize(b.device)
    rc = b.lib.ekf_smooth_history_cov(b.h, history.data_ptr(), history.numel(), ws.data_ptr(), need.value, 0,
                                      out["smoothed"].data_ptr(), out["cam_cov"].data_ptr(), out["filt_cam_cov"].data_ptr(),
                                      out["first_cov"].data_ptr())
    b.sync()
    torch.cuda.synchronize(b.device)
    return rc, {key: v.cpu().numpy() for key, v in out.items()}


@functools.lru_cache(maxsize=None)
def device_case(name):
    """{"flt", "history", "frames", "traj", "blocked" (smooth_history(blocked=True), taken BEFORE the covariance pass),
    "state", "P" (the filter before the pass), "out" (the pass's outputs as arrays), "records", "ref" (the oracle on the
    device's own records)} of one scene."""
    log, motion, scale = scene(name)
    size = 10 if name == "tracking" else 8      # (tracking: the filter of the top-level test, so that the bits compare)
    flt = new_filter(n=size, m=size, motion=motion is not None, frame_scale=scale is not None)
    traj, history = recorded_replay(flt, log, motion, scale)
    b = flt.backend
    frames = traj.shape[0]
    blocked = b.smooth_history(history, frames, blocked=True).cpu().numpy()
    state, cov = b.get_state(), b.get_cov()
    res = b.smooth_history_cov(history, frames)
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}
    records, _info = su.device_records(b, history)
    ref = smooth_cov_records(records)
    return {"flt": flt, "history": history, "frames": frames, "traj": traj, "blocked": blocked, "state": state, "P": cov,
            "out": out, "records": records, "ref": ref}
