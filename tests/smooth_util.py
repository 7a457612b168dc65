"""Helpers of the smoothing tests (``test_smooth_cpu.py`` here, ``test_smooth.py`` on the GPU): the backward rule of
``include/ekf_slam_hip.h`` ("Offline smoothing") restated in NumPy for any float type -- ``np.longdouble`` is the oracle,
``np.float64`` the plain run that shows the bound has room -- with its own Cholesky and substitutions, the bound, the
records of the CPU oracle filter (what a recorded replay leaves on the device, without a device) and the scenes.

A record is {"frame", "dims", "s_eff", "u" [6], "stepped", "x" [N], "P" [N, N]}; the GPU tests fill the same dicts from
``history_info`` / ``history_record``, so the filter's own rounding does not enter the comparison.

Bound for output frame t (the classical forward error of a Cholesky solve, constant 1, linear in the steps because the
smoother gain contracts), u = 2^-53:
    |x_dev - x_ref|[0:7] <= u sum_{r >= rec(t)} N_r kappa_2(P_p,r) |c_r|_inf + 4 u max(1, |x_ref|)
with kappa and c from the oracle's own run.
"""
from __future__ import annotations

import numpy as np

import frame_scale_util as fs
import motion_util as mu

LD = np.longdouble
U = 2.0 ** -53
Q_CAM, Q_ERR, Q_LM = 0.3, 0.5, 0.01      # filters/extended_kalman_filter.py
TRACK_SMOOTH_RATIO = 0.5                 # the condition: smoothed mean position error <= 1/2 of the filtered one
RESIDENT_DIMS = 160                      # csrc/ekf_kernels.h: EKF_SMOOTH_RESIDENT_DIMS
RAGGED_SCALE = 0.5 + 0.5 * (np.arange(len(mu.RAGGED_PLAN)) % 4)


# --------------------------------------------------------------------------------------------------------------------
# the rule, in any float type
# --------------------------------------------------------------------------------------------------------------------
def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], dtype=a.dtype)


def residual(xs, xp, dt=LD):
    """delta of the backward step: additive on 0..2 and 10.., zero on 3..6, 2 vec(dq) / dq_w on 7..9."""
    xs, xp = np.asarray(xs, dtype=dt), np.asarray(xp, dtype=dt)
    n = xp.shape[0]
    d = np.zeros(n, dtype=dt)
    d[0:3] = xs[0:3] - xp[0:3]
    d[10:] = xs[10:n] - xp[10:]
    conj = xp[3:7] * np.array([1, -1, -1, -1], dtype=dt)
    dq = _qmul(xs[3:7], conj)
    d[7:10] = dt(2) * dq[1:4] / dq[0]
    return d


def inject(xr, c, dt=LD):
    """x^s = inject(x_r, c): the filter's scalar-first injection."""
    xr, c = np.asarray(xr, dtype=dt), np.asarray(c, dtype=dt)
    out = xr.copy()
    out[0:3] += c[0:3]
    out[10:] += c[10:]
    d = np.concatenate((np.ones(1, dtype=dt), c[7:10] / dt(2)))
    q = _qmul(d / np.sqrt(d @ d), xr[3:7] / np.sqrt(xr[3:7] @ xr[3:7]))
    out[3:7] = q / np.sqrt(q @ q)
    out[7:10] = 0
    return out


def cholesky_solve(a, b):
    """a^-1 b by an own right-looking Cholesky and the two substitutions, in the dtype of a."""
    a, y = a.copy(), b.copy()
    n = a.shape[0]
    for j in range(n):
        if not a[j, j] > 0:
            raise np.linalg.LinAlgError("not positive definite")
        a[j, j] = np.sqrt(a[j, j])
        a[j + 1:, j] /= a[j, j]
        y[j] /= a[j, j]
        y[j + 1:] -= a[j + 1:, j] * y[j]
        a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j + 1:, j])
    for j in range(n - 1, -1, -1):
        y[j] /= a[j, j]
        y[:j] -= a[j, :j] * y[j]
    return y


def smooth_records(records, frames, start_cam, dt=LD):
    """The backward pass over the records: {"smoothed" [F, 7] in dt, "kappa" [R-1], "cnorm" [R-1], "frame_record" [F]}."""
    count = len(records)
    frame_record = np.full(frames, -1, dtype=np.int64)
    for r, rec in enumerate(records):
        frame_record[rec["frame"]:] = r
    out = np.empty((frames, 7), dtype=dt)
    out[:] = np.asarray(start_cam[:7], dtype=dt)
    kappa, cnorm = np.zeros(max(count - 1, 0)), np.zeros(max(count - 1, 0))
    if count == 0:
        return {"smoothed": out, "kappa": kappa, "cnorm": cnorm, "frame_record": frame_record}
    xs = np.asarray(records[-1]["x"], dtype=dt)
    out[frame_record == count - 1] = xs[:7]
    for r in range(count - 2, -1, -1):
        rec, nxt = records[r], records[r + 1]
        n = rec["dims"]
        xr, pr = np.asarray(rec["x"], dtype=dt), np.asarray(rec["P"], dtype=dt)
        u = np.asarray(nxt["u"], dtype=np.float64)
        ft = np.eye(n, dtype=dt)
        xp = xr.copy()
        if u.any():
            f, c1, q1 = mu.motion_parts(xr[:10], u, dt)
            ft[:10, :10] = f
            xp[0:3], xp[3:7] = c1, q1
        s_eff = np.float64(nxt["s_eff"])
        qd = np.full(n, s_eff * np.float64(Q_LM))
        qd[0:3], qd[3:7], qd[7:10] = s_eff * np.float64(Q_CAM), 0.0, s_eff * np.float64(Q_ERR)
        pp = ft @ pr @ ft.T + np.diag(qd.astype(dt))      # (the factorisation reads its lower triangle)
        y = cholesky_solve(pp, residual(xs, xp, dt))
        c = pr @ (ft.T @ y)
        xs = inject(xr, c, dt)
        out[frame_record == r] = xs[:7]
        kappa[r] = np.linalg.cond(pp.astype(np.float64))
        cnorm[r] = float(np.abs(c).max())
    return {"smoothed": out, "kappa": kappa, "cnorm": cnorm, "frame_record": frame_record}


def bound(ref, records):
    """[F, 7]: the bound of the module docstring for every output entry, from the oracle's run ``ref``."""
    dims = np.array([rec["dims"] for rec in records[:-1]], dtype=np.float64)
    term = dims * ref["kappa"] * ref["cnorm"]
    tail = np.concatenate((np.cumsum(term[::-1])[::-1], [0.0]))      # tail[r] = sum over the steps r .. R-2
    rec_of = ref["frame_record"]
    first = np.where(rec_of >= 0, tail[np.maximum(rec_of, 0)], 0.0)
    x = np.abs(ref["smoothed"].astype(np.float64))
    return U * first[:, None] + 4.0 * U * np.maximum(1.0, x)


def worst_ratio(got, ref, records):
    """max |got - ref| / bound over the log; <= 1 passes."""
    err = np.abs(np.asarray(got, dtype=LD) - ref["smoothed"]).astype(np.float64)
    return float((err / bound(ref, records)).max())


# --------------------------------------------------------------------------------------------------------------------
# records without a device: the CPU oracle filter over a log
# --------------------------------------------------------------------------------------------------------------------
def oracle_records(log, motion=None, scale=None):
    """(records, filtered [F, 7], start camera) of the oracle filter (scalar_first) over the log, by the recording rule: one
    record behind every frame that was stepped or moved by a non-zero motion."""
    orc = mu.oracle_for("ekf")
    offs = log["offsets"]
    start = np.asarray(orc.state[:7], dtype=np.float64).copy()
    records, filtered, pending = [], [], 0.0
    for t in range(len(offs) - 1):
        u = np.zeros(6) if motion is None else np.asarray(motion[t], dtype=np.float64)
        moved = bool(u.any())
        if moved:
            orc.move(u[0:3], u[3:6])
        s_eff = 1.0 if scale is None else pending + float(scale[t])
        sl = slice(int(offs[t]), int(offs[t + 1]))
        stepped = sl.stop > sl.start
        if stepped:
            with fs.scaled(orc, s_eff):
                orc.observe(log["ids"][sl].tolist(), log["poses"][sl])
            pending = 0.0
        elif scale is not None:
            pending = s_eff
        if moved or stepped:
            records.append({"frame": t, "dims": int(np.asarray(orc.state).shape[0]), "s_eff": s_eff if stepped else 0.0,
                            "u": u, "stepped": stepped, "x": np.asarray(orc.state, dtype=np.float64).copy(),
                            "P": np.asarray(orc.uncertainty, dtype=np.float64).copy()})
        filtered.append(np.asarray(orc.state[:7], dtype=np.float64).copy())
    return records, np.array(filtered), start


def device_records(backend, history):
    """The same dicts from the device: ``history_info`` and ``history_record`` of a recorded replay."""
    info = backend.history_info()
    records = []
    for r in range(len(info["frame"])):
        x, p = backend.history_record(history, r, int(info["dims"][r]))
        records.append({"frame": int(info["frame"][r]), "dims": int(info["dims"][r]), "s_eff": float(info["s_eff"][r]),
                        "u": info["motion"][r].copy(), "stepped": bool(info["stepped"][r]), "x": x, "P": p})
    return records, info


# --------------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------------
def growing_scene(first, later, tail=2, seed=0):
    """The camera of the tracking scene among ``first + later`` landmarks: frame 0 sights the first ``first`` of them, each
    of the next ``later`` frames four known ones and ONE new one, each of the last ``tail`` frames four known ones.  No
    odometry.  {"ids", "poses", "offsets", "truth"}; ids are 100 + landmark."""
    rng = np.random.default_rng(77 + 1000 * first + 10 * later + seed)
    total = first + later
    dirs = rng.normal(size=(total, 3))
    lms = dirs / np.linalg.norm(dirs, axis=1)[:, None] * rng.uniform(2.5, 5.0, total)[:, None]
    c, q = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    ids, poses, offsets, truth = [], [], [0], []
    for t in range(1 + later + tail):
        if t > 0:
            _f, c, q = mu.motion_parts(np.concatenate((c, q)), mu.TRACK_STEP)
        truth.append(c.copy())
        rcm = mu.rotmat(q)
        if t == 0:
            seen = list(range(first))
        else:
            known = first + min(t - 1, later)
            seen = sorted(rng.choice(known, 4, replace=False).tolist())
            if t <= later:
                seen.append(first + t - 1)
        for i in seen:
            ids.append(100 + int(i))
            poses.append(np.concatenate((rcm.T @ (lms[i] - c) + rng.normal(0.0, mu.TRACK_SIGMA, 3), np.zeros(3))))
        offsets.append(len(ids))
    return {"ids": np.array(ids), "poses": np.array(poses), "offsets": np.array(offsets, dtype=np.int64),
            "truth": np.array(truth)}


def scene(name):
    """(log, motion, scale) of the named fixture: the logs the GPU tests smooth."""
    if name == "tracking":          # 40 frames, N = 40, no odometry
        return mu.tracking_scene("ekf"), None, None
    if name == "ragged":            # 14 frames, n <= 8: empty frames, moved-only frames, first sightings mid-log
        log = mu.ragged_motion_log("ekf")
        return log, log["motion"], RAGGED_SCALE
    if name == "n50":               # 6 frames, the last adds the 50th marker: N_r grows to 160 inside the pass
        return _n50(), None, None
    if name == "n18":               # N = 64: exactly one block
        return growing_scene(18, 0, tail=5), None, None
    if name == "n19":               # N = 67
        return growing_scene(19, 0, tail=5), None, None
    if name == "n51":               # N = 163: the first size past the resident tier, three blocks with a ragged edge
        return growing_scene(51, 0, tail=4), None, None
    if name == "n49_52":            # the tier choice sees a mixed history
        return growing_scene(49, 3, tail=2), None, None
    if name == "n82":               # N = 256: exactly four blocks, no padding row at all, behind an 82-detection frame
        return growing_scene(82, 0, tail=3), None, None
    if name == "g81_2":             # dims 253, 256, 259, 259: npad goes 256 -> 320 (4 -> 5 blocks) inside the pass
        return growing_scene(81, 2, tail=1), None, None
    raise KeyError(name)


def _n50():
    """49 markers in frame 0, four frames of four known ones, then the 50th in the last frame (6 frames)."""
    log = growing_scene(49, 5, tail=0)
    offs, keep = log["offsets"], np.ones(len(log["ids"]), dtype=bool)
    for t in range(1, 5):      # frames 1 .. 4 lose their new marker; frame 5 renames its own to the 50th
        keep[offs[t + 1] - 1] = False
    ids = log["ids"].copy()
    ids[offs[6] - 1] = 100 + 49
    counts = np.add.reduceat(keep.astype(np.int64), offs[:-1])
    return {"ids": ids[keep], "poses": log["poses"][keep], "truth": log["truth"],
            "offsets": np.concatenate(([0], np.cumsum(counts))).astype(np.int64)}


SCENES = ("tracking", "ragged", "n50", "n18", "n19", "n51", "n49_52", "n82", "g81_2")
EXPECTED_DIMS = {"tracking": 40, "ragged": 34, "n50": 160, "n18": 64, "n19": 67, "n51": 163, "n49_52": 166, "n82": 256,
                 "g81_2": 259}
BLOCKED_SCENES = ("n51", "n49_52", "n82", "g81_2")      # a record past RESIDENT_DIMS: the blocked tier without being asked

# the table of ekf_history_info for the ragged log with its motions and RAGGED_SCALE: (frame, dims, stepped, s_eff) of every
# record -- frame 0 is empty but moved, frames 4 .. 6 and 10 are empty and moved (their scales stay pending: 0.5 + 1 + 1.5
# before frame 7, 1.5 before frame 11), frames 2 and 9 carry exact-zero motions and are stepped
RAGGED_TABLE = [(0, 10, False, 0.0), (1, 22, True, 1.5), (2, 22, True, 1.5), (3, 28, True, 2.0), (4, 28, False, 0.0),
                (5, 28, False, 0.0), (6, 28, False, 0.0), (7, 28, True, 5.0), (8, 34, True, 0.5), (9, 34, True, 1.0),
                (10, 34, False, 0.0), (11, 34, True, 3.5), (12, 34, True, 0.5), (13, 34, True, 1.0)]


# --------------------------------------------------------------------------------------------------------------------
# the table under a gate, the layout of a history, and the pass through the library itself (``test_smooth_edges*.py``)
# --------------------------------------------------------------------------------------------------------------------
def expected_table(log, motion, scale, rejected):
    """The record table of a recorded replay by the header's rules, from the log and the gate's verdicts alone.  rejected:
    bool [D], indexed like the log's detections (first sightings are exempt, so never rejected).  A frame is stepped iff a
    detection survives; the scale of a frame that is not stepped stays pending and folds into the next stepped frame; a
    record exists iff the frame was moved by a non-zero motion or stepped; dims come from the landmarks known after the
    frame.  Returns (rows [(frame, dims, stepped, s_eff)], motions [R, 6], frame_record [F])."""
    offs = np.asarray(log["offsets"], dtype=np.int64)
    frames = len(offs) - 1
    rejected = np.asarray(rejected, dtype=bool)
    known, rows, motions, frame_record, pending = set(), [], [], np.full(frames, -1, dtype=np.int64), 0.0
    for t in range(frames):
        u = np.zeros(6) if motion is None else np.asarray(motion[t], dtype=np.float64)
        sl = slice(int(offs[t]), int(offs[t + 1]))
        known.update(int(i) for i in log["ids"][sl])
        s_eff = 1.0 if scale is None else pending + float(scale[t])
        stepped = bool((~rejected[sl]).any())
        if scale is not None:
            pending = 0.0 if stepped else s_eff
        if stepped or u.any():
            rows.append((t, 10 + 3 * len(known), stepped, s_eff if stepped else 0.0))
            motions.append(u)
        frame_record[t] = len(rows) - 1
    return rows, np.array(motions).reshape(-1, 6), frame_record


def record_bytes(dims):
    """``ekf_history_record_bytes`` restated: state [N] and the packed triangle in f64, rounded up to 256 bytes."""
    return -(-(dims + dims * (dims + 1) // 2) * 8 // 256) * 256


def record_offset(dims, r):
    """Byte offset of record r of a single filter's history whose records have ``dims`` [R]: the 256-byte header, then the
    records one behind the other."""
    return 256 + sum(record_bytes(int(n)) for n in dims[:r])


def diag_word(n, k):
    """Double index of P[k][k] within a record of n dims: the state, then the lower triangle column by column."""
    return n + k * (2 * n - k + 1) // 2


def tamper(history, sync, byte_offset, want_x, want_p, k, value=-1e3):
    """Write ``value`` over P[k][k] of the packed record at ``byte_offset`` of the caller's history buffer (a uint8 device
    tensor).  BEFORE it writes, the state doubles and that diagonal word are compared bit for bit with ``want_x`` [N] and
    ``want_p`` [N, N] (``history_record``): the check of the layout arithmetic.  ``sync()`` waits for the handle.  Returns
    a function that puts the original word back."""
    import torch
    n = int(np.asarray(want_x).shape[0])
    words = history.view(torch.float64)
    first = byte_offset // 8
    assert byte_offset % 256 == 0 and 0 <= k < n and first + diag_word(n, k) < words.numel()
    sync()
    torch.cuda.synchronize(history.device)
    assert np.array_equal(words[first:first + n].cpu().numpy(), want_x)
    at = first + diag_word(n, k)
    old = words[at:at + 1].clone()
    assert np.array_equal(old.cpu().numpy(), np.asarray(want_p)[k:k + 1, k])
    words[at] = value
    torch.cuda.synchronize(history.device)

    def restore():
        words[at:at + 1] = old
        torch.cuda.synchronize(history.device)
    return restore


# a pivot that fails inside the pass: (scene, blocked flag, r_bad, the k whose P[k][k] of record r_bad becomes -1e3)
#   tracking: the resident tier, first and last pivot; n19 forced blocked (N = 67): the first pivot of block 0 and the last
#   of the ragged block 1; n51 natural blocked (N = 163): a pivot of block 2
FAIL_STATE = (("tracking", False, 20, (0, 39)), ("n19", True, 2, (0, 66)), ("n51", False, 2, (162,)))
# the covariance pass: n19 as above, n49_52 with k = N_r - 1 of record 2 (N_r = 163)
FAIL_COV = (("n19", 2, (0, 66)), ("n49_52", 2, (162,)))
TAMPER_VALUE = -1e3
EKF_ERR_NUMERIC = -5
SENTINEL = 7.0      # what the outputs of a direct call hold before it: a row that still holds it was not written


def direct_smooth(b, history, frames, blocked, poison=False):
    """``ekf_smooth_history`` through the library itself: a workspace of exactly ``ekf_smooth_workspace_bytes`` (zeros, or
    with ``poison`` 0xFF bytes: every double a NaN) and an output pre-filled with SENTINEL.  Returns (rc, smoothed [F, 7])."""
    import ctypes as C

    import torch
    need = C.c_size_t()
    assert b.lib.ekf_smooth_workspace_bytes(b.h, C.byref(need)) == 0
    ws = torch.full((need.value,), 0xFF if poison else 0, dtype=torch.uint8, device=b.device)
    out = torch.full((frames, 7), SENTINEL, dtype=torch.float64, device=b.device)
    torch.cuda.synchronize(b.device)
    rc = b.lib.ekf_smooth_history(b.h, history.data_ptr(), history.numel(), ws.data_ptr(), need.value, int(bool(blocked)),
                                  out.data_ptr())
    b.sync()
    torch.cuda.synchronize(b.device)
    return rc, out.cpu().numpy()
