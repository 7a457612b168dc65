"""Expected values of the localisation mode (``freeze_map``; include/ekf_slam_hip.h, "Localisation mode") from the NumPy
oracle, and the filters and frames the frozen-map tests share.

``schmidt_step`` is the oracle's own step with the landmark state and P[10:, 10:] put back; ``joseph_schmidt_step`` is the
textbook Schmidt-Kalman update (Joseph form with the landmark rows of the gain zero) that ``test_frozen_map_cpu.py`` pins it
against."""
import numpy as np

import support as sp

INIT = sp.INIT
LMD = {"ekf": 3, "ekf_rotations": 10}
CAM = 10


def new_oracle(model, quat="scalar_first"):
    from oracle.ekf_numpy import OracleEKF, OracleEKFRotations
    if model == "ekf_rotations":
        return OracleEKFRotations(INIT, mode="fast")
    return OracleEKF(INIT, mode="fast", quat_mode=quat)


def schmidt_step(orc, ids, poses):
    """One frozen frame on the oracle: its ``observe`` (every id is in the map), then the landmark state and P[10:, 10:]
    back as they were -- neither predicted nor updated."""
    ids = [int(i) for i in ids]
    assert all(i in orc.landmarks for i in ids)
    lm_state = np.array(orc.state[CAM:], dtype=np.float64)
    p_ll = np.array(np.asarray(orc.uncertainty)[CAM:, CAM:], dtype=np.float64)
    orc.observe(ids, poses)
    state = np.array(orc.state, dtype=np.float64)
    state[CAM:] = lm_state
    p = np.array(orc.uncertainty, dtype=np.float64)
    p[CAM:, CAM:] = p_ll
    orc.state, orc.uncertainty = state, p


def joseph_schmidt_step(orc, ids, poses):
    """The textbook Schmidt-Kalman update of the prior ``orc`` holds, without touching it: P- = P + Q, K = P- H^T S^-1 with
    K[10:] = 0, P+ = (I - K H) P- (I - K H)^T + K R K^T.  Its landmark block is the predicted one, P_ll + Q_lm; the filter
    never stores that inflation (rule 3), so Q_lm comes off again.  Returns (delta [N] with zero landmark rows, P+ [N, N])."""
    from oracle.ekf_numpy import R_UNCERTAINTY
    ids = [int(i) for i in ids]
    z, h, jac, col = orc.measurement_blocks(ids, poses)
    dh = orc.dense_jacobian(jac, col)
    qd = orc.process_noise_diag()
    pm = np.array(orc.uncertainty, dtype=np.float64) + np.diag(qd)
    s = dh @ pm @ dh.T + R_UNCERTAINTY * np.eye(dh.shape[0])
    gain = np.linalg.solve(s, dh @ pm).T
    gain[CAM:] = 0.0
    ikh = np.eye(pm.shape[0]) - gain @ dh
    pp = ikh @ pm @ ikh.T + R_UNCERTAINTY * (gain @ gain.T)
    pp[np.arange(CAM, pp.shape[0]), np.arange(CAM, pp.shape[0])] -= qd[CAM:]
    return gain @ (z - h), pp


def ekf(n, m, dtype="float64", quat="as_written", fused=True, **kw):
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    return EKF(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, quat_update=quat, fused=fused, **kw)


def rot(n, m, dtype="float64", fused=True, **kw):
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    return EKF_Rotations(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, fused=fused, **kw)


def make(model, n, m, **kw):
    kw = dict(kw)
    if model == "ekf_rotations":
        kw.pop("quat", None)
        return rot(n, m, **kw)
    return ekf(n, m, **kw)


def stream(model, n, m, seed):
    from aruco_slam_amd.synthetic import SyntheticStream
    return SyntheticStream(n, min(n, m), seed=seed, rvec_sigma=0.05 if model == "ekf_rotations" else 0.0)


def prior(model, n, seed, **kw):
    """(state, P [f64 copy], marker ids in index order) after a short mapping run that first-sights all ``n`` landmarks,
    at most 8 per frame, and steps two steady frames; built with the filter arguments ``kw``."""
    mb = min(n, 8)
    flt = make(model, n, mb, **kw)
    s = stream(model, n, mb, seed)
    for ids, poses in list(s.bootstrap()) + list(s.steady(2)):
        flt.observe(ids, poses)
    ids = [k for k, _ in sorted(flt.landmarks.items(), key=lambda kv: kv[1])]
    return np.array(flt.state, dtype=np.float64), np.array(flt.uncertainty, dtype=np.float64), ids


def restore(flt, state, p, ids):
    """``state`` / ``p`` into ``flt`` through set_state / set_cov, with the id table."""
    flt.backend.set_state_cov(state, p)
    flt.landmarks = {int(k): i for i, k in enumerate(ids)}
    flt.num_landmarks = len(ids)


def frame(model, n, m, seed, duplicate=False):
    """One frame of ``m`` detections of known landmarks 0 .. n-1 (``m`` > ``n`` or ``duplicate``: ids repeat, every
    detection with its own noisy pose), seen from camera frame 3 of the synthetic track."""
    s = stream(model, n, 1, seed)
    s.frame = 3
    rng = np.random.default_rng(seed + 100)
    if m <= n and not duplicate:
        ids = np.sort(rng.choice(n, m, replace=False))
    else:
        ids = rng.integers(0, n, m)
        ids[-1] = ids[0]
    return s._observe(ids)


def arrays(flt):
    return np.array(flt.state, dtype=np.float64), np.array(flt.uncertainty, dtype=np.float64)


def raw_cov(flt):
    """The whole device covariance, capacity padding included, as float64."""
    flt.backend.sync()
    return flt.backend.cov_t.double().cpu().numpy()


def assert_frozen_frame(frozen, mapping, state0, p0):
    """Test 1 of the issue: the camera rows / columns of ``frozen`` are bitwise the mapping frame's; its landmarks and
    P[10:, 10:] are bitwise the prior; the padding is exactly zero; P is bitwise symmetric."""
    sf, pf = arrays(frozen)
    sm, pm = arrays(mapping)
    n = state0.shape[0]
    assert sf.shape == sm.shape == (n,) and pf.shape == pm.shape == (n, n)
    assert np.array_equal(sf[:CAM], sm[:CAM]), ("camera state", float(np.abs(sf[:CAM] - sm[:CAM]).max()))
    assert np.array_equal(pf[:CAM, :], pm[:CAM, :]), ("camera rows", float(np.abs(pf[:CAM] - pm[:CAM]).max()))
    assert np.array_equal(pf[:, :CAM], pm[:, :CAM]), "camera columns"
    assert np.array_equal(sf[CAM:], state0[CAM:]), "landmark state"
    assert np.array_equal(pf[CAM:, CAM:], p0[CAM:, CAM:]), "landmark block"
    assert np.array_equal(pf, pf.T), "symmetry"
    raw = raw_cov(frozen)
    assert np.array_equal(raw[:n, :n], pf)
    assert not raw[n:, :].any() and not raw[:, n:].any(), "padding"
    assert not np.array_equal(pm[CAM:, CAM:], p0[CAM:, CAM:])      # (the mapping frame did move the map)


def sequence_run(dtype="float32"):
    """A mapping filter (n = 32, m = 4) after its bootstrap and one sequence call over 64 steady frames of a fixed m:
    (filter, the frames, the device tensors of the call)."""
    import torch
    s = stream("ekf", 32, 4, seed=9)
    flt = ekf(32, 4, dtype=dtype)
    for ids, poses in s.bootstrap():
        flt.observe(ids, poses)
    frames = list(s.steady(64))
    be = flt.backend
    idx_t = torch.from_numpy(np.stack([i for i, _ in frames]).astype(np.int32)).to(be.device)
    z_t = torch.from_numpy(np.stack([p[:, :3] for _, p in frames]).copy()).to(be.device)
    be.observe_sequence(idx_t, z_t)
    be.sync()
    return flt, frames, idx_t, z_t


def record_c1():
    """c1_detections on filters that were never frozen: per-frame loop and log call, f64 and f32 covariance; and the
    sequence call of ``sequence_run``.  The arrays tests/golden/frozen_c1_parent.npz holds, as the commit before the
    localisation mode computed them."""
    from conftest import load_npz
    det = load_npz("c1_detections.npz")
    offs, has = det["offsets"], det["has_detections"]
    out = {}
    for dtype in ("float64", "float32"):
        loop, replay = ekf(16, 8, dtype=dtype), ekf(16, 8, dtype=dtype)
        rows = []
        for t in range(len(offs) - 1):
            sl = slice(int(offs[t]), int(offs[t + 1]))
            _, cam, _, _ = loop.process_detections(det["ids"][sl] if has[t] else None, det["poses"][sl])
            rows.append(np.asarray(cam, dtype=np.float64)[:7])
        out[f"loop_traj_{dtype}"] = np.array(rows)
        out[f"loop_state_{dtype}"], out[f"loop_cov_{dtype}"] = arrays(loop)
        out[f"log_traj_{dtype}"] = replay.process_detection_log(det["ids"], det["poses"], offs, has)
        out[f"log_state_{dtype}"], out[f"log_cov_{dtype}"] = arrays(replay)
        out[f"log_stats_{dtype}"] = np.array([replay.backend.last_log_stats()[k] for k in replay.backend.LOG_STATS])
        out[f"seq_state_{dtype}"], out[f"seq_cov_{dtype}"] = arrays(sequence_run(dtype)[0])
    return out
