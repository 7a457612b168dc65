"""The per-detection chi-square gate of the single filter (``EKF`` / ``EKF_Rotations``: ``gate=``, ``set_gate``,
``last_mahal`` / ``last_rejected``, ``process_detection_log(..., mahal=True)``) on an MI355X: distances and decisions
against the oracle on the device's own prior, the bit rule (a gated frame is the same call on the frame without the rejected
detections) per frame and in the log replay, the smallest shapes at which the gate kernel can go wrong, gate off is the
filter without the gate, agreement with ``EKFBatch``, and a failed pivot."""
import ctypes as C
import functools

import numpy as np
import pytest

import gating_util as gu
import support as sp
from conftest import load_npz, report

pytestmark = pytest.mark.gpu

INIT = gu.INIT
LOG_SEED = 0          # (test_filter_gating_cpu.py checks the logs of this seed)
DTYPES = ["float64", "float32"]
MODELS = ["ekf", "ekf_rotations"]
QM = {"ekf": "ekf", "ekf_rotations": "rot"}          # update_sweep_util's names
EKF_ERR_STATE, EKF_ERR_NUMERIC = -4, -5


def _filter(model, n, m, dtype="float64", gate=None, fused=True, quat="scalar_first"):
    if model == "ekf_rotations":
        from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
        return EKF_Rotations(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, gate=gate, fused=fused)
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    return EKF(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, gate=gate, fused=fused, quat_update=quat)


def _load_prior(flt, state, p, lm_ids):
    flt.backend.set_state_cov(state, p)
    flt.landmarks = {int(k): i for i, k in enumerate(lm_ids)}
    flt.num_landmarks = len(lm_ids)


def _log_family(model):
    kw, n, _m_range = gu.FAMILIES[(model, "column")]
    return n, kw["max_visible"]          # (the batch's limits: a dirty frame, two detections more than a clean one, fits)


@functools.lru_cache(maxsize=None)
def _logs(model):
    clean = gu.clean_log(model, "column", seed=LOG_SEED)
    dirty, marks = gu.dirty_log(model, clean, seed=LOG_SEED)
    return clean, dirty, marks


def _frames(log):
    offs = log["offsets"]
    for t in range(len(offs) - 1):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        yield t, sl, log["ids"][sl], log["poses"][sl]


# ---- 1. distances, teacher-forced ----------------------------------------------------------------------------------------
_TEACHER = {}


def _teacher_expected(case, dtype, flt):
    """(frames, [(d^2, kappa)]) of a case on the prior as the device holds it after the upload (an f32 covariance rounds
    it): computed once per (case, dtype) and shared by the fused and the stage-kernel filter, whose uploads are the same."""
    key = (case, dtype)
    if key not in _TEACHER:
        model, frames = gu.teacher_frames(case)
        want = []
        for s0, p0, lm, ids, poses in frames:
            _load_prior(flt, s0, p0, lm)
            want.append(gu.teacher_distances(model, s0, flt.uncertainty, lm, ids, poses))
        _TEACHER[key] = (frames, want)
    return _TEACHER[key]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stage"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["c1", "g5"])
def test_distances_and_decisions_against_the_oracle_teacher_forced(case, dtype, fused):
    """|d^2 - want| / want <= max(1e-9, 100 kappa(S_d) 2^-52) for every detection of the C1 / G5 frames (each with an
    outlier appended) on the prior the device holds, and every decision at GATES[model] is the oracle's."""
    model = "ekf" if case == "c1" else "ekf_rotations"
    gate = gu.GATES[model]
    flt = _filter(model, 16 if case == "c1" else 8, 10, dtype, gate=gate, fused=fused, quat="as_written")
    frames, wants = _teacher_expected(case, dtype, flt)
    worst, checked, rejected = 0.0, 0, 0
    for (s0, p0, lm, ids, poses), (want, kappa) in zip(frames, wants):
        _load_prior(flt, s0, p0, lm)
        flt.observe(ids, poses)
        flt.backend.sync()
        got = flt.last_mahal
        assert got.shape == want.shape
        for j in range(len(ids)):
            rel, tol = abs(got[j] - want[j]) / want[j], gu.tolerance(kappa[j])
            assert abs(want[j] - gate) / want[j] > tol, "input: an expected distance within the tolerance of the gate"
            assert rel <= tol, (j, got[j], want[j], rel, tol)
            worst = max(worst, rel / tol)
            checked += 1
        assert np.array_equal(flt.last_rejected, want > gate)
        rejected += int(flt.last_rejected.sum())
        assert flt.backend.last_gate_stats() == {"tested": len(ids), "rejected": int((want > gate).sum())}
    report(f"filter_gating_oracle_{case}_{dtype}_{'fused' if fused else 'stage'}", detections=checked, rejected=rejected,
           worst_over_tol=worst)
    assert checked >= 9 and 0 < rejected < checked


# ---- 2. bit rule, per frame ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _per_frame_gated(model, dtype):
    """The dirty log through ``observe`` with the gate, frame by frame: (trajectory [F,7], d^2 [D], rejected [D], state, P,
    landmarks, the frames after which P was compared and found unchanged)."""
    _clean, dirty, _marks = _logs(model)
    n, m = _log_family(model)
    flt = _filter(model, n, m, dtype, gate=gu.GATES[model])
    d2, rej = np.zeros(len(dirty["ids"])), np.zeros(len(dirty["ids"]), dtype=bool)
    rows, unstepped = [], []
    for t, sl, ids, poses in _frames(dirty):
        if len(ids):
            before = sp.snap_filter(flt) if flt.num_landmarks and _outliers_only(model, t) else None
            flt.observe(ids, poses)
            d2[sl], rej[sl] = flt.last_mahal, flt.last_rejected
            if before is not None:
                sp.assert_same(sp.snap_filter(flt), before, f"frame {t}: no survivor, so no predict")
                unstepped.append(t)
        rows.append(np.asarray(flt.get_poses()[0], dtype=np.float64)[:7])
    state, cov = sp.snap_filter(flt)
    return np.array(rows), d2, rej, state, cov, dict(flt.landmarks), unstepped


def _outliers_only(model, t):
    _clean, dirty, marks = _logs(model)
    offs = dirty["offsets"]
    return offs[t + 1] > offs[t] and marks[offs[t]:offs[t + 1]].all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_a_gated_frame_is_the_frame_without_the_rejected_detections(model, dtype):
    _clean, dirty, marks = _logs(model)
    traj, d2, rej, state, cov, landmarks, unstepped = _per_frame_gated(model, dtype)
    _want_d2, want_rej = gu.oracle_gated_replay(model, dirty, gu.GATES[model])
    assert np.array_equal(rej, want_rej) and np.array_equal(rej, marks)
    # the same loop, gate off (a filter without the gate), over the log without the rejected detections
    n, m = _log_family(model)
    plain = _filter(model, n, m, dtype)
    assert plain.gate is None and plain.last_mahal is None
    rows = []
    for _t, _sl, ids, poses in _frames(gu.delete(dirty, rej)):
        if len(ids):
            plain.observe(ids, poses)
        rows.append(np.asarray(plain.get_poses()[0], dtype=np.float64)[:7])
    assert np.array_equal(traj, np.array(rows))
    sp.assert_same((state, cov), sp.snap_filter(plain), "gated loop = loop without the rejected")
    assert landmarks == plain.landmarks
    # inserted outlier-only frames are not stepped: the row repeats (and P was unchanged, checked in the loop)
    offs = dirty["offsets"]
    alone = [t for t in range(len(offs) - 1) if offs[t + 1] > offs[t] and marks[offs[t]:offs[t + 1]].all()]
    assert alone and alone == unstepped
    for t in alone:
        assert np.array_equal(traj[t], traj[t - 1])
    # first occurrences of new markers report exactly 0; every other distance was tested
    first = np.zeros(len(d2), dtype=bool)
    first[np.unique(dirty["ids"], return_index=True)[1]] = True
    assert (d2[first] == 0).all() and (d2[~first] > 0).all() and np.isfinite(d2).all()


# ---- 3. bit rule, log replay ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_gated_log_replay(model, dtype):
    """``process_detection_log`` with the gate: bit for bit the gate-off replay of the log without the rejected detections
    (both models).  Against the per-frame gated loop of the test above: EKF, whose replay takes z from the log as the loop
    does, the same bits, d^2 included; EKF_Rotations, whose replay forms z on the device (its quaternion may differ from the
    host's in the last place: include/ekf_slam_hip.h, ekf_observe_log), the same decisions, and d^2 and trajectory within
    the 1e-9 the project's replay comparisons use."""
    _clean, dirty, marks = _logs(model)
    n, m = _log_family(model)
    flt = _filter(model, n, m, dtype, gate=gu.GATES[model])
    traj, d2 = flt.process_detection_log(dirty["ids"], dirty["poses"], dirty["offsets"], mahal=True)
    b = flt.backend
    assert b.last_sequence_mode() == "serial"
    stats = b.last_log_stats()
    assert stats["frames_pipelined"] == 0 and stats["pipelined_runs"] == 0
    assert stats["frames_stepped"] == int((~gu.extra_frames(dirty, marks)).sum())
    rej = d2 > gu.GATES[model]
    assert np.array_equal(rej, marks)
    assert b.last_gate_stats() == {"tested": len(d2) - len(flt.landmarks), "rejected": int(marks.sum())}
    plain = _filter(model, n, m, dtype)
    cut = gu.delete(dirty, rej)
    want = plain.process_detection_log(cut["ids"], cut["poses"], cut["offsets"])
    assert np.array_equal(traj, want)
    sp.assert_same(sp.snap_filter(flt), sp.snap_filter(plain), "gated replay = replay without the rejected")
    assert flt.landmarks == plain.landmarks
    traj_pf, d2_pf, rej_pf, state_pf, cov_pf, lm_pf, _ = _per_frame_gated(model, dtype)
    assert np.array_equal(rej, rej_pf) and flt.landmarks == lm_pf
    if model == "ekf":
        assert np.array_equal(traj, traj_pf) and np.array_equal(d2, d2_pf)
        sp.assert_same(sp.snap_filter(flt), (state_pf, cov_pf), "gated replay = gated per-frame loop")
    else:
        tested = d2_pf > 0
        assert np.array_equal(d2 > 0, tested)
        err = dict(traj=float(np.abs(traj - traj_pf).max()),
                   mahal=float((np.abs(d2 - d2_pf)[tested] / d2_pf[tested]).max()))
        report(f"filter_gating_log_vs_per_frame_{dtype}", **err)
        assert err["traj"] <= 1e-9 and err["mahal"] <= 1e-9, err


# ---- 4. the smallest shapes at which the kernel can go wrong --------------------------------------------------------------
def _oracle_frame(model, flt, lm_ids, ids, poses):
    """Expected (d^2, kappa) of a frame from the support blocks of the prior the device holds."""
    from update_sweep_util import oracle_at
    state, cov = sp.snap_filter(flt)
    return gu.block_distances(model, oracle_at(QM[model], state, cov, lm_ids), ids, poses)


def _check_frame(model, dtype, n, m, outliers, max_visible=None, seed=5, capacity=None):
    """A dense random prior of n landmarks and a frame of m detections (landmarks repeat when m > n), the detections
    ``outliers`` grossly off; the gated filter against the oracle, and against a filter without the gate on the frame
    without the rejected detections.  Returns (d^2, rejected)."""
    from update_sweep_util import dense_prior
    state, p, lm, ids, poses = dense_prior(QM[model], n, m, seed, dtype)
    rng = np.random.default_rng(seed)
    for j in outliers:
        poses[j] = gu._outlier(model, poses[j], rng, j)
    gate = gu.GATES[model]
    cap, mv = capacity or n, max_visible or m
    flt, plain = _filter(model, cap, mv, dtype, gate=gate), _filter(model, cap, mv, dtype)
    for f in (flt, plain):
        _load_prior(f, state, p, lm)
    want, kappa = _oracle_frame(model, flt, lm, ids, poses)
    before = sp.snap_filter(flt)
    flt.observe(ids, poses)
    flt.backend.sync()
    got, rej = flt.last_mahal, flt.last_rejected
    tol = np.array([gu.tolerance(k) for k in kappa])
    assert (np.abs(want - gate) / want > tol).all(), "input: an expected distance within the tolerance of the gate"
    rel = np.abs(got - want) / want
    assert (rel <= tol).all(), (model, dtype, n, m, float((rel / tol).max()))
    expect = np.zeros(m, dtype=bool)
    expect[list(outliers)] = True
    assert np.array_equal(rej, want > gate) and np.array_equal(rej, expect)
    assert flt.backend.last_gate_stats() == {"tested": m, "rejected": len(outliers)}
    keep = ~rej
    if keep.any():
        plain.observe([i for i, s in zip(ids, keep) if s], poses[keep])
        plain.backend.sync()
        sp.assert_same(sp.snap_filter(flt), sp.snap_filter(plain), "gated frame = frame without the rejected")
    else:
        sp.assert_same(sp.snap_filter(flt), before, "no survivor: not stepped")
    return got, rej


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_one_detection(model, dtype):
    _check_frame(model, dtype, 6, 1, ())
    _check_frame(model, dtype, 6, 1, (0,))          # ... rejected: nothing is stepped


@pytest.mark.parametrize("model,m", [("ekf", 64), ("ekf", 65), ("ekf_rotations", 50), ("ekf_rotations", 51)])
def test_at_the_wide_frame_threshold(model, m):
    """The widest frame the fused / stage kernels take and the first wide one (EKF_FLAG_WIDE_FRAMES): with one detection
    rejected, the frame of m = cap + 1 runs where a frame of cap detections runs."""
    _check_frame(model, "float32" if m % 2 else "float64", 30 if model == "ekf" else 12, m, (3,), max_visible=m + 3)
    _check_frame(model, "float64", 30 if model == "ekf" else 12, m, (), max_visible=m + 3)


@pytest.mark.parametrize("model", MODELS)
def test_130_detections_on_40_landmarks(model):
    """Several chunks of the gate kernel (64 / 16 detections each), every landmark seen more than once, rejected detections
    in the first, a middle and the last chunk and on both sides of a chunk boundary."""
    _check_frame(model, "float64", 40, 130, (0, 15, 16, 63, 64, 100, 129), max_visible=130)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model,n", [("ekf", 82), ("ekf_rotations", 63)])
def test_first_and_last_landmark_at_the_padding_edge(model, n, dtype):
    """n at the capacity with 3 n + 10 = 256 (10 n + 10 = 640): the state dimension is the leading dimension, and the
    support block of landmark n - 1 ends in the last row and column of the buffer."""
    from update_sweep_util import dense_prior
    state, p, lm, _ids, _poses = dense_prior(QM[model], n, 2, 9, dtype)
    flt = _filter(model, n, 4, dtype, gate=gu.GATES[model])
    assert flt.backend.ld == state.shape[0]
    _load_prior(flt, state, p, lm)
    ids = [0, n - 1, n - 1]
    _s, _p, _lm, _i, poses = dense_prior(QM[model], n, n, 9, dtype)          # (a pose of every landmark: ids = a permutation)
    by_lm = {i: pose for i, pose in zip(_i, poses)}
    frame = np.array([by_lm[0], by_lm[n - 1], gu._outlier(model, by_lm[n - 1], np.random.default_rng(1), 1)])
    want, kappa = _oracle_frame(model, flt, lm, ids, frame)
    flt.observe(ids, frame)
    flt.backend.sync()
    rel = np.abs(flt.last_mahal - want) / want
    assert (rel <= [gu.tolerance(k) for k in kappa]).all(), rel
    assert flt.last_rejected.tolist() == [False, False, True] == (want > gu.GATES[model]).tolist()


@pytest.mark.parametrize("model", MODELS)
def test_duplicates_of_one_landmark_only_the_outlier_goes(model):
    from update_sweep_util import dense_prior
    state, p, lm, _i, poses = dense_prior(QM[model], 6, 6, 11)
    by_lm = {i: pose for i, pose in zip(_i, poses)}
    ids = [2, 4, 2, 2]
    frame = np.array([by_lm[2], by_lm[4], gu._outlier(model, by_lm[2], np.random.default_rng(2), 1), by_lm[2]])
    flt, plain = _filter(model, 6, 4, gate=gu.GATES[model]), _filter(model, 6, 4)
    for f in (flt, plain):
        _load_prior(f, state, p, lm)
    flt.observe(ids, frame)
    assert flt.last_rejected.tolist() == [False, False, True, False]
    assert flt.last_mahal[0] == flt.last_mahal[3] > 0          # (a detection's distance does not depend on its neighbours)
    plain.observe([2, 4, 2], frame[[0, 1, 3]])
    sp.assert_same(sp.snap_filter(flt), sp.snap_filter(plain), "only the outlier is rejected")


@pytest.mark.parametrize("model", MODELS)
def test_every_detection_rejected_and_first_sightings_only(model):
    _d2, rej = _check_frame(model, "float64", 8, 5, (0, 1, 2, 3, 4))
    assert rej.all()
    # a frame of first sightings only: all exempt, d^2 = 0 exactly, nothing rejected by the tightest gate
    clean, _dirty, _marks = _logs(model)
    n0 = int(clean["offsets"][1])
    each = np.sort(np.unique(clean["ids"][:n0], return_index=True)[1])          # (one detection of every marker)
    n, m = _log_family(model)
    flt, plain = _filter(model, n, m, gate=1e-300), _filter(model, n, m)
    for f in (flt, plain):
        f.observe(clean["ids"][:n0][each], clean["poses"][:n0][each])
    assert len(flt.landmarks) == len(each) >= 1
    assert (flt.last_mahal == 0).all() and not flt.last_rejected.any()
    assert flt.backend.last_gate_stats() == {"tested": 0, "rejected": 0}
    sp.assert_same(sp.snap_filter(flt), sp.snap_filter(plain), "first sightings only")


# ---- 5. gate off is the filter without the gate ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,model", [("c1_detections.npz", "ekf"), ("g5_detections.npz", "ekf_rotations")])
def test_gate_off_is_the_filter_without_the_gate(name, model, dtype):
    det = load_npz(name)
    log = {k: det[k] for k in ("ids", "poses", "offsets", "has_detections")}

    def per_frame(flt):
        rows = []
        for t, _sl, ids, poses in _frames(log):
            if log["has_detections"][t]:
                flt.observe(ids, poses)
            rows.append(np.asarray(flt.get_poses()[0], dtype=np.float64)[:7])
        return np.array(rows)

    def replay(flt, **kw):
        return flt.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"], **kw)

    make = functools.partial(_filter, model, 16, 8, dtype, quat="as_written")
    plain, off = make(), make(gate=np.inf)
    assert plain.backend.cfg.flags & 64 == 0 and off.backend.cfg.flags & 64 == 64 and off.gate == np.inf
    assert off.backend.ws_t.numel() > plain.backend.ws_t.numel()
    want = per_frame(plain)
    assert np.array_equal(per_frame(off), want)          # (through ekf_observe_gated: distances reported, gate off)
    sp.assert_same(sp.snap_filter(off), sp.snap_filter(plain), "per frame, gate off")
    assert off.last_mahal is not None and not off.last_rejected.any()
    plain2, off2, off3 = make(), make(gate=np.inf), make(gate=np.inf)
    want2 = replay(plain2)
    assert np.array_equal(replay(off2), want2)          # (mahal not asked for: ekf_observe_log, pipelined runs included)
    assert off2.backend.last_log_stats() == plain2.backend.last_log_stats()
    sp.assert_same(sp.snap_filter(off2), sp.snap_filter(plain2), "replay, gate off")
    traj3, d2 = replay(off3, mahal=True)          # (distances asked for: serial, nothing rejected, the same bits)
    assert np.array_equal(traj3, want2)
    sp.assert_same(sp.snap_filter(off3), sp.snap_filter(plain2), "replay with mahal, gate off")
    assert off3.backend.last_gate_stats()["rejected"] == 0 and off3.backend.last_log_stats()["frames_pipelined"] == 0
    has = np.repeat(log["has_detections"], np.diff(log["offsets"]))
    assert np.isnan(d2[~has]).all() and np.isfinite(d2[has]).all() and (d2[has] >= 0).all() and (d2[has] > 0).any()


# ---- 6. agreement with the batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_agrees_with_a_one_member_batch(model):
    """One EKFBatch member (f64) and a filter (f64 covariance) with the same gate on the same dirty log: the same rejected
    set, and distances within tolerance(kappa(S_d)) plus the 1e-9 of the project's replay comparisons (the two run
    different update kernels, so their priors differ by rounding from the second frame on)."""
    from aruco_slam_amd.batch import EKFBatch
    _clean, dirty, marks = _logs(model)
    gate = gu.GATES[model]
    kw = dict(gu.FAMILIES[(model, "column")][0])
    out = EKFBatch(1, INIT, model=model, gate=gate, **kw).process_detection_logs([dirty])
    n, m = _log_family(model)
    flt = _filter(model, n, m, gate=gate)
    _traj, d2 = flt.process_detection_log(dirty["ids"], dirty["poses"], dirty["offsets"], mahal=True)
    assert np.array_equal(out.rejected[0], d2 > gate) and np.array_equal(d2 > gate, marks)
    # kappa(S_d) of every detection from the oracle's replay with the same decisions
    from oracle.ekf_numpy import OracleEKF, OracleEKFRotations
    orc = OracleEKFRotations(INIT, mode="fast") if model == "ekf_rotations" else OracleEKF(INIT, mode="fast",
                                                                                            quat_mode="scalar_first")
    worst = 0.0
    for _t, sl, ids, poses in _frames(dirty):
        ids = [int(i) for i in ids]
        if not ids:
            continue
        for k, pose in zip(ids, poses):
            if k not in orc.landmarks:
                orc.add_marker(k, pose)
        _want, kappa = gu.block_distances(model, orc, ids, poses)
        a, b = d2[sl], out.mahal[0][sl]
        for j in range(len(ids)):
            if a[j] == 0 or b[j] == 0:
                assert a[j] == b[j] == 0
                continue
            rel, tol = abs(a[j] - b[j]) / b[j], gu.tolerance(kappa[j]) + 1e-9
            assert rel <= tol, (sl.start + j, a[j], b[j], rel, tol)
            worst = max(worst, rel / tol)
        keep = ~marks[sl]
        if keep.any():
            orc.predict()
            orc.update([k for k, s in zip(ids, keep) if s], poses[keep])
    report(f"filter_gating_vs_batch_{model}", worst_over_tol=worst)


@pytest.mark.parametrize("model,family,m", [("ekf", "column", 1), ("ekf", "column", 16), ("ekf", "wide", 64),
                                            ("ekf_rotations", "column", 1), ("ekf_rotations", "column", 8),
                                            ("ekf_rotations", "wide", 17), ("ekf_rotations", "wide", 33)])
def test_same_prior_same_bits_as_a_one_member_batch(model, family, m):
    """Filter and batch run one code on a detection (ekf_gate_device.h): from the same prior, one further frame gives the
    same d^2 bit for bit and the same rejected set.  The prior is the bootstrap of a clean log without its last landmark
    on a one-member batch, handed over by ``to_filter`` (f64 and bitwise symmetric: the upload is exact).  The frame of m
    detections: known landmarks (repeating once m exceeds the map), in the middle a duplicate of one grossly off, at the
    end the first sighting of the landmark held back (exempt: exactly 0 in both) and a second detection of it grossly off
    (tested against what the first one placed); m = 1 is one known landmark.  m = 16 / 8 fill a one-column frame, m = 64
    fills the filter's chunk (four blocks in the batch), m = 17 and 33 cross the chunk of 16 once and twice."""
    from aruco_slam_amd.batch import EKFBatch
    kw, n, _m_range = gu.FAMILIES[(model, family)]
    kw = dict(kw, max_visible=max(kw["max_visible"], m))
    gate = gu.GATES[model]
    clean = gu.clean_log(model, family, seed=LOG_SEED)
    end = int(clean["offsets"][int(clean["bootstrap_frames"])])
    boot = {"ids": clean["ids"][:end], "poses": clean["poses"][:end],
            "offsets": clean["offsets"][:int(clean["bootstrap_frames"]) + 1]}
    # the frame's poses: every landmark as the log's steady frames first see it (the camera has moved: r = z - h is far
    # from zero, which it is not for the bootstrap's own poses)
    first = end + np.unique(clean["ids"][end:], return_index=True)[1]
    assert clean["ids"][first].tolist() == list(range(n))
    seen = clean["poses"][first]
    new = n - 1
    batch = EKFBatch(1, INIT, model=model, gate=gate, **kw)
    batch.process_detection_logs([gu.delete(boot, boot["ids"] == new)])
    assert batch.status() == [0] and batch.num_landmarks == [n - 1]
    flt = batch.to_filter(0)
    if m == 1:
        ids, poses, tested = np.array([0], np.int32), seen[[0]], np.array([True])
    else:
        ids = np.arange(m - 3) % (n - 1)
        poses, rng, at = seen[ids], np.random.default_rng(m), m // 2
        ids = np.concatenate((ids[:at], ids[[0]], ids[at:], [new, new])).astype(np.int32)
        poses = np.vstack((poses[:at], gu._outlier(model, poses[0], rng, 0), poses[at:], seen[[new]],
                           gu._outlier(model, seen[new], rng, 1)))
        tested = np.arange(m) != m - 2
    offsets = np.array([0, m], np.int64)
    out = batch.process_detection_logs([{"ids": ids, "poses": poses, "offsets": offsets}], mahal=True)
    _traj, d2 = flt.process_detection_log(ids, poses, offsets, mahal=True)
    want = out.mahal[0]
    assert d2.shape == want.shape == (m,) and batch.status() == [0]
    assert np.isfinite(want).all() and (want[tested] > 0).all() and (want[~tested] == 0).all()
    assert np.array_equal(d2, want), (model, m, np.flatnonzero(d2 != want), d2[d2 != want], want[d2 != want])
    assert np.array_equal(d2 > gate, out.rejected[0])
    if m > 1:
        assert out.rejected[0][[m // 2, m - 1]].all() and not out.rejected[0][m - 2]


def test_to_filter_and_load_filter_and_checkpoints_carry_the_gate(tmp_path):
    from aruco_slam_amd.batch import EKFBatch
    batch = EKFBatch(2, INIT, max_landmarks=8, max_visible=4, gate=[7.815, np.inf])
    a, b = batch.to_filter(0), batch.to_filter(1)
    assert a.gate == 7.815 and b.gate == np.inf
    assert EKFBatch(1, INIT, max_landmarks=8, max_visible=4).to_filter(0).gate is None
    a.observe([3, 5], np.array([[0.1, 0.2, 1.0, 0, 0, 0], [-0.2, 0.1, 1.5, 0, 0, 0]]))
    a.set_gate(16.266)
    batch.load_filter(1, a)
    assert batch.gate.tolist() == [7.815, 16.266]
    a.save_checkpoint(str(tmp_path / "ck.npz"))
    c = _filter("ekf", 8, 4, gate=np.inf, quat="as_written")
    c.load_checkpoint(str(tmp_path / "ck.npz"))
    assert c.gate == 16.266 and c.landmarks == a.landmarks
    with pytest.raises(ValueError, match="gate"):
        _filter("ekf", 8, 4, quat="as_written").load_checkpoint(str(tmp_path / "ck.npz"))


# ---- 7. a failed pivot, and the ABI on a handle ----------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_a_failed_pivot_keeps_the_detection_and_the_frame_fails_as_ungated(model):
    from aruco_slam_amd.hip_backend import EkfError
    from update_sweep_util import dense_prior
    state, _p, lm, ids, poses = dense_prior(QM[model], 6, 3, 13)
    flt, plain = _filter(model, 6, 4, gate=gu.GATES[model]), _filter(model, 6, 4)
    for f in (flt, plain):
        _load_prior(f, state, -np.eye(state.shape[0]), lm)          # (no S_d and no S can be positive definite)
        f.observe(ids, poses)
    assert np.isnan(flt.last_mahal).all() and not flt.last_rejected.any()
    assert flt.backend.last_gate_stats() == {"tested": 3, "rejected": 0}
    for f in (flt, plain):
        with pytest.raises(EkfError) as err:
            f.backend.sync()
        assert err.value.code == EKF_ERR_NUMERIC
    # the error is sticky: nothing is tested any more, every detection stays
    flt.observe(ids, poses)
    assert np.isnan(flt.last_mahal).all() and not flt.last_rejected.any()
    flt.reset()
    assert flt.gate == gu.GATES[model]          # (persistent across a reset)


def test_set_gate_on_a_handle():
    from aruco_slam_amd.hip_backend import EkfError
    flt, plain = _filter("ekf", 8, 4, gate=11.345), _filter("ekf", 8, 4)
    lib, h = flt.backend.lib, flt.backend.h
    for bad in (np.nan, 0.0, -3.0, -np.inf):
        assert lib.ekf_set_gate(h, C.c_double(bad)) == -1
        with pytest.raises(ValueError, match="gate"):
            flt.set_gate(bad)
        with pytest.raises(ValueError, match="gate"):
            _filter("ekf", 8, 4, gate=bad)
    assert flt.gate == 11.345
    assert lib.ekf_set_gate(h, C.c_double(np.inf)) == 0 and lib.ekf_set_gate(h, C.c_double(7.815)) == 0
    # a filter created without EKF_FLAG_GATE
    assert lib.ekf_set_gate(plain.backend.h, C.c_double(7.815)) == EKF_ERR_STATE
    assert lib.ekf_observe_gated(plain.backend.h, None, None, 1, None, None, None) == EKF_ERR_STATE
    with pytest.raises(ValueError, match="gate"):
        plain.set_gate(7.815)
    plain.set_gate(None)
    assert plain.gate is None and isinstance(EkfError, type)
    # the gate travels with ekf_grow, and the flags stay equal to the library's
    flt.set_gate(7.815)
    flt.backend.grow(32, 8)
    assert flt.gate == 7.815 and flt.backend.cfg.flags & 64
    flt.observe([1, 2], np.array([[0.1, 0.2, 1.0, 0, 0, 0], [-0.2, 0.1, 1.5, 0, 0, 0]]))
    flt.observe([1, 2], np.array([[0.1, 0.2, 1.0, 0, 0, 0], [150.0, -120.0, 130.0, 0, 0, 0]]))
    assert flt.last_rejected.tolist() == [False, True]

