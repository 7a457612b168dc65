"""Per-frame process-noise scale (``frame_scale=True``, ``observe(..., scale=)``, ``advance``) of the single filter on an
MI355X: one step of every update path against the extended-precision step with Q_eff, the bit rules of
``include/ekf_slam_hip.h`` ("Per-frame process-noise scale"), pipelined against serial runs with a scale per frame, the gate
and the rows composing with scales, and the lock-out fixture.  Cases and expected values: ``frame_scale_util.py``
(``test_frame_scale_cpu.py`` checks them without a GPU)."""
import numpy as np
import pytest

import frame_scale_util as fs
import gating_util as gu
import row_noise_util as rn
import support as sp
import update_sweep_util as sw
from conftest import load_npz, report

pytestmark = pytest.mark.gpu

INIT = sw.INIT
DTYPES = ["float64", "float32"]
MODELS = ["ekf", "ekf_rotations"]
QM = {"ekf": "ekf", "ekf_rotations": "rot"}


def _filter(model, n, m, dtype="float64", **kw):
    """model: "ekf" / "rot" (update_sweep_util's names) or gating_util's."""
    kw.setdefault("frame_scale", True)
    if model in ("rot", "ekf_rotations"):
        from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
        kw.pop("quat_update", None)
        return EKF_Rotations(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, **kw)
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    return EKF(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, **kw)


def _loop(flt, log, scale=None, rows=None):
    """The per-frame loop over a log (process_detections); returns the trajectory [F, 7], d^2 [D] and rejected [D] (filters
    with a gate)."""
    offs = log["offsets"]
    traj, d2, rej = [], np.full(len(log["ids"]), np.nan), np.zeros(len(log["ids"]), dtype=bool)
    for t in range(len(offs) - 1):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        kw = {} if scale is None else {"scale": scale[t]}
        if rows is not None and offs[t + 1] > offs[t]:
            kw["noise"] = rows[sl]
        _, cam, _, _ = flt.process_detections(log["ids"][sl] if offs[t + 1] > offs[t] else None, log["poses"][sl], **kw)
        traj.append(np.asarray(cam, dtype=np.float64)[:7])
        if flt.backend.can_gate and offs[t + 1] > offs[t]:
            d2[sl], rej[sl] = flt.last_mahal, flt.last_rejected
    return np.array(traj), d2, rej


# ---- 1. one step against the extended reference ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_refs():
    return fs.step_references()


@pytest.mark.parametrize("group", list(dict.fromkeys(c[0] for c in fs.STEP_CASES)))
def test_one_step_with_a_scale_against_the_extended_reference(group, step_refs):
    """|P' - P'_ref| <= c_P (k+1) u M_P and |x' - x'_ref| <= c_x tau_x M_x with update_sweep_util.C_BOUNDS of the case's
    group, unchanged: their derivation uses kappa(S) <= 1e3 only (asserted in test_frame_scale_cpu.py and here), never the
    size of Q."""
    filters, failures = {}, []
    for dt in DTYPES:
        worst = [0.0, 0.0, 0.0]
        for case in (c for c in fs.STEP_CASES if c[0] == group):
            _g, model, n, m, fused, mv, _range = case
            prior, s, ref = step_refs[(case, dt)]
            assert ref["kappa"] <= sw.KAPPA_MAX and s != 1.0, (case, dt, ref["kappa"])
            key = (model, n, mv, dt, fused)
            if key not in filters:
                filters[key] = _filter(model, n, mv, dt, fused=fused, lookahead=False)
            flt = filters[key]
            sp.restore(flt, prior)
            flt.observe(prior[3], prior[4], scale=s)
            x, p = sp.snap_filter(flt)
            assert np.array_equal(p, p.T), (case, dt)
            r_p, r_x = sw.ratios(ref, p, x, dt)
            worst = [max(worst[0], r_p), max(worst[1], r_x), max(worst[2], ref["kappa"])]
            c_p, c_x = sw.C_BOUNDS[group][dt]
            if r_p > c_p or r_x > c_x:
                failures.append((case[:4], dt, s, r_p, r_x))
        c_p, c_x = sw.C_BOUNDS[group][dt]
        report(f"frame_scale[{group},{dt}]", ratio_P=worst[0], ratio_x=worst[1], c_P=c_p, c_x=c_x, kappa_max=worst[2])
    assert not failures, failures


# ---- 2. bit rule 5(b): a frame with s_eff is the plain frame on a filter configured with the products ---------------------
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gate"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stage"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["ekf", "rot"])
def test_a_scaled_frame_is_the_plain_frame_with_the_products(model, dtype, fused, gated):
    """s_eff in {0, 0.3, 1, 7.5} on a default filter against the plain call on a ``set_state_cov`` twin built with
    (fl(s_eff q_cam), fl(s_eff q_err), fl(s_eff q_lm)): state, P and, with the gate kernel in front (gate=inf: distances
    only), d^2.  The pending part: advance(a), then a frame with b, is the twin with fl((a + b) q).  m = 1, 16, 17 and one
    wide frame (m > 64 / 50), n = 40."""
    n = 40
    wide_m = 52 if model == "rot" else 66
    gate = float("inf") if gated else None
    flt = _filter(model, n, wide_m, dtype, fused=fused, gate=gate)
    a, b = 0.7, 2.4
    twins = {s: _filter(model, n, wide_m, dtype, fused=fused, gate=gate, frame_scale=False, noise=fs.scaled_constants(model, s))
             for s in (0.0, 0.3, 1.0, 7.5, float(np.float64(a) + np.float64(b)))}
    for m in (1, 16, 17, wide_m):
        prior = sw.dense_prior(model, n, m, 500 + m, dtype)
        seen = []
        for s, twin in twins.items():
            sp.restore(flt, prior)
            sp.restore(twin, prior)
            if s == a + b:
                flt.advance(a)
                assert flt.pending_scale == a
                flt.observe(prior[3], prior[4], scale=b)
            else:
                flt.observe(prior[3], prior[4], scale=s)
            assert flt.pending_scale == 0.0
            twin.observe(prior[3], prior[4])
            got = sp.snap_filter(flt)
            sp.assert_same(got, sp.snap_filter(twin), (model, dtype, fused, gated, m, s))
            if gated:
                assert flt.last_mahal.shape == (m,) and (flt.last_mahal > 0).all()
                assert np.array_equal(flt.last_mahal, twin.last_mahal), (m, s)
            assert all(not np.array_equal(got[1], other) for other in seen), (m, s)      # (the scale is not ignored)
            seen.append(got[1])


# ---- 3. bit rule 5(c): a log is its folded form -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_a_log_is_its_folded_form(model, dtype):
    """The ragged log with empty frames (a leading one, single ones, a run of three, a trailing one), first sightings and
    scales (two exact zeros) against the log with its empty frames deleted and their scales folded into the next stepped
    frame: through process_detection_log and through the per-frame loop; EKF: the two agree bit for bit as well."""
    log, scale = fs.ragged_scaled_log(model)
    folded, fscale, left = fs.fold_log(log, scale)
    stepped = np.diff(log["offsets"]) > 0
    n, m = 12, 5
    ends = {}
    for how in ("log", "loop"):
        full, short = _filter(model, n, m, dtype), _filter(model, n, m, dtype)
        if how == "log":
            traj = full.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"], scale=scale)
            want = short.process_detection_log(folded["ids"], folded["poses"], folded["offsets"], scale=fscale)
            assert full.backend.last_log_stats()["frames_stepped"] == stepped.sum()
        else:
            traj = _loop(full, log, scale)[0]
            want = _loop(short, folded, fscale)[0]
        assert full.pending_scale == left == scale[-1] and short.pending_scale == 0.0
        sp.assert_same(sp.snap_filter(full), sp.snap_filter(short), (how, "folded"))
        assert np.array_equal(traj[stepped], want)
        first = int(np.argmax(stepped))
        for t in range(first + 1, len(stepped)):      # (a frame that is not stepped repeats the row before it)
            if not stepped[t]:
                assert np.array_equal(traj[t], traj[t - 1]), t
        ends[how] = (sp.snap_filter(full), traj)
        # the scales matter: the same log without them ends elsewhere
        plain = _filter(model, n, m, dtype)
        plain.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"])
        assert not np.array_equal(plain.uncertainty, ends[how][0][1])
    if model == "ekf":
        sp.assert_same(ends["log"][0], ends["loop"][0], "log = loop")
        first = int(np.argmax(stepped))
        assert np.array_equal(ends["log"][1][first:], ends["loop"][1][first:])
    else:      # (the replay forms z on the device)
        assert np.abs(ends["log"][0][0] - ends["loop"][0][0]).max() <= 1e-9
        assert np.abs(ends["log"][0][1] - ends["loop"][0][1]).max() <= (1e-9 if dtype == "float64" else 1e-5)


# ---- 4. pipelined runs: the two Q of the front kernel -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_pipelined_sequence_with_a_scale_per_frame_is_the_serial_order(model, dtype):
    """n = 64, m = 8, 12 steady frames, a different scale for every frame (one exact 0), a pending scale in front,
    lookahead=True (flags bit 1: always pipeline).  The front kernel of frame t+1 completes its rows of P_{t+1} with frame
    t's Q_eff and predicts with its own: the sequence call gives the bits of the serial sequence call and of the per-frame
    loop, and reports the pipelined mode, so a serial fallback cannot pass.  float32 runs the MFMA tile update."""
    import torch
    from aruco_slam_amd.filters.ekf_with_rotations import euler_xyz_to_quat
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m, steady = 64, 8, 12
    stream = SyntheticStream(n, m, seed=6)
    boot = list(stream.bootstrap())
    frames = list(stream.steady(steady))
    scale = np.exp(np.random.default_rng(13).uniform(np.log(0.25), np.log(8.0), steady))
    scale[4] = 0.0
    assert len(set(scale.tolist())) == steady

    def booted(lookahead):
        flt = _filter(model, n, m, dtype, lookahead=lookahead)
        for ids, poses in boot:
            flt.observe(ids, poses)
        flt.advance(1.75)
        return flt

    loop = booted(False)
    want_traj = []
    for (ids, poses), s in zip(frames, scale):
        loop.observe(ids, poses, scale=s)
        want_traj.append(np.asarray(loop.get_poses()[0], dtype=np.float64)[:7])
    want_traj, want = np.array(want_traj), sp.snap_filter(loop)
    plain = booted(False)
    for ids, poses in frames:
        plain.observe(ids, poses)
    assert not np.array_equal(plain.uncertainty, want[1])

    idx = np.array([[loop.landmarks[int(i)] for i in ids] for ids, _ in frames], dtype=np.int32)
    if model == "ekf":
        z = np.stack([np.asarray(p, dtype=np.float64)[:, :3] for _, p in frames])
    else:
        z = np.stack([np.hstack((np.asarray(p)[:, :3], euler_xyz_to_quat(np.asarray(p)[:, 3:6]))) for _, p in frames])
    for lookahead, mode in ((True, "pipelined"), (False, "serial")):
        seq = booted(lookahead)
        dev = seq.backend.device
        traj_t = torch.empty((steady, 7), dtype=torch.float64, device=dev)
        seq.backend.observe_sequence(torch.tensor(idx, device=dev), torch.tensor(z, dtype=torch.float64, device=dev), traj_t,
                                     scale=scale)
        assert seq.backend.last_sequence_mode() == mode
        assert seq.pending_scale == 0.0
        sp.assert_same(sp.snap_filter(seq), want, mode)
        assert np.array_equal(traj_t.cpu().numpy(), want_traj), mode

    # the log replay plans pipelined runs of its own: with scales they are still the loop (EKF: bit for bit)
    rep = booted(True)
    ids_all = np.concatenate([np.asarray(ids, dtype=np.int32) for ids, _ in frames])
    poses_all = np.concatenate([np.asarray(p, dtype=np.float64).reshape(m, -1)[:, :6] for _, p in frames])
    got_traj = rep.process_detection_log(ids_all, poses_all, np.arange(steady + 1, dtype=np.int64) * m, scale=scale)
    stats = rep.backend.last_log_stats()
    assert stats["frames_pipelined"] > 0 and stats["frames_stepped"] == steady, stats
    if model == "ekf":
        sp.assert_same(sp.snap_filter(rep), want, "log")
        assert np.array_equal(got_traj, want_traj)
    else:
        got = sp.snap_filter(rep)
        tol = 1e-9 if dtype == "float64" else 1e-5
        assert np.abs(got_traj - want_traj).max() <= 1e-9 and np.abs(got[1] - want[1]).max() <= tol


# ---- 5. bit rule 5(a) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", [("c1_detections.npz", "ekf"), ("g5_detections.npz", "ekf_rotations")])
def test_the_flag_without_scales_is_the_filter_without_the_flag(name, model):
    """The golden logs (empty frames included), no scale given: per frame and as a log, a filter with the flag against one
    without it, bit for bit; the pending scale stays 0."""
    det = load_npz(name)
    log = {k: det[k] for k in det.files}
    n, m = (16, 8) if model == "ekf" else (8, 6)
    runs = []
    for flag in (True, False):
        flt = _filter(model, n, m, frame_scale=flag)
        offs, has = log["offsets"], log["has_detections"]
        rows = []
        for t in range(len(offs) - 1):
            sl = slice(int(offs[t]), int(offs[t + 1]))
            _, cam, _, _ = flt.process_detections(log["ids"][sl] if has[t] else None, log["poses"][sl])
            rows.append(np.asarray(cam, dtype=np.float64)[:7])
        rep = _filter(model, n, m, frame_scale=flag)
        traj = rep.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"])
        assert flt.pending_scale == 0.0 and rep.pending_scale == 0.0
        runs.append((np.array(rows), sp.snap_filter(flt), traj, sp.snap_filter(rep), rep.backend.last_log_stats()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2]) and runs[0][4] == runs[1][4]
    sp.assert_same(runs[0][1], runs[1][1], "per frame")
    sp.assert_same(runs[0][3], runs[1][3], "log")


@pytest.mark.parametrize("model", MODELS)
def test_scales_all_one_are_no_scale(model):
    """A log whose frames are all stepped: scale = 1.0 everywhere against no scale, per frame and as a log (pipelined runs
    included), bit for bit."""
    log = gu.clean_log(model, "column", seed=1)
    kw, n, _range = gu.FAMILIES[(model, "column")]
    frames = len(log["offsets"]) - 1
    assert (np.diff(log["offsets"]) > 0).all()
    ones = np.ones(frames)
    a, b = _filter(model, n, kw["max_visible"]), _filter(model, n, kw["max_visible"])
    ta = a.process_detection_log(log["ids"], log["poses"], log["offsets"], scale=ones)
    tb = b.process_detection_log(log["ids"], log["poses"], log["offsets"])
    assert a.backend.last_log_stats() == b.backend.last_log_stats()
    assert np.array_equal(ta, tb)
    sp.assert_same(sp.snap_filter(a), sp.snap_filter(b), "log")
    c, d = _filter(model, n, kw["max_visible"]), _filter(model, n, kw["max_visible"], frame_scale=False)
    tc, td = _loop(c, log, ones)[0], _loop(d, log)[0]
    assert np.array_equal(tc, td)
    sp.assert_same(sp.snap_filter(c), sp.snap_filter(d), "loop")


# ---- 6. gate and rows compose -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_gate_rows_and_scales_compose(model, dtype):
    """gating_util's dirty log (family "column": outliers, frames of outliers only, empty frames) with rows and a scale per
    frame: the rejected set is the marks, a frame whose detections are all rejected moves its scale into the pending scale
    and the next frame runs with p + s, and the gated run is bit for bit the ungated run on the log without the rejected
    detections, with their rows deleted alike and the same scales, per frame and as a log."""
    clean = gu.clean_log(model, "column", seed=0)
    dirty, marks = gu.dirty_log(model, clean, seed=0)
    rows = rn.log_rows(model, dirty, 0)
    kw, n, _range = gu.FAMILIES[(model, "column")]
    m, gate = kw["max_visible"], gu.GATES[model]
    frames = len(dirty["offsets"]) - 1
    scale = np.exp(np.random.default_rng(31).uniform(np.log(0.5), np.log(2.0), frames))
    flt = _filter(model, n, m, dtype, gate=gate, row_noise=True, quat_update="scalar_first")
    offs = dirty["offsets"]
    traj, rej, pend = [], np.zeros(len(dirty["ids"]), dtype=bool), []
    for t in range(frames):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        before = flt.pending_scale
        if offs[t + 1] > offs[t]:
            flt.observe(dirty["ids"][sl], dirty["poses"][sl], noise=rows[sl], scale=scale[t])
            rej[sl] = flt.last_rejected
            survivors = int((~flt.last_rejected).sum())
        else:
            flt.advance(scale[t])
            survivors = 0
        assert flt.pending_scale == (0.0 if survivors else before + scale[t]), t
        pend.append(flt.pending_scale)
        traj.append(np.asarray(flt.get_poses()[0], dtype=np.float64)[:7])
    assert np.array_equal(rej, marks) and marks.any()
    extra = gu.extra_frames(dirty, marks)
    assert extra.sum() >= 4 and all(pend[t] > 0 for t in np.nonzero(extra)[0]) and max(pend) > 0
    # the ungated loop on delete(log, rejected): the frames stay (possibly empty), and so do their scales
    cut, cut_rows = gu.delete(dirty, rej), rows[~rej]
    plain = _filter(model, n, m, dtype, row_noise=True, quat_update="scalar_first")
    traj_p = _loop(plain, cut, scale, cut_rows)[0]
    assert np.array_equal(np.array(traj)[1:], traj_p[1:])
    sp.assert_same(sp.snap_filter(flt), sp.snap_filter(plain), "gated loop = loop without the rejected")
    # ... and as a log
    glog = _filter(model, n, m, dtype, gate=gate, row_noise=True, quat_update="scalar_first")
    g_traj, g_d2 = glog.process_detection_log(dirty["ids"], dirty["poses"], dirty["offsets"], mahal=True, noise=rows, scale=scale)
    assert np.array_equal(g_d2 > gate, marks)
    plog = _filter(model, n, m, dtype, row_noise=True, quat_update="scalar_first")
    p_traj = plog.process_detection_log(cut["ids"], cut["poses"], cut["offsets"], noise=cut_rows, scale=scale)
    assert np.array_equal(g_traj, p_traj)
    sp.assert_same(sp.snap_filter(glog), sp.snap_filter(plog), "gated log = log without the rejected")
    assert glog.pending_scale == plog.pending_scale == flt.pending_scale
    if model == "ekf":
        sp.assert_same(sp.snap_filter(glog), sp.snap_filter(flt), "log = loop")


# ---- 7. the lock-out fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_lockout_fixture_on_the_device(model, dtype):
    """Without scales nothing survives after the gap (ekf_last_gate_stats agrees) and the camera stays where it was; with
    the scales of the timestamps the rejected mask is the oracle's (nothing), the first frame after the gap runs with
    G + 1, and the run ends within LOCKOUT_FACTOR of the position error without the jump."""
    gate = fs.LOCKOUT_GATES[model]
    log = fs.lockout_log(model)
    offs, fa = log["offsets"], log["first_after"]
    after = slice(int(offs[fa]), None)
    want = fs.oracle_scaled_replay(model, log, log["scale"], gate)

    plain = _filter(model, 10, 4, dtype, gate=gate, quat_update="scalar_first", frame_scale=False)
    for t in range(len(offs) - 1):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        if offs[t + 1] == offs[t]:
            continue
        plain.observe(log["ids"][sl], log["poses"][sl])
        stats = plain.backend.last_gate_stats()
        if t >= fa:
            assert plain.last_rejected.all() and stats == {"tested": sl.stop - sl.start, "rejected": sl.stop - sl.start}, t
        else:
            assert stats["rejected"] == 0, t
    assert fs.position_error(np.asarray(plain.get_poses()[0], dtype=np.float64)[None, :7], log) > 0.9 * fs.LOCKOUT[model][1]

    timed = _filter(model, 10, 4, dtype, gate=gate, quat_update="scalar_first")
    traj, d2, rej = _loop(timed, log, log["scale"])
    assert np.array_equal(rej, want["rejected"]) and not rej[after].any()
    assert (d2[int(offs[fa]):int(offs[fa + 1])] <= 0.5 * gate).all()
    still = fs.lockout_log(model, jump=0.0)
    base = fs.oracle_scaled_replay(model, still, still["scale"], gate)
    err, err0 = fs.position_error(traj, log), fs.position_error(base, still)
    report(f"frame_scale_lockout_device[{model},{dtype}]", position_error=err, position_error_no_jump=err0)
    assert err <= fs.LOCKOUT_FACTOR * err0
    # ... and as one replay call
    rep = _filter(model, 10, 4, dtype, gate=gate, quat_update="scalar_first")
    r_traj, r_d2 = rep.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"], mahal=True,
                                             scale=log["scale"])
    assert np.array_equal(r_d2 > gate, want["rejected"])
    if model == "ekf":
        assert np.array_equal(r_traj[1:], traj[1:])


# ---- 8. the pending scale as state of the filter ----------------------------------------------------------------------------
def test_pending_scale_survives_grow_remove_and_checkpoints(tmp_path):
    ids = list(range(6))
    poses = np.column_stack((np.linspace(-0.5, 0.5, 6), np.linspace(0.3, -0.3, 6), np.linspace(1.5, 2.5, 6), np.zeros((6, 3))))
    flt = _filter("ekf", 4, 4)
    assert flt.pending_scale == 0.0
    flt.advance(0.5)
    flt.process_detections(None, np.array([]), scale=0.25)
    assert flt.pending_scale == 0.75
    flt.observe(ids, poses, scale=2.0)      # grows landmarks and detections per frame: s_eff = 2.75
    big = _filter("ekf", 16, 8, frame_scale=False, noise=fs.scaled_constants("ekf", 2.75))
    big.observe(ids, poses)
    sp.assert_same(sp.snap_filter(flt), sp.snap_filter(big), "a grown filter used its pending scale")
    assert flt.pending_scale == 0.0 and flt.backend.can_frame_scale
    flt.advance(1.5)
    flt.backend.grow(32)
    assert flt.pending_scale == 1.5
    flt.remove_markers([4])
    assert flt.pending_scale == 1.5 and flt.num_landmarks == 5
    # predicted landmark variances: diag(P) + fl(p q_lm) on the host
    var = flt.get_lm_uncertainties()
    assert np.array_equal(flt.get_lm_uncertainties(predicted=True), var + 1.5 * 0.01)
    flt.save_checkpoint(tmp_path / "ck.npz")
    with pytest.raises(ValueError, match="frame_scale=True"):
        _filter("ekf", 8, 8, frame_scale=False).load_checkpoint(tmp_path / "ck.npz")
    back = _filter("ekf", 8, 8)
    back.load_checkpoint(tmp_path / "ck.npz")
    assert back.pending_scale == 1.5
    keep = [i for i in ids if i != 4]
    back.observe(keep, poses[keep], scale=0.5)
    flt.observe(keep, poses[keep], scale=0.5)
    sp.assert_same(sp.snap_filter(back), sp.snap_filter(flt), "checkpoint")
    # a checkpoint without the key leaves the pending scale 0
    with np.load(tmp_path / "ck.npz") as ck:
        old = {k: ck[k] for k in ck.files if k not in ("frame_scale", "pending_scale")}
    np.savez(tmp_path / "old.npz", **old)
    back.advance(3.0)
    back.load_checkpoint(tmp_path / "old.npz")
    assert back.pending_scale == 0.0
    flt.advance(2.0)
    flt.reset()
    assert flt.pending_scale == 0.0 and flt.num_landmarks == 0


# ---- argument checks that need a handle ---------------------------------------------------------------------------------
def test_scales_are_validated_before_the_frame_changes_anything():
    flt = _filter("ekf", 8, 4)
    ids, poses = [3, 5], np.array([[0.1, 0.2, 1.5, 0, 0, 0], [-0.2, 0.1, 2.0, 0, 0, 0]])
    for bad in (np.nan, np.inf, -1.0, [1.0, 2.0], "x"):
        with pytest.raises(ValueError, match="scale"):
            flt.observe(ids, poses, scale=bad)
        with pytest.raises(ValueError, match="scale"):
            flt.advance(bad)
    for bad in ([1.0], [1.0, np.nan], [1.0, -2.0], 1.0):
        with pytest.raises(ValueError, match="scale"):
            flt.process_detection_log(np.array(ids), poses, np.array([0, 1, 2]), scale=bad)
    assert flt.num_landmarks == 0 and flt.landmarks == {} and flt.pending_scale == 0.0
    flt.observe(ids, poses, scale=0.0)
    assert flt.num_landmarks == 2
    plain = _filter("ekf", 8, 4, frame_scale=False)
    for call in (lambda: plain.observe(ids, poses, scale=1.0), lambda: plain.advance(1.0),
                 lambda: plain.process_detections(None, np.array([]), scale=1.0),
                 lambda: plain.process_detection_log(np.array(ids), poses, np.array([0, 2]), scale=[1.0])):
        with pytest.raises(ValueError, match="frame_scale=True"):
            call()
    assert plain.num_landmarks == 0 and plain.pending_scale == 0.0
    # the C ABI itself: a scale on a handle without the flag, and a bad scale on one with it
    import ctypes as C
    plain.observe(ids, poses)
    idx, z = np.array([0, 1], np.int32), np.ascontiguousarray(poses[:, :3])
    dp = C.POINTER(C.c_double)
    args = (idx.ctypes.data_as(C.POINTER(C.c_int32)), z.ctypes.data_as(dp), None, 2, None, None, None)
    pb, fb = plain.backend, flt.backend
    assert pb.lib.ekf_observe_scaled(pb.h, *args, 1.0) == -4 and pb.lib.ekf_advance(pb.h, 1.0) == -4
    assert pb.lib.ekf_set_pending_scale(pb.h, 1.0) == -4
    before = sp.snap_filter(flt)
    one = np.array([np.nan])
    for bad in (np.nan, np.inf, -1.0):
        one[0] = bad
        assert fb.lib.ekf_observe_scaled(fb.h, *args, bad) == -1 and fb.lib.ekf_advance(fb.h, bad) == -1
        assert fb.lib.ekf_set_pending_scale(fb.h, bad) == -1
        assert fb.lib.ekf_observe_sequence_device_scaled(fb.h, 8, 8, None, one.ctypes.data_as(dp), 2, 1, None) == -1
    assert flt.pending_scale == 0.0
    sp.assert_same(sp.snap_filter(flt), before, "a rejected call enqueues nothing")


# ---- run_slam --frame-period ------------------------------------------------------------------------------------------------
def _run_slam(tmp_path, name, log_path, resident, frame_period=None, gate=None):
    import argparse
    from aruco_slam_amd.main import run_slam
    out = tmp_path / name
    args = argparse.Namespace(video="input_video.mp4", filter="ekf", detections=str(log_path), output_dir=str(out),
                              filter_kwargs={"max_landmarks": 16, "max_visible": 8}, resident=resident, gate=gate,
                              frame_period=frame_period)
    run_slam.main(args)
    return (out / "trajectory.txt").read_text(), (out / "map.txt").read_text()


def test_run_slam_frame_period(tmp_path, golden_dir):
    """C1 (empty frames, 30 fps timestamps) with --frame-period: the frame loop and --resident write the same bytes, with
    and without --gate; the lines are the camera poses of the Python loop with scale = dt / period; without the option
    nothing changes; a doubled period halves the scales and gives other bytes."""
    from aruco_slam_amd.main import run_slam
    path = golden_dir / "c1_detections.npz"
    det = load_npz("c1_detections.npz")
    log = {k: det[k] for k in det.files}
    plain = _run_slam(tmp_path, "plain", path, False)
    assert _run_slam(tmp_path, "plain_res", path, True) == plain
    loop = _run_slam(tmp_path, "loop", path, False, 33.3)
    assert _run_slam(tmp_path, "resident", path, True, 33.3) == loop
    assert loop != plain and _run_slam(tmp_path, "slow", path, False, 66.6) != loop
    assert _run_slam(tmp_path, "gate_res", path, True, 33.3, 11.345) == _run_slam(tmp_path, "gate_loop", path, False, 33.3, 11.345)
    scale = run_slam.frame_scales(str(path), 33.3)
    flt = _filter("ekf", 16, 8)
    offs, has = log["offsets"], log["has_detections"]
    want = []
    for t in range(len(has)):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        _, cam, _, _ = flt.process_detections(log["ids"][sl] if has[t] else None, log["poses"][sl], scale=scale[t])
        want.append(np.asarray(cam, dtype=np.float64)[:7])
    got = np.array([[float(v) for v in ln.split()[1:]] for ln in loop[0].splitlines()])
    assert got.shape == (len(has), 7) and np.allclose(got, np.array(want), rtol=0, atol=1e-12)
    np.savez(tmp_path / "back.npz", **{**log, "timestamps_ms": log["timestamps_ms"][::-1].copy()})
    with pytest.raises(ValueError, match="decrease"):
        _run_slam(tmp_path, "back", tmp_path / "back.npz", False, 33.3)
