"""Per-detection measurement noise (``R = diag(rows)``; ``row_noise=True``, ``observe(..., noise=)``) of the single filter
on an MI355X: one step of every update path against the extended-precision step with the same rows, the bit rules of
``include/ekf_slam_hip.h`` (rows equal to a constant are that constant; the flag alone changes nothing; gate and rows
compose), sequence / log / pipelined runs, and the gate deciding by the rows.  Cases and expected values:
``row_noise_util.py`` (``test_row_noise_cpu.py`` checks them without a GPU)."""
import functools

import numpy as np
import pytest

import gating_util as gu
import row_noise_util as rn
import support as sp
import update_sweep_util as sw
from conftest import load_npz, report

pytestmark = pytest.mark.gpu

INIT = sw.INIT
LOG_SEED = 0
DTYPES = ["float64", "float32"]
MODELS = ["ekf", "ekf_rotations"]
QM = {"ekf": "ekf", "ekf_rotations": "rot"}


def _filter(model, n, m, dtype="float64", **kw):
    """model: "ekf" / "rot" (update_sweep_util's names) or gating_util's."""
    if model in ("rot", "ekf_rotations"):
        from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
        kw.pop("quat_update", None)
        return EKF_Rotations(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, **kw)
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    return EKF(INIT, max_landmarks=n, max_visible=m, cov_dtype=dtype, **kw)


# ---- 1. one step against the extended reference ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_refs():
    return rn.step_references()


@pytest.mark.parametrize("group", list(dict.fromkeys(c[0] for c in rn.STEP_CASES)))
def test_one_step_with_rows_against_the_extended_reference(group, step_refs):
    """|P' - P'_ref| <= c_P (k+1) u M_P and |x' - x'_ref| <= c_x tau_x M_x with update_sweep_util.C_BOUNDS of the case's
    group, unchanged: their derivation uses kappa(S) <= 1e3 only (asserted), never R = r I."""
    filters, failures = {}, []
    for dt in DTYPES:
        worst = [0.0, 0.0, 0.0]
        for case in (c for c in rn.STEP_CASES if c[0] == group):
            _g, model, n, m, fused, mv, _range = case
            prior, rows, ref = step_refs[(case, dt)]
            assert ref["kappa"] <= sw.KAPPA_MAX, (case, dt, ref["kappa"])
            key = (model, n, mv, dt, fused)
            if key not in filters:
                filters[key] = _filter(model, n, mv, dt, fused=fused, lookahead=False, row_noise=True)
            flt = filters[key]
            sp.restore(flt, prior)
            flt.observe(prior[3], prior[4], noise=rows)
            x, p = sp.snap_filter(flt)
            assert np.array_equal(p, p.T), (case, dt)
            r_p, r_x = sw.ratios(ref, p, x, dt)
            worst = [max(worst[0], r_p), max(worst[1], r_x), max(worst[2], ref["kappa"])]
            c_p, c_x = sw.C_BOUNDS[group][dt]
            if r_p > c_p or r_x > c_x:
                failures.append((case[:4], dt, r_p, r_x))
        c_p, c_x = sw.C_BOUNDS[group][dt]
        report(f"row_noise[{group},{dt}]", ratio_P=worst[0], ratio_x=worst[1], c_P=c_p, c_x=c_x, kappa_max=worst[2])
    assert not failures, failures


# ---- 2. bit rule 1: rows equal to c are r_uncertainty = c -----------------------------------------------------------------
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gate"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stage"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["ekf", "rot"])
def test_uniform_rows_are_the_constant_bit_for_bit(model, dtype, fused, gated):
    """rows = 0.37 everywhere on a default filter (r_uncertainty 0.9) against the plain call on a filter built with
    r_uncertainty = 0.37: state, P and, with the gate kernel in front (gate=inf: distances only), d^2.  m = 1, 16, 17 and one
    wide frame (m > 64 / 50), n = 40."""
    n, c = 40, 0.37
    wide_m = 52 if model == "rot" else 66
    gate = float("inf") if gated else None
    with_rows = _filter(model, n, wide_m, dtype, fused=fused, gate=gate, row_noise=True)
    constant = _filter(model, n, wide_m, dtype, fused=fused, gate=gate, noise={"r_uncertainty": c})
    rd = rn.RD[model]
    for m in (1, 16, 17, wide_m):
        prior = sw.dense_prior(model, n, m, 300 + m, dtype)
        sp.restore(with_rows, prior)
        sp.restore(constant, prior)
        with_rows.observe(prior[3], prior[4], noise=np.full(m, c) if m % 2 else np.full((m, rd), c))
        constant.observe(prior[3], prior[4])
        sp.assert_same(sp.snap_filter(with_rows), sp.snap_filter(constant), (model, dtype, fused, gated, m))
        if gated:
            assert with_rows.last_mahal.shape == (m,) and (with_rows.last_mahal > 0).all()
            assert np.array_equal(with_rows.last_mahal, constant.last_mahal), m
        # ... and the rows are not ignored: the filter's own constant gives other bits
        sp.restore(with_rows, prior)
        with_rows.observe(prior[3], prior[4])
        assert not np.array_equal(with_rows.uncertainty, constant.uncertainty), m


# ---- 3. bit rule 2: the flag alone changes nothing ------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", [("c1_detections.npz", "ekf"), ("g5_detections.npz", "ekf_rotations")])
def test_the_flag_without_noise_is_the_filter_without_the_flag(name, model):
    det = load_npz(name)
    log = {k: det[k] for k in det.files}
    offs, has = log["offsets"], log["has_detections"]
    n, m = (16, 8) if model == "ekf" else (8, 6)
    per_frame = []
    for flag in (True, False):
        flt = _filter(model, n, m, row_noise=flag)
        rows = []
        for t in range(len(offs) - 1):
            sl = slice(int(offs[t]), int(offs[t + 1]))
            _, cam, _, _ = flt.process_detections(log["ids"][sl] if has[t] else None, log["poses"][sl])
            rows.append(np.asarray(cam, dtype=np.float64)[:7])
        per_frame.append((np.array(rows), sp.snap_filter(flt), dict(flt.landmarks)))
    assert np.array_equal(per_frame[0][0], per_frame[1][0]) and per_frame[0][2] == per_frame[1][2]
    sp.assert_same(per_frame[0][1], per_frame[1][1], "per frame")
    replay = []
    for flag in (True, False):
        flt = _filter(model, n, m, row_noise=flag)
        traj = flt.process_detection_log(log["ids"], log["poses"], log["offsets"], log["has_detections"])
        replay.append((traj, sp.snap_filter(flt), flt.backend.last_log_stats()))
    assert np.array_equal(replay[0][0], replay[1][0]) and replay[0][2] == replay[1][2]
    sp.assert_same(replay[0][1], replay[1][1], "log")
    assert replay[0][1][0].tobytes() == replay[1][1][0].tobytes() and replay[0][1][1].tobytes() == replay[1][1][1].tobytes()


# ---- 4. sequence, log and pipelined runs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_sequence_log_and_per_frame_loop_agree_with_rows_in_the_pipelined_mode(model):
    """n = 64, m = 8, 24 steady frames, non-uniform rows, lookahead=True (flags bit 1: always pipeline).  EKF: the sequence
    call, the log replay and the per-frame loop agree in every bit; EKF_Rotations: to 1e-9 (the replay forms z on the
    device).  Both calls report the pipelined mode, so a serial fallback cannot pass."""
    import torch
    from aruco_slam_amd.filters.ekf_with_rotations import euler_xyz_to_quat
    from aruco_slam_amd.synthetic import SyntheticStream
    n, m, steady = 64, 8, 24
    stream = SyntheticStream(n, m, seed=5)
    boot = list(stream.bootstrap())
    frames = list(stream.steady(steady))
    rd = gu.RD[model]
    rows = np.exp(np.random.default_rng(9).uniform(np.log(0.3), np.log(3.0), (steady, m, rd)))

    def booted():
        flt = _filter(model, n, m, lookahead=True, row_noise=True)
        for ids, poses in boot:
            flt.observe(ids, poses)
        return flt

    loop = booted()
    want_traj = []
    for (ids, poses), r in zip(frames, rows):
        loop.observe(ids, poses, noise=r)
        want_traj.append(np.asarray(loop.get_poses()[0], dtype=np.float64)[:7])
    want_traj = np.array(want_traj)
    want = sp.snap_filter(loop)
    plain = booted()      # (the rows matter: the same frames without them end elsewhere)
    for ids, poses in frames:
        plain.observe(ids, poses)
    assert not np.array_equal(plain.uncertainty, want[1])

    seq = booted()
    idx = np.array([[seq.landmarks[int(i)] for i in ids] for ids, _ in frames], dtype=np.int32)
    if model == "ekf":
        z = np.stack([np.asarray(p, dtype=np.float64)[:, :3] for _, p in frames])
    else:
        z = np.stack([np.hstack((np.asarray(p)[:, :3], euler_xyz_to_quat(np.asarray(p)[:, 3:6]))) for _, p in frames])
    dev = seq.backend.device
    traj_t = torch.empty((steady, 7), dtype=torch.float64, device=dev)
    seq.backend.observe_sequence(torch.tensor(idx, device=dev), torch.tensor(z, dtype=torch.float64, device=dev), traj_t,
                                 rows=torch.tensor(rows, dtype=torch.float64, device=dev))
    assert seq.backend.last_sequence_mode() == "pipelined"
    sp.assert_same(sp.snap_filter(seq), want, "sequence")
    assert np.array_equal(traj_t.cpu().numpy(), want_traj)

    rep = booted()
    ids_all = np.concatenate([np.asarray(ids, dtype=np.int32) for ids, _ in frames])
    poses_all = np.concatenate([np.asarray(p, dtype=np.float64).reshape(m, -1)[:, :6] for _, p in frames])
    offsets = np.arange(steady + 1, dtype=np.int64) * m
    got_traj = rep.process_detection_log(ids_all, poses_all, offsets, noise=rows.reshape(-1, rd))
    stats = rep.backend.last_log_stats()
    assert stats["frames_pipelined"] > 0 and stats["frames_stepped"] == steady, stats
    if model == "ekf":
        sp.assert_same(sp.snap_filter(rep), want, "log")
        assert np.array_equal(got_traj, want_traj)
    else:
        got = sp.snap_filter(rep)
        assert np.abs(got_traj - want_traj).max() <= 1e-9 and np.abs(got[0] - want[0]).max() <= 1e-9
        assert np.abs(got[1] - want[1]).max() <= 1e-9


# ---- 5. the gate ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _logs(model):
    clean = gu.clean_log(model, "column", seed=LOG_SEED)
    dirty, marks = gu.dirty_log(model, clean, seed=LOG_SEED)
    return dirty, marks, rn.log_rows(model, dirty, LOG_SEED)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_gated_log_with_rows(model, dtype):
    """gating_util's dirty log (family "column") with rows: the rejected set is the oracle's, d^2 within
    gating_util.tolerance(kappa) of block_distances_rows on the filter's own prior (f64; an f32 filter: the oracle's
    decisions), and the gated run is bit for bit the ungated run on the log without the rejected detections and their rows
    (bit rule 3), per frame and as a log."""
    dirty, marks, rows = _logs(model)
    kw, n, _range = gu.FAMILIES[(model, "column")]
    m = kw["max_visible"]
    gate = gu.GATES[model]
    flt = _filter(model, n, m, dtype, gate=gate, row_noise=True, quat_update="scalar_first")
    offs = dirty["offsets"]
    d2, rej = np.zeros(len(dirty["ids"])), np.zeros(len(dirty["ids"]), dtype=bool)
    traj, worst, checked = [], 0.0, 0
    for t in range(len(offs) - 1):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        ids, poses = dirty["ids"][sl], dirty["poses"][sl]
        if len(ids):
            known = all(int(i) in flt.landmarks for i in ids)
            if dtype == "float64" and known:      # the oracle's distances on the prior the device holds
                lm = [k for k, _ in sorted(flt.landmarks.items(), key=lambda kv: kv[1])]
                orc = sw.oracle_at(QM[model], flt.state, flt.uncertainty, lm, "scalar_first")
                want, kappa = rn.block_distances_rows(model, orc, [int(i) for i in ids], poses, rows[sl])
            flt.observe(ids, poses, noise=rows[sl])
            d2[sl], rej[sl] = flt.last_mahal, flt.last_rejected
            if dtype == "float64" and known:
                for j in range(len(ids)):
                    rel, tol = abs(d2[sl][j] - want[j]) / want[j], gu.tolerance(kappa[j])
                    assert rel <= tol, (t, j, d2[sl][j], want[j])
                    worst, checked = max(worst, rel / tol), checked + 1
        traj.append(np.asarray(flt.get_poses()[0], dtype=np.float64)[:7])
    assert np.array_equal(rej, marks) and marks.any()      # (test_row_noise_cpu.py: the oracle rejects exactly the marks)
    if dtype == "float64":
        assert checked > 100
        report(f"row_noise_gate[{model}]", detections=checked, worst_over_tol=worst)
    # bit rule 3, per frame: the ungated loop on delete(log, rejected) with the rows deleted alike
    cut, cut_rows = gu.delete(dirty, rej), rows[~rej]
    plain = _filter(model, n, m, dtype, row_noise=True, quat_update="scalar_first")
    coffs, rows_p = cut["offsets"], []
    for t in range(len(coffs) - 1):
        sl = slice(int(coffs[t]), int(coffs[t + 1]))
        if coffs[t + 1] > coffs[t]:
            plain.observe(cut["ids"][sl], cut["poses"][sl], noise=cut_rows[sl])
        rows_p.append(np.asarray(plain.get_poses()[0], dtype=np.float64)[:7])
    assert np.array_equal(np.array(traj), np.array(rows_p))
    sp.assert_same(sp.snap_filter(flt), sp.snap_filter(plain), "gated loop = loop without the rejected")
    # ... and as a log
    glog = _filter(model, n, m, dtype, gate=gate, row_noise=True, quat_update="scalar_first")
    g_traj, g_d2 = glog.process_detection_log(dirty["ids"], dirty["poses"], dirty["offsets"], mahal=True, noise=rows)
    assert np.array_equal(g_d2 > gate, marks)
    plog = _filter(model, n, m, dtype, row_noise=True, quat_update="scalar_first")
    p_traj = plog.process_detection_log(cut["ids"], cut["poses"], cut["offsets"], noise=cut_rows)
    assert np.array_equal(g_traj, p_traj)
    sp.assert_same(sp.snap_filter(glog), sp.snap_filter(plog), "gated log = log without the rejected")
    if model == "ekf":      # (the EKF replay takes z from the log as the loop does: the same bits, d^2 included)
        assert np.array_equal(g_d2, d2)
        sp.assert_same(sp.snap_filter(glog), sp.snap_filter(flt), "log = loop")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stage"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", MODELS)
def test_rows_reach_the_gate_both_ways(model, dtype, fused):
    """One frame (row_noise_util.two_sided_frame): under the constant detection 0 is rejected and detection 1 kept; with a
    large row for 0 and a small one for 1, detection 0 is kept and detection 1 rejected."""
    frame = rn.two_sided_frame(model)
    gate = gu.GATES[model]
    m = len(frame["ids"])
    flt = _filter(model, 12, m, dtype, gate=gate, fused=fused, row_noise=True)
    prior = frame["prior"]
    sp.restore(flt, prior)
    flt.observe(frame["ids"], frame["poses"])
    assert flt.last_rejected.tolist() == [True, False] + [False] * (m - 2)
    assert np.allclose(flt.last_mahal, frame["d2_const"], rtol=1e-3 if dtype == "float32" else 1e-9)
    after_const = sp.snap_filter(flt)
    sp.restore(flt, prior)
    flt.observe(frame["ids"], frame["poses"], noise=frame["rows"])
    assert flt.last_rejected.tolist() == [False, True] + [False] * (m - 2)
    assert np.allclose(flt.last_mahal, frame["d2_rows"], rtol=1e-3 if dtype == "float32" else 1e-9)
    assert flt.backend.last_gate_stats() == {"tested": m, "rejected": 1}
    assert not np.array_equal(sp.snap_filter(flt)[1], after_const[1])


# ---- argument checks that need a handle ----------------------------------------------------------------------------------
def test_noise_is_validated_before_the_frame_changes_anything():
    flt = _filter("ekf", 8, 4, row_noise=True)
    ids, poses = [3, 5], np.array([[0.1, 0.2, 1.5, 0, 0, 0], [-0.2, 0.1, 2.0, 0, 0, 0]])
    for bad in ([0.5], np.ones((2, 2)), [0.5, np.nan], [0.5, 0.0], [0.5, -1.0], [np.inf, 1.0]):
        with pytest.raises(ValueError, match="noise"):
            flt.observe(ids, poses, noise=bad)
    assert flt.num_landmarks == 0 and flt.landmarks == {}
    flt.observe(ids, poses, noise=[0.5, 2.0])
    assert flt.num_landmarks == 2
    plain = _filter("ekf", 8, 4)
    with pytest.raises(ValueError, match="row_noise=True"):
        plain.observe(ids, poses, noise=[0.5, 2.0])
    with pytest.raises(ValueError, match="row_noise=True"):
        plain.process_detection_log(np.array(ids), poses, np.array([0, 2]), noise=[0.5, 2.0])
    assert plain.num_landmarks == 0
    # the C ABI itself: rows on a handle without the flag, and a bad row on one with it
    import ctypes as C
    plain.observe(ids, poses)
    b = plain.backend
    idx, z, r = np.array([0, 1], np.int32), np.ascontiguousarray(poses[:, :3]), np.full((2, 3), 0.5)
    dp = C.POINTER(C.c_double)
    args = (idx.ctypes.data_as(C.POINTER(C.c_int32)), z.ctypes.data_as(dp))
    assert b.lib.ekf_observe_rows(b.h, *args, r.ctypes.data_as(dp), 2, None, None, None) == -4
    before = sp.snap_filter(flt)
    for bad in (0.0, -1.0, np.nan, np.inf):
        r[1, 2] = bad
        assert flt.backend.lib.ekf_observe_rows(flt.backend.h, *args, r.ctypes.data_as(dp), 2, None, None, None) == -1
    sp.assert_same(sp.snap_filter(flt), before, "a rejected call enqueues nothing")


def test_checkpoint_and_grow_carry_the_capability(tmp_path):
    flt = _filter("ekf", 4, 4, row_noise=True)
    stream_ids = list(range(6))
    poses = np.column_stack((np.linspace(-0.5, 0.5, 6), np.linspace(0.3, -0.3, 6), np.linspace(1.5, 2.5, 6), np.zeros((6, 3))))
    flt.observe(stream_ids, poses, noise=np.linspace(0.4, 2.0, 6))      # grows landmarks and detections per frame
    assert flt.backend.can_row_noise and flt.num_landmarks == 6
    flt.observe(stream_ids, poses, noise=np.linspace(0.4, 2.0, 6))
    big = _filter("ekf", 16, 8, row_noise=True)
    big.observe(stream_ids, poses, noise=np.linspace(0.4, 2.0, 6))
    big.observe(stream_ids, poses, noise=np.linspace(0.4, 2.0, 6))
    sp.assert_same(sp.snap_filter(flt), sp.snap_filter(big), "a grown filter continues as one built large")
    flt.save_checkpoint(tmp_path / "ck.npz")
    with pytest.raises(ValueError, match="row_noise=True"):
        _filter("ekf", 8, 8).load_checkpoint(tmp_path / "ck.npz")
    back = _filter("ekf", 8, 8, row_noise=True)
    back.load_checkpoint(tmp_path / "ck.npz")
    back.observe(stream_ids, poses, noise=np.linspace(0.4, 2.0, 6))
    flt.observe(stream_ids, poses, noise=np.linspace(0.4, 2.0, 6))
    sp.assert_same(sp.snap_filter(back), sp.snap_filter(flt), "checkpoint")


# ---- run_slam: the optional noise array of a replay file ------------------------------------------------------------------
def _run_slam(tmp_path, name, log_path, resident, gate=None):
    import argparse
    from aruco_slam_amd.main import run_slam
    out = tmp_path / name
    args = argparse.Namespace(video="input_video.mp4", filter="ekf", detections=str(log_path), output_dir=str(out),
                              filter_kwargs={"max_landmarks": 16, "max_visible": 8}, resident=resident, gate=gate)
    run_slam.main(args)
    return (out / "trajectory.txt").read_text(), (out / "map.txt").read_text()


def test_run_slam_uses_the_noise_array_of_a_replay_file(tmp_path, golden_dir):
    """C1 with a ``noise`` array ([D, 3], and [D] in a second file): the frame loop and ``--resident`` write the same bytes,
    with and without ``--gate``; the trajectory is the one ``process_detection_log(noise=)`` gives; a file without the
    array behaves as it did, and a [D] array is its broadcast."""
    from aruco_slam_amd.main import run_slam
    det = load_npz("c1_detections.npz")
    base = {k: det[k] for k in det.files}
    d = len(base["ids"])
    rows = np.exp(np.random.default_rng(21).uniform(np.log(0.3), np.log(3.0), (d, 3)))
    np.savez(tmp_path / "rows.npz", noise=rows, **base)
    np.savez(tmp_path / "per_detection.npz", noise=rows[:, 0], **base)
    np.savez(tmp_path / "broadcast.npz", noise=np.repeat(rows[:, :1], 3, axis=1), **base)
    assert run_slam.detection_noise(str(golden_dir / "c1_detections.npz")) is None
    assert np.array_equal(run_slam.detection_noise(str(tmp_path / "rows.npz")), rows)
    plain = _run_slam(tmp_path, "plain", golden_dir / "c1_detections.npz", False)
    loop = _run_slam(tmp_path, "loop", tmp_path / "rows.npz", False)
    assert _run_slam(tmp_path, "resident", tmp_path / "rows.npz", True) == loop
    assert loop != plain      # (the rows are used)
    for gate in (11.345,):
        assert _run_slam(tmp_path, "gate_res", tmp_path / "rows.npz", True, gate) == \
            _run_slam(tmp_path, "gate_loop", tmp_path / "rows.npz", False, gate)
    assert _run_slam(tmp_path, "one", tmp_path / "per_detection.npz", False) == \
        _run_slam(tmp_path, "three", tmp_path / "broadcast.npz", False)
    # the lines are the camera poses process_detection_log(noise=) returns
    flt = _filter("ekf", 16, 8, row_noise=True)
    traj = flt.process_detection_log(base["ids"], base["poses"], base["offsets"], base["has_detections"], noise=rows)
    stepped = base["has_detections"].astype(bool) & (np.diff(base["offsets"]) > 0)
    got = np.array([[float(v) for v in ln.split()[1:]] for ln in loop[0].splitlines()])
    assert got.shape == (len(stepped), 7)
    first = int(np.argmax(stepped))
    assert np.allclose(got[first:], traj[first:], rtol=0, atol=1e-12)
