"""Per-frame process-noise scale in ``EKFBatch`` (``frame_scale=True``; ``"scale"`` in a log, ``observe_indexed(scale=)``,
``pending_scale``) on an MI355X, for the three window kernels (``gating_util.FAMILIES``) and both models: the bit rules of
``include/ekf_slam_hip.h`` ("Per-frame process-noise scale"), one teacher-forced step against the extended-precision step with
Q_eff, large-map and wide-frame kernels bitwise the one-column kernel, the gate composing with scales, the lock-out fixture,
and the pending scale as state of a member."""
import numpy as np
import pytest

import frame_scale_util as fs
import gating_util as gu
import support as sp
import update_sweep_util as sw
from conftest import report

pytestmark = pytest.mark.gpu

INIT = gu.INIT
ALL = list(gu.FAMILIES)
MODELS = ["ekf", "ekf_rotations"]
QM = {"ekf": "ekf", "ekf_rotations": "rot"}
EXTRA = {"column": {}, "large": {"large_maps": True}, "wide": {"wide_frames": True}}
STEP_MEMBERS = {"ekf": [(1, 1), (39, 3), (82, 8), (39, 16)], "ekf_rotations": [(1, 1), (12, 2), (24, 5), (12, 8)]}
STEP_WIDE = {"ekf": [(40, 17), (40, 36)], "ekf_rotations": [(20, 9), (20, 18)]}
Q_KEYS = ("q_cam", "q_err", "q_lm")


def _same_outputs(got, want, what, names=("trajectory", "nis", "cam_cov", "dof", "mahal", "rejected")):
    for name in names:
        for b, (u, v) in enumerate(zip(getattr(got, name), getattr(want, name))):
            assert np.array_equal(u, v, equal_nan=True), (what, name, b)


# ---- bit rule 5(c) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,family", ALL)
def test_a_batch_log_is_its_folded_form(model, family):
    """Three members, each with its own ragged log with empty frames, first sightings and scales, against the folded logs:
    state, P, and trajectory / nis / cam_cov of the stepped frames, bit for bit; a frame that is not stepped repeats its
    rows with nis 0; the trailing empty frame's scale is left pending."""
    pairs = [fs.ragged_scaled_log(model, seed=s) for s in (3, 4, 5)]
    folded = [fs.fold_log(log, scale) for log, scale in pairs]
    full = sp.family_batch(3, model, family, frame_scale=True)
    got = full.process_detection_logs([dict(log, scale=scale) for log, scale in pairs], nis=True, cam_cov=True)
    short = sp.family_batch(3, model, family, frame_scale=True)
    want = short.process_detection_logs([dict(log, scale=scale) for log, scale, _left in folded], nis=True, cam_cov=True)
    assert full.status() == short.status() == [0] * 3
    sp.assert_same(sp.snap_batch(full), sp.snap_batch(short), "folded", equal_nan=True)
    assert np.array_equal(full.pending_scale, [scale[-1] for _log, scale in pairs]) and not short.pending_scale.any()
    for b, (log, _scale) in enumerate(pairs):
        stepped = np.diff(log["offsets"]) > 0
        for name in ("trajectory", "nis", "cam_cov"):
            assert np.array_equal(getattr(got, name)[b][stepped], getattr(want, name)[b]), (name, b)
        assert (got.nis[b][~stepped] == 0).all()
        for t in range(int(np.argmax(stepped)) + 1, len(stepped)):
            if not stepped[t]:
                assert np.array_equal(got.trajectory[b][t], got.trajectory[b][t - 1])
                assert np.array_equal(got.cam_cov[b][t], got.cam_cov[b][t - 1])
    plain = sp.family_batch(3, model, family, frame_scale=True)      # (the scales are not ignored)
    plain.process_detection_logs([log for log, _scale in pairs])
    assert not np.array_equal(plain.get_cov(0), full.get_cov(0)) and not plain.pending_scale.any()


# ---- bit rule 5(b) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,family", ALL)
def test_a_constant_scale_is_the_members_products_bit_for_bit(model, family):
    """Member b's log carries the scale c_b on every frame (every frame is stepped), c = 0, 0.3, 1, 7.5; the twin, a batch
    without the flag, has (fl(c_b q_cam), fl(c_b q_err), fl(c_b q_lm)) per member: every output -- d^2 and nis included --
    and every member's state and P agree in every bit."""
    consts = [0.0, 0.3, 1.0, 7.5]
    logs = [gu.clean_log(model, family, seed=s) for s in range(4)]
    assert all((np.diff(lg["offsets"]) > 0).all() for lg in logs)
    scaled = sp.family_batch(4, model, family, frame_scale=True)
    got = scaled.process_detection_logs([dict(lg, scale=np.full(len(lg["offsets"]) - 1, c)) for lg, c in zip(logs, consts)],
                                        nis=True, cam_cov=True, mahal=True)
    products = {k: np.array([fs.scaled_constants(model, c)[k] for c in consts]) for k in Q_KEYS}
    twin = sp.family_batch(4, model, family, noise=products)
    want = twin.process_detection_logs(logs, nis=True, cam_cov=True, mahal=True)
    assert scaled.status() == twin.status() == [0] * 4
    _same_outputs(got, want, "scale = c")
    sp.assert_same(sp.snap_batch(scaled), sp.snap_batch(twin), "scale = c", equal_nan=True)
    plain = sp.family_batch(4, model, family)      # (member 2, c = 1, is the plain member; the others are not)
    ref = plain.process_detection_logs(logs)
    assert np.array_equal(ref[2], got.trajectory[2]) and not np.array_equal(ref[3], got.trajectory[3])


# ---- bit rule 5(a) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,family", ALL)
def test_the_flag_alone_and_scales_all_one_change_nothing(model, family):
    """Dirty logs (empty frames, frames of outliers only) with a gate and no scale: a batch with the flag against one
    without it, bit for bit, and the pending scales stay 0.  Clean logs (every frame stepped) with scale = 1.0 everywhere
    against no scale, bit for bit."""
    dirty = [gu.dirty_log(model, gu.clean_log(model, family, seed=s), seed=s)[0] for s in range(2)]
    outs = []
    for flag in (True, False):
        batch = sp.family_batch(2, model, family, gate=gu.GATES[model], frame_scale=flag)
        outs.append((batch.process_detection_logs(dirty, nis=True, cam_cov=True), sp.snap_batch(batch)))
        assert not batch.pending_scale.any()
    _same_outputs(outs[0][0], outs[1][0], "flag")
    sp.assert_same(outs[0][1], outs[1][1], "flag", equal_nan=True)
    clean = [gu.clean_log(model, family, seed=s) for s in range(2)]
    ones = sp.family_batch(2, model, family, frame_scale=True)
    got = ones.process_detection_logs([dict(lg, scale=np.ones(len(lg["offsets"]) - 1)) for lg in clean], nis=True)
    none = sp.family_batch(2, model, family)
    want = none.process_detection_logs(clean, nis=True)
    _same_outputs(got, want, "ones", names=("trajectory", "nis", "dof"))
    sp.assert_same(sp.snap_batch(ones), sp.snap_batch(none), "ones", equal_nan=True)


# ---- one step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,family", ALL)
def test_one_teacher_forced_step_against_the_extended_reference(model, family):
    """Every member one step from its own dense prior (set_member) with its own scale, log-uniform in [0.25, 8], against
    frame_scale_util.extended_step_scaled under update_sweep_util.C_BOUNDS["batch"] (kappa(S) <= 1e3 asserted)."""
    from aruco_slam_amd.batch import EKFBatch
    members = STEP_MEMBERS[model] + (STEP_WIDE[model] if family == "wide" else [])
    kw = dict(gu.FAMILIES[(model, family)][0])
    kw.update(max_landmarks=max(n for n, _ in members), max_visible=max(kw["max_visible"], max(m for _, m in members)))
    kw.pop("quat_update", None)
    batch = EKFBatch(len(members), INIT, model=model, frame_scale=True, **kw)
    logs, refs = [], []
    for b, (n, m) in enumerate(members):
        key = sw.RefKey(QM[model], n, m, "float64", "as_written")
        state, p, lm_ids, ids, poses = sw.dense_prior(key.model, n, m, sw.prior_seed(key))
        s = fs.case_scale(key, *fs.WIDE_SCALES)
        refs.append(fs.extended_step_scaled(sw.oracle_at(key.model, state, p, lm_ids), ids, poses, s))
        batch.set_member(b, state, p, lm_ids)
        logs.append({"ids": np.asarray(ids, np.int32), "poses": poses, "offsets": np.array([0, m], np.int64),
                     "scale": np.array([s])})
    batch.process_detection_logs(logs)
    assert batch.status() == [0] * len(members)
    worst = np.zeros(2)
    for b, ref in enumerate(refs):
        assert ref["kappa"] <= sw.KAPPA_MAX, (members[b], ref["kappa"])
        p = batch.get_cov(b)
        assert np.array_equal(p, p.T)
        worst = np.maximum(worst, sw.ratios(ref, p, batch.get_state(b), "float64"))
    c_p, c_x = sw.C_BOUNDS["batch"]["float64"]
    report(f"frame_scale_batch[{model},{family}]", members=len(members), ratio_P=worst[0], ratio_x=worst[1], c_P=c_p, c_x=c_x)
    assert worst[0] <= c_p and worst[1] <= c_x, worst


# ---- bit rule 5(e), and the gate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_large_and_wide_kernels_are_bitwise_the_one_column_kernel_with_scales(model):
    """A dirty log with a gate and a scale per frame, and the ragged log with empty frames, in all three kernels: the same
    bits in every output, state, P and pending scale."""
    from aruco_slam_amd.batch import EKFBatch
    dirty = gu.dirty_log(model, gu.clean_log(model, "column", seed=0), seed=0)[0]
    frames = len(dirty["offsets"]) - 1
    ragged, rscale = fs.ragged_scaled_log(model)
    logs = [dict(dirty, scale=np.exp(np.random.default_rng(41).uniform(np.log(0.25), np.log(4.0), frames))),
            dict(ragged, scale=rscale)]
    outs = []
    for family in ("column", "large", "wide"):
        kw = dict(gu.FAMILIES[(model, "column")][0], gate=gu.GATES[model], frame_scale=True)
        kw.update(EXTRA[family])
        batch = EKFBatch(2, INIT, model=model, **kw)
        outs.append((batch.process_detection_logs(logs, nis=True, cam_cov=True), sp.snap_batch(batch), batch.pending_scale))
        assert batch.status() == [0, 0]
    assert outs[0][0].rejected[0].any() and outs[0][2][1] == rscale[-1]
    for family, (out, snap, pending) in zip(("large", "wide"), outs[1:]):
        _same_outputs(out, outs[0][0], family)
        sp.assert_same(snap, outs[0][1], family, equal_nan=True)
        assert np.array_equal(pending, outs[0][2]), family


@pytest.mark.parametrize("model,family", ALL)
def test_gate_and_scales_compose(model, family):
    """A dirty log with a gate and a scale per frame is bit for bit the ungated replay of the log without the rejected
    detections (its frames stay, possibly empty, with their scales): a frame whose detections are all rejected leaves its
    scale pending like an empty one.  The last frame of the second member holds outliers only: its scale ends up pending."""
    logs, marks = zip(*(gu.dirty_log(model, gu.clean_log(model, family, seed=s), seed=s) for s in range(2)))
    logs = [dict(lg) for lg in logs]
    # member 1: one more frame of outliers only at the end
    lg = logs[1]
    t = int(np.nonzero(gu.extra_frames(lg, marks[1]) & (np.diff(lg["offsets"]) > 0))[0][0])
    sl = slice(int(lg["offsets"][t]), int(lg["offsets"][t + 1]))
    lg["ids"] = np.concatenate((lg["ids"], lg["ids"][sl]))
    lg["poses"] = np.concatenate((lg["poses"], lg["poses"][sl]))
    lg["offsets"] = np.concatenate((lg["offsets"], [len(lg["ids"])])).astype(np.int64)
    lg["has_detections"] = np.concatenate((lg["has_detections"], [True]))
    marks = [marks[0], np.concatenate((marks[1], np.ones(sl.stop - sl.start, dtype=bool)))]
    rng = np.random.default_rng(51)
    scales = [np.exp(rng.uniform(np.log(0.5), np.log(2.0), len(lg["offsets"]) - 1)) for lg in logs]
    gated = sp.family_batch(2, model, family, gate=gu.GATES[model], frame_scale=True)
    got = gated.process_detection_logs([dict(lg, scale=s) for lg, s in zip(logs, scales)], nis=True, cam_cov=True)
    for b in range(2):
        assert np.array_equal(got.rejected[b], marks[b]), b
    cut = [dict(gu.delete(lg, mk), scale=s) for lg, mk, s in zip(logs, marks, scales)]
    plain = sp.family_batch(2, model, family, frame_scale=True)
    want = plain.process_detection_logs(cut, nis=True, cam_cov=True)
    _same_outputs(got, want, "gated = cut", names=("trajectory", "nis", "cam_cov"))
    sp.assert_same(sp.snap_batch(gated), sp.snap_batch(plain), "gated = cut", equal_nan=True)
    pending = gated.pending_scale
    assert np.array_equal(pending, plain.pending_scale) and pending[0] == 0.0 and pending[1] == scales[1][-1]


# ---- the lock-out fixture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_lockout_fixture_in_a_batch(model):
    """Without scales nothing survives after the gap; with the scales of the timestamps the rejected mask is the oracle's
    and the run ends within LOCKOUT_FACTOR of the position error without the jump."""
    gate = fs.LOCKOUT_GATES[model]
    log = fs.lockout_log(model)
    still = fs.lockout_log(model, jump=0.0)
    offs, fa = log["offsets"], log["first_after"]
    after = slice(int(offs[fa]), None)
    bare = {k: log[k] for k in ("ids", "poses", "offsets", "has_detections")}
    kw = {"quat_update": "scalar_first"} if model == "ekf" else {}
    plain = sp.family_batch(1, model, "column", gate=gate, **kw).process_detection_logs([bare])
    assert plain.rejected[0][after].all() and not plain.rejected[0][:int(offs[fa])].any()
    assert (plain.dof[0][fa:] == 0).all() and (plain.mahal[0][after] >= 2.0 * gate).all()
    assert fs.position_error(plain.trajectory[0], log) > 0.9 * fs.LOCKOUT[model][1]
    timed = sp.family_batch(2, model, "column", gate=gate, frame_scale=True, **kw)
    got = timed.process_detection_logs([dict(bare, scale=log["scale"]),
                                        dict({k: still[k] for k in bare}, scale=still["scale"])])
    want = fs.oracle_scaled_replay(model, log, log["scale"], gate)
    assert np.array_equal(got.rejected[0], want["rejected"]) and not got.rejected[0].any()
    assert (got.mahal[0][int(offs[fa]):int(offs[fa + 1])] <= 0.5 * gate).all()
    err, err0 = fs.position_error(got.trajectory[0], log), fs.position_error(got.trajectory[1], still)
    report(f"frame_scale_lockout_batch[{model}]", position_error=err, position_error_no_jump=err0)
    assert err <= fs.LOCKOUT_FACTOR * err0


# ---- the pending scale as state of a member ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_pending_scale_of_a_member(model):
    family = "column"
    log = gu.clean_log(model, family, seed=2)
    batch = sp.family_batch(3, model, family, frame_scale=True)
    assert batch.pending_scale.tolist() == [0.0, 0.0, 0.0]
    batch.process_detection_logs([log, log, log])
    batch.set_pending_scale([0.5, 1.25, 2.0])
    batch.set_pending_scale(3.0, 2)
    assert batch.pending_scale.tolist() == [0.5, 1.25, 3.0]
    var = batch.get_lm_uncertainties(1)
    q_lm = float(batch.noise[1, 5])
    assert np.array_equal(batch.get_lm_uncertainties(1, predicted=True), var + 1.25 * q_lm)
    # remove_markers keeps it, set_member and reset zero it
    marker = next(iter(batch.landmarks[0]))
    batch.remove_markers({0: [marker]})
    assert batch.pending_scale.tolist() == [0.5, 1.25, 3.0]
    # to_filter / load_filter carry the capability and the pending scale
    flt = batch.to_filter(1)
    assert flt.backend.can_frame_scale and flt.pending_scale == 1.25
    flt.advance(0.25)
    batch.load_filter(2, flt)
    assert batch.pending_scale.tolist() == [0.5, 1.25, 1.5]
    sp.assert_same([sp.snap_batch(batch)[2]], [sp.snap_batch(batch)[1]], "load_filter", equal_nan=True)
    # the member and the filter step on with the same pending scale: a frame without a scale runs with p + 1
    head = int(log["offsets"][int(log["bootstrap_frames"]) + 1])
    t0 = int(log["bootstrap_frames"])
    frame = {"ids": log["ids"][int(log["offsets"][t0]):head], "poses": log["poses"][int(log["offsets"][t0]):head] + 0.0,
             "offsets": np.array([0, head - int(log["offsets"][t0])], np.int64)}
    twin = sp.family_batch(1, model, family, noise={k: fs.scaled_constants(model, 2.25)[k] for k in Q_KEYS})
    twin.set_member(0, batch.get_state(1), batch.get_cov(1), [k for k, _ in sorted(batch.landmarks[1].items(), key=lambda kv: kv[1])])
    batch.process_detection_logs([None, frame, None])
    twin.process_detection_logs([frame])
    sp.assert_same([sp.snap_batch(batch)[1]], sp.snap_batch(twin), "p + 1", equal_nan=True)
    assert batch.pending_scale.tolist() == [0.5, 0.0, 1.5]
    batch.set_member(0, batch.get_state(0), batch.get_cov(0), [k for k, _ in sorted(batch.landmarks[0].items(), key=lambda kv: kv[1])])
    assert batch.pending_scale.tolist() == [0.0, 0.0, 1.5]
    batch.reset(2)
    assert batch.pending_scale.tolist() == [0.0, 0.0, 0.0]
    batch.set_pending_scale(1.0)
    batch.reset()
    assert not batch.pending_scale.any()
    plain = sp.family_batch(1, model, family)
    assert plain.pending_scale.tolist() == [0.0] and plain.to_filter(0).backend.can_frame_scale is False
    with pytest.raises(ValueError, match="frame_scale=True"):
        plain.load_filter(0, flt)


def test_scale_arguments_of_the_batch_are_validated():
    model, family = "ekf", "column"
    log = gu.clean_log(model, family, seed=0)
    frames = len(log["offsets"]) - 1
    plain = sp.family_batch(1, model, family)
    with pytest.raises(ValueError, match="frame_scale=True"):
        plain.process_detection_logs([dict(log, scale=np.ones(frames))])
    with pytest.raises(ValueError, match="frame_scale=True"):
        plain.observe_indexed(np.zeros(1, np.int32), [0, 1], [0, 1], np.zeros((1, 6)), scale=[1.0])
    with pytest.raises(ValueError, match="frame_scale=True"):
        plain.set_pending_scale(1.0)
    batch = sp.family_batch(2, model, family, frame_scale=True)
    for bad in (np.ones(frames - 1), np.ones((frames, 1)), np.full(frames, np.nan), np.full(frames, -1.0), np.full(frames, np.inf)):
        with pytest.raises(ValueError, match="scale"):
            batch.process_detection_logs([dict(log, scale=bad), dict(log, scale=np.ones(frames))])
    with pytest.raises(ValueError, match="every log"):
        batch.process_detection_logs([dict(log, scale=np.ones(frames)), log])
    for bad in (np.nan, -1.0, np.inf):
        with pytest.raises(ValueError, match="pending"):
            batch.set_pending_scale(bad)
    assert batch.num_landmarks == [0, 0] and not batch.pending_scale.any()
    # the C ABI itself
    import ctypes as C
    one = np.ones(1)
    dp = C.POINTER(C.c_double)
    assert plain.lib.ekf_batch_set_pending_scale(plain.h, -1, one.ctypes.data_as(dp)) == -4
    assert plain.lib.ekf_batch_observe_logs_scaled(plain.h, None, None, None, None, None, 8, None, 0, None, None, None,
                                                   None) == -4
    one[0] = -1.0
    assert batch.lib.ekf_batch_set_pending_scale(batch.h, 0, one.ctypes.data_as(dp)) == -1
