"""The edges of offline smoothing on the device, around a good pass: a pivot that fails INSIDE each of the four passes
(tampered records), workspaces and histories that hold NaN bytes before the call and outputs that hold a sentinel, records
of four and five blocks behind a wide first frame, the record table under a gate against the header's rules, and a batch
of more members than the GPU has compute units.  Bounds are ``smooth_util.bound`` and ``smooth_cov_util.record_bound``;
everything else is bit for bit.  The poisoned workspaces and the sentinel-filled outputs reach the library by ctypes
(``direct_smooth``, ``direct_smooth_cov``, ``direct_batch_smooth``): the Python wrappers allocate their own buffers.
``test_smooth_edges_cpu.py`` checks the helpers without a GPU."""
import numpy as np
import pytest

import batch_smooth_util as bu
import smooth_cov_util as sc
import smooth_util as su
import support as sp

pytestmark = pytest.mark.gpu
INIT = sc.INIT
GATE = 1e-3
GATE_TIGHT = 1e-4      # under the ragged log's scales d^2 is a few 1e-4: this gate leaves whole frames without a survivor
OUT_KEYS = ("smoothed", "cam_cov", "filt_cam_cov", "first_cov")


def _fresh(name):
    """(log, filter, history, frames, records, info) of an own recorded replay: these tests write into the history."""
    log, motion, scale = sc.scene(name)
    size = 10 if name == "tracking" else 8
    flt = sc.new_filter(n=size, m=size, motion=motion is not None, frame_scale=scale is not None)
    traj, history = sc.recorded_replay(flt, log, motion, scale)
    records, info = su.device_records(flt.backend, history)
    return log, flt, history, traj.shape[0], records, info


def _rows(info, r_bad):
    """Masks over the frames: before the first record, of a record behind r_bad, of a record up to r_bad."""
    rec_of = info["frame_record"]
    return rec_of < 0, rec_of > r_bad, (rec_of >= 0) & (rec_of <= r_bad)


def _filter_snap(flt):
    return flt.backend.get_state(), flt.backend.get_cov()


def _nothing_sticky(name, log, flt):
    """One further frame on the filter gives the bits of a twin that replayed the log and never smoothed."""
    size = 10 if name == "tracking" else 8
    twin = sc.new_filter(n=size, m=size)
    sc.recorded_replay(twin, log, record=False)
    sl = slice(int(log["offsets"][-2]), int(log["offsets"][-1]))
    for f in (flt, twin):
        f.observe(log["ids"][sl], log["poses"][sl])
    for u, v in zip(_filter_snap(flt), _filter_snap(twin)):
        assert np.array_equal(u, v)


# ---- 1. a pivot that fails inside the pass -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,blocked,r_bad,ks", su.FAIL_STATE)
def test_a_failed_pivot_in_the_state_pass(name, blocked, r_bad, ks):
    """P[k][k] = -1e3 in record r_bad of the caller's history: ``ekf_smooth_history`` returns EKF_ERR_NUMERIC, the lead rows
    and the rows of the records behind r_bad have the bits of the untampered pass of the same tier, the rows of the records
    up to r_bad still hold the sentinel, the filter keeps its bits and nothing sticky is left, and with the word restored
    the call returns the reference bits.  tracking: the resident tier's early return; n19 forced blocked: the first pivot
    of block 0 and the last of the ragged block 1; n51 natural blocked: a pivot of block 2."""
    log, flt, history, frames, records, info = _fresh(name)
    b = flt.backend
    assert (max(r["dims"] for r in records) > su.RESIDENT_DIMS) == (name in su.BLOCKED_SCENES)
    rc, ref = su.direct_smooth(b, history, frames, blocked)
    assert rc == 0 and not (ref == su.SENTINEL).any()
    before = _filter_snap(flt)
    lead, later, upto = _rows(info, r_bad)
    assert later.any() and upto.any()
    for k in ks:
        restore = su.tamper(history, b.sync, su.record_offset(info["dims"], r_bad), records[r_bad]["x"], records[r_bad]["P"], k,
                            su.TAMPER_VALUE)
        rc, got = su.direct_smooth(b, history, frames, blocked)
        assert rc == su.EKF_ERR_NUMERIC, (k, rc)
        assert np.array_equal(got[lead], ref[lead]) and np.array_equal(got[later], ref[later]), k
        assert (got[upto] == su.SENTINEL).all(), k
        for u, v in zip(before, _filter_snap(flt)):
            assert np.array_equal(u, v)
        restore()
        rc, again = su.direct_smooth(b, history, frames, blocked)
        assert rc == 0 and np.array_equal(again, ref), k
    _nothing_sticky(name, log, flt)


@pytest.mark.parametrize("name,r_bad,ks", su.FAIL_COV)
def test_a_failed_pivot_in_the_covariance_pass(name, r_bad, ks):
    """The same through ``ekf_smooth_history_cov``: EKF_ERR_NUMERIC; `smoothed`, `cam_cov` and `filt_cam_cov` keep the
    reference bits on the lead rows and behind r_bad and the sentinel up to r_bad, and so does all of `first_cov`."""
    log, flt, history, frames, records, info = _fresh(name)
    b = flt.backend
    n0 = records[0]["dims"]
    rc, ref = sc.direct_smooth_cov(b, history, frames, n0)
    assert rc == 0 and not any((ref[key] == su.SENTINEL).any() for key in OUT_KEYS)
    before = _filter_snap(flt)
    lead, later, upto = _rows(info, r_bad)
    assert later.any() and upto.any()
    for k in ks:
        assert k < records[r_bad]["dims"]
        restore = su.tamper(history, b.sync, su.record_offset(info["dims"], r_bad), records[r_bad]["x"], records[r_bad]["P"], k,
                            su.TAMPER_VALUE)
        rc, got = sc.direct_smooth_cov(b, history, frames, n0)
        assert rc == su.EKF_ERR_NUMERIC, (k, rc)
        for key in ("smoothed", "cam_cov", "filt_cam_cov"):
            assert sp.same(got[key][lead], ref[key][lead], equal_nan=True), (k, key)
            assert np.array_equal(got[key][later], ref[key][later]), (k, key)
            assert (got[key][upto] == su.SENTINEL).all(), (k, key)
        assert (got["first_cov"] == su.SENTINEL).all(), k
        for u, v in zip(before, _filter_snap(flt)):
            assert np.array_equal(u, v)
        restore()
        rc, again = sc.direct_smooth_cov(b, history, frames, n0)
        assert rc == 0 and all(sp.same(again[key], ref[key], equal_nan=True) for key in OUT_KEYS), k
    _nothing_sticky(name, log, flt)


def test_a_failed_pivot_in_one_member_of_a_batch():
    """Three members over the tracking scene behind one empty frame (so that every member has a lead row); record 20 of
    member 1 is tampered.  The call returns EKF_OK, the pass's status is [0, -5, 0], EVERY row of member 1 is NaN -- the
    lead row and the last record's rows included --, members 0 and 2 keep their bits, and status, state and P of every
    member are unchanged."""
    log = bu.scene_log("tracking")
    log = {"ids": log["ids"], "poses": log["poses"], "offsets": np.concatenate(([0], log["offsets"])),
           "has_detections": np.concatenate(([False], log["has_detections"]))}
    batch = bu.new_batch(3, max_landmarks=10, noise={"q_cam": [0.3, 0.1, 0.5]})
    batch.process_detection_logs([log] * 3, record=True)
    rc, ref, status = bu.direct_batch_smooth(batch)
    assert rc == 0 and status.tolist() == [0, 0, 0] and not any((r == su.SENTINEL).any() or np.isnan(r).any() for r in ref)
    records = batch.history_records(1)
    assert len(records) == 40 and records[20]["frame"] == 21 and records[0]["frame"] == 1
    snap, replay_status = sp.snap_batch(batch, tables=True), batch.status()
    for k in (0, 39):
        restore = bu.tamper_member(batch, 1, 20, k, su.TAMPER_VALUE)
        rc, got, status = bu.direct_batch_smooth(batch)
        assert rc == 0 and status.tolist() == [0, su.EKF_ERR_NUMERIC, 0], (k, rc, status)
        assert got[1].shape == (41, 7) and np.isnan(got[1]).all(), k
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]), k
        wrapped = batch.smooth_history()
        assert batch.last_smooth_status.tolist() == [0, su.EKF_ERR_NUMERIC, 0]
        assert all(sp.same(wrapped[b], got[b], equal_nan=True) for b in range(3))
        assert batch.status() == replay_status == [0, 0, 0] and sp.same(snap, sp.snap_batch(batch, tables=True))
        restore()
        rc, again, status = bu.direct_batch_smooth(batch)
        assert rc == 0 and status.tolist() == [0, 0, 0] and all(np.array_equal(again[b], ref[b]) for b in range(3)), k


# ---- 2. dirty buffers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,blocked", [("ragged", False), ("ragged", True), ("n49_52", False)])
def test_state_pass_on_a_poisoned_workspace(name, blocked):
    """A workspace of exactly ``ekf_smooth_workspace_bytes`` whose every double is a NaN, an output full of the sentinel:
    the bits of the wrapper's run, and no sentinel left.  ragged: resident and forced blocked; n49_52: natural blocked."""
    case = sc.device_case(name)
    b, history, frames = case["flt"].backend, case["history"], case["frames"]
    want = b.smooth_history(history, frames, blocked=blocked).cpu().numpy()
    if blocked or name in su.BLOCKED_SCENES:
        assert np.array_equal(want, case["blocked"])
    rc, got = su.direct_smooth(b, history, frames, blocked, poison=True)
    assert rc == 0 and np.array_equal(got, want) and not (got == su.SENTINEL).any()


@pytest.mark.parametrize("name", ["ragged", sc.GROWING, "n49_52"])
def test_covariance_pass_on_a_poisoned_workspace(name):
    """M, A, Z, T and xinv are reused at a changing npad (g17_3: 64 -> 128 inside the pass) without a memset: a read of
    memory the pass has not written would carry a NaN into the outputs.  Every frame of `smoothed`, `cam_cov` and
    `filt_cam_cov` (NaN on lead rows) and all of `first_cov` are written and have the bits of the wrapper's run."""
    case = sc.device_case(name)
    b = case["flt"].backend
    rc, got = sc.direct_smooth_cov(b, case["history"], case["frames"], case["records"][0]["dims"], poison=True)
    assert rc == 0
    for key in OUT_KEYS:
        assert sp.same(got[key], case["out"][key], equal_nan=True), key
        assert not (got[key] == su.SENTINEL).any(), key
    assert np.isfinite(got["first_cov"]).all() and np.isfinite(got["smoothed"]).all()


@pytest.fixture(scope="module")
def mixed():
    logs = bu.mixed_logs()
    batch = bu.new_batch(4, noise=bu.MIXED_NOISE, motion=True, frame_scale=True)
    filtered, smoothed = batch.smooth_detection_logs(logs)
    assert batch.last_smooth_status.tolist() == [0] * 4
    return logs, batch, filtered, smoothed


def test_batch_pass_on_a_poisoned_workspace(mixed):
    _logs, batch, _filtered, smoothed = mixed
    rc, got, status = bu.direct_batch_smooth(batch, poison=True)
    assert rc == 0 and status.tolist() == [0] * 4
    for b in range(4):
        assert np.array_equal(got[b], smoothed[b]) and not (got[b] == su.SENTINEL).any(), b


def _table(records):
    return [(r["frame"], r["dims"], r["stepped"], r["s_eff"]) for r in records]


def _same_records(a, b):
    return _table(a) == _table(b) and all(np.array_equal(u["u"], v["u"]) and np.array_equal(u["x"], v["x"])
                                          and np.array_equal(u["P"], v["P"]) for u, v in zip(a, b))


def test_a_single_filter_records_into_a_poisoned_history():
    """The history holds 0xFF bytes before the recorded replay of the ragged log: records, table and every smoothed output
    equal those of the ordinary run."""
    case = sc.device_case("ragged")
    log, motion, scale = sc.scene("ragged")
    flt = sc.new_filter(motion=True, frame_scale=True)
    traj, history = sc.recorded_replay(flt, log, motion, scale, poison=True)
    b, frames = flt.backend, case["frames"]
    assert np.array_equal(traj, case["traj"])
    records, info = su.device_records(b, history)
    assert _same_records(records, case["records"]) and _table(records) == su.RAGGED_TABLE
    assert info["frame_record"].tolist() == list(range(14))
    plain = case["flt"].backend
    assert np.array_equal(b.smooth_history(history, frames).cpu().numpy(),
                          plain.smooth_history(case["history"], frames).cpu().numpy())
    assert np.array_equal(b.smooth_history(history, frames, blocked=True).cpu().numpy(), case["blocked"])
    out = b.smooth_history_cov(history, frames)
    for key in OUT_KEYS:
        assert sp.same(out[key].cpu().numpy(), case["out"][key], equal_nan=True), key


def test_a_batch_records_into_a_poisoned_history(mixed):
    """The same for the mixed batch: with 0xFF bytes in it, a flag word the device did not write reads -1 (the member has
    failed), an s_eff word NaN.  Trajectories, records and smoothed rows equal those of the ordinary run."""
    logs, batch, filtered, smoothed = mixed
    twin = bu.new_batch(4, noise=bu.MIXED_NOISE, motion=True, frame_scale=True)
    bu.record_into_poison(twin, batch.last_history.numel())
    filtered2, smoothed2 = twin.smooth_detection_logs(logs)
    assert twin.last_history.numel() == batch.last_history.numel()
    assert twin.last_smooth_status.tolist() == [0] * 4 and twin.status() == batch.status() == [0] * 4
    for b in range(4):
        assert np.array_equal(filtered2[b], filtered[b]) and np.array_equal(smoothed2[b], smoothed[b]), b
        assert _same_records(twin.history_records(b), batch.history_records(b)), b


# ---- 3. records of four and five blocks, behind a wide first frame -------------------------------------------------------------
@pytest.mark.parametrize("name", ["n82", "g81_2"])
def test_four_and_five_blocks_behind_a_wide_frame(name):
    """n82: N = 256 on every record, exactly four blocks, no padding row; g81_2: dims 253, 256, 259, 259, npad 256 -> 320
    inside the pass.  Frame 0 has 82 / 81 detections: the first pack behind the wide update.  The recorded replay is the
    plain one bit for bit (trajectory, state, P, stats), record 0 is the filter after a plain replay of frame 0 alone, and
    the natural blocked state pass and the covariance pass stay under their bounds.  Measured worst error / bound on one
    MI355X (state / cam_cov / first_cov): n82 0.0050 / 0.0018 / 0.0078, g81_2 0.0081 / 0.0015 / 0.0078."""
    case = sc.device_case(name)
    log = sc.scene(name)[0]
    records, frames, b = case["records"], case["frames"], case["flt"].backend
    assert int(np.diff(log["offsets"])[0]) == (82 if name == "n82" else 81) > 64
    assert [r["dims"] for r in records] == ([256] * 4 if name == "n82" else [253, 256, 259, 259])
    twin = sc.new_filter()
    traj, _none = sc.recorded_replay(twin, log, record=False)
    assert np.array_equal(traj, case["traj"])
    assert np.array_equal(twin.backend.get_state(), case["state"]) and np.array_equal(twin.backend.get_cov(), case["P"])
    plain_stats, stats = twin.backend.last_log_stats(), b.last_log_stats()
    assert stats["frames_stepped"] == plain_stats["frames_stepped"] == 4
    assert stats["markers_added"] == plain_stats["markers_added"] == (82 if name == "n82" else 83)
    # (a recorded replay runs in serial order; the plain one of a log without motions runs frames 1 .. 3 pipelined -- measured:
    # 3 and 2 frames in one run -- with the same bits, so these two counters are the only thing that may differ)
    assert stats["frames_pipelined"] == stats["pipelined_runs"] == 0
    d1 = int(log["offsets"][1])
    one = sc.new_filter()
    sc.recorded_replay(one, {"ids": log["ids"][:d1], "poses": log["poses"][:d1], "offsets": log["offsets"][:2]}, record=False)
    assert np.array_equal(records[0]["x"], one.backend.get_state()) and np.array_equal(records[0]["P"], one.backend.get_cov())
    # the passes against the oracle (the covariance pass and its oracle: one per scene, shared with test_smooth_cov.py)
    natural = b.smooth_history(case["history"], frames).cpu().numpy()
    assert np.array_equal(natural, case["blocked"]) and np.array_equal(natural, case["out"]["smoothed"])
    r_state = su.worst_ratio(natural, su.smooth_records(records, frames, INIT), records)
    cam, fb, rec_of = sc.frame_rows(case["ref"], records, frames)
    assert (rec_of >= 0).all()
    err = np.abs(case["out"]["cam_cov"].astype(sc.LD) - cam).astype(np.float64).max(axis=(1, 2))
    r_cam = float((err / fb).max())
    r_first = float(np.abs(case["out"]["first_cov"].astype(sc.LD) - case["ref"]["Ps"][0]).max()) / sc.record_bound(case["ref"], records)[0]
    print(f"{name}: worst error / bound: state {r_state:.4f}, cam_cov {r_cam:.4f}, first_cov {r_first:.4f}")
    assert r_state <= 1.0 and r_cam <= 1.0 and r_first <= 1.0


# ---- 4. the table under a gate ---------------------------------------------------------------------------------------------------
def _shared_rows_repeat(rows, frame_record):
    for t in range(1, len(frame_record)):
        if frame_record[t] == frame_record[t - 1] >= 0:
            assert sp.same(rows[t], rows[t - 1], equal_nan=True), t


def _gate_unstepped(log, rejected):
    """The frames with detections of which none survived."""
    offs = log["offsets"]
    return [t for t in range(len(offs) - 1) if offs[t + 1] > offs[t] and rejected[offs[t]:offs[t + 1]].all()]


@pytest.mark.parametrize("gate", [GATE, GATE_TIGHT])
def test_the_table_under_a_gate_single_filter(gate):
    """The ragged log with its motions and RAGGED_SCALE under a gate.  The expected table comes from the replay's own d^2
    and from the header's rules (``smooth_util.expected_table``): a frame is stepped iff a detection survives, the scales
    of frames that are not stepped fold into the next stepped one, a record exists iff the frame was moved or stepped.  It
    equals ``history_info`` exactly, `u` and `frame_record` included.  Then both tiers and the covariance pass against the
    oracle under the bound, and the frames that share a record repeat its rows.
    Under the scales (Q_eff up to 5 q) the distances are small: at 1e-3 the gate rejects single detections only and every
    frame keeps a survivor (2 detections rejected on the device), so the table is the ungated one.  At 1e-4 the log holds
    what the table rules are about (15 rejected; frames 2 and 9 unstepped and not moved: no record, their scales stay
    pending; frames 11 .. 13 unstepped and moved: records with s_eff = 0), next to stepped frames that lost detections.
    Measured worst error / bound on one MI355X (resident / blocked / cam_cov / first_cov): 1e-3: 0.0448 / 0.0448 /
    0.0110 / 0.0000; 1e-4: 0.4775 / 0.4775 / 0.0001 / 0.0000.  (The 0.48 is rounding of the last place: behind the moved-only
    records at the end of the log the residual is the rounding of the move alone, |c| is about 1e-16, the bound is its
    floor of 4 .. 7 u and the error about 2 u; the plain f64 NumPy run on the CPU oracle's records is at 0.32 there.)"""
    log, motion, scale = su.scene("ragged")
    flt = sc.new_filter(motion=True, frame_scale=True, gate=gate)
    traj, history, d2 = sc.recorded_replay(flt, log, motion, scale, mahal=True)
    b, frames = flt.backend, traj.shape[0]
    rejected = d2 > gate
    rows, motions, frame_record = su.expected_table(log, motion, scale, rejected)
    records, info = su.device_records(b, history)
    print(f"gate {gate:g}: {int(rejected.sum())} rejected, unstepped frames {_gate_unstepped(log, rejected)}, {len(rows)} records")
    assert _table(records) == rows
    assert np.array_equal(info["motion"], motions) and info["frame_record"].tolist() == frame_record.tolist()
    if gate == GATE_TIGHT:
        # the log holds a frame the gate left unstepped that was moved, and one that was not moved (no record at all)
        unstepped = _gate_unstepped(log, rejected)
        assert any(motion[t].any() for t in unstepped) and any(not motion[t].any() for t in unstepped), unstepped
        assert any(frame_record[t] == frame_record[t - 1] for t in unstepped) and rows != su.RAGGED_TABLE
    assert any(r[3] > scale[r[0]] for r in rows if r[2])      # a stepped frame took pending scales with its own
    ref = su.smooth_records(records, frames, INIT)
    ratios = []
    for blocked in (False, True):
        got = b.smooth_history(history, frames, blocked=blocked).cpu().numpy()
        ratios.append(su.worst_ratio(got, ref, records))
        _shared_rows_repeat(got, frame_record)
        assert np.array_equal(got[records[-1]["frame"]:], traj[records[-1]["frame"]:])
    out = {k: v.cpu().numpy() for k, v in b.smooth_history_cov(history, frames).items()}
    cref = sc.smooth_cov_records(records)
    cam, fb, rec_of = sc.frame_rows(cref, records, frames)
    assert (rec_of == frame_record).all() and (rec_of >= 0).all()
    err = np.abs(out["cam_cov"].astype(sc.LD) - cam).astype(np.float64).max(axis=(1, 2))
    ratios.append(float((err / fb).max()))
    ratios.append(float(np.abs(out["first_cov"].astype(sc.LD) - cref["Ps"][0]).max()) / sc.record_bound(cref, records)[0])
    for key in ("smoothed", "cam_cov", "filt_cam_cov"):
        _shared_rows_repeat(out[key], frame_record)
    print(f"gate {gate:g}: worst error / bound: " + "resident {:.4f}, blocked {:.4f}, cam_cov {:.4f}, first_cov {:.4f}".format(*ratios))
    assert max(ratios) <= 1.0


def test_the_table_under_a_gate_batch():
    """Three members over the ragged log that differ in initial pose, q_cam and gate (1e-3, 1e-4, 1e-5: from single
    rejections in frames that keep a survivor to whole frames without one).  The device decides `stepped` and `s_eff` frame
    by frame; the expected tables come from ``rep.rejected[b]`` and the header's rules and equal ``history_records(b)``
    exactly.  Then every member's pass against the oracle under the bound.  Measured worst error / bound on one MI355X:
    0.035, 0.206, 0.233."""
    log = bu.scene_log("ragged")
    gates = np.array([GATE, GATE_TIGHT, 1e-5])
    batch = bu.new_batch(3, motion=True, frame_scale=True, gate=gates, noise={"q_cam": [0.3, 0.1, 0.5]})
    rep = batch.process_detection_logs([log] * 3, mahal=True, record=True)
    smoothed = batch.smooth_history()
    assert batch.status() == [0] * 3 and batch.last_smooth_status.tolist() == [0] * 3
    poses, tables, ratios, moved_only, no_record = bu.initial_poses(3), [], [], 0, 0
    for m in range(3):
        unstepped = _gate_unstepped(log, rep.rejected[m])
        moved_only += sum(bool(log["motion"][t].any()) for t in unstepped)
        no_record += sum(not log["motion"][t].any() for t in unstepped)
        assert np.array_equal(rep.rejected[m], rep.mahal[m] > gates[m])
        rows, motions, frame_record = su.expected_table(log, log["motion"], log["scale"], rep.rejected[m])
        records = batch.history_records(m)
        assert _table(records) == rows, m
        assert np.array_equal(np.array([r["u"] for r in records]).reshape(-1, 6), motions), m
        tables.append(rows)
        ref = bu.member_oracle(records, 14, poses[m], batch.noise[m])
        assert ref["frame_record"].tolist() == frame_record.tolist()
        ratios.append(su.worst_ratio(smoothed[m], ref, records))
        _shared_rows_repeat(smoothed[m], frame_record)
        last = records[-1]["frame"]
        assert np.array_equal(smoothed[m][last:], rep.trajectory[m][last:])
    print("gated batch: worst error / bound per member:", " ".join(f"{r:.4f}" for r in ratios))
    print("records per member:", [len(t) for t in tables], "stepped:", [sum(r[2] for r in t) for t in tables])
    # the batch holds frames the gate left unstepped that were moved (a record with s_eff = 0) and that were not (no record)
    assert moved_only > 0 and no_record > 0 and tables[0] != tables[2] and tables[2] != su.RAGGED_TABLE
    assert max(ratios) <= 1.0


# ---- 5. more members than compute units ------------------------------------------------------------------------------------------
def test_more_members_than_compute_units():
    """300 identical members over the first 6 frames of the tracking scene: further rounds of workgroups.  Every member's
    smoothed rows are member 0's bits, which are the single oracle's under the bound, and the pass's status is all zero."""
    import torch
    members = 300
    log = bu.prefix(bu.scene_log("tracking"), 6)
    batch = bu.new_batch(members, poses=bu.INIT, max_landmarks=10)
    assert members > torch.cuda.get_device_properties(batch.device).multi_processor_count
    filtered, smoothed = batch.smooth_detection_logs([log] * members)
    assert batch.last_smooth_status.tolist() == [0] * members and batch.status() == [0] * members
    first = np.asarray(smoothed[0])
    assert first.shape == (6, 7) and np.isfinite(first).all() and not np.array_equal(first, filtered[0])
    assert all(np.array_equal(smoothed[m], first) and np.array_equal(filtered[m], filtered[0]) for m in range(members))
    records = batch.history_records(members - 1)
    ref = bu.member_oracle(records, 6, bu.INIT, batch.noise[members - 1])
    assert su.worst_ratio(first, ref, records) <= 1.0
