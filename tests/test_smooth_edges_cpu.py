"""The edges of offline smoothing without a GPU (``test_smooth_edges.py`` runs the device against the same helpers): the
room under the bound on the scenes of four and five blocks, the tampered record that must fail the oracle at the step the
device is expected to fail at, the layout arithmetic of the tamper helper against ``ekf_history_record_bytes``, and the
table builder of the gated cases against the hand-pinned table."""
import numpy as np
import pytest

import batch_smooth_util as bu
import smooth_cov_util as sc
import smooth_util as su
from support import lib

BIG = ("n82", "g81_2")
BIG_DIMS = {"n82": [256] * 4, "g81_2": [253, 256, 259, 259]}


@pytest.fixture(scope="module")
def oracle():
    """name -> (records, frames, start) of the CPU oracle filter, computed once per scene."""
    cache = {}

    def get(name):
        if name not in cache:
            log, motion, scale = su.scene(name)
            records, _filtered, start = su.oracle_records(log, motion, scale)
            cache[name] = (records, len(log["offsets"]) - 1, start)
        return cache[name]
    return get


# ---- 3. records of four and five blocks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BIG)
def test_the_big_scenes_have_room_under_the_bound(oracle, name):
    """n82: every record has N = 256, exactly four blocks; g81_2: dims 253, 256, 259, 259, so npad goes 256 -> 320 inside the
    pass and one record is an exact multiple of 64.  kappa(P_p) is about 11.  Plain f64 / bound, measured: state 0.0012 and
    0.0024, covariances in the products form 0.014 and 0.015; asserted at 1/8 like every other fixture."""
    records, frames, start = oracle(name)
    assert [r["dims"] for r in records] == BIG_DIMS[name] and frames == 4
    log = su.scene(name)[0]
    assert int(np.diff(log["offsets"])[0]) == (82 if name == "n82" else 81)      # frame 0 is a wide frame (> 64 detections)
    ref, f64 = su.smooth_records(records, frames, start), su.smooth_records(records, frames, start, np.float64)
    r_state = su.worst_ratio(f64["smoothed"], ref, records)
    cref, c64 = sc.smooth_cov_records(records), sc.smooth_cov_records(records, np.float64, "products")
    r_cov = sc.worst_record_ratio(c64["Ps"], cref, records)
    print(f"{name}: kappa <= {ref['kappa'].max():.1f}, plain f64 / bound: state {r_state:.4f}, covariances {r_cov:.4f}")
    assert ref["kappa"].max() < 100.0
    assert r_state <= 0.125 and r_cov <= 0.125


# ---- 1. the tampered record fails the oracle where the device must fail ------------------------------------------------------
def _tampered(records, r_bad, k):
    bad = [dict(r) for r in records]
    bad[r_bad]["P"] = records[r_bad]["P"].copy()
    bad[r_bad]["P"][k, k] = su.TAMPER_VALUE
    return bad


@pytest.mark.parametrize("name,r_bad,ks", [(n, r, ks) for n, _b, r, ks in su.FAIL_STATE] + list(su.FAIL_COV))
def test_a_tampered_record_fails_the_oracle_at_its_own_step(oracle, monkeypatch, name, r_bad, ks):
    """P[k][k] = -1e3 in record r_bad: ``smooth_records`` and ``smooth_cov_records`` raise LinAlgError, and they raise at
    step r_bad -- the R - 2 - r_bad steps before it factorise (counted), the one of r_bad does not."""
    records, frames, start = oracle(name)
    assert 0 < r_bad < len(records) - 1
    solves, factors = [], []
    plain_solve, plain_factor = su.cholesky_solve, sc.cholesky_factor

    def solve(a, b):
        out = plain_solve(a, b)
        solves.append(a.shape[0])
        return out

    def factor(a):
        out = plain_factor(a)
        factors.append(a.shape[0])
        return out
    monkeypatch.setattr(su, "cholesky_solve", solve)
    monkeypatch.setattr(sc, "cholesky_factor", factor)
    for k in ks:
        assert 0 <= k < records[r_bad]["dims"]
        bad = _tampered(records, r_bad, k)
        del solves[:], factors[:]
        with pytest.raises(np.linalg.LinAlgError):
            su.smooth_records(bad, frames, start, np.float64)
        with pytest.raises(np.linalg.LinAlgError):
            sc.smooth_cov_records(bad, np.float64, "products")
        want = [r["dims"] for r in records[len(records) - 2:r_bad:-1]]      # steps R-2 .. r_bad+1 ran, step r_bad raised
        assert solves == want and factors == want, (k, solves, factors)
    assert records[r_bad]["P"][ks[0], ks[0]] > 0      # (the records themselves are untouched)


# ---- the layout arithmetic of the tamper helper ------------------------------------------------------------------------------
def test_record_offsets_and_diagonal_words_follow_the_header(lib):
    """Record r starts at 256 + sum of ``ekf_history_record_bytes`` of the records before it; the state comes first, then the
    triangle column by column, so P[k][k] is double N + k (2 N - k + 1) / 2: compared with the packing written out."""
    from aruco_slam_amd import hip_backend
    C = hip_backend.C
    n = C.c_size_t()
    for dims in (10, 13, 16, 19, 40, 64, 67, 160, 163, 166, 253, 256, 259):
        assert lib.ekf_history_record_bytes(dims, C.byref(n)) == 0
        assert n.value == su.record_bytes(dims) == bu.record_bytes(dims) and n.value % 256 == 0
        assert n.value >= 8 * (su.diag_word(dims, dims - 1) + 1) > n.value - 256      # the last diagonal word is the last word
    assert [su.record_offset([16, 16, 19], r) for r in range(4)] == [256, 1536, 2816, 4608]
    for dims in (10, 13, 67):
        packed = [("x", i, i) for i in range(dims)] + [("p", i, j) for j in range(dims) for i in range(j, dims)]
        for k in (0, 1, dims // 2, dims - 1):
            assert packed[su.diag_word(dims, k)] == ("p", k, k)
    # the words at the tail of a batch history, counted back from its end, begin where the members' regions end
    members = [[(16, True), (16, False), (19, True)], [(13, True)], []]
    for with_motion in (False, True):
        total = bu.history_bytes(members, with_motion)
        at = bu.tail_offsets(total, 3, 4, with_motion)
        regions = sum(256 + sum(bu.record_bytes(d) for d, has in m if has or with_motion) for m in members)
        assert at["head"] == regions and at["slot"] == regions + 256 and at["flag"] == regions + 512
        assert at["s_eff"] == regions + 768 and at["motion"] == regions + 1024 == total - (256 if with_motion else 0)


# ---- 4. the table builder of the gated cases ---------------------------------------------------------------------------------
def test_the_expected_table_without_rejections_is_the_pinned_one():
    """``expected_table`` with nothing rejected gives RAGGED_TABLE, a record per frame; with every detection of frames 2, 7
    and 9 rejected, frame 7 (moved) keeps a record with s_eff = 0 and its scale folds into frame 8, frames 2 and 9 (exact-zero
    motions) lose theirs and share the record before them."""
    log, motion, scale = su.scene("ragged")
    none = np.zeros(len(log["ids"]), dtype=bool)
    rows, motions, frame_record = su.expected_table(log, motion, scale, none)
    assert rows == su.RAGGED_TABLE and frame_record.tolist() == list(range(14))
    assert np.array_equal(motions, motion)
    rej = none.copy()
    offs = log["offsets"]
    for t in (2, 7, 9):
        rej[offs[t]:offs[t + 1]] = True
    rows, motions, frame_record = su.expected_table(log, motion, scale, rej)
    assert [r[0] for r in rows] == [0, 1, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13]
    assert frame_record.tolist() == [0, 1, 1, 2, 3, 4, 5, 6, 7, 7, 8, 9, 10, 11]
    by_frame = {r[0]: r for r in rows}
    assert by_frame[3] == (3, 28, True, 1.5 + 2.0)                       # frame 2's scale was pending
    assert by_frame[7] == (7, 28, False, 0.0)
    assert by_frame[8] == (8, 34, True, 0.5 + 1.0 + 1.5 + 2.0 + 0.5)     # frames 4 .. 7 pending, then its own
    assert by_frame[11] == (11, 34, True, 1.0 + 1.5 + 2.0)               # frames 9 and 10 pending
    assert np.array_equal(motions, motion[[r[0] for r in rows]])
