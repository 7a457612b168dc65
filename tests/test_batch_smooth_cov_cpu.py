"""Batch smoothed covariances without a GPU: the exported symbols and the header, the Python layer against a fake back end,
the margin the oracle's bound leaves to plain f64 on the members the GPU tests run, the facts those tests lean on (record 0
of ``g17_3`` moves, the smoothed block lies below the filtered one on consistent records), and the compiler's resource
report of the three resident kernels.  ``test_batch_smooth_cov.py`` runs the device against the same helpers."""
import numpy as np
import pytest

import batch_smooth_cov_util as bcu
import batch_smooth_util as bu
import smooth_cov_util as scu
import smooth_util as su
import support as sp
import update_sweep_util as sw
from support import lib

NEW_SYMBOLS = ("ekf_batch_smooth_cov_workspace_bytes", "ekf_batch_smooth_history_cov")


def test_new_symbols_are_declared_exported_and_refuse_a_null_handle(lib):
    from aruco_slam_amd import _build, hip_backend
    sp.assert_abi(lib, NEW_SYMBOLS)
    header = sp.HEADER.read_text()
    assert "ekf_batch_smooth_cov.hip" in _build.SOURCES and "ekf_smooth_resident.h" in _build.HEADERS
    block = header[header.index("Batch smoothing: recorded replays"):]
    assert "Batch smoothing, covariances." in block
    for word in ("first_ld", "NOT written", "EKF_ERR_NUMERIC", "EKF_ERR_INVALID", "bitwise symmetric", "zeroed by the kernel"):
        assert word in block[block.index("Batch smoothing, covariances."):], word
    missing = block[block.index("Not in this interface"):]
    missing = missing[:missing.index("*/")]
    assert "covariances" not in missing
    for word in ("blocked tier", "large maps, wide frames", "smoothed landmark outputs"):
        assert word in missing, word
    C = hip_backend.C
    n = C.c_size_t()
    assert lib.ekf_batch_smooth_cov_workspace_bytes(None, C.byref(n)) == -1
    assert lib.ekf_batch_smooth_history_cov(None, None, 0, None, 0, 0, None, None, None, None, 0, None) == -1


# ---- the Python layer, with a fake back end ---------------------------------------------------------------------------------
def _fake_batch():
    from aruco_slam_amd.batch import EKFBatch
    batch = EKFBatch.__new__(EKFBatch)
    batch.gate = None
    seen = []
    batch.process_detection_logs = lambda logs, **kw: seen.append(("replay", kw)) or "filtered"
    batch.smooth_history = lambda: seen.append("state") or "smoothed"
    batch.smooth_history_cov = lambda: seen.append("cov") or ("smoothed", "smoothed_cov", "filtered_cov")
    return batch, seen


def test_python_layer_cov_is_keyword_only_and_changes_nothing_without_it():
    from aruco_slam_amd.batch import EKFBatch
    assert callable(EKFBatch.smooth_history_cov)
    batch, seen = _fake_batch()
    assert batch.smooth_detection_logs("logs") == ("filtered", "smoothed")
    assert batch.smooth_detection_logs("logs", cov=False) == ("filtered", "smoothed")
    assert batch.smooth_detection_logs("logs", cov=True) == ("filtered", "smoothed", "filtered_cov", "smoothed_cov")
    assert [s for s in seen if isinstance(s, str)] == ["state", "state", "cov"]
    with pytest.raises(TypeError):      # (keyword-only)
        batch.smooth_detection_logs("logs", False, True)
    with pytest.raises(TypeError):
        EKFBatch.smooth_replicas(batch, "log", 0.1, 1, 0, True)
    # gated: the Mahalanobis pair stays the last value
    from types import SimpleNamespace
    batch.process_detection_logs = lambda logs, **kw: SimpleNamespace(trajectory="filtered", mahal="d2", rejected="rej")
    assert batch.smooth_detection_logs("logs", mahal=True) == ("filtered", "smoothed", ("d2", "rej"))
    assert batch.smooth_detection_logs("logs", mahal=True, cov=True) == ("filtered", "smoothed", "filtered_cov", "smoothed_cov",
                                                                         ("d2", "rej"))


def test_batch_bench_has_the_cov_mode():
    text = (sw.REPO / "tools" / "batch_bench.py").read_text()
    assert '"--cov"' in text and "smooth_history_cov" in text


# ---- the oracle: the bound has room, and the facts the GPU tests lean on ------------------------------------------------------
def _margins(records, noise_row):
    ref = bcu.member_cov_oracle(records, noise_row)
    out = []
    for form in ("products", "direct"):
        f64 = bcu.member_cov_oracle(records, noise_row, np.float64, form)
        out.append(scu.worst_record_ratio(f64["Ps"], ref, records))
    return ref, out


@pytest.mark.parametrize("member", [0, 1, 2, 3])
def test_plain_f64_stays_below_an_eighth_of_the_bound_on_the_mixed_members(member):
    """The four members of ``mixed_logs()``: records of the oracle filter, the rule under the member's MIXED_NOISE constants
    (the error of the arithmetic does not ask for records that are consistent with the q of the rule)."""
    log = bu.mixed_logs()[member]
    noise = bcu.oracle_noise_row(bu.MIXED_NOISE["q_cam"][member], su.Q_ERR, bu.MIXED_NOISE["q_lm"][member])
    records, _f, _s = su.oracle_records(log, log.get("motion"), log.get("scale"))
    ref, (products, direct) = _margins(records, noise)
    print(f"mixed member {member}: products {products:.4f}, direct {direct:.4f}, kappa <= {ref['kappa'].max():.0f}")
    assert products <= 0.125 and direct <= 0.125


@pytest.mark.parametrize("name", [scu.GROWING, "n18", "n19"])
def test_plain_f64_stays_below_an_eighth_of_the_bound_on_the_cut_scenes(name):
    log = bcu.scene_log(name)
    records, _f, _s = su.oracle_records(log)
    assert sorted({r["dims"] for r in records}) == bcu.EXPECTED_DIMS[name]
    ref, (products, direct) = _margins(records, bcu.oracle_noise_row())
    print(f"{name}: products {products:.4f}, direct {direct:.4f}, kappa <= {ref['kappa'].max():.0f}")
    assert products <= 0.125 and direct <= 0.125


def test_cut_scenes_keep_their_markers_and_fit_the_batch_frame():
    for name in bcu.CUT_SCENES:
        whole, cut = scu.scene(name)[0], bcu.scene_log(name)
        assert np.array_equal(whole["ids"], cut["ids"]) and np.array_equal(whole["poses"], cut["poses"])
        assert len(cut["offsets"]) == len(whole["offsets"]) + 1 and int(np.diff(cut["offsets"]).max()) == bcu.WIDTH
        assert cut["has_detections"].all()


def test_record_zero_of_the_growing_scene_moves_and_the_smoothed_block_lies_below_the_filtered_one():
    """On the cut ``g17_3`` with the oracle filter's default constants: record 0's smoothed camera block differs from the
    filtered one by at least 5 % of its largest entry (a pass that returned P_r cannot meet the GPU test), and on every
    record filt - smoothed is positive semidefinite within N_r bound_r."""
    records, _f, _s = su.oracle_records(bcu.scene_log(scu.GROWING))
    ref = scu.smooth_cov_records(records)
    bound = scu.record_bound(ref, records)
    p0, s0 = records[0]["P"][:10, :10], ref["Ps"][0][:10, :10].astype(np.float64)
    moved = np.abs(s0 - p0).max() / np.abs(p0).max()
    print(f"record 0: max |P^s - P| / max |P| = {moved:.3f}")
    assert moved >= 0.05
    for r, rec in enumerate(records):
        gap = rec["P"][:10, :10] - ref["Ps"][r][:10, :10].astype(np.float64)
        assert np.linalg.eigvalsh(gap).min() >= -rec["dims"] * bound[r], r
        assert (np.diag(gap)[:3] >= -rec["dims"] * bound[r]).all(), r


# ---- the compiler's resource report -----------------------------------------------------------------------------------------
def test_resident_smooth_kernels_use_no_scratch_and_no_vgpr_spill():
    """The new kernel and the two state kernels that share the pass with it: no scratch memory, no VGPR spill; the static LDS
    of the pass (six vectors of 160 doubles, F and the 10 x 10 block) is the same 8 840 bytes in all three."""
    found = sp.kernel_resources("ekf_batch_smooth_cov.hip", r"ekf_batch_smooth_cov_kernel")
    found.update(sp.kernel_resources("ekf_smooth.hip", r"ekf_smooth_resident_kernel|ekf_batch_smooth_kernel"))
    assert len(found) == 3, found
    for name, res in found.items():
        assert [res[k] for k in sp.BUDGET_FIELDS] == [0, 0, 8840], (name, res)
