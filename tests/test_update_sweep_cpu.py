"""CPU side of the update-kernel sweep (``test_update_sweep.py``): the componentwise checker has teeth, the
extended-precision reference agrees with the pinned oracle, and the sweep's case table reaches every compiled kernel
instance (``update_sweep_util.instances_of``, a restatement of the dispatch with file:line references)."""
import numpy as np
import pytest

from conftest import load_npz
import update_sweep_util as sw

LD = np.longdouble


def _faults(ref, qd):
    """Simulated kernel faults applied to the reference P' (longdouble): name -> faulty P' (f64)."""
    k = ref["k"]
    p1 = ref["P1"].astype(LD) + ref["P1_lo"].astype(LD)
    w = ref["W"].astype(LD)
    pq = p1 + w.T @ w
    n = p1.shape[0]
    out = {}
    f = p1.copy()          # one 32 x 32 tail tile (last tile row, one tile left of the diagonal) left at P+Q, both halves
    r0 = (n - 1) // 32 * 32
    c0 = r0 - 32
    f[r0:r0 + 32, c0:c0 + 32] = pq[r0:r0 + 32, c0:c0 + 32]
    f[c0:c0 + 32, r0:r0 + 32] = pq[c0:c0 + 32, r0:r0 + 32]
    out["tail_tile_not_updated"] = f
    kp = -(-k // 16) * 16
    out["last_16_row_block_of_W_dropped"] = pq - w[:kp - 16].T @ w[:kp - 16]
    f = p1.copy()
    i = np.arange(128, 256)
    f[i, i] -= qd[i]
    out["Q_missing_on_one_128_tile"] = f
    ws = w.copy()
    ws[k // 2] = np.roll(w[k // 2], 1)
    out["one_row_of_W_shifted_by_a_column"] = pq - ws.T @ ws
    w32 = w.astype(np.float32).astype(LD)
    out["downdate_from_W_rounded_to_f32"] = pq - w32.T @ w32
    return {name: v.astype(np.float64) for name, v in out.items()}


@pytest.mark.parametrize("m", [43, 48])
def test_checker_rejects_simulated_kernel_faults(m):
    """Each simulated fault must exceed the f64 bound by >= 100x and the f32 bound by >= 10x (the f32-rounded downdate only
    the f64 one); the unmodified step passes.  Dense prior at n = 125: m = 43 (k = 129, the last 16-row block holds one
    row) and m = 48 (k = 144, the last block is full).

    Measured (ratio / c of the ekf_fused path, f64 | f32): the structural faults sit 1e12-1e14 (f64) and 6e3-6e5 (f32)
    times above their bound units; the f32-rounded downdate 2e6 (f64).

    The existing per-step tolerances (STEP_TOL / ELEM_TOL of test_hip_parity.py) on a bootstrapped SyntheticStream prior
    at the same n and m: the four structural faults give rel_err 1e-3..0.14 and would be rejected by both dtypes' bounds;
    the f32-rounded downdate gives rel_err 3e-8 / rel_err_elem 2e-6..1e-5 -- rejected by the f64 bounds, but accepted by
    the f32 ones (2e-6 / 2e-4), i.e. a one-ulp-of-f32 loss in the f32 path goes unseen there.  What the existing tests
    miss is mostly coverage: they compare most instances with another path, not with the oracle."""
    c64 = sw.C_BOUNDS["ekf_fused"]["float64"][0]
    c32 = sw.C_BOUNDS["ekf_fused"]["float32"][0]
    prior, ref = sw.reference(sw.RefKey("ekf", 125, m, "float64", "as_written"), factors=True)
    assert ref["kappa"] <= sw.KAPPA_MAX
    r_p, r_x = sw.ratios(ref, ref["P1"], ref["x1"], "float64")
    assert r_p < 0.05 and r_x == 0.0           # (the f64 rounding of the reference itself: a few hundredths of the unit)
    qd = sw.oracle_at("ekf", *prior[:3]).process_noise_diag()
    for name, p in _faults(ref, qd).items():
        m64 = sw.ratios(ref, p, ref["x1"], "float64")[0] / c64
        assert m64 >= 100, (name, m64)
        if name != "downdate_from_W_rounded_to_f32":
            m32 = sw.ratios(ref, p, ref["x1"], "float32")[0] / c32
            assert m32 >= 10, (name, m32)


@pytest.mark.parametrize("name,model,tol_p", [("g2_teacher_forced.npz", "ekf", 5e-13), ("g5_rotations.npz", "rot", 3e-11)])
def test_extended_reference_agrees_with_the_oracle(name, model, tol_p):
    """OracleEKF / OracleEKFRotations (mode="fast", f64) and the longdouble step agree componentwise (in units of M_P and
    M_x) on the reference's golden teacher-forced frames (first-sighted markers are added first, as observe does).
    Measured: state 6e-15 (G2) and 4e-15 (G5); P 2.7e-13 (G2) and 1.1e-11 (G5, whose priors come from a real sequence:
    the f64 oracle forms P - (L^-1 P H^T)^T (L^-1 H P) from two solves and is the less accurate side there)."""
    from oracle.ekf_extended import extended_step
    g = load_npz(name)
    worst = np.zeros(2)
    for f in g["frames"]:
        orc = sw.oracle_at(model, g[f"f{f}_state0"], g[f"f{f}_P0"], g[f"f{f}_lm_ids"])
        if model == "rot":
            sl = slice(g["offsets"][f], g["offsets"][f + 1])
            ids, poses = [int(i) for i in g["ids"][sl]], g["poses"][sl]
        else:
            ids, poses = [int(i) for i in g[f"f{f}_ids"]], g[f"f{f}_poses"]
        for i, pose in zip(ids, poses):
            if i not in orc.landmarks:
                orc.add_marker(i, pose)
        ref = extended_step(orc, ids, poses)
        orc.predict()
        orc.update(ids, poses)
        tiny = np.finfo(np.float64).tiny
        ep = np.abs((orc.uncertainty - ref["P1"]) - ref["P1_lo"]) / np.maximum(ref["M_P"], tiny)
        ex = np.abs(orc.state - ref["x1"]) / np.maximum(ref["M_x"], tiny)
        worst = np.maximum(worst, [ep.max(), ex.max()])
    assert worst[0] <= tol_p and worst[1] <= 2e-14, worst


def test_extended_reference_needs_an_extended_long_double():
    assert np.finfo(np.longdouble).nmant >= 63


def test_dense_prior_properties():
    for model, dt in (("ekf", "float64"), ("ekf", "float32"), ("rot", "float64")):
        state, p, lm_ids, ids, poses = sw.dense_prior(model, 20, 8, 3, dt)
        assert np.array_equal(p, p.T)
        if dt == "float32":
            assert np.array_equal(p, p.astype(np.float32).astype(np.float64))
        assert np.linalg.eigvalsh(p).min() > 0
        off = np.abs(p[~np.eye(p.shape[0], dtype=bool)])
        assert np.median(off) > 0.02 and np.unique(off).size > 0.9 * off.size / 2
        assert np.all(np.diag(p) >= 0.05 ** 2 * 0.99) and np.all(np.diag(p) <= 4.0)
    _, ref = sw.reference(sw.RefKey("ekf", 39, 13, "float64", "as_written"))
    assert ref["kappa"] <= sw.KAPPA_MAX


# ---------------------------------------------------------------------------------------------------------------------
# coverage guard
# ---------------------------------------------------------------------------------------------------------------------
def _reached(cases):
    out = set()
    for c in cases:
        out |= sw.instances_of(c)
    return out


def test_launcher_tables_parse():
    """The parse of the launchers finds what the sources hold today (a launcher rewritten beyond recognition fails here)."""
    inst = sw.compiled_instances()
    assert sum(i[0] == "front" for i in inst) == 2 * (12 + 12)      # EKF NB 1..6 (NU 4) + 7..12 (NU 8), Rotations NB 1..12
    assert {i[1] for i in inst if i[0] == "solve"} == set(range(1, 25))
    assert {i[1] for i in inst if i[0] == "cov_tile"} == set(range(1, 25))
    assert {i[1] for i in inst if i[0] == "cov_macro"} == set(range(1, 25))
    assert sw.f64_split_items() == 2048
    assert sw.macro_min_tiles() > 0


def test_sweep_reaches_every_compiled_instance():
    """Every instance the launchers can select, per model (front kernel) and covariance dtype, is run by at least one case
    of the sweep; a new instantiation fails here until the sweep covers it."""
    missing = sw.compiled_instances() - _reached(sw.sweep_cases())
    assert not missing, sorted(missing, key=str)


def test_coverage_guard_notices_a_removed_case():
    """Dropping the cases that reach any one instance leaves a hole the guard reports."""
    cases = sw.sweep_cases()
    for inst in sorted(sw.compiled_instances(), key=str):
        rest = [c for c in cases if inst not in sw.instances_of(c)]
        assert inst in sw.compiled_instances() - _reached(rest), inst


def test_case_table_shapes():
    """The case table hits the shapes the dispatch turns on: f64 both sides of the split / full threshold, blocked wide
    frames in chunks of 384 + 216 rows, the N tails, and every KB of each forced f32 covariance kernel."""
    cases = sw.sweep_cases()
    t = lambda n: -(-(3 * n + 10) // 32)      # noqa: E731
    f64n = {c.n for c in cases if c.group.startswith("f64_")}
    assert {t(n) * (t(n) + 1) // 2 <= sw.f64_split_items() for n in f64n} == {True, False}
    assert any(c.m == 200 and c.group == "ekf_blocked" for c in cases)       # k = 600: chunks of 384 + 216 rows
    assert {3 * n + 10 for n, _ in sw.TAILS} == {13, 64, 127, 193, 256, 385}
    for kern in ("valu", "mfma_tile", "mfma_macro"):
        kbs = {-(-3 * c.m // 16) for c in cases if c.group == f"f32_{kern}"}
        assert kbs == set(range(1, 25)), kern
