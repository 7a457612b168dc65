"""Expected values of the per-detection measurement noise (``R = diag(rows)``) from the oracle, and the cases the row-noise
tests share (``test_row_noise_cpu.py`` checks them on the CPU, ``test_row_noise.py`` / ``test_batch_row_noise.py`` run them
on the GPU).  ``oracle/`` knows the constant ``r I`` only, so the two restatements live here:

``extended_step_rows``  ``oracle.ekf_extended.extended_step`` with ``S[diag] += rows`` in place of ``+= r``, built from the
                        oracle's own pieces (``measurement_blocks``, ``process_noise_diag``, ``_inject``, ``cholesky_ld``,
                        ``forward_ld``); with rows all 0.9 it is ``extended_step``, bit for bit.
``block_distances_rows``  ``gating_util.block_distances`` with ``S_d = H_d (P+Q) H_d^T + diag(rows_d)``.

Rows of a case are log-uniform in [lo, hi]: ``exp(U(ln lo, ln hi))`` drawn with ``default_rng(prior_seed(key) + 99)``.
The componentwise bounds of ``update_sweep_util`` are derived from kappa(S) <= 1e3 alone (never from R being a multiple of
the identity), so its constants apply to these cases as they stand; the ranges below keep kappa(S) under that limit."""
from __future__ import annotations

import numpy as np

import gating_util as gu
import update_sweep_util as sw

LD = np.longdouble
RD = {"ekf": 3, "rot": 7}
WIDE = (0.3, 3.0)        # a decade of row variances around the reference's 0.9
NARROW = (0.45, 1.8)     # the frames with more than 380 rows: the wide range takes their kappa(S) past 1e3

# (group, model, n, m, fused, max_visible, (lo, hi)): the smallest m on either side of every dispatch boundary, and m = 1
STEP_CASES = (
    [("ekf_fused", "ekf", 125, m, True, 64, WIDE) for m in (1, 5, 6, 16, 33, 64)]
    + [("ekf_stage", "ekf", 125, m, False, 64, WIDE) for m in (1, 5, 6, 16, 33, 64)]
    + [("ekf_wide", "ekf", 167, 69, True, 128, WIDE), ("ekf_wide", "ekf", 167, 128, True, 128, NARROW),
       ("ekf_blocked", "ekf", 210, 129, True, 200, NARROW)]
    + [("rot_fused", "rot", 63, m, True, 55, WIDE) for m in (1, 2, 9, 27)]
    + [("rot_stage", "rot", 63, m, True, 55, WIDE) for m in (28, 50)]
    + [("rot_wide", "rot", 63, 51, True, 55, WIDE), ("rot_blocked", "rot", 63, 55, True, 55, WIDE)]
)


def case_key(case, dtype):
    _group, model, n, m, _fused, _mv, _rng = case
    return sw.RefKey(model, n, m, dtype, "as_written")


def case_rows(key, lo, hi):
    """The rows [m, RD] of a case: k = RD m values, log-uniform in [lo, hi]."""
    rd = RD[key.model]
    rng = np.random.default_rng(sw.prior_seed(key) + 99)
    return np.exp(rng.uniform(np.log(lo), np.log(hi), rd * key.m)).reshape(key.m, rd)


def extended_step_rows(orc, ids, poses, rows, factors=False):
    """``oracle.ekf_extended.extended_step`` with the measurement noise diag(rows) (rows [m, RD] or [k], > 0): the same
    dict, every product in longdouble, the injection the oracle's own."""
    from oracle.ekf_extended import _split, cholesky_ld, forward_ld
    z, hv, jac, col = orc.measurement_blocks(ids, poses)
    rd, lmd = jac.shape[1], jac.shape[2] - 10
    k = rd * len(ids)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1)
    assert rows.shape == (k,) and (rows > 0).all()
    p = np.asarray(orc.uncertainty, dtype=np.float64)
    qd = orc.process_noise_diag()
    n_dims = p.shape[0]
    pq = p.astype(LD)
    pq[np.arange(n_dims), np.arange(n_dims)] += qd.astype(LD)
    jl = jac.astype(LD)
    a = np.empty((k, n_dims), dtype=LD)
    for j, c0 in enumerate(col):
        r = slice(rd * j, rd * j + rd)
        a[r] = jl[j][:, :10] @ pq[:10] + jl[j][:, 10:] @ pq[c0:c0 + lmd]
    s = np.empty((k, k), dtype=LD)
    for j, c0 in enumerate(col):
        r = slice(rd * j, rd * j + rd)
        s[:, r] = a[:, :10] @ jl[j][:, :10].T + a[:, c0:c0 + lmd] @ jl[j][:, 10:].T
    s = 0.5 * (s + s.T)
    s[np.arange(k), np.arange(k)] += rows.astype(LD)
    lf = cholesky_ld(s)
    w = forward_ld(lf, a)
    y = forward_ld(lf, (z.astype(LD) - hv.astype(LD)))
    delta = w.T @ y
    p1 = pq - w.T @ w
    p1 = 0.5 * (p1 + p1.T)
    wa = np.abs(w).astype(np.float64)
    mp = np.abs(pq).astype(np.float64) + wa.T @ wa
    md = wa.T @ np.abs(y).astype(np.float64)
    x0 = np.asarray(orc.state, dtype=np.float64)
    saved = orc.state
    try:
        orc.state = x0.copy()
        orc._inject(delta.astype(np.float64))
        x1 = np.asarray(orc.state, dtype=np.float64).copy()
    finally:
        orc.state = saved
    mx = np.abs(x0) + md
    quats = [(3, 7)] + ([(10 + 10 * i + 3, 10 + 10 * i + 7) for i in range((n_dims - 10) // 10)] if lmd == 10 else [])
    for q0, _ in quats:
        mx[q0:q0 + 4] = np.abs(x0[q0:q0 + 4]) + md[q0 + 4:q0 + 7].max()
    ev = np.linalg.eigvalsh(s.astype(np.float64))
    hi, lo = _split(p1)
    out = {"P1": hi, "P1_lo": lo, "x1": x1, "M_P": mp, "M_x": mx, "delta": delta.astype(np.float64), "k": k,
           "kappa": float(ev[-1] / ev[0])}
    if factors:
        out.update(S=s.astype(np.float64), A=a.astype(np.float64), L=lf.astype(np.float64), W=w.astype(np.float64))
    return out


def step_reference(case, dtype):
    """(prior, rows [m, RD], extended-precision step with those rows) of a STEP_CASES entry."""
    key = case_key(case, dtype)
    prior = sw.dense_prior(key.model, key.n, key.m, sw.prior_seed(key), key.dtype)
    state, p, lm_ids, ids, poses = prior
    rows = case_rows(key, *case[6])
    return prior, rows, extended_step_rows(sw.oracle_at(key.model, state, p, lm_ids, key.quat), ids, poses, rows)


def step_references(dtypes=sw.DTYPES):
    """step_reference of every case and dtype, on a thread pool (the longdouble products release the GIL)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    todo = [(case, dt) for dt in dtypes for case in STEP_CASES]
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    workers = max(1, min(16, cpus, int(os.environ.get("OMP_NUM_THREADS", cpus))))
    with ThreadPoolExecutor(workers) as pool:
        return dict(zip(todo, pool.map(lambda cd: step_reference(*cd), todo)))


def block_distances_rows(model, orc, ids, poses, rows):
    """d^2 and kappa(S_d) of every detection of a frame on the prior ``orc`` holds (all ids known), with
    S_d = H_d (P+Q) H_d^T + diag(rows_d); ``model`` as in gating_util ("ekf" / "ekf_rotations"), rows [m, RD]."""
    rd, lmd = gu.RD[model], gu.LMD[model]
    rows = np.asarray(rows, dtype=np.float64).reshape(len(ids), rd)
    z, h, jac, col = orc.measurement_blocks(ids, poses)
    r = z - h
    pq = np.array(orc.uncertainty, dtype=np.float64)
    pq[np.arange(pq.shape[0]), np.arange(pq.shape[0])] += orc.process_noise_diag()
    d2, kappa = np.empty(len(ids)), np.empty(len(ids))
    for j, c0 in enumerate(col):
        sl = slice(rd * j, rd * j + rd)
        supp = np.concatenate((np.arange(10), np.arange(c0, c0 + lmd)))
        sd = jac[j] @ pq[np.ix_(supp, supp)] @ jac[j].T + np.diag(rows[j])
        sd = 0.5 * (sd + sd.T)
        ev = np.linalg.eigvalsh(sd)
        d2[j] = float(r[sl] @ np.linalg.solve(sd, r[sl]))
        kappa[j] = float(ev[-1] / ev[0])
    return d2, kappa


def log_rows(model, log, seed, lo=0.3, hi=3.0):
    """Log-uniform rows [D, RD] for every detection of a log (model as in gating_util)."""
    rng = np.random.default_rng(5000 + seed)
    return np.exp(rng.uniform(np.log(lo), np.log(hi), (len(log["ids"]), gu.RD[model])))


def oracle_gated_replay_rows(model, log, rows, gate):
    """``gating_util.oracle_gated_replay`` with per-detection noise: the f64 oracle replays ``log`` with the gate's
    semantics, S_d and the update's R from ``rows`` [D, RD].  Returns (d^2 [D], rejected [D], kappa(S_d) [D]; exempt first
    sightings have d^2 = 0)."""
    orc = gu._new_oracle(model, "scalar_first")
    offs = log["offsets"]
    d2_all, kap_all = np.zeros(len(log["ids"])), np.ones(len(log["ids"]))
    for t in range(len(offs) - 1):
        sl = slice(int(offs[t]), int(offs[t + 1]))
        ids = [int(i) for i in log["ids"][sl]]
        poses = log["poses"][sl]
        if not ids:
            continue
        exempt = np.zeros(len(ids), dtype=bool)
        for j, (k, pose) in enumerate(zip(ids, poses)):
            if k not in orc.landmarks:
                orc.add_marker(k, pose)
                exempt[j] = True
        d2, kappa = block_distances_rows(model, orc, ids, poses, rows[sl])
        d2[exempt] = 0.0
        d2_all[sl], kap_all[sl] = d2, kappa
        keep = ~(d2 > gate)
        if keep.any():
            kept_ids = [k for k, s in zip(ids, keep) if s]
            ref = extended_step_rows(orc, kept_ids, poses[keep], rows[sl][keep])
            p1 = ref["P1"] + ref["P1_lo"]
            orc.state = ref["x1"]
            orc.uncertainty = 0.5 * (p1 + p1.T)
    return d2_all, d2_all > gate, kap_all


def two_sided_frame(model, n=12, m=4, big=100.0, small=0.01):
    """One frame on a dense prior that shows rows reach the gate (model as in gating_util).  Detection 0 carries a large
    row variance and detection 1 a small one; the x residual of each is scaled (bisection on the oracle's distances) so
    that its d^2 under the constant 0.9 and under the rows lie on either side of the gate, at the same ratio to it.  So
    under the constant detection 0 is rejected and 1 kept, under the rows 0 is kept and 1 rejected; the others stay.
    Returns prior (state, P, lm_ids), ids, poses, rows [m, RD], d2_const [m], d2_rows [m]."""
    qm = "rot" if model == "ekf_rotations" else "ekf"
    rd, gate = gu.RD[model], gu.GATES[model]
    state, p, lm_ids, ids, poses = sw.dense_prior(qm, n, m, 4242)
    orc = sw.oracle_at(qm, state, p, lm_ids)
    const = np.full((m, rd), 0.9)
    rows = const.copy()
    rows[0], rows[1] = big, small
    _z, h, _jac, _col = orc.measurement_blocks(ids, poses)
    poses = np.array(poses, dtype=np.float64)

    def product(j, t):
        trial = poses.copy()
        trial[j, 0] = h[rd * j] + t
        a, _ = block_distances_rows(model, orc, ids, trial, const)
        b, _ = block_distances_rows(model, orc, ids, trial, rows)
        return a[j] * b[j]

    for j in (0, 1):
        lo, hi = 0.0, 1.0
        while product(j, hi) < gate * gate:
            lo, hi = hi, 2.0 * hi
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if product(j, mid) < gate * gate else (lo, mid)
        poses[j, 0] = h[rd * j] + hi
    d2_const, _ = block_distances_rows(model, orc, ids, poses, const)
    d2_rows, _ = block_distances_rows(model, orc, ids, poses, rows)
    return {"prior": (state, p, lm_ids), "ids": ids, "poses": poses, "rows": rows, "d2_const": d2_const, "d2_rows": d2_rows}
