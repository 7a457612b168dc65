"""Aggregate throughput of EKFBatch (aruco_slam_amd/batch.py) against one filter's process_detection_log.

Seeded synthetic.ragged_log logs, one seed per member, a bootstrap segment that first-sights every landmark, then 500 steady
frames.  --model ekf (EKF): n = 50 landmarks (DICT_5X5_50), m ~ U[1, 10] per frame.  --model ekf_rotations (EKF_Rotations):
n = 24 (the batch's largest map), m ~ U[1, 8], marker orientations with rvec_sigma = 0.05.  --large-maps: large maps
(EKF_FLAG_BATCH_LARGE_MAPS: the kernel of csrc/ekf_batch_wide.hip, one block per frame) with n = 250 (EKF, m ~ U[1, 10]) or
n = 100 (EKF_Rotations, m ~ U[1, 8]) by default.  --max-visible M: m ~ U[1, M]; above 16 (EKF) / 8 (EKF_Rotations) the batch
takes wide frames (EKF_FLAG_BATCH_WIDE_FRAMES, the same kernel with several blocks per frame) and the single filter takes
max_visible = M.  For every batch size: one warm-up call of the same shape,
then one timed call (host clock around the call, which ends in a synchronise).  The rate is stepped steady frames of all
members over wall time; the bootstrap frames run in the warm-up call, so the timed call is the steady segment alone.
Beside it, the single-filter rate of process_detection_log on member 0's steady segment (same timing rule).  One JSON line
per point, printed and appended to profiles/batch/batch_bench.jsonl (--out).
Kernel times: a separate `rocprofv3 --kernel-trace --stats -- python tools/batch_bench.py --members 256` run (the large-map
ones in profiles/batch/rocprof_large_*.json, the wide-frame ones in profiles/batch/rocprof_wide_*.json).
--replicas: Monte-Carlo replicas of ONE log (member 0's whole log, bootstrap included) with sigma = 0.01 on the tvec, for
B in {16, 64, 256, 1024} by default: the rate of EKFBatch.replay_replicas (noise drawn on the device) against
process_detection_logs on B copies of the log re-noised on the host (numpy draws included in its wall time, and reported
apart).  Same timing rule: one warm-up call, a reset, one timed call.  --nis / --cam-cov ask both paths for the per-frame
outputs.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/batch_bench.py --replicas --members 256
[--nis --cam-cov]` (profiles/batch/rocprof_replicas_*.json).
--replicas --corners [--sigma-px X]: the same ONE-log study with the noise on the marker corners, X pixels (default 0.5):
a synthetic.corner_log scene seen through the calibrated camera of tests/golden/calibration.npz, the rate of
EKFBatch.replay_corner_replicas (corner noise, IPPE and flip labels on the device) beside replay_replicas on the log's clean
poses (sigma = 0.01 on the tvec), and the share of flipped detections.  Lines carry "corners": true.  Kernel times:
`rocprofv3 --kernel-trace --stats -- python tools/batch_bench.py --replicas --corners --members 256`
(profiles/batch/rocprof_corner_replicas_*.json).
--frozen: localisation against mapping on the same build (EKFBatch.freeze_map).  The chosen shape runs twice in one process
on identical logs, from an identical restored map: a mapping bootstrap (the logs' bootstrap segments; with --replicas one
member's), get_state / get_cov, then set_member into two batches, one with every member frozen, the other mapping; each runs
the steady segment once as a warm-up, is restored again and runs it timed.  Lines carry "frozen": true and the frames/s of
both.  Composes with --replicas, --corners, --large-maps, --max-visible, --model and --motion (motions on every frame of both
batches).  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/batch_bench.py --frozen --members 256 ...`
(profiles/batch_frozen/).
--smooth: batch smoothing (EKFBatch.smooth_detection_logs; EKF, scalar_first, n <= 50).  Every member replays its whole
ragged log (bootstrap and --steady frames, default 200 here; every frame is a record) from a reset batch.  One untimed round,
then five timed ones of: the plain replay, the recorded replay (us per frame, aggregate, and the bytes/s the history implies),
and the batched backward pass (EKFBatch.smooth_history: us per record per member, aggregate records/s); median and
min .. max.  Beside them the same work the only way there was before: EKF.smooth_detection_log, one filter after the other,
timed over --single-members of the logs and scaled to the batch size.  Default members: 16 256.  Lines go to
profiles/batch_smooth/batch_bench.jsonl.
--smooth --cov: the same rounds with the smoothed covariances: every round also times EKFBatch.smooth_history_cov over the
same history (the state pass beside it is the first comparison), and the single-filter loop runs
EKF.smooth_detection_log(cov=True) (the second).  The method's wall time includes the copies of its outputs to the host
(200 doubles per frame); "state_call" / "cov_call" time the two library calls alone, on buffers allocated once.  Lines
carry "cov": true; default members 1 16 256.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.float64)


def split(log, t, key="poses"):
    offs = log["offsets"]
    d = int(offs[t])

    def part(t0, t1, d0, d1):
        return {"ids": log["ids"][d0:d1], key: log[key][d0:d1], "offsets": offs[t0:t1 + 1] - d0,
                "has_detections": log["has_detections"][t0:t1]}
    return part(0, t, 0, d), part(t, len(offs) - 1, d, int(offs[-1]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--members", type=int, nargs="*", default=None,
                    help="default: 1 16 64 256 1024 (--replicas: 16 64 256 1024)")
    ap.add_argument("--model", choices=("ekf", "ekf_rotations"), default="ekf")
    ap.add_argument("--landmarks", type=int, default=None,
                    help="default: 50 (ekf), 24 (ekf_rotations); with --large-maps or wide frames 250 (ekf), 100 (ekf_rotations)")
    ap.add_argument("--large-maps", action="store_true", help="run the large-map kernel (EKFBatch(large_maps=True))")
    ap.add_argument("--max-visible", type=int, default=None,
                    help="m ~ U[1, M] (default: 10 for ekf, 8 for ekf_rotations); above 16 / 8 the wide-frame kernel runs")
    ap.add_argument("--steady", type=int, default=500)
    ap.add_argument("--out", default=str(REPO / "profiles" / "batch" / "batch_bench.jsonl"))
    ap.add_argument("--replicas", action="store_true", help="replay_replicas against host-noised process_detection_logs")
    ap.add_argument("--nis", action="store_true", help="--replicas: ask for the per-frame NIS")
    ap.add_argument("--cam-cov", action="store_true", help="--replicas: ask for the per-frame camera covariance")
    ap.add_argument("--corners", action="store_true",
                    help="--replicas: pixel noise on the marker corners (replay_corner_replicas) beside pose noise")
    ap.add_argument("--sigma-px", type=float, default=0.5, help="--corners: the corner noise in pixels")
    ap.add_argument("--gate", type=float, default=None,
                    help="chi-square gate of every member (EKFBatch(gate=X)); 1e300 tests every detection and rejects none. "
                         "With a gate the wall times include the copy of mahal and the host's rejected / dof bookkeeping: "
                         "compare window-kernel times of a rocprofv3 kernel trace, not wall_s")
    ap.add_argument("--row-noise", action="store_true",
                    help="also time the same logs with per-detection noise (EKFBatch(row_noise=True), log-uniform rows in "
                         "[0.3, 3]) and report its frames/s beside the figure without")
    ap.add_argument("--frame-scale", action="store_true",
                    help="also time the same logs with a process-noise scale on every frame (EKFBatch(frame_scale=True), "
                         "log-uniform scales in [0.5, 2]) and report its frames/s beside the figure without")
    ap.add_argument("--motion", action="store_true",
                    help="also time the same logs with a small camera motion on every frame (EKFBatch(motion=True), "
                         "N(0, 1e-3^2) per component) and report its frames/s beside the figure without")
    ap.add_argument("--frozen", action="store_true",
                    help="the shape twice from one restored map: every member frozen (freeze_map) against mapping; "
                         "frames/s of both")
    ap.add_argument("--smooth", action="store_true",
                    help="batch smoothing: recorded against plain replay, the batched backward pass, and the same logs "
                         "through a loop of single filters (EKF.smooth_detection_log)")
    ap.add_argument("--cov", action="store_true",
                    help="--smooth: time the covariance pass (EKFBatch.smooth_history_cov) beside the state pass, and the "
                         "single-filter loop with cov=True")
    ap.add_argument("--single-members", type=int, default=8,
                    help="--smooth: how many members the single-filter loop really runs (its time per member is reported)")
    args = ap.parse_args()
    if args.smooth:
        return smooth(args)
    import torch
    from aruco_slam_amd.batch import EKFBatch
    from aruco_slam_amd.filters.ekf_with_rotations import EKF_Rotations
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    from aruco_slam_amd.synthetic import ragged_log
    if not torch.cuda.is_available():
        raise SystemExit("batch_bench needs a HIP device")
    rot = args.model == "ekf_rotations"
    m_hi = args.max_visible or (8 if rot else 10)
    wide = m_hi > (8 if rot else 16)
    n = args.landmarks or ((100 if rot else 250) if args.large_maps or wide else (24 if rot else 50))
    visible = max(m_hi, 8 if rot else 16)
    if args.corners and not args.replicas:
        raise SystemExit("--corners goes with --replicas")
    if args.frozen:
        return frozen(args, n, m_hi, visible)
    if args.replicas:
        return (corner_replicas if args.corners else replicas)(args, n, m_hi, visible)
    args.members = args.members or [1, 16, 64, 256, 1024]
    logs = [split(lg, lg["bootstrap_frames"]) for lg in
            (ragged_log(n, (1, m_hi), args.steady, seed=s, rvec_sigma=0.05 if rot else 0.0)
             for s in range(max(args.members)))]
    lines = []
    # one filter: bootstrap segment as warm-up, then the steady segment timed
    flt = (EKF_Rotations if rot else EKF)(INIT, max_landmarks=n, max_visible=visible, cov_dtype="float64")
    boot, steady = logs[0]
    flt.process_detection_log(boot["ids"], boot["poses"], boot["offsets"], boot["has_detections"])
    t0 = time.perf_counter()
    flt.process_detection_log(steady["ids"], steady["poses"], steady["offsets"], steady["has_detections"])
    single = args.steady / (time.perf_counter() - t0)
    for B in args.members:
        batch = EKFBatch(B, INIT, max_landmarks=n, max_visible=visible, model=args.model,
                         large_maps=True if args.large_maps else None, **({} if args.gate is None else {"gate": args.gate}))
        batch.process_detection_logs([lg[0] for lg in logs[:B]])           # warm-up: bootstrap frames, same launch shape
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch.process_detection_logs([lg[1] for lg in logs[:B]])
        wall = time.perf_counter() - t0
        assert batch.status() == [0] * B
        rate = B * args.steady / wall
        line = {"tool": "batch_bench", **({"model": args.model} if rot else {}),
                **({"large_maps": True} if args.large_maps else {}),
                **({"wide_frames": True} if batch.wide_frames else {}), "members": B, "n": n, "m": [1, m_hi],
                "steady_frames": args.steady, **({} if args.gate is None else {"gate": args.gate}),
                "wall_s": round(wall, 6), "aggregate_frames_per_s": round(rate, 1),
                "single_filter_frames_per_s": round(single, 1), "ratio": round(rate / single, 2)}
        if args.row_noise:
            rd, rng = (7 if rot else 3), np.random.default_rng(99)
            noisy = [tuple(dict(part, noise=np.exp(rng.uniform(np.log(0.3), np.log(3.0), (len(part["ids"]), rd))))
                           for part in lg) for lg in logs[:B]]
            rows = EKFBatch(B, INIT, max_landmarks=n, max_visible=visible, model=args.model, row_noise=True,
                            large_maps=True if args.large_maps else None, **({} if args.gate is None else {"gate": args.gate}))
            rows.process_detection_logs([lg[0] for lg in noisy])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows.process_detection_logs([lg[1] for lg in noisy])
            wall_rows = time.perf_counter() - t0
            assert rows.status() == [0] * B
            line["row_noise_wall_s"] = round(wall_rows, 6)
            line["row_noise_frames_per_s"] = round(B * args.steady / wall_rows, 1)
            del rows
        if args.frame_scale:
            rng = np.random.default_rng(98)
            timed = [tuple(dict(part, scale=np.exp(rng.uniform(np.log(0.5), np.log(2.0), len(part["offsets"]) - 1)))
                           for part in lg) for lg in logs[:B]]
            scaled = EKFBatch(B, INIT, max_landmarks=n, max_visible=visible, model=args.model, frame_scale=True,
                              large_maps=True if args.large_maps else None, **({} if args.gate is None else {"gate": args.gate}))
            scaled.process_detection_logs([lg[0] for lg in timed])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scaled.process_detection_logs([lg[1] for lg in timed])
            wall_scaled = time.perf_counter() - t0
            assert scaled.status() == [0] * B
            line["frame_scale_wall_s"] = round(wall_scaled, 6)
            line["frame_scale_frames_per_s"] = round(B * args.steady / wall_scaled, 1)
            del scaled
        if args.motion:
            rng = np.random.default_rng(99)
            timed = [tuple(dict(part, motion=rng.normal(0.0, 1e-3, (len(part["offsets"]) - 1, 6))) for part in lg)
                     for lg in logs[:B]]
            moved = EKFBatch(B, INIT, max_landmarks=n, max_visible=visible, model=args.model, motion=True,
                             large_maps=True if args.large_maps else None, **({} if args.gate is None else {"gate": args.gate}))
            moved.process_detection_logs([lg[0] for lg in timed])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            moved.process_detection_logs([lg[1] for lg in timed])
            wall_moved = time.perf_counter() - t0
            assert moved.status() == [0] * B
            line["motion_wall_s"] = round(wall_moved, 6)
            line["motion_frames_per_s"] = round(B * args.steady / wall_moved, 1)
            del moved
        if args.large_maps or batch.wide_frames:     # every stepped frame reads and writes the member's N x N f64 covariance
            # once (wide frames: once per block)
            dims = (10 if rot else 3) * n + 10
            sweeps = 1.0
            if batch.wide_frames:       # one read-modify-write of P per block of 16 / 8 detections
                m = np.diff(np.concatenate([lg[1]["offsets"] for lg in logs[:1]]))
                sweeps = float(np.ceil(m[m > 0] / (8 if rot else 16)).mean())
                line["p_sweeps_per_frame"] = round(sweeps, 3)
            line["p_stream_tb_per_s"] = round(rate * 2 * dims * dims * 8 * sweeps / 1e12, 3)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del batch
    append(args.out, lines)


def append(path, lines):
    out = Path(path)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


def frozen(args, n, m_hi, visible):
    """--frozen: see the module docstring."""
    import torch
    from aruco_slam_amd.batch import EKFBatch
    from aruco_slam_amd.synthetic import corner_log, ragged_log
    rot = args.model == "ekf_rotations"
    rvs = 0.05 if rot else 0.0
    sigma = np.array([0.01, 0.01, 0.01, 0.0, 0.0, 0.0])
    key = "corners" if args.corners else "poses"
    if args.corners:
        cal = np.load(REPO / "tests" / "golden" / "calibration.npz", allow_pickle=False)
        cam = (cal["camera_matrix"], cal["dist_coeffs"].reshape(-1))
    members = args.members or ([16, 64, 256, 1024] if args.replicas else [1, 16, 64, 256, 1024])
    if args.corners:
        one = corner_log(n, (1, m_hi), args.steady, 0, *cam)
        boot_src = split(dict(one, poses=one["poses_clean"] + 0.0), one["bootstrap_frames"])[0]
        logs = [(boot_src, split(one, one["bootstrap_frames"], "corners")[1])]
    else:
        count = 1 if args.replicas else max(members)
        logs = [split(lg, lg["bootstrap_frames"]) for lg in (ragged_log(n, (1, m_hi), args.steady, seed=s, rvec_sigma=rvs)
                                                             for s in range(count))]
    if args.motion:
        rng = np.random.default_rng(99)
        logs = [tuple(dict(part, motion=rng.normal(0.0, 1e-3, (len(part["offsets"]) - 1, 6))) for part in lg) for lg in logs]
    kw = dict(max_landmarks=n, max_visible=visible, model=args.model, large_maps=True if args.large_maps else None,
              motion=args.motion and not args.replicas, **({} if args.gate is None else {"gate": args.gate}))
    lines = []
    for B in members:
        # the mapping bootstrap, once: every member's map (--replicas: one map for all)
        boot = EKFBatch(len(logs[:B]), INIT, **kw)
        boot.process_detection_logs([lg[0] for lg in logs[:B]])
        assert boot.status() == [0] * boot.members
        maps = [(boot.get_state(b), boot.get_cov(b),
                 [k for k, _ in sorted(boot.landmarks[b].items(), key=lambda kv: kv[1])]) for b in range(boot.members)]
        del boot

        def restore(batch):
            for b in range(B):
                batch.set_member(b, *maps[b % len(maps)])

        def run(batch, seed):
            if args.corners:
                batch.replay_corner_replicas(logs[0][1], args.sigma_px, seed)
            elif args.replicas:
                batch.replay_replicas({k: v for k, v in logs[0][1].items() if k != "motion"}, sigma, seed)
            else:
                batch.process_detection_logs([lg[1] for lg in logs[:B]])

        rates, stopped = {}, {}
        for name in ("mapping", "frozen"):
            batch = EKFBatch(B, INIT, **kw)
            if args.corners:
                batch.set_camera(*cam)
            restore(batch)
            if name == "frozen":
                batch.freeze_map()
            run(batch, 1)          # warm-up
            restore(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(batch, 2)
            wall = time.perf_counter() - t0
            stopped[name] = sum(1 for v in batch.status() if v != 0)
            assert args.corners or stopped[name] == 0      # (a flipped pose can stop a member of a corner study)
            assert batch.map_frozen.all() == (name == "frozen")
            rates[name] = (wall, B * args.steady / wall)
            del batch
        line = {"tool": "batch_bench", "frozen": True, **({"model": args.model} if rot else {}),
                **({"replicas": True} if args.replicas else {}), **({"corners": True, "sigma_px": args.sigma_px} if args.corners else {}),
                **({"large_maps": True} if args.large_maps else {}), **({"motion": True} if kw["motion"] else {}),
                **({"wide_frames": True} if m_hi > (8 if rot else 16) else {}),
                "members": B, "n": n, "m": [1, m_hi], "steady_frames": args.steady,
                **({} if args.gate is None else {"gate": args.gate}),
                **({"members_stopped": stopped} if args.corners else {}),
                "mapping_wall_s": round(rates["mapping"][0], 6), "mapping_frames_per_s": round(rates["mapping"][1], 1),
                "frozen_wall_s": round(rates["frozen"][0], 6), "frozen_frames_per_s": round(rates["frozen"][1], 1),
                "frozen_over_mapping": round(rates["frozen"][1] / rates["mapping"][1], 3)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    append(args.out, lines)


def _smooth_calls(batch, torch):
    """(state, cov): closures that run ekf_batch_smooth_history / ekf_batch_smooth_history_cov on the batch's last history
    with buffers allocated here, once -- the library call alone (it waits for the stream), without the copies to the host."""
    import ctypes as C
    from aruco_slam_amd.batch import _iptr
    need, need_cov = C.c_size_t(), C.c_size_t()
    batch._check(batch.lib.ekf_batch_smooth_workspace_bytes(batch.h, C.byref(need)))
    batch._check(batch.lib.ekf_batch_smooth_cov_workspace_bytes(batch.h, C.byref(need_cov)))
    frames, hist = int(batch._history_frames[-1]), batch.last_history
    dev = batch.device
    ws = torch.empty((max(need_cov.value, need.value, 256),), dtype=torch.uint8, device=dev)
    rows = torch.empty((frames, 7), dtype=torch.float64, device=dev)
    cam, filt = (torch.empty((frames, 10, 10), dtype=torch.float64, device=dev) for _ in range(2))
    status = np.zeros(batch.members, dtype=np.int32)
    torch.cuda.synchronize()

    def state():
        batch._check(batch.lib.ekf_batch_smooth_history(batch.h, hist.data_ptr(), hist.numel(), ws.data_ptr(), need.value,
                                                        rows.data_ptr(), _iptr(status)))

    def cov():
        batch._check(batch.lib.ekf_batch_smooth_history_cov(batch.h, hist.data_ptr(), hist.numel(), ws.data_ptr(),
                                                            need_cov.value, 0, rows.data_ptr(), cam.data_ptr(),
                                                            filt.data_ptr(), None, 0, _iptr(status)))
    return state, cov


def smooth(args):
    """--smooth: see the module docstring."""
    import torch
    from aruco_slam_amd.batch import EKFBatch
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    from aruco_slam_amd.synthetic import ragged_log
    if not torch.cuda.is_available():
        raise SystemExit("batch_bench needs a HIP device")
    n = args.landmarks or 50
    m_hi = args.max_visible or 10
    if n > 50 or m_hi > 16 or args.model != "ekf":
        raise SystemExit("--smooth: EKF, at most 50 landmarks and 16 detections per frame (the resident tier)")
    steady = args.steady if args.steady != 500 else 200
    members = args.members or ([1, 16, 256] if args.cov else [16, 256])
    logs = []
    for s in range(max(members)):
        lg = ragged_log(n, (1, m_hi), steady, seed=s)
        logs.append({k: lg[k] for k in ("ids", "poses", "offsets", "has_detections")})
    kw = dict(max_landmarks=n, max_visible=16, quat_update="scalar_first")
    median = lambda v: float(np.median(v))
    lines = []
    # the loop of single filters: what smoothing many logs costs without the batch
    single = []
    for lg in logs[:max(1, args.single_members) + 1]:      # (the first one is the warm-up)
        flt = EKF(INIT, max_landmarks=n, max_visible=16, cov_dtype="float64", quat_update="scalar_first")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flt.smooth_detection_log(lg["ids"], lg["poses"], lg["offsets"], lg["has_detections"], **({"cov": True} if args.cov else {}))
        single.append(time.perf_counter() - t0)
        del flt
    single = single[1:] or single
    for B in members:
        frames = sum(len(lg["offsets"]) - 1 for lg in logs[:B])
        walls = {"plain": [], "recorded": [], "pass": [],
                 **({"cov_pass": [], "state_call": [], "cov_call": []} if args.cov else {})}
        batch = EKFBatch(B, INIT, **kw)
        for rnd in range(6):      # one untimed round, five timed
            for name in ("plain", "recorded"):
                batch.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batch.process_detection_logs(logs[:B], record=name == "recorded")
                walls[name].append(time.perf_counter() - t0)
            assert batch.status() == [0] * B
            t0 = time.perf_counter()
            batch.smooth_history()
            walls["pass"].append(time.perf_counter() - t0)
            assert not batch.last_smooth_status.any()
            if args.cov:
                t0 = time.perf_counter()
                batch.smooth_history_cov()
                walls["cov_pass"].append(time.perf_counter() - t0)
                assert not batch.last_smooth_status.any()
                for name, call in zip(("state_call", "cov_call"), _smooth_calls(batch, torch)):
                    t0 = time.perf_counter()
                    call()
                    walls[name].append(time.perf_counter() - t0)
        records = [len(batch.history_records(b)) for b in range(min(B, 4))]
        per_member = float(np.mean(records))      # (every frame of these logs is a record)
        hist_bytes = int(batch.last_history.numel())
        stat = {k: (median(v[1:]), min(v[1:]), max(v[1:])) for k, v in walls.items()}
        line = {"tool": "batch_bench", "smooth": True, "members": B, "n": n, "m": [1, m_hi], "frames_per_member": frames / B,
                "records_per_member": per_member, "rounds": 5, "history_bytes": hist_bytes,
                "plain_us_per_frame": round(1e6 * stat["plain"][0] / frames, 3),
                "recorded_us_per_frame": round(1e6 * stat["recorded"][0] / frames, 3),
                "plain_wall_s": [round(x, 6) for x in stat["plain"]], "recorded_wall_s": [round(x, 6) for x in stat["recorded"]],
                "recording_bytes_per_s": round(hist_bytes / max(stat["recorded"][0], 1e-12), 1),
                "pass_wall_s": [round(x, 6) for x in stat["pass"]],
                "pass_us_per_record_per_member": round(1e6 * stat["pass"][0] / per_member, 3),
                "pass_records_per_s": round(B * per_member / stat["pass"][0], 1),
                "single_loop_members_timed": len(single), "single_smooth_s_per_member": round(median(single), 6),
                "single_loop_s_for_these_members": round(median(single) * B, 4),
                "batch_smooth_s": round(stat["recorded"][0] + stat["pass"][0], 6),
                "speedup_over_single_loop": round(median(single) * B / (stat["recorded"][0] + stat["pass"][0]), 2)}
        if args.cov:
            cov = stat["cov_pass"]
            line.update({"cov": True, "cov_pass_wall_s": [round(x, 6) for x in cov],
                         "cov_pass_us_per_record_per_member": round(1e6 * cov[0] / per_member, 3),
                         "cov_pass_over_state_pass": round(cov[0] / stat["pass"][0], 3),
                         "state_call_wall_s": [round(x, 6) for x in stat["state_call"]],
                         "cov_call_wall_s": [round(x, 6) for x in stat["cov_call"]],
                         "state_call_us_per_record_per_member": round(1e6 * stat["state_call"][0] / per_member, 3),
                         "cov_call_us_per_record_per_member": round(1e6 * stat["cov_call"][0] / per_member, 3),
                         "cov_call_over_state_call": round(stat["cov_call"][0] / stat["state_call"][0], 3),
                         "batch_smooth_s": round(stat["recorded"][0] + cov[0], 6),
                         "speedup_over_single_loop": round(median(single) * B / (stat["recorded"][0] + cov[0]), 2)})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del batch
    out = args.out if args.out != str(REPO / "profiles" / "batch" / "batch_bench.jsonl") else \
        str(REPO / "profiles" / "batch_smooth" / "batch_bench.jsonl")
    append(out, lines)


def replicas(args, n, m_hi, visible):
    import torch
    from aruco_slam_amd.batch import EKFBatch
    from aruco_slam_amd.synthetic import ragged_log
    rot = args.model == "ekf_rotations"
    log = ragged_log(n, (1, m_hi), args.steady, seed=0, rvec_sigma=0.05 if rot else 0.0)
    log = {k: log[k] for k in ("ids", "poses", "offsets", "has_detections")}
    frames, dets = len(log["offsets"]) - 1, int(log["offsets"][-1])
    sigma = np.array([0.01, 0.01, 0.01, 0.0, 0.0, 0.0])
    outs = {"nis": args.nis, "cam_cov": args.cam_cov}
    rng = np.random.default_rng(1)
    lines = []
    for B in args.members or [16, 64, 256, 1024]:
        batch = EKFBatch(B, INIT, max_landmarks=n, max_visible=visible, model=args.model,
                         large_maps=True if args.large_maps else None, **({} if args.gate is None else {"gate": args.gate}))

        def host_logs():
            return [dict(log, poses=log["poses"] + sigma * rng.standard_normal(log["poses"].shape)) for _ in range(B)]

        batch.replay_replicas(log, sigma, 1, **outs)          # warm-up
        batch.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch.replay_replicas(log, sigma, 2, **outs)
        wall_rep = time.perf_counter() - t0
        assert batch.status() == [0] * B
        batch.reset()
        kw = outs if args.nis or args.cam_cov else {}
        batch.process_detection_logs(host_logs(), **kw)      # warm-up
        batch.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        noisy = host_logs()
        t1 = time.perf_counter()
        batch.process_detection_logs(noisy, **kw)
        wall_host = time.perf_counter() - t0
        assert batch.status() == [0] * B
        line = {"tool": "batch_bench", "replicas": True, **({"model": args.model} if rot else {}),
                **({"large_maps": True} if args.large_maps else {}),
                **({"wide_frames": True} if batch.wide_frames else {}), "members": B, "n": n, "m": [1, m_hi],
                "frames": frames, "detections": dets, "nis": args.nis, "cam_cov": args.cam_cov,
                **({} if args.gate is None else {"gate": args.gate}),
                "replay_replicas_wall_s": round(wall_rep, 6),
                "replay_replicas_frames_per_s": round(B * frames / wall_rep, 1),
                "host_noised_wall_s": round(wall_host, 6), "host_noise_draw_s": round(t1 - t0, 6),
                "host_noised_frames_per_s": round(B * frames / wall_host, 1),
                "speedup": round(wall_host / wall_rep, 2)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del batch
    append(args.out, lines)


def corner_replicas(args, n, m_hi, visible):
    import torch
    from aruco_slam_amd.batch import EKFBatch
    from aruco_slam_amd.synthetic import corner_log
    rot = args.model == "ekf_rotations"
    cal = np.load(REPO / "tests" / "golden" / "calibration.npz", allow_pickle=False)
    k, dist = cal["camera_matrix"], cal["dist_coeffs"].reshape(-1)
    full = corner_log(n, (1, m_hi), args.steady, 0, k, dist)
    log = {key: full[key] for key in ("ids", "corners", "offsets", "has_detections")}
    pose_log = {"ids": full["ids"], "poses": full["poses_clean"] + 0.0, "offsets": full["offsets"],
                "has_detections": full["has_detections"]}
    frames, dets = len(log["offsets"]) - 1, int(log["offsets"][-1])
    sigma = np.array([0.01, 0.01, 0.01, 0.0, 0.0, 0.0])
    outs = {"nis": args.nis, "cam_cov": args.cam_cov}
    lines = []
    for B in args.members or [16, 64, 256, 1024]:
        batch = EKFBatch(B, INIT, max_landmarks=n, max_visible=visible, model=args.model,
                         large_maps=True if args.large_maps else None, **({} if args.gate is None else {"gate": args.gate}))
        batch.set_camera(k, dist)
        batch.replay_corner_replicas(log, args.sigma_px, 1, **outs)          # warm-up
        batch.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = batch.replay_corner_replicas(log, args.sigma_px, 2, **outs)
        wall_corner = time.perf_counter() - t0
        stopped = sum(1 for v in batch.status() if v != 0)      # (a flipped pose can stop an EKF_Rotations member)
        batch.reset()
        batch.replay_replicas(pose_log, sigma, 1, **outs)          # warm-up
        batch.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch.replay_replicas(pose_log, sigma, 2, **outs)
        wall_pose = time.perf_counter() - t0
        line = {"tool": "batch_bench", "replicas": True, "corners": True, **({"model": args.model} if rot else {}),
                **({"large_maps": True} if args.large_maps else {}),
                **({"wide_frames": True} if batch.wide_frames else {}), "members": B, "n": n, "m": [1, m_hi],
                "frames": frames, "detections": dets, "nis": args.nis, "cam_cov": args.cam_cov,
                **({} if args.gate is None else {"gate": args.gate}), "sigma_px": args.sigma_px,
                "flipped_share": round(float(got.flipped.mean()), 5), "members_stopped": stopped,
                "replay_corner_replicas_wall_s": round(wall_corner, 6),
                "replay_corner_replicas_frames_per_s": round(B * frames / wall_corner, 1),
                "replay_replicas_wall_s": round(wall_pose, 6),
                "replay_replicas_frames_per_s": round(B * frames / wall_pose, 1)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del batch
    append(args.out, lines)


if __name__ == "__main__":
    main()
