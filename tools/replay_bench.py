"""Replay throughput: a seeded ragged synthetic log (synthetic.ragged_log: a bootstrap segment that first-sights every
landmark, then steady frames with m ~ U[m_lo, m_hi]) through three entry points, one JSON line each:

    per_frame   BaseFilter.process_detections, one frame at a time (the host round trip per frame)
    log         BaseFilter.process_detection_log, the bootstrap segment in one call, the steady segment in another
    sequence    HipEkf.observe_sequence at a fixed m = the mean m of the log (rectangular block, for reference)

updates/s is steady frames per second of the steady segment; the bootstrap segment is reported separately.

    python tools/replay_bench.py --n 1024 --m 24 40 --steady 2000 --dtype float32     # C3-like
    python tools/replay_bench.py --n 256 --m 8 24 --steady 2000 --dtype float64       # C2-like
    python tools/replay_bench.py --gate 1e300      # every frame through the gate kernel, nothing rejected: the price of
                                                   # the host round trip per frame and of losing the pipelined mode
    python tools/replay_bench.py --row-noise       # every detection with its own row variances (log-uniform in [0.3, 3])
    python tools/replay_bench.py --frame-scale     # every frame with its own process-noise scale (log-uniform in [0.5, 2])
    python tools/replay_bench.py --motion          # every frame with a small camera motion (N(0, 1e-3^2) per component): the
                                                   # price of the motion launch per frame and of losing the pipelined mode
    python tools/replay_bench.py --frozen          # localisation: after the bootstrap the steady segment is replayed on a frozen
                                                   # map (camera-strip update) and, on a second filter of the same build, as
                                                   # mapping frames in serial order: us per frame of both, and the kernel's own
                                                   # time from the covariance update's timing slot
    python tools/replay_bench.py --smooth          # offline smoothing: for n = 10, 50 (resident tier) and 51, 338 (blocked tier)
                                                   # the backward pass in us per record, next to the plain by-frame replay
                                                   # and the recorded replay of the same log on the same build (us per
                                                   # frame); writes profiles/smooth/summary.json
    python tools/replay_bench.py --smooth --cov    # smoothed covariances: at the same four map sizes the covariance pass
                                                   # (HipEkf.smooth_history_cov) and the forced-blocked state pass of the same
                                                   # run, us per record, and the f64 matrix-core rate of the pass's N^3 terms;
                                                   # writes profiles/smooth/cov_summary.json
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

INIT = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0])


def _segment(log, t0, t1):
    offs = log["offsets"]
    d0, d1 = int(offs[t0]), int(offs[t1])
    return log["ids"][d0:d1], log["poses"][d0:d1], offs[t0:t1 + 1] - d0, log["has_detections"][t0:t1]


def _filter(args, **kw):
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    return EKF(INIT, max_landmarks=args.n, max_visible=args.m[1], cov_dtype=args.dtype, gate=args.gate, row_noise=args.row_noise,
               frame_scale=args.frame_scale, motion=args.motion, **kw)


def _frozen_vs_mapping(args, log, boot, frames, seg_noise, emit):
    """--frozen: the steady segment as one log call on a frozen map and, on a second filter, as mapping frames in serial
    order (lookahead=False: what a frozen call runs), each after the same bootstrap and one untimed pass over the first 50
    frames; then 200 frames more with the kernel's own start / stop stamps (timing slot 3)."""
    out = {}
    for name, frozen in (("mapping_serial", False), ("frozen", True)):
        flt = _filter(args, lookahead=False)
        b = flt.backend
        flt.process_detection_log(*_segment(log, 0, boot), **seg_noise(0, boot))
        if frozen:
            flt.freeze_map()
        warm = min(frames, boot + 50)
        flt.process_detection_log(*_segment(log, boot, warm), **seg_noise(boot, warm))
        t = time.perf_counter()
        flt.process_detection_log(*_segment(log, boot, frames), **seg_noise(boot, frames))
        dt = time.perf_counter() - t
        st = b.last_log_stats()
        b.set_kernel_timing(2)
        timed = min(frames, boot + 200)
        flt.process_detection_log(*_segment(log, boot, timed), **seg_noise(boot, timed))
        kern_us, launches = b.kernel_timing()["cov_update"]
        b.set_kernel_timing(0)
        out[name] = {"us_per_frame": 1e6 * dt / (frames - boot), "cov_slot_us": kern_us, "cov_slot_launches": launches,
                     "frames_stepped": st["frames_stepped"], "frames_pipelined": st["frames_pipelined"],
                     "ignored": len(flt.last_ignored)}
        del flt, b
    emit(variant="frozen", frozen_us_per_frame=out["frozen"]["us_per_frame"],
         mapping_serial_us_per_frame=out["mapping_serial"]["us_per_frame"], strip_kernel_us=out["frozen"]["cov_slot_us"],
         cov_update_kernel_us=out["mapping_serial"]["cov_slot_us"], detail=out)


def _smooth_bench(args):
    """--smooth: per map size a mapping log (float64, scalar-first) replayed by frame without and with recording, then the
    backward pass (HipEkf.smooth_history).  The plain by-frame replay is the call with all-zero motions: they enqueue nothing
    and select the serial frame loop the recorded call runs.  One untimed round, then `reps` timed ones on a reset filter;
    median and range."""
    import torch
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    from aruco_slam_amd.synthetic import ragged_log
    rows = []
    for n, tier in ((10, "resident"), (50, "resident"), (51, "blocked"), (338, "blocked")):
        m = (min(4, n), min(12, n))
        log = ragged_log(n, m, args.steady, seed=args.seed)
        frames = len(log["has_detections"])
        zero = np.zeros((frames, 6))
        flt = EKF(INIT, max_landmarks=n, max_visible=m[1], cov_dtype="float64", quat_update="scalar_first", motion=True)
        b = flt.backend
        plan_args = (log["ids"], log["poses"], log["offsets"], log["has_detections"])
        t_plain, t_rec, t_smooth, records = [], [], [], 0
        for rep in range(args.reps + 1):
            flt.reset()
            t = time.perf_counter()
            flt.process_detection_log(*plan_args, motion=zero)
            t_plain.append(time.perf_counter() - t)
            flt.reset()
            from aruco_slam_amd.filters.base_filter import plan_detection_log
            plan = plan_detection_log(flt.landmarks, flt.num_landmarks, log["ids"], log["offsets"], log["has_detections"])
            history = b.new_history(plan.index, plan.offsets)
            traj = torch.empty((frames, 7), dtype=torch.float64, device=b.device)
            torch.cuda.synchronize(b.device)
            t = time.perf_counter()
            b.observe_log(plan.index, plan.offsets, log["poses"], traj, motion=zero, history=history)
            b.sync()
            t_rec.append(time.perf_counter() - t)
            records = len(b.history_info()["frame"])
            t = time.perf_counter()
            b.smooth_history(history, frames)
            t_smooth.append(time.perf_counter() - t)
            del history
        def stat(v, per):
            v = 1e6 * np.array(v[1:]) / per
            return {"median_us": float(np.median(v)), "min_us": float(v.min()), "max_us": float(v.max())}
        row = {"n": n, "dims": 3 * n + 10, "tier": tier, "frames": frames, "records": records, "m_range": list(m),
               "reps": args.reps, "history_bytes_per_record": 8 * ((3 * n + 10) + (3 * n + 10) * (3 * n + 11) // 2),
               "smooth_per_record": stat(t_smooth, records), "plain_by_frame_per_frame": stat(t_plain, frames),
               "recorded_per_frame": stat(t_rec, frames)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del flt, b
    out = Path(__file__).resolve().parent.parent / "profiles" / "smooth"
    out.mkdir(parents=True, exist_ok=True)
    (out / "summary.json").write_text(json.dumps({"steady_frames": args.steady, "rows": rows}, indent=1) + "\n")


def _smooth_cov_bench(args):
    """--smooth --cov: per map size one recorded replay, then per round the forced-blocked state pass and the covariance
    pass over the same history (host clock around calls that end in a synchronisation).  One untimed round, then `reps`
    timed ones; median and range.  flop_per_record counts the N^3 terms of a step at the padded size p (W = L^-1 A: p^3,
    Z = L^-T W: p^3, T = P^s Z: 2 p^3, the lower tiles of -W^T W + Z^T T: 2 p^3 (1 + 64 / p)), the factorisation left out."""
    import torch
    from aruco_slam_amd.filters.base_filter import plan_detection_log
    from aruco_slam_amd.filters.extended_kalman_filter import EKF
    from aruco_slam_amd.synthetic import ragged_log
    rows = []
    for n in (10, 50, 51, 338):
        m = (min(4, n), min(12, n))
        log = ragged_log(n, m, args.steady, seed=args.seed)
        frames = len(log["has_detections"])
        flt = EKF(INIT, max_landmarks=n, max_visible=m[1], cov_dtype="float64", quat_update="scalar_first", motion=True)
        b = flt.backend
        plan = plan_detection_log(flt.landmarks, flt.num_landmarks, log["ids"], log["offsets"], log["has_detections"])
        history = b.new_history(plan.index, plan.offsets)
        traj = torch.empty((frames, 7), dtype=torch.float64, device=b.device)
        b.observe_log(plan.index, plan.offsets, log["poses"], traj, motion=np.zeros((frames, 6)), history=history)
        b.sync()
        records = len(b.history_info()["frame"])
        t_state, t_cov = [], []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize(b.device)
            t = time.perf_counter()
            b.smooth_history(history, frames, blocked=True)
            t_state.append(time.perf_counter() - t)
            t = time.perf_counter()
            b.smooth_history_cov(history, frames)
            t_cov.append(time.perf_counter() - t)
        def stat(v):
            v = 1e6 * np.array(v[1:]) / records
            return {"median_us": float(np.median(v)), "min_us": float(v.min()), "max_us": float(v.max())}
        dims = 3 * n + 10
        pad = -(-dims // 64) * 64
        flop = 4.0 * pad ** 3 + 2.0 * pad ** 3 * (1.0 + 64.0 / pad)
        row = {"n": n, "dims": dims, "padded": pad, "frames": frames, "records": records, "m_range": list(m), "reps": args.reps,
               "cov_per_record": stat(t_cov), "state_blocked_per_record": stat(t_state), "flop_per_record": flop}
        row["cov_pass_gflops"] = flop / (1e3 * row["cov_per_record"]["median_us"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        del flt, b, history
    out = Path(__file__).resolve().parent.parent / "profiles" / "smooth"
    out.mkdir(parents=True, exist_ok=True)
    (out / "cov_summary.json").write_text(json.dumps({"steady_frames": args.steady, "rows": rows}, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--m", type=int, nargs=2, default=(24, 40), metavar=("LO", "HI"))
    ap.add_argument("--steady", type=int, default=2000)
    ap.add_argument("--dtype", default="float32", choices=("float32", "float64"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--variants", default="per_frame,log,sequence")
    ap.add_argument("--gate", type=float, default=None, help="chi-square gate on every detection (default: a filter without)")
    ap.add_argument("--row-noise", action="store_true", help="per-detection measurement noise on every detection (noise=)")
    ap.add_argument("--frame-scale", action="store_true", help="a process-noise scale on every frame (scale=)")
    ap.add_argument("--motion", action="store_true", help="a camera motion on every frame (motion=)")
    ap.add_argument("--frozen", action="store_true",
                    help="replay the steady segment on a frozen map and as mapping frames in serial order, instead of the variants")
    ap.add_argument("--smooth", action="store_true",
                    help="offline smoothing: backward pass per record vs by-frame replay per frame, four map sizes")
    ap.add_argument("--cov", action="store_true",
                    help="with --smooth: the covariance pass next to the forced-blocked state pass, four map sizes")
    ap.add_argument("--reps", type=int, default=5, help="--smooth: timed rounds (after one untimed)")
    args = ap.parse_args()
    if args.cov and not args.smooth:
        ap.error("--cov goes with --smooth")
    if args.smooth:
        (_smooth_cov_bench if args.cov else _smooth_bench)(args)
        return
    import torch
    from aruco_slam_amd.synthetic import SyntheticStream, ragged_log

    log = ragged_log(args.n, args.m, args.steady, seed=args.seed)
    boot = log["bootstrap_frames"]
    frames = len(log["has_detections"])
    m_steady = np.diff(log["offsets"])[boot:]
    noise = None
    if args.row_noise:
        noise = np.exp(np.random.default_rng(args.seed + 7).uniform(np.log(0.3), np.log(3.0), (len(log["ids"]), 3)))

    scale = None
    if args.frame_scale:
        scale = np.exp(np.random.default_rng(args.seed + 9).uniform(np.log(0.5), np.log(2.0), frames))

    motion = None
    if args.motion:
        motion = np.random.default_rng(args.seed + 11).normal(0.0, 1e-3, (frames, 6))

    def seg_noise(t0, t1):
        kw = {} if noise is None else {"noise": noise[int(log["offsets"][t0]):int(log["offsets"][t1])]}
        if scale is not None:
            kw["scale"] = scale[t0:t1]
        if motion is not None:
            kw["motion"] = motion[t0:t1]
        return kw

    common = {"n": args.n, "m_range": list(args.m), "m_mean": float(m_steady.mean()), "dtype": args.dtype, "gate": args.gate,
              "row_noise": bool(args.row_noise), "frame_scale": bool(args.frame_scale), "motion": bool(args.motion),
              "bootstrap_frames": boot, "steady_frames": args.steady}

    def emit(**kv):
        print(json.dumps({**kv, **common}), flush=True)

    if args.frozen:
        _frozen_vs_mapping(args, log, boot, frames, seg_noise, emit)
        return
    rates = {}
    for variant in args.variants.split(","):
        flt = _filter(args)
        b = flt.backend
        if variant == "per_frame":
            offs = log["offsets"]

            def run(t0, t1):
                for t in range(t0, t1):
                    sl = slice(int(offs[t]), int(offs[t + 1]))
                    kw = {} if noise is None else {"noise": noise[sl]}
                    if scale is not None:
                        kw["scale"] = scale[t]
                    if motion is not None:
                        kw["motion"] = motion[t]
                    flt.process_detections(log["ids"][sl], log["poses"][sl], **kw)
            t = time.perf_counter()
            run(0, boot)
            b.sync()
            t_boot = time.perf_counter() - t
            t = time.perf_counter()
            run(boot, frames)
            b.sync()
            t_steady = time.perf_counter() - t
            rates[variant] = args.steady / t_steady
            emit(variant=variant, updates_per_s=rates[variant], steady_s=t_steady, bootstrap_s=t_boot)
        elif variant == "log":
            t = time.perf_counter()
            flt.process_detection_log(*_segment(log, 0, boot), **seg_noise(0, boot))
            t_boot = time.perf_counter() - t
            boot_stats = b.last_log_stats()
            t = time.perf_counter()
            flt.process_detection_log(*_segment(log, boot, frames), **seg_noise(boot, frames))
            t_steady = time.perf_counter() - t
            st = b.last_log_stats()
            rates[variant] = args.steady / t_steady
            extra = {"speedup_vs_per_frame": rates[variant] / rates["per_frame"]} if "per_frame" in rates else {}
            emit(variant=variant, updates_per_s=rates[variant], steady_s=t_steady, bootstrap_s=t_boot,
                 frames_stepped=st["frames_stepped"], frames_pipelined=st["frames_pipelined"],
                 pipelined_runs=st["pipelined_runs"], pipelined_fraction=st["frames_pipelined"] / max(1, st["frames_stepped"]),
                 bootstrap=boot_stats, **extra)
        elif variant == "sequence":
            t = time.perf_counter()
            flt.process_detection_log(*_segment(log, 0, boot))
            t_boot = time.perf_counter() - t
            m = int(round(common["m_mean"]))
            stream = SyntheticStream(args.n, m, seed=args.seed + 1)
            ids, zs = zip(*stream.steady(args.steady))
            idx_t = torch.from_numpy(np.stack(ids).astype(np.int32)).to(b.device)
            z_t = torch.from_numpy(np.stack(zs)[:, :, 0:3].copy()).to(b.device)
            rows_t = None
            if args.row_noise:
                rows_t = torch.from_numpy(np.exp(np.random.default_rng(args.seed + 8).uniform(
                    np.log(0.3), np.log(3.0), tuple(z_t.shape)))).to(b.device)
            torch.cuda.synchronize(b.device)
            t = time.perf_counter()
            b.observe_sequence(idx_t, z_t, rows=rows_t, scale=None if scale is None else scale[boot:boot + args.steady],
                               motion=None if motion is None else motion[boot:boot + args.steady])
            b.sync()
            t_steady = time.perf_counter() - t
            rates[variant] = args.steady / t_steady
            emit(variant=variant, m=m, updates_per_s=rates[variant], steady_s=t_steady, bootstrap_s=t_boot,
                 mode=b.last_sequence_mode())
        else:
            raise SystemExit(f"unknown variant {variant}")
        del flt, b
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
