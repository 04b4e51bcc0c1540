"""Fleet SLAM measurements on the ring world of cfg2_sliding (1280 x 720), R robots at evenly spread lap phases,
one front camera each (w.K), every robot building its own map:
  - tick: aslam_fleet_add_images with all R robots, p50 / p99 latency;
  - singles: the same R robots as R SLAM contexts, one aslam_add_encoder + aslam_add_image each, called one after another
    (p50 / p99 of the whole round);
  - staged: robot-frames / s of aslam_fleet_run_staged over calls of 64 slots (each waited for), every call on the robots' next
    ticks, with the landmarks appended, corrections and "stationary" no-ops per frame it did.

    python scripts/fleet_slam_bench.py [--robots 1,4,16,64] [--only {tick,singles,staged}] [--ticks N] [--out FILE]

Prints one JSON line per measurement (and appends them to --out).  --only with a single --robots value runs nothing else (for a
rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from aruco_slam_amd import capi, synth  # noqa: E402

LAP = 320


def world():
    cfg = synth.CONFIGS["cfg2_sliding"]
    return synth.RingWorld(synth.SceneConfig(**{**cfg.__dict__, "ring_lap_frames": LAP}))


def frames(w, R, ticks):
    """per tick and robot: (Frame, image) rendered once on a scratch context"""
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=1, max_landmarks=w.L + 8)
    out = []
    for t in range(ticks):
        row = []
        for r in range(R):
            fr = w.frame((r * LAP) // R + t)
            row.append((fr, ctx.synth_render(0, cfg.rows, cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=1000 * r + t)))
        out.append(row)
    ctx.close()
    return out


def fleet_context(w, R, batch):
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=batch, max_landmarks=w.L + 8)
    synth.apply_detector(cfg, ctx=ctx)
    ctx.fleet_slam_begin([(w.K, np.zeros(5), (0.0, 0.0, 0.0))] * R)
    return ctx


def pct(ts):
    ts = np.array(ts) * 1e6
    return dict(p50_us=round(float(np.percentile(ts, 50)), 1), p99_us=round(float(np.percentile(ts, 99)), 1))


def tick(w, R, fr, warm=3):
    ctx = fleet_context(w, R, R)
    ts = []
    for t, row in enumerate(fr):
        t0 = time.perf_counter()
        ctx.fleet_add_images(range(R), [im for _, im in row], [f.wl for f, _ in row], [f.wr for f, _ in row], [f.dt for f, _ in row])
        if t >= warm:
            ts.append(time.perf_counter() - t0)
    return dict(what="fleet_slam_tick", robots=R, ticks=len(ts), **pct(ts))


def singles(w, R, fr, warm=3):
    cfg = w.cfg
    cs = []
    for r in range(R):
        c = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=1, max_landmarks=w.L + 8)
        c.set_camera(w.K, np.zeros(5))
        synth.apply_detector(cfg, ctx=c)
        cs.append(c)
    ts, now = [], 0.0
    for t, row in enumerate(fr):
        now += row[0][0].dt
        t0 = time.perf_counter()
        for c, (f, im) in zip(cs, row):
            c.add_encoder(f.wl, f.wr, now)
            c.add_image(im)
        if t >= warm:
            ts.append(time.perf_counter() - t0)
    return dict(what="slam_singles_round", robots=R, ticks=len(ts), **pct(ts))


def staged(w, R, batch=64, reps=5):
    """robot-frames / s of aslam_fleet_run_staged in calls of batch slots (each waited for).  Every call, the untimed first one
    included, gets the next ticks of every robot: the same frames again would make the second pass all "stationary" no-ops"""
    per = max(1, batch // R)
    B = per * R
    ctx = fleet_context(w, R, B)
    fr = frames(w, R, per * (reps + 1))
    robots = [r for _ in range(per) for r in range(R)]
    ts, stats = [], []
    for k in range(reps + 1):
        sel = fr[k * per:(k + 1) * per]
        ctx.stage_frames(np.stack([im for row in sel for _, im in row]))
        ctx.stage_encoders(*[[getattr(f, key) for row in sel for f, _ in row] for key in ("wl", "wr", "dt")])
        t0 = time.perf_counter()
        ctx.fleet_run_staged(0, robots)
        ctx.sync()
        if k:
            ts.append(time.perf_counter() - t0)
            stats.append(ctx.get_slot_ekf_stats(0, B))
    st = np.concatenate(stats)
    return dict(what="fleet_slam_staged", robots=R, slots_per_call=B, robot_frames_per_s=round(B / float(np.median(ts)), 1),
                appended_per_frame=round(float(st[:, 1].mean()), 2), corrections_per_frame=round(float(st[:, 2].mean()), 2), stationary_per_frame=round(float(st[:, 3].mean()), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="1,4,16,64")
    ap.add_argument("--only", choices=["tick", "singles", "staged"])
    ap.add_argument("--ticks", type=int, default=23)
    ap.add_argument("--out")
    a = ap.parse_args()
    w = world()
    for R in [int(x) for x in a.robots.split(",")]:
        fr = frames(w, R, a.ticks) if a.only != "staged" else None
        for name, fn in (("tick", tick), ("singles", singles), ("staged", lambda w, R, _: staged(w, R))):
            if a.only and a.only != name:
                continue
            res = fn(w, R, fr)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
