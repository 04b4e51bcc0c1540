"""Localization measurements: SLAM against localization on a frozen map (aslam_localize_begin) on the same frames of
the ring world of cfg2_sliding (1280 x 720, about 20 markers per camera): staged batches of 320 frames, aslam_add_image latency and
aslam_add_images latency for 1, 2 and 4 cameras (the MOUNTS of scripts/rig_bench.py).  The localizing contexts start from the world's
true map (world.world) and first pose.

    python scripts/localize_bench.py [--only {staged,add_image,add_images4}] [--out FILE]

Prints one JSON line per measurement (and writes them to --out).  --only runs nothing but that localization measurement (for a
rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

from aruco_slam_amd import capi, synth  # noqa: E402
from rig_bench import MOUNTS, render_steps, world  # noqa: E402

SIG0 = np.diag([1e-4, 1e-4, 1e-5])


def context(w, batch, localize, C=0, max_updates=24):
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=batch, max_landmarks=w.L + 8, max_updates_per_frame=max_updates)
    ctx.set_camera(w.K, np.zeros(5))
    if C:
        ctx.set_camera_rig([(w.K, np.zeros(5), m) for m in MOUNTS[:C]])
    synth.apply_detector(cfg, ctx=ctx)
    if localize:
        ctx.localize_begin(w.ids, w.world, w.pose[0], SIG0)
    return ctx


def staged(localize, n_batches=6, B=320):
    """frames / s of aslam_run_staged in calls of B frames = one lap (each waited for); SLAM builds its map during the first, untimed lap"""
    cfg = synth.CONFIGS["cfg2_sliding"]
    w = synth.RingWorld(synth.SceneConfig(**{**cfg.__dict__, "ring_lap_frames": B}))
    cfg = w.cfg
    ctx = context(w, B, localize)
    frs = [w.frame(i) for i in range(B)]
    for i, fr in enumerate(frs):
        ctx.synth_render(i, cfg.rows, cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=i, download=False)
    ctx.stage_encoders([fr.wl for fr in frs], [fr.wr for fr in frs], [fr.dt for fr in frs])
    ctx.run_staged(0, B, with_ekf=True)
    ctx.sync()
    turn = w.frame(1)                                  # later passes over the same frames: every sample moves the robot
    ctx.stage_encoders([turn.wl], [turn.wr], [turn.dt], slot0=0)
    ctx.profile_reset()
    times = []
    for _ in range(n_batches):
        t0 = time.perf_counter()
        ctx.run_staged(0, B, with_ekf=True)
        ctx.sync()
        times.append(time.perf_counter() - t0)
    st = ctx.get_slot_ekf_stats(0, B)
    return dict(what="run_staged", mode="localize" if localize else "slam", batch=B, frames_per_s=round(B / float(np.median(times)), 1),
                corrections_per_frame=round(float(st[:, 2].mean()), 2), plan=ctx.plan_stats())


def add_image(localize, n=60, reps=3):
    w = world()
    cfg = w.cfg
    ctx = context(w, 1, localize)
    frs = [w.frame(i) for i in range(n)]
    imgs = [ctx.synth_render(0, cfg.rows, cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=i) for i, fr in enumerate(frs)]
    ctx.add_encoder(0.0, 0.0, 0.0)
    t_now, lat = 0.0, []
    for _ in range(reps):
        for i, fr in enumerate(frs):
            t_now += fr.dt
            ctx.add_encoder(fr.wl, fr.wr, t_now)
            t0 = time.perf_counter()
            ctx.add_image(imgs[i])
            lat.append(time.perf_counter() - t0)
    a = np.array(lat[10:]) * 1e6
    return dict(what="add_image", mode="localize" if localize else "slam", calls=len(a), p50_us=round(float(np.percentile(a, 50)), 1),
                p99_us=round(float(np.percentile(a, 99)), 1))


def add_images(localize, C, n_steps=60, reps=3):
    w = world()
    ctx = context(w, C, localize, C=C, max_updates=128 if C > 2 else (64 if C == 2 else 24))
    imgs, enc = render_steps(ctx, w, C, n_steps)
    ctx.add_encoder(0.0, 0.0, 0.0)
    t_now, lat = 0.0, []
    for _ in range(reps):
        for s in range(n_steps):
            t_now += enc[s][2]
            ctx.add_encoder(enc[s][0], enc[s][1], t_now)
            t0 = time.perf_counter()
            ctx.add_images(imgs[s])
            lat.append(time.perf_counter() - t0)
    a = np.array(lat[10:]) * 1e6
    st = ctx.get_rig_step_ekf_stats(0, 1)[0]
    return dict(what="add_images", mode="localize" if localize else "slam", cameras=C, calls=len(a),
                markers_per_step=round(float(np.mean([e[3] for e in enc])), 1), corrections_last_step=int(st[2]),
                p50_us=round(float(np.percentile(a, 50)), 1), p99_us=round(float(np.percentile(a, 99)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["staged", "add_image", "add_images4"], default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    if a.only == "staged":
        res.append(staged(True))
    elif a.only == "add_image":
        res.append(add_image(True))
    elif a.only == "add_images4":
        res.append(add_images(True, 4))
    else:
        for loc in (False, True):
            res.append(staged(loc))
        for loc in (False, True):
            res.append(add_image(loc))
        for C in (1, 2, 4):
            for loc in (False, True):
                res.append(add_images(loc, C))
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
