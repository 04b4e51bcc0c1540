"""Camera-rig measurements: latency of aslam_add_images for C = 1, 2, 4 cameras beside aslam_add_image on the same
frames, and the throughput of aslam_run_staged_rig, on the ring world of cfg2_sliding (1280 x 720, about 20 markers per camera).

    python scripts/rig_bench.py [--latency-only C] [--steps N] [--out FILE]

Prints one JSON line per measurement (and writes them to --out).  --latency-only C runs nothing but C-camera add_images calls
(for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from aruco_slam_amd import capi, synth  # noqa: E402

MOUNTS = [(0.20, 0.0, 0.0), (-0.22, 0.0, math.pi), (0.0, 0.15, math.pi / 2), (0.0, -0.15, -math.pi / 2)]


def world():
    return synth.RingWorld(synth.CONFIGS["cfg2_sliding"])


def render_steps(ctx, w, C, n_steps, slot0=0):
    """host images of n_steps rig steps (rendered in slot slot0 + c) and the steps' encoder samples"""
    cfg = w.cfg
    imgs, enc = [], []
    for s in range(n_steps):
        frs = w.rig_frame(s, MOUNTS[:C])
        imgs.append([ctx.synth_render(slot0 + c, cfg.rows, cfg.cols, w.K, f.ids, f.poses, noise_amp=2, seed=s * C + c) for c, f in enumerate(frs)])
        enc.append((frs[0].wl, frs[0].wr, frs[0].dt, sum(len(f.ids) for f in frs)))
    return imgs, enc


def latency(C, n_steps, reps, single=False):
    """p50 / p99 of aslam_add_images (or of aslam_add_image on camera 0's frames) over reps passes of n_steps steps"""
    w = world()
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=C, max_landmarks=w.L + 8,
                       max_updates_per_frame=128 if C > 2 else (64 if C == 2 else 24))
    if single:
        ctx.set_camera(w.K, np.zeros(5))
    ctx.set_camera_rig([(w.K, np.zeros(5), m) for m in MOUNTS[:C]])
    imgs, enc = render_steps(ctx, w, C, n_steps)
    ctx.add_encoder(0.0, 0.0, 0.0)
    t_now, lat, parts = 0.0, [], []
    for _ in range(reps):
        for s in range(n_steps):
            t_now += enc[s][2]
            ctx.add_encoder(enc[s][0], enc[s][1], t_now)
            t0 = time.perf_counter()
            if single:
                ctx.add_image(imgs[s][0])
            else:
                ctx.add_images(imgs[s])
            lat.append(time.perf_counter() - t0)
            parts.append(ctx.last_timing())
    a = np.array(lat[10:]) * 1e6
    ph = {k: round(float(np.percentile([p[k] for p in parts[10:]], 50)), 1) for k in parts[0]}
    return dict(what="add_image" if single else "add_images", cameras=1 if single else C, calls=len(a),
                markers_per_step=round(float(np.mean([e[3] for e in enc])), 1) if not single else None,
                p50_us=round(float(np.percentile(a, 50)), 1), p99_us=round(float(np.percentile(a, 99)), 1), phases_p50_us=ph)


def throughput(C, n_steps, batch_frames):
    """steps / s and frames / s of aslam_run_staged_rig in calls of batch_frames // C steps, each call waited for"""
    w = world()
    cfg = w.cfg
    spc = batch_frames // C
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=spc * C, max_landmarks=w.L + 8,
                       max_updates_per_frame=128 if C > 2 else (64 if C == 2 else 24))
    ctx.set_camera_rig([(w.K, np.zeros(5), m) for m in MOUNTS[:C]])
    total, done, markers = 0.0, 0, 0
    ctx.profile_reset()
    for s0 in range(0, n_steps, spc):
        nb = min(spc, n_steps - s0)
        encs = []
        for s in range(nb):
            frs = w.rig_frame(s0 + s, MOUNTS[:C])
            for c, f in enumerate(frs):
                ctx.synth_render(s * C + c, cfg.rows, cfg.cols, w.K, f.ids, f.poses, noise_amp=2, seed=(s0 + s) * C + c, download=False)
                encs.append((f.wl, f.wr, f.dt))
                markers += len(f.ids)
        e = np.array(encs)
        ctx.stage_encoders(e[:, 0], e[:, 1], e[:, 2])
        ctx.sync()
        t0 = time.perf_counter()
        ctx.run_staged_rig(0, nb, with_ekf=True)
        ctx.sync()
        dt = time.perf_counter() - t0
        if s0 > 0:                                   # the first call pays the first-use costs
            total += dt
            done += nb
    ps = ctx.plan_stats()
    return dict(what="run_staged_rig", cameras=C, steps_per_call=spc, steps_timed=done, steps_per_s=round(done / total, 1),
                frames_per_s=round(done * C / total, 1), markers_per_step=round(markers / n_steps, 1), plan=ps,
                share_in_windows=round(ps["frames_in_windows"] / max(1, ps["frames_in_windows"] + ps["frames_per_frame_chain"]), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latency-only", type=int, default=0)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--throughput-steps", type=int, default=400)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    if a.latency_only:
        res.append(latency(a.latency_only, a.steps, 2))
    else:
        res.append(latency(1, a.steps, 3, single=True))
        for C in (1, 2, 4):
            res.append(latency(C, a.steps, 3))
        for C in (1, 2, 4):
            res.append(throughput(C, a.throughput_steps, 128))
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
