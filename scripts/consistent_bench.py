"""Consistent innovations: what the switch costs and what it is for.

kernels: device time per launch, through aslam_profile_get, of the kernels that have a RunningMean twin - k_loc_steps and k_fleet_steps
(fixed and uncertain map, ungated and gated), k_ekf_mid, k_ekf_mid64 and k_ekf_small (both of its paths; ungated and gated) - with the
switch off and on, on the same injected frames: 20 sightings per frame (k_ekf_small: 20 and 40) of a dense map, the filter re-seated
before every launch.

fps: the headline workload (cfg2, 320 frames per step, one lap already mapped) with the switch off and on in one process.  With the
switch on no window is planned: every frame takes the per-frame chain.

lap: §31's experiment - localization on the true map of the rendered ring of cfg2_sliding (one lap of 320 frames), the observation
covariance on, the innovation gate at +inf - with this switch off and on: the filter's own NIS from the slot records (chi^2_3 has mean 3)
and the trajectory error against the scene's true poses.

    python scripts/consistent_bench.py [--only {kernels,fps,lap}] [--out FILE]

Prints one JSON object."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from aruco_slam_amd import capi, synth  # noqa: E402

CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
SIG0 = np.diag([1e-4, 1e-4, 1e-5])


def wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def state(rng, L):
    N = 3 + 3 * L
    mu = np.zeros(N)
    mu[:3] = [0.3, -0.2, 0.4]
    ang, rad = rng.uniform(0, 2 * math.pi, L), rng.uniform(1.0, 6.0, L)
    mu[3::3], mu[4::3], mu[5::3] = rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-3, 3, L)
    A = rng.standard_normal((N, 24)) * 0.05
    return mu, A @ A.T + np.diag(rng.uniform(0.01, 0.05, N))


def sightings(mu, ids, m, rng):
    sel = rng.permutation(ids.size)[:m]
    c, s = math.cos(mu[2]), math.sin(mu[2])
    dx, dy = mu[3 + 3 * sel] - mu[0], mu[4 + 3 * sel] - mu[1]
    z = np.stack([dx * c + dy * s, -dx * s + dy * c, wrap(mu[5 + 3 * sel] - mu[2])], 1) + rng.normal(0, 0.03, (m, 3))
    return ids[sel], z, rng.uniform(0.02, 0.2, (m, 3))


def us(prof, name):
    calls, ms = prof[name]
    return round(1e3 * ms / max(calls, 1), 2)


def slam_kernel(cap, m, name, gated, consistent, reps=20, L=60):
    rng = np.random.RandomState(cap + m)
    mu, S = state(rng, L)
    ids = rng.permutation(1024)[:L].astype(np.int32)
    banks = [sightings(mu, ids, m, rng) for _ in range(2)]
    os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        ctx = capi.Context(max_rows=64, max_cols=64, max_batch=3, max_landmarks=L, max_updates_per_frame=cap)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)
    if gated:
        ctx.set_slam_gate()
    ctx.set_consistent_innovations(consistent)
    for b in range(2):
        i, z, rd = banks[b]
        ctx.inject_observations(b, i, np.ones(m, np.int32), z, rd)
    ctx.inject_observations(2, [], [], np.zeros((0, 3)), np.zeros((0, 3)))
    ctx.stage_encoders([0.0] * 3, [0.0] * 3, [0.05] * 3)
    ctx.set_state(mu, S, ids)
    ctx.run_staged(2, 1, with_ekf=2)                                # arms the filter
    ctx.sync()
    ctx.profile_enable(True)
    for k in range(3 + reps):
        if k == 3:
            ctx.profile_reset()
        ctx.set_state(mu, S, ids)
        ctx.run_staged(k % 2, 1, with_ekf=2)
        ctx.sync()
    t = us(ctx.profile_get(), name)
    ctx.close()
    return t


def loc_kernel(R, umap, gated, consistent, reps=20, L=60, m=20, frames=8):
    rng = np.random.RandomState(7 + R)
    mu, _ = state(rng, L)
    ids = rng.permutation(1024)[:L].astype(np.int32)
    xyth = mu[3:].reshape(-1, 3)
    A = rng.normal(0, 0.03, (L, 3, 3))
    C = A @ A.transpose(0, 2, 1) + 1e-6 * np.eye(3)
    n = max(R, 1)
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=n * frames, max_landmarks=L)
    if gated:
        ctx.set_innovation_gate()
    ctx.set_consistent_innovations(consistent)
    if R:
        (ctx.fleet_begin_uncertain([CAM] * R, ids, xyth, C, [mu[:3]] * R, [SIG0] * R) if umap else
         ctx.fleet_begin([CAM] * R, ids, xyth, [mu[:3]] * R, [SIG0] * R))
    else:
        (ctx.localize_begin_uncertain(ids, xyth, C, mu[:3], SIG0) if umap else ctx.localize_begin(ids, xyth, mu[:3], SIG0))
    for s in range(n * frames):
        i, z, rd = sightings(mu, ids, m, rng)
        ctx.inject_observations(s, i, np.ones(m, np.int32), z, rd)
    ctx.stage_encoders([0.0] * (n * frames), [0.0] * (n * frames), [0.05] * (n * frames))
    ctx.profile_enable(True)
    order = [r for _ in range(frames) for r in range(n)]
    for k in range(3 + reps):
        if k == 3:
            ctx.profile_reset()
        if R:
            ctx.fleet_run_staged(0, order, with_ekf=2)
        else:
            ctx.run_staged(0, frames, with_ekf=2)
        ctx.sync()
    t = us(ctx.profile_get(), "k_fleet_steps" if R else "k_loc_steps")
    ctx.close()
    return t


def kernels():
    out = []
    for cap, m, name in ((24, 20, "k_ekf_mid"), (64, 20, "k_ekf_mid64"), (64, 50, "k_ekf_mid64"), (128, 20, "k_ekf_small"), (128, 40, "k_ekf_small")):
        for gated in (False, True):
            off, on = slam_kernel(cap, m, name, gated, False), slam_kernel(cap, m, name, gated, True)
            out.append(dict(kernel=name, corrections=m, gated=gated, frozen_us=off, running_us=on, ratio=round(on / off, 3)))
    for R in (0, 16):
        for umap in (False, True):
            for gated in (False, True):
                off, on = loc_kernel(R, umap, gated, False), loc_kernel(R, umap, gated, True)
                out.append(dict(kernel="k_fleet_steps" if R else "k_loc_steps", robots=R, slots_per_filter=8, corrections=20, uncertain_map=umap,
                                gated=gated, frozen_us=off, running_us=on, ratio=round(on / off, 3)))
    return out


def fps(steps=20, warmup=3):
    args = argparse.Namespace(waves=0, reserve=0)
    cfg, world, lap, ctx, frames, host = bench.scene_setup(np, capi, synth, "cfg2", 0, 0, args, True, 0, detector="scene", qualify=True)
    ctx.run_staged(0, lap, with_ekf=True)                           # the map: one lap through the augment path
    ctx.sync()
    turn = world.frame(lap)
    ctx.stage_encoders([turn.wl], [turn.wr], [turn.dt], slot0=0)
    ctx.stage_encoders([turn.wl], [turn.wr], [turn.dt], slot0=lap)
    mu, S, ids = (*ctx.get_state(), ctx.get_landmark_ids())
    res = {"frames_per_step": lap, "steps": steps}
    for name, on in (("switch_off", False), ("switch_on", True), ("switch_off_again", False)):
        ctx.set_consistent_innovations(on)
        ctx.set_state(mu, S, ids)
        for k in range(warmup):
            ctx.run_staged((k & 1) * lap, lap, with_ekf=True)
        ctx.sync()
        ctx.profile_reset()
        t0 = time.perf_counter()
        for k in range(steps):
            ctx.run_staged(((k + warmup) & 1) * lap, lap, with_ekf=True)
        ctx.sync()
        el = time.perf_counter() - t0
        res[name] = {"frames_per_s": round(steps * lap / el, 1), "plan": ctx.plan_stats()}
    ctx.close()
    return res


def lap_run(consistent, B=320):
    cfg = synth.CONFIGS["cfg2_sliding"]
    w = synth.RingWorld(synth.SceneConfig(**{**cfg.__dict__, "ring_lap_frames": B}))
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=B, max_landmarks=w.L + 8)
    ctx.set_camera(w.K, np.zeros(5))
    synth.apply_detector(cfg, ctx=ctx)
    ctx.set_innovation_gate(gate_d2=math.inf)
    ctx.set_observation_covariance()
    ctx.set_consistent_innovations(consistent)
    ctx.localize_begin(w.ids, w.world, w.pose[0], SIG0)
    frs = [w.frame(i) for i in range(B)]
    for i, fr in enumerate(frs):
        ctx.synth_render(i, cfg.rows, cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=i, download=False)
    ctx.stage_encoders([fr.wl for fr in frs], [fr.wr for fr in frs], [fr.dt for fr in frs])
    pos, th = [], []
    for i, fr in enumerate(frs):                                    # frame by frame: the pose after every frame against the truth
        ctx.run_staged(i, 1, with_ekf=True)
        mu, _ = ctx.get_state()
        pos.append(math.hypot(mu[0] - fr.true_pose[0], mu[1] - fr.true_pose[1]))
        th.append(abs(wrap(mu[2] - fr.true_pose[2])))
    h = ctx.get_slot_health(0, B)
    att = h["attempted"] > 0
    per_frame = h["nis_sum"][att] / h["attempted"][att]
    res = {"consistent": bool(consistent), "frames": B, "corrections": int(h["attempted"].sum()),
           "filter_nis_mean": round(float(h["nis_sum"].sum() / max(h["attempted"].sum(), 1)), 4),
           "filter_nis_frame_mean_median": round(float(np.median(per_frame)), 4),
           "filter_d2_max": round(float(h["d2_max"].max()), 3),
           "position_error_m": {"median": round(float(np.median(pos)), 5), "max": round(float(np.max(pos)), 5), "last": round(pos[-1], 5)},
           "heading_error_rad": {"median": round(float(np.median(th)), 5), "max": round(float(np.max(th)), 5)}}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["kernels", "fps", "lap"], default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {}
    if a.only in ("", "kernels"):
        out["kernels"] = kernels()
    if a.only in ("", "fps"):
        out["fps"] = fps()
    if a.only in ("", "lap"):
        out["lap"] = [lap_run(False), lap_run(True)]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
