"""Observation covariance.

cost: the profile families k_pose, k_pose_cov and k_pose_alt on the same frames of the headline configuration (cfg2: 320 frames per
batch, 20 markers per frame) with both switches on, per batch of 320 frames and for the single-frame call.

gate: §19's experiment - localization on the true map of the rendered ring of cfg2_sliding (one lap of 320 frames), the innovation gate
at gate_d2 = inf (monitor only) - with the switch off and on.  Reported against chi^2_3: the filter's own NIS (mean d^2 over all
corrections, and the quantiles of the per-frame mean and maximum, from the slot health records), and per sighting
d^2 = sum_i e_i^2 / R_i of the raw observation against the scene's truth (true robot pose, true landmark), which needs no filter; and how
many sightings the range gate, the reference's covariance gate (switch off) and the new gate (switch on) drop.

    python scripts/obs_cov_bench.py [--only {cost,gate}] [--out FILE]

Prints one JSON object."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from aruco_slam_amd import capi, synth  # noqa: E402

CHI2_3 = {"0.5": 2.366, "0.9": 6.251, "0.99": 11.345}
SIG0 = np.diag([1e-4, 1e-4, 1e-5])


def quantiles(v):
    v = np.asarray(v, np.float64)
    return {q: round(float(np.quantile(v, float(q))), 4) for q in CHI2_3} if v.size else {}


def cost(steps=20):
    args = argparse.Namespace(waves=0, reserve=0)
    cfg, world, lap, ctx, frames, host = bench.scene_setup(np, capi, synth, "cfg2", 0, 0, args, False, 0, detector="scene", qualify=True)
    ctx.set_observation_covariance()
    ctx.set_pose_ambiguity()
    ctx.run_staged(0, lap, with_ekf=False)
    ctx.sync()
    sums = np.array([tuple(ctx.get_slot_obs_covariance(s)[1])[:3] for s in range(lap)])
    res = {"frames": lap, "params": ctx.get_observation_covariance(), "checked": int(sums[:, 0].sum()), "degenerate": int(sums[:, 1].sum()),
           "gated": int(sums[:, 2].sum())}
    ctx.profile_enable(True)
    kernels = ("k_pose", "k_pose_cov", "k_pose_alt")
    for name, first, count in (("batch_320", 0, lap), ("single_frame", 7, 1)):
        ctx.profile_reset()
        for _ in range(steps):
            ctx.run_staged(first, count, with_ekf=False)
        ctx.sync()
        prof = ctx.profile_get()
        res[name] = {k: {"calls": prof[k][0], "us_per_call": round(1e3 * prof[k][1] / max(prof[k][0], 1), 2)} for k in kernels}
        res[name]["ratio_cov_over_pose"] = round(prof["k_pose_cov"][1] / prof["k_pose"][1], 3)
        res[name]["ratio_cov_over_alt"] = round(prof["k_pose_cov"][1] / prof["k_pose_alt"][1], 3)
    ctx.profile_enable(False)
    ctx.close()
    return res


def gate(switch, B=320):
    cfg = synth.CONFIGS["cfg2_sliding"]
    w = synth.RingWorld(synth.SceneConfig(**{**cfg.__dict__, "ring_lap_frames": B}))
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=B, max_landmarks=w.L + 8)
    ctx.set_camera(w.K, np.zeros(5))
    synth.apply_detector(cfg, ctx=ctx)
    ctx.set_innovation_gate(gate_d2=math.inf)
    if switch:
        ctx.set_observation_covariance()
    ctx.localize_begin(w.ids, w.world, w.pose[0], SIG0)
    frs = [w.frame(i) for i in range(B)]
    for i, fr in enumerate(frs):
        ctx.synth_render(i, cfg.rows, cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=i, download=False)
    ctx.stage_encoders([fr.wl for fr in frs], [fr.wr for fr in frs], [fr.dt for fr in frs])
    ctx.run_staged(0, B, with_ekf=True)
    ctx.sync()
    health = ctx.get_slot_health(0, B)
    index = {int(m): k for k, m in enumerate(w.ids)}
    d2, sightings, invalid, flags = [], 0, 0, np.zeros(0, np.int32)
    for i, fr in enumerate(frs):
        ids, valid, xyth, Rd = ctx.get_slot_raw_observations(i)
        sightings += len(ids)
        invalid += int((valid == 0).sum())
        if switch:
            flags = np.concatenate([flags, ctx.get_slot_obs_covariance(i)[0]["flags"]])
        px, py, phi = fr.true_pose
        c, s = math.cos(phi), math.sin(phi)
        for m, v, z, r in zip(ids, valid, xyth, Rd):
            if not v or int(m) not in index:
                continue
            lx, ly, lth = w.world[index[int(m)]]
            dx, dy = lx - px, ly - py
            e = np.array([dx * c + dy * s - z[0], -dx * s + dy * c - z[1], (lth - phi - z[2] + math.pi) % (2 * math.pi) - math.pi])
            d2.append(float(np.sum(e * e / r)))
    att = health["attempted"] > 0
    res = {"switch": bool(switch), "frames": B, "sightings": sightings, "dropped": invalid,
           "corrections": int(health["attempted"].sum()), "filter_nis_mean": round(float(health["nis_sum"].sum() / max(health["attempted"].sum(), 1)), 4),
           "filter_nis_frame_mean_quantiles": quantiles(health["nis_sum"][att] / health["attempted"][att]),
           "filter_d2_frame_max_quantiles": quantiles(health["d2_max"][att]),
           "truth_d2_quantiles": quantiles(d2), "truth_d2_mean": round(float(np.mean(d2)), 4) if d2 else None, "truth_d2_count": len(d2)}
    if switch:
        res.update(dropped_degenerate=int(((flags & 1) != 0).sum()), dropped_new_gate=int(((flags & 2) != 0).sum()),
                   dropped_range_gate=int(((flags & 4) != 0).sum()))
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["cost", "gate"], default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"chi2_3_quantiles": CHI2_3}
    if a.only != "gate":
        out["cost"] = cost()
    if a.only != "cost":
        out["gate"] = [gate(False), gate(True)]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
