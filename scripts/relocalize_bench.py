"""Relocalization measurements: wall time of one aslam_fleet_relocalize(apply = 1) over R robots with 20 observations
each (14 sightings from the robot's true pose, 6 wrong-id outliers), against the host route on the same slots: R x
aslam_get_slot_raw_observations, tests/relocalize_reference.py per robot, R x aslam_fleet_set_pose for the solved ones.

    python scripts/relocalize_bench.py [--robots 4,16,64,256] [--only device] [--out FILE]

Prints one JSON line per R (and appends it to --out): p50 and max over 20 timed calls after 3 warm-up calls.  --only device skips
the host route (for a rocprofv3 --kernel-trace run)."""
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
from tests import relocalize_reference as ref  # noqa: E402

LANDMARKS, INLIERS, OUTLIERS = 40, 14, 6


def sighting(pose, lm, rng, noise=0.01):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    dx, dy = lm[0] - pose[0], lm[1] - pose[1]
    return np.array([dx * c + dy * s, -dx * s + dy * c, ref.wrap(lm[2] - pose[2])]) + rng.normal(0, noise, 3)


def install(ctx, R, ids, xyth, rng):
    """slot r: robot r's 20 observations; returns the true poses"""
    truth = np.stack([rng.uniform(-3, 3, R), rng.uniform(-3, 3, R), rng.uniform(-3, 3, R)], 1)
    for r in range(R):
        sel = rng.permutation(LANDMARKS)[:INLIERS + OUTLIERS]
        label = sel.copy()
        label[INLIERS:] = np.roll(sel[INLIERS:], 1)                      # an outlier: one landmark reported under another's id
        order = rng.permutation(INLIERS + OUTLIERS)
        z = np.array([sighting(truth[r], xyth[li], rng) for li in sel])
        ctx.inject_observations(r, ids[label][order], np.ones(len(sel), np.int32), z[order], rng.uniform(0.01, 0.05, (len(sel), 3)))
    return truth


def host_route(ctx, R, ids, xyth):
    out = []
    for r in range(R):
        i, v, z, rd = ctx.get_slot_raw_observations(r)
        out.append(ref.relocalize(ids, xyth, [(int(i[k]), int(v[k]), z[k], rd[k]) for k in range(len(i))]))
    for r in range(R):
        if out[r]["status"] == 0:
            ctx.fleet_set_pose(r, out[r]["pose"], 0.5 * (out[r]["sigma"] + out[r]["sigma"].T))
    return out


def stats(ts):
    return round(float(np.percentile(ts, 50)) * 1e6, 1), round(float(np.max(ts)) * 1e6, 1)


def measure(R, only_device, reps=20, warm=3):
    rng = np.random.RandomState(R)
    ids = rng.permutation(1024)[:LANDMARKS].astype(np.int32)
    xyth = np.stack([rng.uniform(-5, 5, LANDMARKS), rng.uniform(-5, 5, LANDMARKS), rng.uniform(-math.pi, math.pi, LANDMARKS)], 1)
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=R, max_landmarks=LANDMARKS)
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    ctx.fleet_begin([cam] * R, ids, xyth, np.zeros((R, 3)), [np.eye(3)] * R)
    truth = install(ctx, R, ids, xyth, rng)
    robots = list(range(R))
    ts = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        got = ctx.fleet_relocalize(0, robots, apply=True)
        ts.append(time.perf_counter() - t0)
    d = got["pose"] - truth
    d[:, 2] = [ref.wrap(a) for a in d[:, 2]]
    out = dict(what="fleet_relocalize", robots=R, observations_per_robot=INLIERS + OUTLIERS, solved=int((got["status"] == 0).sum()),
               mean_inliers=round(float(got["n_inliers"].mean()), 2), worst_to_truth_m=round(float(np.hypot(d[:, 0], d[:, 1]).max()), 4),
               worst_to_truth_rad=round(float(np.abs(d[:, 2]).max()), 4))
    out["device_p50_us"], out["device_max_us"] = stats(ts[warm:])
    if not only_device:
        hs = []
        for k in range(warm + reps):
            t0 = time.perf_counter()
            want = host_route(ctx, R, ids, xyth)
            hs.append(time.perf_counter() - t0)
        out["host_route_p50_us"], out["host_route_max_us"] = stats(hs[warm:])
        dp = np.array([g - w["pose"] for g, w in zip(got["pose"], want)])
        dp[:, 2] = [ref.wrap(a) for a in dp[:, 2]]
        out.update(max_abs_diff_pose=float(np.abs(dp).max()),
                   same_counts=bool(all(int(g[k]) == int(w[k]) for g, w in zip(got, want) for k in ("status", "n_inliers", "runner_up", "best"))))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4,16,64,256")
    ap.add_argument("--only", choices=["device"])
    ap.add_argument("--out")
    a = ap.parse_args()
    for R in [int(x) for x in a.robots.split(",")]:
        line = json.dumps(measure(R, a.only == "device"))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
