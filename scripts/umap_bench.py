"""Uncertain-map measurements: wall time of one fleet tick, aslam_fleet_run_staged(with_ekf = 2) plus aslam_sync, over
R robots with 20 injected observations each (true sightings from the robot's pose with noise drawn from their own R) on maps of 40
and 256 landmarks: on the exact map (aslam_fleet_begin), on the uncertain map (aslam_fleet_begin_uncertain) ungated and at the
default gate, and at the default gate with every sighting displaced so far that all 20 corrections are rejected.

    python scripts/umap_bench.py [--robots 4,16,64,256] [--landmarks 40,256] [--modes fixed,umap,umap_gate,umap_gate_rejected]
                                 [--without-umap-api] [--out FILE]

Prints one JSON line per (landmarks, R) (and appends it to --out): p50 and max over 20 timed calls after 3 warm-up calls, in one
process.  Two banks of slots with different observations alternate, so that no tick finds its observations "stationary".
--without-umap-api binds a library built before the feature existed (ARUCO_SLAM_LIB names it): only --modes fixed can run then,
which is the parent's tick."""
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

OBS = 20
UMAP_API = ("aslam_localize_begin_uncertain", "aslam_fleet_begin_uncertain", "aslam_is_map_uncertain", "aslam_fleet_get_cross")


def wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def sightings(pose, ids, xyth, rng, off):
    sel = rng.permutation(len(ids))[:OBS]
    r = rng.uniform(0.01, 0.05, (OBS, 3))
    c, s = math.cos(pose[2]), math.sin(pose[2])
    dx, dy = xyth[sel, 0] - pose[0], xyth[sel, 1] - pose[1]
    z = np.stack([dx * c + dy * s, -dx * s + dy * c, wrap(xyth[sel, 2] - pose[2])], 1) + rng.normal(0, 1, r.shape) * np.sqrt(r) + off
    return ids[sel], z, r


def stats(ts):
    return round(float(np.percentile(ts, 50)) * 1e6, 1), round(float(np.max(ts)) * 1e6, 1)


def measure(L, R, modes, reps=20, warm=3):
    rng = np.random.RandomState(1000 * L + R)
    ids = rng.permutation(1024)[:L].astype(np.int32)
    xyth = np.stack([rng.uniform(-5, 5, L), rng.uniform(-5, 5, L), rng.uniform(-math.pi, math.pi, L)], 1)
    A = rng.normal(0, 0.03, (L, 3, 3))
    C = A @ A.transpose(0, 2, 1)
    truth = np.stack([rng.uniform(-3, 3, R), rng.uniform(-3, 3, R), rng.uniform(-3, 3, R)], 1)
    good = [[sightings(truth[r], ids, xyth, rng, 0.0) for r in range(R)] for _ in range(2)]
    bad = [[sightings(truth[r], ids, xyth, rng, np.array([8.0, -6.0, 0.0])) for r in range(R)] for _ in range(2)]
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    robots = list(range(R))
    sig = [np.diag([0.02, 0.02, 0.01])] * R
    out = dict(what="fleet tick, with_ekf = 2", landmarks=L, robots=R, observations_per_robot=OBS, strip_columns_per_lane=-(-3 * L // 128))
    for mode in modes:
        ctx = capi.Context(max_rows=64, max_cols=64, max_batch=2 * R, max_landmarks=L)
        if mode.startswith("umap_gate"):
            ctx.set_innovation_gate()
        if mode == "fixed":
            ctx.fleet_begin([cam] * R, ids, xyth, truth, sig)
        else:
            ctx.fleet_begin_uncertain([cam] * R, ids, xyth, C, truth, sig)
        banks = bad if mode == "umap_gate_rejected" else good
        for b in range(2):
            for r in range(R):
                i, z, rd = banks[b][r]
                ctx.inject_observations(b * R + r, i, np.ones(len(i), np.int32), z, rd)
        ctx.stage_encoders([0.0] * (2 * R), [0.0] * (2 * R), [0.05] * (2 * R))
        ts = []
        for k in range(warm + reps):
            t0 = time.perf_counter()
            ctx.fleet_run_staged((k % 2) * R, robots, with_ekf=2)
            ctx.sync()
            ts.append(time.perf_counter() - t0)
        out[f"tick_{mode}_p50_us"], out[f"tick_{mode}_max_us"] = stats(ts[warm:])
        out[f"fused_per_robot_{mode}"] = round(float(ctx.get_slot_ekf_stats(((warm + reps - 1) % 2) * R, R)[:, 2].mean()), 2)
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4,16,64,256")
    ap.add_argument("--landmarks", default="40,256")
    ap.add_argument("--modes", default="fixed,umap,umap_gate,umap_gate_rejected")
    ap.add_argument("--without-umap-api", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    modes = a.modes.split(",")
    if a.without_umap_api:
        if modes != ["fixed"]:
            ap.error("--without-umap-api runs --modes fixed only")
        for name in UMAP_API:
            capi._SIGS.pop(name, None)
    for L in [int(x) for x in a.landmarks.split(",")]:
        for R in [int(x) for x in a.robots.split(",")]:
            line = json.dumps(measure(L, R, modes))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
