"""Innovation-gate measurements: wall time of one fleet tick, aslam_fleet_run_staged(with_ekf = 2) plus aslam_sync,
over R robots with 20 injected observations each (16 sightings from the robot's true pose with noise drawn from their own R, 4
wrong-id outliers), with the gate off, at +inf (monitor only) and at the default; and of one aslam_fleet_get_health.

    python scripts/gate_bench.py [--robots 4,16,64,256] [--modes off,inf,default] [--without-gate-api] [--out FILE]

Prints one JSON line per R (and appends it to --out): p50 and max over 20 timed calls after 3 warm-up calls.  Two banks of slots
with different observations alternate, so that no tick finds its observations "stationary".  --without-gate-api binds a library
built before the gate existed (ARUCO_SLAM_LIB names it): only --modes off can run then, which is the parent's tick."""
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

LANDMARKS, TRUE, WRONG = 40, 16, 4
GATE_API = ("aslam_default_gate_params", "aslam_set_innovation_gate", "aslam_get_innovation_gate", "aslam_get_slot_health",
            "aslam_get_track_health", "aslam_fleet_get_health")


def wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def sightings(pose, ids, xyth, rng):
    sel = rng.permutation(LANDMARKS)[:TRUE + WRONG]
    label = sel.copy()
    label[TRUE:] = np.roll(sel[TRUE:], 1)                                # an outlier: one landmark reported under another's id
    r = rng.uniform(0.01, 0.05, (len(sel), 3))
    c, s = math.cos(pose[2]), math.sin(pose[2])
    dx, dy = xyth[sel, 0] - pose[0], xyth[sel, 1] - pose[1]
    z = np.stack([dx * c + dy * s, -dx * s + dy * c, wrap(xyth[sel, 2] - pose[2])], 1) + rng.normal(0, 1, r.shape) * np.sqrt(r)
    order = rng.permutation(len(sel))
    return ids[label][order], z[order], r[order]


def stats(ts):
    return round(float(np.percentile(ts, 50)) * 1e6, 1), round(float(np.max(ts)) * 1e6, 1)


def measure(R, modes, reps=20, warm=3):
    rng = np.random.RandomState(R)
    ids = rng.permutation(1024)[:LANDMARKS].astype(np.int32)
    xyth = np.stack([rng.uniform(-5, 5, LANDMARKS), rng.uniform(-5, 5, LANDMARKS), rng.uniform(-math.pi, math.pi, LANDMARKS)], 1)
    truth = np.stack([rng.uniform(-3, 3, R), rng.uniform(-3, 3, R), rng.uniform(-3, 3, R)], 1)
    banks = [[sightings(truth[r], ids, xyth, rng) for r in range(R)] for _ in range(2)]
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    robots = list(range(R))
    out = dict(what="fleet tick, with_ekf = 2", robots=R, observations_per_robot=TRUE + WRONG)
    for mode in modes:
        ctx = capi.Context(max_rows=64, max_cols=64, max_batch=2 * R, max_landmarks=LANDMARKS)
        if mode != "off":
            ctx.set_innovation_gate(**(dict(gate_d2=float("inf")) if mode == "inf" else {}))
        ctx.fleet_begin([cam] * R, ids, xyth, truth, [np.diag([0.02, 0.02, 0.01])] * R)
        for b in range(2):
            for r in range(R):
                i, z, rd = banks[b][r]
                ctx.inject_observations(b * R + r, i, np.ones(len(i), np.int32), z, rd)
        ctx.stage_encoders([0.0] * (2 * R), [0.0] * (2 * R), [0.05] * (2 * R))
        ts, hs = [], []
        for k in range(warm + reps):
            t0 = time.perf_counter()
            ctx.fleet_run_staged((k % 2) * R, robots, with_ekf=2)
            ctx.sync()
            ts.append(time.perf_counter() - t0)
            if mode != "off":
                t0 = time.perf_counter()
                health = ctx.fleet_get_health()
                hs.append(time.perf_counter() - t0)
        out[f"tick_{mode}_p50_us"], out[f"tick_{mode}_max_us"] = stats(ts[warm:])
        fused = ctx.get_slot_ekf_stats(((warm + reps - 1) % 2) * R, R)[:, 2]
        out[f"fused_per_robot_{mode}"] = round(float(fused.mean()), 2)
        if mode != "off":
            out[f"get_health_{mode}_p50_us"], out[f"get_health_{mode}_max_us"] = stats(hs[warm:])
            out[f"rejected_share_{mode}"] = round(float(health["rejected_total"].sum()) /
                                                  max(int(health["rejected_total"].sum() + health["accepted_total"].sum()), 1), 4)
            out[f"lost_{mode}"] = int(health["lost"].sum())
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4,16,64,256")
    ap.add_argument("--modes", default="off,inf,default")
    ap.add_argument("--without-gate-api", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    modes = a.modes.split(",")
    if a.without_gate_api:
        if modes != ["off"]:
            ap.error("--without-gate-api runs --modes off only")
        for name in GATE_API:
            capi._SIGS.pop(name, None)
    for R in [int(x) for x in a.robots.split(",")]:
        line = json.dumps(measure(R, modes))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
