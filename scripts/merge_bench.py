"""Map merge measurements: wall time of aslam_fleet_merge_maps on a SLAM fleet of R robots at the default capacity
(max_landmarks 256), against the host route on the same states: R x aslam_fleet_get_state (+ the landmark ids), records built in
numpy, tests/merge_reference.py.

Every robot's filter is installed with aslam_fleet_set_state: a map of 20 landmarks in the robot's own random frame, 14 of its
own and 6 of the robot (r - 1) // 4's own, so the overlap graph is a 4-ary tree (1, 2 and 3 alignment rounds at R = 4, 16, 64).

    python scripts/merge_bench.py [--robots 4,16,64] [--only device] [--out FILE]

Prints one JSON line per R (and appends it to --out).  --only device skips the host route (for a rocprofv3 --kernel-trace run)."""
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
from tests import merge_reference as ref  # noqa: E402

OWN, SHARED = 14, 6


def install(ctx, R, rng):
    ids = rng.permutation(1024)[:R * OWN].astype(np.int32).reshape(R, OWN)
    xyth = np.stack([rng.uniform(-20, 20, R * OWN), rng.uniform(-20, 20, R * OWN), rng.uniform(-1, 1, R * OWN)], 1).reshape(R, OWN, 3)
    for r in range(R):
        held = [(ids[r, k], xyth[r, k]) for k in range(OWN)]
        if r:
            p = (r - 1) // 4
            held += [(ids[p, k], xyth[p, k]) for k in rng.permutation(OWN)[:SHARED]]
        fx, fy, fth = rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-0.6, 0.6)
        c, s = math.cos(fth), math.sin(fth)
        mu = [0.0, 0.0, 0.0]
        for _, (x, y, th) in held:
            mu += [c * (x - fx) + s * (y - fy) + rng.normal(0, 0.01), -s * (x - fx) + c * (y - fy) + rng.normal(0, 0.01), th - fth]
        N = len(mu)
        S = np.zeros((N, N))
        for i in range(len(held)):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            S[3 + 3 * i:6 + 3 * i, 3 + 3 * i:6 + 3 * i] = q @ np.diag(10.0 ** rng.uniform(-4, -2, 3)) @ q.T
        ctx.fleet_set_state(r, np.array(mu), S, np.array([h[0] for h in held], np.int32))


def host_route(ctx, R, per_map):
    rec = np.zeros((R, per_map), ref.MAP_DTYPE)
    rec["id"] = -1
    rec["index"] = -1
    for r in range(R):
        mu, S = ctx.fleet_get_state(r)
        for i, lid in enumerate(ctx.fleet_get_landmark_ids(r)):
            li = 3 + 3 * i
            rec[r, i] = (lid, i, mu[li], mu[li + 1], mu[li + 2], S[li:li + 3, li:li + 3].reshape(9))
    return ref.merge(rec, R, per_map)


def measure(R, only_device, reps=20):
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=R, max_landmarks=256)
    ctx.fleet_slam_begin([(synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))] * R)
    install(ctx, R, np.random.RandomState(R))
    for _ in range(3):
        got = ctx.fleet_merge_maps()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.fleet_merge_maps()
        ts.append(time.perf_counter() - t0)
    out = dict(what="fleet_merge_maps", robots=R, max_landmarks=256, landmarks_per_robot=OWN + (SHARED if R > 1 else 0),
               merged_ids=int(got[0].size), rounds=int(got[4].max()), aligned=int((got[4] >= 0).sum()),
               device_p50_us=round(float(np.percentile(ts, 50)) * 1e6, 1), device_max_us=round(float(np.max(ts)) * 1e6, 1))
    if not only_device:
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = host_route(ctx, R, 256)
            hs.append(time.perf_counter() - t0)
        out.update(host_route_p50_us=round(float(np.median(hs)) * 1e6, 1),
                   max_abs_diff_xyth=float(np.abs(got[1] - want[1]).max()), same_ids_rounds=bool(np.array_equal(got[0], want[0]) and np.array_equal(got[4], want[4])))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4,16,64")
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
