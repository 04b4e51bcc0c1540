"""SLAM-gate measurements: wall time of one tick, aslam_run_staged(with_ekf = 2) on a single windows-off context or
aslam_fleet_run_staged(with_ekf = 2) over R robots of a SLAM fleet, plus aslam_sync.  Every filter holds a dense map of 40 or 200
landmarks and gets 20 injected observations per tick: 16 true sightings (noise 0.03) and 4 displaced by (2.7, -2.1, 0).  Modes: the
gate off, at +inf (monitor only), at the default, and at 1e-9, where every correction is rejected.

    python scripts/slam_gate_bench.py [--robots 0,4,16,64] [--landmarks 40,200] [--caps 24,64] [--modes off,inf,default,all]
                                      [--without-gate-api] [--out FILE]

Prints one JSON line per configuration (and appends it to --out): p50 and max over 20 timed ticks after 3 warm-up ticks.  R = 0 is the
single context.  Every tick starts from the same injected state (aslam_set_state / aslam_fleet_set_state outside the timed span), and
two banks of slots with different observations alternate, so that no tick finds its observations "stationary".  --without-gate-api
binds a library built before the gate existed (ARUCO_SLAM_LIB names it): only --modes off can run then, which is the parent's tick."""
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

TRUE, WRONG = 16, 4
OUTLIER = np.array([2.7, -2.1, 0.0])
GATE_API = ("aslam_set_slam_gate", "aslam_get_slam_gate")
GATES = dict(inf=dict(gate_d2=float("inf")), default={}, all=dict(gate_d2=1e-9))


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


def sightings(mu, ids, rng):
    L = ids.size
    sel = rng.permutation(L)[:TRUE + WRONG]
    c, s = math.cos(mu[2]), math.sin(mu[2])
    dx, dy = mu[3 + 3 * sel] - mu[0], mu[4 + 3 * sel] - mu[1]
    z = np.stack([dx * c + dy * s, -dx * s + dy * c, wrap(mu[5 + 3 * sel] - mu[2])], 1) + rng.normal(0, 0.03, (sel.size, 3))
    z[TRUE:] += OUTLIER
    order = rng.permutation(sel.size)
    return ids[sel][order], z[order], rng.uniform(0.02, 0.2, (sel.size, 3))[order]


def stats(ts):
    return round(float(np.percentile(ts, 50)) * 1e6, 1), round(float(np.max(ts)) * 1e6, 1)


def measure(R, L, cap, modes, reps=20, warm=3):
    rng = np.random.RandomState(1000 * R + L + cap)
    n = max(R, 1)
    filters = [state(rng, L) for _ in range(n)]
    ids = rng.permutation(1024)[:L].astype(np.int32)
    banks = [[sightings(filters[r][0], ids, rng) for r in range(n)] for _ in range(2)]
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    out = dict(what="SLAM tick, with_ekf = 2", robots=R, landmarks=L, max_updates_per_frame=cap, observations=TRUE + WRONG)
    for mode in modes:
        os.environ["ASLAM_NO_WINDOWS"] = "1"
        try:
            ctx = capi.Context(max_rows=64, max_cols=64, max_batch=2 * n + 1, max_landmarks=L, max_updates_per_frame=cap)
        finally:
            os.environ.pop("ASLAM_NO_WINDOWS", None)
        if mode != "off":
            ctx.set_slam_gate(**GATES[mode])
        if R:
            ctx.fleet_slam_begin([cam] * R)
        for b in range(2):
            for r in range(n):
                i, z, rd = banks[b][r]
                ctx.inject_observations(b * n + r, i, np.ones(len(i), np.int32), z, rd)
        ctx.inject_observations(2 * n, [], [], np.zeros((0, 3)), np.zeros((0, 3)))
        ctx.stage_encoders([0.0] * (2 * n + 1), [0.0] * (2 * n + 1), [0.05] * (2 * n + 1))

        def seat():
            for r in range(n):
                if R:
                    ctx.fleet_set_state(r, filters[r][0], filters[r][1], ids)
                else:
                    ctx.set_state(filters[r][0], filters[r][1], ids)

        ts = []
        armed = False
        for k in range(warm + reps):
            seat()
            if not armed:                                        # the first sample of a filter only arms it: spent before the timed ticks
                if R:
                    for r in range(R):
                        ctx.fleet_run_staged(2 * n, [r], with_ekf=2)
                else:
                    ctx.run_staged(2 * n, 1, with_ekf=2)
                ctx.sync()
                armed = True
            t0 = time.perf_counter()
            if R:
                ctx.fleet_run_staged((k % 2) * n, list(range(R)), with_ekf=2)
            else:
                ctx.run_staged((k % 2) * n, 1, with_ekf=2)
            ctx.sync()
            ts.append(time.perf_counter() - t0)
        out[f"tick_{mode}_p50_us"], out[f"tick_{mode}_max_us"] = stats(ts[warm:])
        fused = ctx.get_slot_ekf_stats(((warm + reps - 1) % 2) * n, n)[:, 2]
        out[f"fused_per_filter_{mode}"] = round(float(fused.mean()), 2)
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="0,4,16,64")
    ap.add_argument("--landmarks", default="40,200")
    ap.add_argument("--caps", default="24,64")
    ap.add_argument("--modes", default="off,inf,default,all")
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
        for L in [int(x) for x in a.landmarks.split(",")]:
            for cap in [int(x) for x in a.caps.split(",")]:
                line = json.dumps(measure(R, L, cap, modes))
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
