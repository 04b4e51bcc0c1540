"""Gated-window measurements: frames/s of aslam_run_staged(with_ekf = 2) over batches of 320 injected frames on a dense
200-landmark map, 16 true sightings (noise 0.03) + 4 displaced by (2.7, -2.1, 0) per frame.  Legs:
  a  gate set, switch off: the per-frame path (the parent's behaviour under the gate)
  b  gate set (default), switch on: gated windows
  c  gate_d2 = inf, switch on
  d  no gate: the ungated windows

    python scripts/slam_gate_window_bench.py [--legs a,b,c,d] [--without-switch-api] [--batches 6] [--out FILE]

Prints one JSON line per leg (and appends it to --out): the median over the timed batches after one warm-up batch, the plan counters
and the rejections of the last batch.  Every batch starts from the same injected state (aslam_set_state outside the timed span); two
banks of landmarks alternate from frame to frame, so that no sighting finds a predecessor of its id in the frame before.
--without-switch-api binds a library built before the switch existed (ARUCO_SLAM_LIB names it): only leg a can run then."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from aruco_slam_amd import capi  # noqa: E402

TRUE, WRONG, L, B = 16, 4, 200, 320
OUTLIER = np.array([2.7, -2.1, 0.0])
SWITCH_API = ("aslam_set_slam_gate_windows", "aslam_get_slam_gate_windows")
WL, WR, DT = 2.0, 2.3, 1 / 30.0


def wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def state(rng):
    N = 3 + 3 * L
    mu = np.zeros(N)
    mu[:3] = [0.3, -0.2, 0.4]
    ang, rad = rng.uniform(0, 2 * math.pi, L), rng.uniform(1.0, 6.0, L)
    mu[3::3], mu[4::3], mu[5::3] = rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-3, 3, L)
    A = rng.standard_normal((N, 24)) * 0.05
    return mu, A @ A.T + np.diag(rng.uniform(0.01, 0.05, N))


def frames(mu, ids, rng):
    """B frames: bank f % 2 of 20 landmarks each (the two banks fit one window set of 40), seen from the pose the odometry predicts"""
    both = rng.permutation(L)[:2 * (TRUE + WRONG)]
    banks = [both[b::2] for b in range(2)]
    pose = mu[:3].copy()
    out = []
    for f in range(B):
        if f:
            dsl, dsr = 0.05 * DT * WL, 0.05 * DT * WR
            dth, ds = (dsr - dsl) / 0.18, 0.5 * (dsr + dsl)
            pose = np.array([pose[0] + ds * math.cos(pose[2] + 0.5 * dth), pose[1] + ds * math.sin(pose[2] + 0.5 * dth), wrap(pose[2] + dth)])
        sel = banks[f % 2]
        c, s = math.cos(pose[2]), math.sin(pose[2])
        dx, dy = mu[3 + 3 * sel] - pose[0], mu[4 + 3 * sel] - pose[1]
        z = np.stack([dx * c + dy * s, -dx * s + dy * c, wrap(mu[5 + 3 * sel] - pose[2])], 1) + rng.normal(0, 0.03, (sel.size, 3))
        z[TRUE:] += OUTLIER
        order = rng.permutation(sel.size)
        out.append((ids[sel][order], z[order], rng.uniform(0.02, 0.2, (sel.size, 3))[order]))
    return out


def measure(leg, batches):
    rng = np.random.RandomState(25)
    mu, S = state(rng)
    ids = rng.permutation(1024)[:L].astype(np.int32)
    fr = frames(mu, ids, rng)
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=B, max_landmarks=L, max_updates_per_frame=24)
    if leg in "abc":
        ctx.set_slam_gate(**(dict(gate_d2=float("inf")) if leg == "c" else {}))
    if leg in "bc":
        ctx.set_slam_gate_windows(True)
    for s, (i, z, rd) in enumerate(fr):
        ctx.inject_observations(s, i, np.ones(len(i), np.int32), z, rd)
    ctx.stage_encoders([0.0] + [WL] * (B - 1), [0.0] + [WR] * (B - 1), [0.0] + [DT] * (B - 1))
    ts = []
    for k in range(1 + batches):
        ctx.set_state(mu, S, ids)
        ctx.sync()
        ctx.profile_reset()
        t0 = time.perf_counter()
        ctx.run_staged(0, B, with_ekf=2)
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    st = ctx.get_slot_ekf_stats(0, B)
    out = dict(what="staged batch of 320 frames, with_ekf = 2, 200 landmarks, 16 + 4 sightings per frame", leg=leg,
               frames_per_s=round(B / float(np.median(ts[1:])), 1), batch_ms_p50=round(float(np.median(ts[1:])) * 1e3, 3),
               batch_ms_max=round(float(np.max(ts[1:])) * 1e3, 3), plan=list(ctx.plan_stats().values()), fused_per_frame=round(float(st[1:, 2].mean()), 2))
    if leg in "abc":
        out["rejected_per_frame"] = round(float(ctx.get_slot_health(0, B)["rejected"][1:].mean()), 2)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--without-switch-api", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    legs = a.legs.split(",")
    if a.without_switch_api:
        if legs != ["a"]:
            ap.error("--without-switch-api runs --legs a only")
        for name in SWITCH_API:
            capi._SIGS.pop(name, None)
    for leg in legs:
        line = json.dumps(measure(leg, a.batches))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
