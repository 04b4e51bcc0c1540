"""SLAM relocalization measurements: wall time of one aslam_slam_relocalize(apply = 1) on a single SLAM filter with
L landmarks, and of one aslam_fleet_slam_relocalize(apply = 1) over R robots with 40 landmarks each; 20 observations per slot (14
sightings from the true pose, 6 wrong-id outliers).  Against the host route on the same filters: aslam_get_state (or
aslam_fleet_get_state) -> tests/slam_relocalize_reference.py -> aslam_set_state (aslam_fleet_set_state) per filter, whose two copies
are also timed on their own.

    python scripts/slam_relocalize_bench.py [--single 200,1000] [--robots 4,16,64] [--only device] [--out FILE]

Prints one JSON line per configuration (and appends it to --out): p50 and max over 20 timed calls after 3 warm-up calls, and the
device time of the two kernels from the library's own event profile.  --only device skips the host route (for a rocprofv3
--kernel-trace run)."""
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
from tests import slam_relocalize_reference as sref  # noqa: E402

FLEET_LANDMARKS, INLIERS, OUTLIERS = 40, 14, 6
KERNELS = ("k_slam_reloc_solve", "k_slam_reloc_seat")


def sighting(pose, lm, rng, noise=0.01):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    dx, dy = lm[0] - pose[0], lm[1] - pose[1]
    return np.array([dx * c + dy * s, -dx * s + dy * c, ref.wrap(lm[2] - pose[2])]) + rng.normal(0, noise, 3)


def random_filter(rng, L):
    """mu, Sigma (symmetric positive definite, the landmarks sharing a common-mode term), ids"""
    N = 3 + 3 * L
    ids = rng.permutation(1024)[:L].astype(np.int32)
    xyth = np.stack([rng.uniform(-5, 5, L), rng.uniform(-5, 5, L), rng.uniform(-math.pi, math.pi, L)], 1)
    A = rng.normal(size=(N, 64)) * 0.01
    S = A @ A.T + 1e-4 * np.eye(N)
    for k in range(3):
        u = np.zeros(N)
        u[3 + k::3] = 1.0
        S += 0.02 * np.outer(u, u)
    return np.concatenate([np.zeros(3), xyth.reshape(-1)]), 0.5 * (S + S.T), ids, xyth


def install(ctx, slot, ids, xyth, rng):
    """slot's 20 observations; returns the true pose"""
    L = len(ids)
    truth = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3, 3)])
    sel = rng.permutation(L)[:INLIERS + OUTLIERS]
    label = sel.copy()
    label[INLIERS:] = np.roll(sel[INLIERS:], 1)                          # an outlier: one landmark reported under another's id
    order = rng.permutation(INLIERS + OUTLIERS)
    z = np.array([sighting(truth, xyth[li], rng) for li in sel])
    ctx.inject_observations(slot, ids[label][order], np.ones(len(sel), np.int32), z[order], rng.uniform(0.01, 0.05, (len(sel), 3)))
    return truth


def slot_obs(ctx, slot):
    i, v, z, rd = ctx.get_slot_raw_observations(slot)
    return [(int(i[k]), int(v[k]), z[k], rd[k]) for k in range(len(i))]


def stats(ts):
    return round(float(np.percentile(ts, 50)) * 1e6, 1), round(float(np.max(ts)) * 1e6, 1)


def timed(fn, reps, warm):
    ts, out = [], None
    for _ in range(warm + reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts[warm:], out


def kernel_us(ctx, fn, reps):
    """device time per call of the two kernels, from the library's event profile"""
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(reps):
        fn()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    return {k: round(prof[k][1] * 1e3 / max(prof[k][0], 1), 1) for k in KERNELS}


def measure(R, L, only_device, reps=20, warm=3):
    """R = 0: the single filter; else a SLAM fleet of R robots"""
    rng = np.random.RandomState(1000 * R + L)
    n = max(R, 1)
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=n, max_landmarks=L)
    filt = [random_filter(rng, L) for _ in range(n)]
    if R:
        cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
        ctx.fleet_slam_begin([cam] * R)
        get = lambda r: ctx.fleet_get_state(r)                                        # noqa: E731
        put = lambda r, mu, S: ctx.fleet_set_state(r, mu, S, filt[r][2])               # noqa: E731
        call = lambda: ctx.fleet_slam_relocalize(0, list(range(R)), apply=True)        # noqa: E731
    else:
        get = lambda r: ctx.get_state()                                               # noqa: E731
        put = lambda r, mu, S: ctx.set_state(mu, S, filt[0][2])                        # noqa: E731
        call = lambda: np.array([ctx.slam_relocalize(0, apply=True)])                  # noqa: E731
    truth = []
    for r in range(n):
        put(r, filt[r][0], filt[r][1])
        truth.append(install(ctx, r, filt[r][2], filt[r][3], rng))
    truth = np.array(truth)
    ts, got = timed(call, reps, warm)
    d = got["pose"] - truth
    d[:, 2] = [ref.wrap(a) for a in d[:, 2]]
    out = dict(what="fleet_slam_relocalize" if R else "slam_relocalize", robots=R, landmarks=L, N=3 + 3 * L,
               observations_per_slot=INLIERS + OUTLIERS, solved=int((got["status"] == 0).sum()),
               mean_inliers=round(float(got["n_inliers"].mean()), 2), worst_to_truth_m=round(float(np.hypot(d[:, 0], d[:, 1]).max()), 4))
    out["device_p50_us"], out["device_max_us"] = stats(ts)
    out["kernel_us"] = kernel_us(ctx, call, 5)
    if not only_device:
        def copies():
            for r in range(n):
                mu, S = get(r)
                put(r, mu, S)

        def route():
            res = []
            for r in range(n):
                mu, S = get(r)
                w = sref.relocalize(mu, S, filt[r][2], slot_obs(ctx, r))
                if w["status"] == 0:
                    put(r, w["mu_new"], w["Sigma_new"])
                res.append(w)
            return res

        cs, _ = timed(copies, reps, warm)
        out["host_copies_p50_us"], out["host_copies_max_us"] = stats(cs)
        for r in range(n):                                                            # the route starts where the device call started
            put(r, filt[r][0], filt[r][1])
        hs, want = timed(route, 3 if L >= 500 else reps, 1 if L >= 500 else warm)
        out["host_route_p50_us"], out["host_route_max_us"] = stats(hs)
        want0 = [sref.relocalize(filt[r][0], filt[r][1], filt[r][2], slot_obs(ctx, r)) for r in range(n)]
        for r in range(n):
            put(r, filt[r][0], filt[r][1])
        got0 = call()
        dp = np.array([g - w["pose"] for g, w in zip(got0["pose"], want0)])
        dp[:, 2] = [ref.wrap(a) for a in dp[:, 2]]
        out.update(max_abs_diff_pose=float(np.abs(dp).max()),
                   max_rel_diff_sigma=float(max(np.abs(g - w["sigma"]).max() / np.abs(w["sigma"]).max() for g, w in zip(got0["sigma"], want0)
                                                if w["status"] == 0)),
                   same_counts=bool(all(int(g[k]) == int(w[k]) for g, w in zip(got0, want0) for k in ("status", "n_inliers", "runner_up", "best"))))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", default="200,1000")
    ap.add_argument("--robots", default="4,16,64")
    ap.add_argument("--only", choices=["device"])
    ap.add_argument("--out")
    a = ap.parse_args()
    configs = [(0, int(x)) for x in a.single.split(",") if x] + [(int(x), FLEET_LANDMARKS) for x in a.robots.split(",") if x]
    for R, L in configs:
        line = json.dumps(measure(R, L, a.only == "device"))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
