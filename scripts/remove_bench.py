"""Landmark-removal measurements: wall time of aslam_remove_landmarks, its final wait included, against the host
route through the same binding (get_state, numpy.delete of the rows and columns, set_state), and of one aslam_fleet_remove_landmarks
over R robots against R single calls.

    python scripts/remove_bench.py [--sizes 200,1000] [--fleets 16,64] [--out FILE] [--timeout SECONDS]

Every case (one size, or one fleet) runs in a child process of its own under a time limit, one after the other; the first one that
fails or runs out of time ends the run.  A case prints one JSON line per removal set (and appends it to --out): p50 and max over
20 timed calls after 3 warm-up calls, every call on a state seeded again outside the timed region, device route and host route in
the same process.  The device time of a call is what aslam_profile_get reports for the three kernels in 5 further calls, and the
bandwidth is that of the two Sigma passes, 2 * 2 * 8 * N^2 bytes (each reads and writes at most N^2 doubles) over it."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from aruco_slam_amd import capi, synth  # noqa: E402

REPS, WARM, PROFILED = 20, 3, 5
KERNELS = ("k_map_plan", "k_map_cols", "k_map_rows")


def stats(ts):
    return round(float(np.percentile(ts, 50)) * 1e6, 1), round(float(np.max(ts)) * 1e6, 1)


def state(rng, L):
    N = 3 + 3 * L
    S = rng.uniform(-1e-3, 1e-3, (N, N))
    S = np.asfortranarray(S + S.T + 0.05 * np.eye(N))
    return rng.uniform(-3, 3, N), S, rng.permutation(1024)[:L].astype(np.int32)


def removal_sets(ids):
    L = len(ids)
    return {"first": ids[:1], "10_percent": ids[:: 10], "50_percent": ids[:: 2]} if L >= 10 else {"first": ids[:1]}


def host_route(ctx, remove):
    mu, S = ctx.get_state()
    ids = ctx.get_landmark_ids()
    gone = np.flatnonzero(np.isin(ids, remove))
    rows = (3 + 3 * gone[:, None] + np.arange(3)[None, :]).ravel()
    ctx.set_state(np.delete(mu, rows), np.delete(np.delete(S, rows, 0), rows, 1), np.delete(ids, gone))
    return len(gone)


def single_case(ML):
    rng = np.random.RandomState(ML)
    mu, S, ids = state(rng, ML)
    N = mu.size
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=2, max_landmarks=ML)
    for name, remove in removal_sets(ids).items():
        out = dict(what="remove landmarks, single filter", max_landmarks=ML, N=N, set=name, removed=int(len(remove)))
        for route in ("device", "host"):
            ts = []
            for k in range(WARM + REPS):
                ctx.set_state(mu, S, ids)
                ctx.sync()
                t0 = time.perf_counter()
                n = ctx.remove_landmarks(remove) if route == "device" else host_route(ctx, remove)
                ts.append(time.perf_counter() - t0)
                assert n == len(remove)
            out[f"{route}_p50_us"], out[f"{route}_max_us"] = stats(ts[WARM:])
        out["host_over_device"] = round(out["host_p50_us"] / out["device_p50_us"], 2)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for k in range(PROFILED):
            ctx.set_state(mu, S, ids)
            ctx.remove_landmarks(remove)
        ctx.sync()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        for kname in KERNELS:
            calls, ms = prof[kname]
            assert calls == PROFILED
            out[f"{kname}_us"] = round(1e3 * ms / calls, 1)
        dev_us = sum(out[f"{k}_us"] for k in KERNELS)
        out["device_time_us"] = round(dev_us, 1)
        out["sigma_passes_GBps"] = round(2 * 2 * 8 * N * N / (dev_us * 1e-6) / 1e9, 1)
        print(json.dumps(out), flush=True)
    ctx.close()


def fleet_case(R, ML=64):
    rng = np.random.RandomState(R)
    states = [state(rng, ML) for _ in range(R)]
    remove = np.unique(np.concatenate([st[2][::4] for st in states[:4]]))       # about a quarter of the first robots' maps, less of the others'
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    fl = capi.Context(max_rows=64, max_cols=64, max_batch=R, max_landmarks=ML)
    fl.fleet_slam_begin([cam] * R)
    one = capi.Context(max_rows=64, max_cols=64, max_batch=2, max_landmarks=ML)
    t_fleet, t_loop = [], []
    for k in range(WARM + REPS):
        for r, st in enumerate(states):
            fl.fleet_set_state(r, *st)
        fl.sync()
        t0 = time.perf_counter()
        removed = fl.fleet_remove_landmarks(remove)
        t_fleet.append(time.perf_counter() - t0)
        total, looped = 0.0, []
        for st in states:
            one.set_state(*st)
            one.sync()
            t0 = time.perf_counter()
            looped.append(one.remove_landmarks(remove))
            total += time.perf_counter() - t0
        t_loop.append(total)
        assert removed.tolist() == looped
    out = dict(what="remove landmarks, SLAM fleet", robots=R, max_landmarks=ML, ids=int(len(remove)), removed_total=int(removed.sum()))
    out["fleet_call_p50_us"], out["fleet_call_max_us"] = stats(t_fleet[WARM:])
    out["single_calls_looped_p50_us"], out["single_calls_looped_max_us"] = stats(t_loop[WARM:])
    out["looped_over_fleet"] = round(out["single_calls_looped_p50_us"] / out["fleet_call_p50_us"], 2)
    print(json.dumps(out), flush=True)
    fl.close()
    one.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,1000", help="max_landmarks of the single-filter cases (N = 3 + 3 max_landmarks: a full map)")
    ap.add_argument("--fleets", default="16,64", help="robots of the fleet cases (max_landmarks 64)")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=240, help="time limit of one case, seconds")
    ap.add_argument("--case", help="internal: run this one case (single:ML or fleet:R) in this process")
    a = ap.parse_args()
    if a.case:
        kind, n = a.case.split(":")
        (single_case if kind == "single" else fleet_case)(int(n))
        return 0
    cases = [f"single:{int(x)}" for x in a.sizes.split(",") if x] + [f"fleet:{int(x)}" for x in a.fleets.split(",") if x]
    for case in cases:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"case {case}: no result within {a.timeout} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if a.out and p.stdout:
            with open(a.out, "a") as f:
                f.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print(f"case {case}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
