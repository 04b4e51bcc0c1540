"""Consistent innovations inside EKF windows: what the windows win back.

fps: the headline workload (cfg2, 320 frames per step, one lap already mapped, 20 steps per leg, one process), the legs of
scripts/consistent_bench.py --only fps with the consistent window between them:
    frozen windows | consistent per-frame | consistent windows | frozen windows again
first without a SLAM gate, then the same legs with the SLAM gate at its defaults and gated windows on.  In the gated half the
consistent_windows leg documents the fallback (the gated consistent window has a switch of its own, so that leg shows the per-frame path
again; its plan says so), and a fifth leg, consistent_gated_windows, follows it with aslam_set_gated_consistent_windows on (DESIGN.md
§37).  A consistent windowed rate is to be compared with the consistent per-frame rate of the same run, and the spread between the two
frozen legs is the run's noise: the gated consistent window passes if it beats consistent_per_frame by more than that spread.

lap: §32's experiment (localization on the true map of the rendered ring of cfg2_sliding, observation covariance on, innovation gate
at +inf, consistent innovations on) with the windows switch off and on.  Localization has no windows: the two rows must agree.

    python scripts/consistent_windows_bench.py [--only {fps,lap}] [--out FILE]

Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import consistent_bench  # noqa: E402
from aruco_slam_amd import capi, synth  # noqa: E402

LEGS = (("frozen_windows", False, False, False), ("consistent_per_frame", True, False, False), ("consistent_windows", True, True, False),
        ("consistent_gated_windows", True, True, True), ("frozen_windows_again", False, False, False))


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
    for gated in (False, True):
        if gated:
            ctx.set_slam_gate()
            ctx.set_slam_gate_windows(True)
        legs = {}
        for name, consistent, windows, gated_consistent in LEGS:
            if gated_consistent and not gated:
                continue
            ctx.set_consistent_innovations(consistent)
            ctx.set_consistent_windows(windows)
            ctx.set_gated_consistent_windows(gated_consistent)
            ctx.set_state(mu, S, ids)
            before = ctx.plan_stats()
            for k in range(warmup):
                ctx.run_staged((k & 1) * lap, lap, with_ekf=True)
            ctx.sync()
            t0 = time.perf_counter()
            for k in range(steps):
                ctx.run_staged(((k + warmup) & 1) * lap, lap, with_ekf=True)
            ctx.sync()
            el = time.perf_counter() - t0
            after = ctx.plan_stats()
            legs[name] = {"frames_per_s": round(steps * lap / el, 1), "plan": {k: after[k] - before[k] for k in after}}
        a, b = legs["frozen_windows"]["frames_per_s"], legs["frozen_windows_again"]["frames_per_s"]
        pf, cw = legs["consistent_per_frame"]["frames_per_s"], legs["consistent_windows"]["frames_per_s"]
        legs["frozen_spread"] = round(abs(a - b), 1)
        legs["windows_over_per_frame"] = round(cw / pf, 3)
        legs["gap_to_frozen_windows"] = round(1.0 - cw / (0.5 * (a + b)), 4)
        if gated:
            gc = legs["consistent_gated_windows"]
            gc["over_consistent_per_frame"] = round(gc["frames_per_s"] / pf, 3)
            gc["gap_to_frozen_windows"] = round(1.0 - gc["frames_per_s"] / (0.5 * (a + b)), 4)
            gc["every_frame_in_windows"] = (gc["plan"]["frames_per_frame_chain"] == 0 and gc["plan"]["frames_device_planned"] == 0
                                            and gc["plan"]["frames_in_windows"] == (steps + warmup) * lap)
            gc["beats_per_frame_by_more_than_the_spread"] = gc["frames_per_s"] - pf > legs["frozen_spread"]
        res["gated" if gated else "ungated"] = legs
    ctx.close()
    return res


def lap(windows):
    """consistent_bench.lap_run(True) with the windows switch set on every context it makes"""
    make = capi.Context

    def context(*a, **kw):
        ctx = make(*a, **kw)
        ctx.set_consistent_windows(windows)
        return ctx

    capi.Context = context
    try:
        out = consistent_bench.lap_run(True)
    finally:
        capi.Context = make
    out["consistent_windows"] = bool(windows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["fps", "lap"], default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {}
    if a.only in ("", "fps"):
        out["fps"] = fps()
    if a.only in ("", "lap"):
        out["lap"] = [lap(False), lap(True)]
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
