"""Pose ambiguity check on the headline configuration (cfg2: 320 frames per batch, 20 markers per frame): the profile
families k_pose and k_pose_alt on the same frames with the switch on, per batch of 320 frames and for the single-frame call, and how
many sightings the default parameters flag and reject on the cfg2 scene with its own detector profile and with the reference's
default detector parameters (counts from the slot sums only).  Prints one JSON object."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from aruco_slam_amd import capi, synth

args = argparse.Namespace(waves=0, reserve=0)
out = {}
for label, detector, qualify in (("cfg2_scene_detector", "scene", True), ("cfg2_reference_defaults", "reference", False)):
    cfg, world, lap, ctx, frames, host = bench.scene_setup(np, capi, synth, "cfg2", 0, 0, args, False, 0, detector=detector, qualify=qualify)
    ctx.set_pose_ambiguity()
    ctx.run_staged(0, lap, with_ekf=False)
    ctx.sync()
    sums = np.array([tuple(ctx.get_slot_pose_ambiguity(s)[1])[:3] for s in range(lap)])
    valid = sum(int(ctx.get_slot_raw_observations(s)[1].sum()) for s in range(lap))
    res = {"frames": lap, "params": ctx.get_pose_ambiguity(), "checked": int(sums[:, 0].sum()), "ambiguous": int(sums[:, 1].sum()),
           "rejected": int(sums[:, 2].sum()), "valid_after": valid}
    if detector == "scene":
        steps = 20
        ctx.profile_enable(True)
        for name, first, count in (("batch_320", 0, lap), ("single_frame", 7, 1)):
            ctx.profile_reset()
            for _ in range(steps):
                ctx.run_staged(first, count, with_ekf=False)
            ctx.sync()
            prof = ctx.profile_get()
            res[name] = {k: {"calls": prof[k][0], "us_per_call": round(1e3 * prof[k][1] / max(prof[k][0], 1), 2)} for k in ("k_pose", "k_pose_alt")}
            res[name]["ratio_alt_over_pose"] = round(prof["k_pose_alt"][1] / prof["k_pose"][1], 3)
        ctx.profile_enable(False)
    out[label] = res
    ctx.close()
print(json.dumps(out, indent=1))
