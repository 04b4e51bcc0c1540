"""Landmark confirmation on the headline configuration (cfg2: 320 frames per batch, 20 markers per frame, a
200-landmark map): end-to-end frames/s with the switch off and on (3 repetitions each, interleaved, 50 batches behind 3 warm-up
batches) and the profile families of a pass with the switch on and of one with it off, per batch.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from aruco_slam_amd import capi, synth

args = argparse.Namespace(waves=0, reserve=0)
cfg, world, lap, ctx, frames, host = bench.scene_setup(np, capi, synth, "cfg2", 0, 0, args, True, 0)
ctx.run_staged(0, lap, with_ekf=True)
ctx.sync()
turn = world.frame(lap)
ctx.stage_encoders([turn.wl], [turn.wr], [turn.dt], slot0=0)
ctx.stage_encoders([turn.wl], [turn.wr], [turn.dt], slot0=lap)
B, steps = lap, 50
pos = [0]


def step():
    ctx.run_staged(pos[0], B, with_ekf=True)
    pos[0] = (pos[0] + B) % (2 * lap)


def timed():
    for _ in range(3):
        step()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    ctx.sync()
    return steps * B / (time.perf_counter() - t0)


out = {"batch": B, "steps": steps, "landmarks": int(world.L), "markers_per_frame": int(world.M), "fps_off": [], "fps_on": []}
for rep in range(3):
    ctx.set_landmark_confirmation(None)
    out["fps_off"].append(round(timed(), 1))
    ctx.set_landmark_confirmation()
    out["fps_on"].append(round(timed(), 1))
rec = ctx.get_slot_confirm(0, 2 * lap)
out["judged_per_slot"] = float(rec["judged"].mean()); out["withheld_total"] = int(rec["withheld"].sum())
st = ctx.get_slot_ekf_stats(0, 2 * lap)
out["fused_min"] = int(st[:, 2].min())
for name, on in (("profile_on", True), ("profile_off", False)):
    ctx.set_landmark_confirmation() if on else ctx.set_landmark_confirmation(None)
    ctx.profile_enable(True); ctx.profile_reset()
    for _ in range(steps):
        step()
    ctx.sync()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    out[name] = {k: {"calls": v[0], "ms_per_batch": round(v[1] / steps, 4)} for k, v in prof.items() if v[0]}
out["d2h_bytes_per_batch"] = B * 128 * 64 + 4 * B
print(json.dumps(out, indent=1))
