"""Where a detection waits for the EKF work that still reads its slots (aruco_slam_amd/csrc/capi.hip, run_detect).  A call that
reuses frame slots whose EKF work may still be in flight makes its detection stream wait for that work.  Of everything a detection
writes, the EKF stream's kernels read d_obs and d_nmarkers alone, and k_pose is the only kernel that writes them (the review of
every argument list is in DESIGN.md §4), so the wait stands in front of the call's first pose stage and the contour, quad and
identification stages run beside the older EKF work.  ASLAM_DETECT_WAIT_AT_HEAD (read at context creation) puts the wait back in
front of the call's first kernel.

The scene is the benchmark's pattern at the smallest size that still reuses slots under a filter in flight: 240 x 320 images, four
markers in view, two slot sets of 32 frames (one panel approach each, a closed tour of two panels), eight calls that alternate
between the sets, so that from the third call on every detection overwrites slots whose EKF work was enqueued two calls earlier.
One context is driven back to back, as the benchmark drives it; one is synchronised after every call, so that nothing is ever in
flight beside a detection.  A second pair runs with the wait at the head.  All four must leave the same bytes: the state, the
landmark ids, every slot's raw observations and detections, the slot statistics and the pop list.

This cannot make the race happen on purpose and is not meant to: the argument-list review is the proof that the slots are safe,
the test catches a wait that has gone missing or an order of kernels that changes what a slot holds."""
import dataclasses
import os

import numpy as np
import pytest

from aruco_slam_amd import capi, synth

ROWS, COLS, SET, CALLS = 240, 320, 32, 8
# cfg1's panels at half the image size; the step makes a panel approach exactly SET frames long, two panels close the tour
CFG = dataclasses.replace(synth.CONFIGS["cfg1"], rows=ROWS, cols=COLS, f=225.0, n_panels=2, step=(2.65 - 1.87) / (SET - 1) - 1e-6)
KNOB = "ASLAM_DETECT_WAIT_AT_HEAD"


def context():
    return capi.Context(max_rows=ROWS, max_cols=COLS, max_batch=2 * SET, persistent_waves=16, max_landmarks=16)


def drive(sync_every_call, at_head):
    world = synth.PanelWorld(CFG)
    assert world.M == 4 and world.lap_length() == 2 * SET
    saved = os.environ.get(KNOB)
    if at_head:
        os.environ[KNOB] = "1"
    else:
        os.environ.pop(KNOB, None)
    try:
        ctx = context()
    finally:
        if saved is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = saved
    ctx.set_camera(world.K, np.zeros(5))
    frames = [world.frame(i) for i in range(2 * SET)]
    for i, fr in enumerate(frames):
        ctx.synth_render(i, ROWS, COLS, world.K, fr.ids, fr.poses, noise_amp=2, seed=i, download=False)
    ctx.stage_encoders([f.wl for f in frames], [f.wr for f in frames], [f.dt for f in frames])
    turn = world.frame(2 * SET)                  # from the second lap on the first frame follows the turn that closes the tour
    per_call = []
    for call in range(CALLS):
        if call == 2:
            if not sync_every_call:
                ctx.sync()                       # (the encoder sample of slot 0 is rewritten once, between the laps: not a part of the pattern)
            ctx.stage_encoders([turn.wl], [turn.wr], [turn.dt], slot0=0)
        ctx.run_staged((call & 1) * SET, SET, with_ekf=True)
        if sync_every_call:
            ctx.sync()
            mu, S = ctx.get_state()
            per_call.append(mu.tobytes() + S.tobytes())
    ctx.sync()
    mu, S = ctx.get_state()
    out = dict(mu=mu.tobytes(), S=S.tobytes(), ids=ctx.get_landmark_ids().tobytes(), stats=ctx.get_slot_ekf_stats(0, 2 * SET).tobytes(),
               pops=b"".join(np.ascontiguousarray(a).tobytes() for a in ctx.get_observations()),
               raw=b"".join(np.ascontiguousarray(a).tobytes() for s in range(2 * SET) for a in ctx.get_slot_raw_observations(s)),
               det=b"".join(np.ascontiguousarray(a).tobytes() for s in range(2 * SET) for a in ctx.get_slot_detections(s)))
    seen = [set(frames[s].ids.tolist()) <= set(ctx.get_slot_raw_observations(s)[0].tolist()) for s in range(2 * SET)]
    plan = ctx.plan_stats()
    ctx.close()
    return out, per_call, seen, plan, mu.size


def check():
    ref, ref_calls, seen, plan, n = drive(sync_every_call=True, at_head=True)
    # the scene does what the pattern needs: every frame's four markers are found (at this size the white bar of a marker is now and
    # then read as id 1023 as well, the same in every run), both panels are mapped, the laps are fused inside windows
    assert all(seen) and n >= 3 + 3 * 8, f"{seen.count(False)} frames miss a marker, state of {n}"
    assert plan["windows"] >= CALLS and plan["frames_in_windows"] >= (CALLS - 2) * SET, plan
    assert len(set(ref_calls)) == CALLS, "a call left the filter where it was"
    for sync_every_call, at_head in ((False, True), (True, False), (False, False)):
        got, calls, _, _, _ = drive(sync_every_call, at_head)
        what = f"{'synchronised' if sync_every_call else 'back to back'}, wait {'at the head' if at_head else 'in front of the pose stage'}"
        for k in ref:
            assert got[k] == ref[k], f"{what}: {k} differs from the synchronised run with the wait at the head"
        if sync_every_call:
            assert calls == ref_calls, f"{what}: the state after a call differs"


def test_detect_wait_placement():
    check()


@pytest.mark.gpu
def test_detect_wait_placement_on_gpu():
    check()
