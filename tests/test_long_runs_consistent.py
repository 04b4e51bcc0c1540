"""Runs of thousands of frames with consistent innovations on: every SLAM chain and the consistent windows against the consistent
literal reference after every call, and localization laps across the heading wrap.

tests/test_long_runs.py (§27) never sets either consistent switch.  This file runs its world, batch schedule (1, 7, 64, 33, 2, 50,
cycled) and context sizes (max_batch 64, persistent_waves 4, 64 x 64 image) with aslam_set_consistent_innovations on before the first
call.  The references are in tests/long_run_world.py: consistent_reference_run (plan_reference.PlanReference on
consistent_reference.ConsistentLiteral: double, dense literal products, e_i = ze_i - Gx (mu_{i-1} - mu_0) with mu_0 taken at the
start of every frame) and consistent_gated_reference_run (ConsistentLiteral under the SLAM gate); consistent_long_double_tail restates
the corrections behind the map build with consistent_reference.consistent_step in long double and gives the floor.

  case  chain / path                                  stream                              switches
  cA    fast per-frame (k_ekf_mid RunningMean)        A's (L 12, m 4, cap 24, seed 1)     windows off
  cB    consistent windows, SP 64                     A's                                 consistent windows on; twin: cA's context
  cC    mid per-frame (k_ekf_mid64, k_ekf_T, MFMA)    C's (L 40, m 26, cap 64)            windows off
  cD    consistent windows, SP 128, sliding sets      D's (L 48, m 26, ML 49)             consistent windows on; twin: per-frame, cap 64
  cE    general (k_ekf_gather, k_ekf_small, ...)      E's (L 48, m 33, cap 128)           windows off
  cF    fleet SLAM, 3 robots, mid chain               F's three streams                   -
  cG    SLAM gate gate_d2 = 1, outlier every 53rd     G's                                 gate, gated windows and consistent windows all on
  cH    fleet SLAM, 3 robots, mid chain, gate_d2 = 1  F's streams, outlier every 53rd     gate on (k_ekf_mid64<EkfFleet, SlamGate, RunningMean>)
  hB    consistent windows, SP 64, honest R           A's draws, R = NOISE^2              consistent windows on; twin: per-frame
  hD    consistent windows, SP 128, honest R          D's draws, R = NOISE^2              consistent windows on
  hG    fast per-frame, gate 16.266, honest R         G's draws, R = NOISE^2              gate on, windows off

The gated consistent window is not built (§33, Dropped): cG sets every window switch and asserts after every call that no window was
planned and that the fast per-frame chain's kernels ran.  cG and hG pin that per-frame fallback.  With honest R = (4e-6, 4e-6, 1e-6)
the gains are of order one and H (mu - mu_0) is as large as the innovation itself.

After EVERY call, with ==: L and the landmark ids, every slot's statistics, the overflow mask (sync raises on one), the pop list of the
call's last frame (single contexts), the kernel set (per-frame cases), the planner's identity frames_in_windows +
frames_per_frame_chain = 1 + frames so far and a new window in every call of more than one frame behind the map build (cB, cD, hB, hD),
slot and track records (cG, cH, hG; cH: every robot's).  Numeric: mu at rtol 1e-9 / atol 1e-11 and Sigma at 1e-9 relative (the
project's bars), the per-case bounds TOL below, the asymmetry of Sigma, and the smallest eigenvalue of (Sigma + Sigma^T) / 2 positive
wherever the reference's exceeds 1e-6 max|Sigma_ref| (§27's fixed 1e-7 would be vacuous with honest R, where the reference's smallest
eigenvalue is of order 1e-9).  cB, hB and cD are also compared after every call with a per-frame consistent twin context on the same
stream at 1e-10 relative in mu and Sigma (§33's bar); the test prints the twin difference per call and its largest value in the first
and in the last quarter of the calls behind the map build.  At the end of a windowed case: at least 90 % of the frames behind the map
build ran inside windows, k_ekf_win_step launches = plan_stats()["windows"], and at 2 000 frames k_ekf_win_next ran (cD, hD) and at least
one frame whose predict wraps the heading lay in a call behind the map build that ran entirely inside windows.  The 200-frame prefix
holds one wrap (frame 79), which in both windowed streams lies no later than the call that completes the map (A's at frame 105; D's at
frame 72, in the call of frames 72 .. 104); the wrap inside a window is therefore asserted on the 2 000-frame runs only.

On the references alone, before any device run: the map is complete within the first lap; every later frame fuses exactly m corrections
less its rejections; the consistent and the frozen literal run of the same stream differ in mu by more than SWITCH_MIN = 1e-6 at the end
of every call behind the map build; assert_margins at 1e-6 on every d2 and ||ze|| compared; cG and cH reject exactly the planted
outliers and hG every planted outlier (whatever else it rejects the device must reproduce); the track is never lost; the reference's
smallest eigenvalue exceeds 1e-6 max|Sigma|.

Lengths.  Marked gpu: 2 000 frames.  On the session's library: the first 200 frames (the whole map build and the first wrap).

Measured worst values over all 78 calls of 2 000 frames, seeds as committed (|dmu| / Sigma relative / asymmetry of the device's Sigma;
floor = the double consistent literal against consistent_long_double_tail, |dmu| / Sigma; the reference's own asymmetry; seconds inside
the calls on the MI355X).  TOL is 10 x the larger of the measured values (§27's rule).  The emulation ran 2 000 frames once, outside the
suite, for the L 12 cases; for the L >= 40 cases it ran the 200-frame prefix only (marked p: 2 000 frames of them did not finish on
the development machine), so their TOL is 10 x the MI355X value, and their floors are the prefix's too.

  case  emulation                         MI355X                          floor                  reference asym.  MI355X s
  cA    2.49e-14 / 8.92e-15 / 1.88e-16    2.49e-14 / 8.92e-15 / 3.22e-16  2.46e-14 / 9.15e-15    1.00e-14         0.11
  cB    1.11e-14 / 1.02e-14 / 8.12e-15    1.11e-14 / 9.95e-15 / 7.60e-15  2.46e-14 / 9.15e-15    1.00e-14         0.03
  cC    1.51e-14 / 2.35e-14 / 3.35e-15 p  4.88e-14 / 3.55e-14 / 3.12e-14  1.25e-14 / 7.46e-15 p  2.93e-14         0.27
  cD    1.07e-14 / 1.17e-14 / 3.43e-15 p  2.62e-14 / 3.40e-14 / 3.93e-14  1.22e-14 / 5.32e-15 p  2.99e-14         0.10
  cE    1.38e-14 / 2.44e-14 / 4.82e-15 p  7.37e-14 / 4.00e-14 / 3.61e-14  1.20e-14 / 8.86e-15 p  3.51e-14         3.64
  cF    1.64e-14 / 2.35e-14 / 3.68e-15 p  5.51e-14 / 3.88e-14 / 3.12e-14  1.25e-14 / 7.46e-15 p  3.23e-14         0.28
  cG    2.00e-14 / 9.94e-15 / 1.92e-16    2.04e-14 / 9.76e-15 / 2.71e-16  2.05e-14 / 8.85e-15    6.15e-15         0.15
  cH    2.13e-14 / 2.54e-14 / 3.51e-15 p  5.37e-14 / 3.57e-14 / 3.11e-14  2.07e-14 / 6.96e-15 p  3.04e-14         0.36
  hB    1.02e-14 / 1.22e-12 / 1.69e-13    9.77e-15 / 1.77e-13 / 1.75e-13  1.66e-14 / 8.24e-15    7.20e-15         0.03
  hD    1.29e-14 / 3.84e-13 / 7.10e-13 p  3.15e-14 / 8.61e-13 / 1.55e-12  1.29e-14 / 8.55e-15 p  3.75e-14         0.10
  hG    1.87e-14 / 3.47e-14 / 2.56e-15    1.87e-14 / 3.54e-14 / 2.47e-15  1.51e-14 / 6.67e-15    1.13e-14         0.15

Twin difference (largest in the first / in the last quarter of the calls behind the map build, MI355X): cB 5.6e-15 / 8.0e-15, cD 1.8e-14 /
3.5e-14, hB 1.0e-13 / 9.6e-14 (emulation: cB 5.3e-15 / 8.1e-15, hB 2.3e-13 / 1.2e-13): no growth by a factor of 10, as §33's induction
predicts.  Wrap frames inside windows, 2 000 frames, all four windowed cases: 236, 394, 552, 710, 867, 1025, 1183, 1341, 1499, 1657, 1814,
1972 (every wrap behind the map build; 1 881 of 1 893 frames (cB, hB) and 1 883 of 1 895 (cD, hD) ran inside windows, 71 and 96 windows,
12 hand-overs in cD and hD).

Errors above 2 x their floor.  (1) hB and hD, Sigma and its asymmetry (1.8e-13 .. 1.6e-12): this file found a defect here and what is
left is its bounded remainder.  The window chain updates P <- P - c^T S^-1 c with c = H P read from rows of P, which adds a symmetric
matrix only while S^-1 is symmetric; S = c H^T + R formed from those rows carries H A H^T of P's antisymmetric part A, and through S^-1
every correction added (K H) A (K H)^T to A.  With stock R (K H of order 1e-2) that is §27's "growing slowly"; with honest R (K H of order
one) A doubled per correction in the observed directions: hB reached 3.8e-10 of max|Sigma| after 627 frames on the MI355X (twin bar
1e-10 missed in call 23) and 1.1e-9 on the emulation (the project's bar missed in the same call).  k_ekf_win_step now inverts S from
one triangle (both waves that form S^-1), so A is no longer fed back: it stays what rounding left while the map was built, when
max|Sigma| was 80 times larger, and no longer grows (hB: 1.6e-13 after 385 frames, 1.7e-13 after 1 955).  (2) hG, Sigma 3.5e-14 against
a floor of 6.7e-15: the fast chain fuses a frame's corrections in one joint solve, whose rounding at gains of order one differs from the
sequential literal's; constant over the run.  (3) cC .. cH at 2 000 frames stand against prefix floors; §27 measured 5e-14 / 2.3e-14 ..
3.5e-14 for the same streams' frozen runs at 2 000 frames, which these values lie within 2 x of.

The test can fail (scratch copies, emulation build, prefix): with the heading column of mu - mu_0 lost in win_running_innovation cB fails
in call 1 (mu differs by 1.52e-6) and hB by 1.29e-3; with k_ekf_mid's ungated RunningMean solve forming the frozen pseudo-innovation again (the H (mu - mu_0)
term dropped) cA fails in call 1 (1.11e-6); the unfixed window chain fails hB at 2 000 frames (above).

Localization laps (the second half of the file): the ring world L 12, m 4 as a fixed, true map, 320 frames (two laps, two heading
wraps) in calls of the same schedule, stock and honest R, consistent innovations on: (a) localize_begin against ConsistentLocalizer,
(b) localize_begin_uncertain (spd_blocks at 0.03) against ConsistentUmapLocalizer, (c) a fleet of 3 on the one map, (d) (a) under the
default innovation gate with an outlier every 53rd frame.  The three robots of (c) need one world, so they cannot take F's three
phases (a phase turns the world): they start at F's phases as headings (0, 0.7, 1.9) in the one world, each against its own
ConsistentLocalizer.  After every call: slot statistics and pop logs with ==, pose and pose covariance with test_innovation_gate.close
/ test_uncertain_map.check_single, (d) health and track records; one k_loc_steps / k_fleet_steps launch per call and no SLAM chain
kernel.  On the references alone: assert_margins, the consistent and the frozen localizer differ in the pose by more than 1e-6 at the
end of every call, (d) never sets `lost`.
"""
import copy
import functools
import math
import os
import time

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from consistent_reference import ConsistentLocalizer, ConsistentUmapLocalizer
from ekf_reference import CHAIN_KERNELS, ekf_kernels_run, rel_err
from long_run_world import (HONEST_R, LAP, MAX_BATCH, OUTLIER_FROM, RDIAG, asymmetry, batches_of, consistent_gated_reference_run,
                            consistent_long_double_tail, consistent_reference_run, first_complete_batch, gated_reference_run, min_eig,
                            reference_run, ring_stream)
from slam_gate_reference import DEFAULTS, check_slot_health, check_track
from tests.gate_reference import GatedLocalizer
from tests.gate_reference import check_slot_health as check_loc_health
from tests.gate_reference import check_track as check_loc_track
from tests.test_innovation_gate import close
from tests.test_localize import SIG0
from tests.test_localize import inject as inject_loc
from tests.test_uncertain_map import check_single, spd_blocks
from tests.umap_reference import UncertainMapLocalizer

GPU_FRAMES, EMU_FRAMES = 2000, 200
OUTLIER_EVERY = 53
EIG_REL = 1e-6                                       # the eigenvalue check holds where the reference's exceeds EIG_REL max|Sigma_ref|
SWITCH_MIN = 1e-6                                    # the consistent and the frozen reference differ by more than this in mu
TWIN_TOL = 1e-10
FINISH = "k_ekf_gate_finish"
CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
F_STREAMS = ((2, 0.0), (12, 0.7), (22, 1.9))

# streams = (seed, phase) per robot; gate = gate_d2 of the SLAM gate; twin = a per-frame consistent context run beside the windows
CASES = {
    "cA": dict(chain="fast", cap=24, windows=False, L=12, m=4, ML=12, streams=((1, 0.0),)),
    "cB": dict(chain="fast", cap=24, windows=True, L=12, m=4, ML=12, streams=((1, 0.0),), twin=True),
    "cC": dict(chain="mid", cap=64, windows=False, L=40, m=26, ML=40, streams=((2, 0.0),)),
    "cD": dict(chain="mid", cap=64, windows=True, L=48, m=26, ML=49, streams=((3, 0.0),), slides=True, twin=True),
    "cE": dict(chain="general", cap=128, windows=False, L=48, m=33, ML=49, streams=((3, 0.0),)),
    "cF": dict(chain="mid", cap=64, windows=False, L=40, m=26, ML=40, streams=F_STREAMS, fleet=True),
    "cG": dict(chain="fast", cap=24, windows=False, L=12, m=4, ML=12, streams=((1, 0.0),), gate=1.0, all_switches=True),
    "cH": dict(chain="mid", cap=64, windows=False, L=40, m=26, ML=40, streams=F_STREAMS, fleet=True, gate=1.0),
    "hB": dict(chain="fast", cap=24, windows=True, L=12, m=4, ML=12, streams=((1, 0.0),), R=HONEST_R, twin=True),
    "hD": dict(chain="mid", cap=64, windows=True, L=48, m=26, ML=49, streams=((3, 0.0),), slides=True, R=HONEST_R),
    "hG": dict(chain="fast", cap=24, windows=False, L=12, m=4, ML=12, streams=((1, 0.0),), gate=DEFAULTS["gate_d2"], R=HONEST_R),
}

# Bounds on the worst error over all calls: (|dmu|, Sigma relative, asymmetry of the device's Sigma), 10 x the larger of the two
# values measured at 2 000 frames (MEASURED); all far below the project's 1e-9, which is asserted as well
TOL = {"cA": (2.5e-13, 8.9e-14, 3.2e-15), "cB": (1.1e-13, 1.0e-13, 8.1e-14), "cC": (4.9e-13, 3.6e-13, 3.1e-13), "cD": (2.6e-13, 3.4e-13, 3.9e-13),
       "cE": (7.4e-13, 4.0e-13, 3.6e-13), "cF": (5.5e-13, 3.9e-13, 3.1e-13), "cG": (2.0e-13, 9.9e-14, 2.7e-15), "cH": (5.4e-13, 3.6e-13, 3.1e-13),
       "hB": (1.0e-13, 1.2e-11, 1.8e-12), "hD": (3.2e-13, 8.6e-12, 1.6e-11), "hG": (1.9e-13, 3.5e-13, 2.6e-14)}


def context(c, windows):
    R = len(c["streams"])
    kw = dict(max_rows=64, max_cols=64, max_batch=(MAX_BATCH + 1) * R if c.get("fleet") else MAX_BATCH, persistent_waves=4,
              max_landmarks=c["ML"], max_updates_per_frame=c["cap"])
    if windows or c.get("fleet"):
        return capi.Context(**kw)
    os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        return capi.Context(**kw)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)


def inject(ctx, slot, obs):
    ctx.inject_observations(slot, [o[0] for o in obs], [o[1] for o in obs], np.array([o[2] for o in obs]).reshape(-1, 3),
                            np.array([o[3] for o in obs]).reshape(-1, 3))


def streams_of(c, frames):
    return [ring_stream(c["L"], c["m"], frames, seed, phase, OUTLIER_EVERY if c.get("gate") else 0, c.get("R", RDIAG)) for seed, phase in c["streams"]]


def references(name, frames):
    """the case's streams, batches and consistent references, with the conditions on the references alone"""
    c = CASES[name]
    batches = batches_of(frames)
    streams = streams_of(c, frames)
    gate = c.get("gate")
    # the frozen runs the consistent ones are told apart from: of every robot in the prefix, of robot 0 alone at 2 000 frames (a literal
    # run of a fleet stream takes 10 s there)
    told = streams if frames <= EMU_FRAMES else streams[:1]
    if gate is None:
        refs = [consistent_reference_run(s, c["ML"], c["cap"], batches) for s in streams]
        frozen = [reference_run(s, c["ML"], c["cap"], batches) for s in told]
    else:
        refs = [consistent_gated_reference_run(s, batches, gate) for s in streams]          # (asserts its margins at 1e-6)
        frozen = [consistent_gated_reference_run(s, batches, gate, consistent=False) for s in told]
    for r, (s, ref) in enumerate(zip(streams, refs)):
        who = f"{name}, robot {r}"
        assert ref["complete"] is not None and ref["complete"] < LAP, f"{who}: the map is not complete within the first lap"
        assert sum(st[1] for st in ref["stats"]) == c["L"] and all(st[3] == 0 for st in ref["stats"]) and not any(ref["mask"])
        rejected = ref.get("rejected", {})
        for f in range(ref["complete"] + 1, frames):
            assert ref["stats"][f] == [c["m"], 0, c["m"] - len(rejected.get(f, ())), 0], f"{who}: frame {f} fused {ref['stats'][f]}"
        if gate is not None:
            assert len(s.outliers) == sum(1 for f in range(OUTLIER_FROM, frames) if f % OUTLIER_EVERY == 0) >= 2 and min(s.outliers) > ref["complete"]
            if name == "hG":                                       # honest R: true sightings are rejected too; the planted ones all are
                assert all(i in rejected.get(f, ()) for f, i in s.outliers.items()), f"{who}: the reference rejects {rejected}"
            else:
                assert rejected == {f: [i] for f, i in s.outliers.items()}, f"{who}: the reference rejects {rejected}"
            assert not any(t["lost"] for t in ref["track"]), f"{who}: the reference loses its track"
        k0 = first_complete_batch(ref, batches)
        assert len(batches) > k0 + 1
        for k in range(k0, len(batches)):
            mu, S = ref["states"][k]
            assert min_eig(S) > EIG_REL * np.abs(S).max(), f"{who}, call {k}: the reference's smallest eigenvalue is {min_eig(S)}"
        if r >= len(frozen):
            continue
        fro = frozen[r]
        k1 = max(k0, first_complete_batch(fro, batches))
        sep = [float(np.abs(ref["states"][k][0] - fro["states"][k][0]).max()) for k in range(k1 + 1, len(batches))
               if ref["ids"][k] == fro["ids"][k]]
        print(f"{who}: the consistent and the frozen reference differ in mu by {min(sep):.3g} .. {max(sep):.3g} behind the map build")
        assert len(sep) == len(batches) - k1 - 1 and min(sep) > SWITCH_MIN, f"{who}: the switch changes mu by {min(sep)} only"
    return c, batches, streams, refs


class Device:
    """one context on the case's streams: the switches set before the first call, then one call per batch"""

    def __init__(self, c, streams, windows):
        self.c, self.streams, self.R, self.fleet = c, streams, len(streams), bool(c.get("fleet"))
        self.ctx = ctx = context(c, windows or c.get("all_switches"))
        if c.get("gate") is not None:
            ctx.set_slam_gate(gate_d2=c["gate"])
        ctx.set_consistent_innovations(True)
        if c.get("all_switches"):
            ctx.set_slam_gate_windows(True)
        if windows or c.get("all_switches"):
            ctx.set_consistent_windows(True)
        if self.fleet:
            ctx.fleet_slam_begin([CAM] * self.R)
        assert ctx.get_consistent_innovations()
        ctx.profile_enable(True)
        ctx.profile_reset()
        self.seconds = 0.0

    def call(self, k, first, count, reset):
        """stage and run frames first .. first + count - 1 (call 0: behind the arming samples); returns the number of arming slots"""
        ctx, R, streams = self.ctx, self.R, self.streams
        arm = 1 if k == 0 else 0
        # slots: the arming samples of every robot first (first call), then the frames, the robots of one frame side by side
        order = list(range(R)) * (arm + count)
        enc = [(0.0, 0.0, 0.0)] * (R * arm) + [streams[r][f][0] for f in range(first, first + count) for r in range(R)]
        ctx.stage_encoders([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc])
        for s in range(R * arm):
            inject(ctx, s, [])
        for i, f in enumerate(range(first, first + count)):
            for r in range(R):
                inject(ctx, R * (arm + i) + r, streams[r][f][1])
        if reset:
            ctx.profile_reset()                                    # (the planner's statistics count from the last reset)
        t0 = time.perf_counter()
        if self.fleet:
            ctx.fleet_run_staged(0, order, with_ekf=2)
        else:
            ctx.run_staged(0, arm + count, with_ekf=2)
        ctx.sync()                                                 # raises on an overflow mask: the reference's is 0
        self.seconds += time.perf_counter() - t0
        return arm

    def state(self, r):
        return self.ctx.fleet_get_state(r) if self.fleet else self.ctx.get_state()


def run_long(name, frames):
    c, batches, streams, refs = references(name, frames)
    floor = frames <= EMU_FRAMES or c["L"] <= 12         # (long double at N = 150 over 2 000 frames takes a minute: measured apart, see the table)
    R = len(streams)
    fleet, gate, windows = bool(c.get("fleet")), c.get("gate"), c["windows"]
    # (fleets: the floor of robot 0, as §27 states F's; the other two streams cost 1.5 s of long double each in the prefix)
    tails = [consistent_long_double_tail(s, c["ML"], c["cap"], batches, gate) if floor and r == 0 else {} for r, s in enumerate(streams)]
    dev = Device(c, streams, windows)
    twin = Device(c, streams, False) if c.get("twin") else None
    ctx = dev.ctx
    kernels = CHAIN_KERNELS[c["chain"]] | ({FINISH} if gate is not None else set())
    tol = TOL.get(name)
    worst = dict(mu=0.0, S=0.0, asym=0.0, asym_ref=0.0, floor_mu=0.0, floor_S=0.0)
    k_complete = max(first_complete_batch(ref, batches) for ref in refs)
    plan_at_complete = frames_at_complete = None
    windows_before = in_before = 0
    wraps_inside, twin_diff = [], {}
    for k, (first, count) in enumerate(batches):
        where = f"{name}, call {k} (frames {first} .. {first + count - 1})"
        arm = dev.call(k, first, count, reset=not windows)
        if not windows:
            ran = ekf_kernels_run(ctx.profile_get())
            assert ran == kernels, f"{where}: ran {sorted(ran)}"
            if c.get("all_switches"):                              # the gated consistent window is not built: the per-frame fallback
                ps = ctx.plan_stats()
                assert ps["windows"] == 0 and ps["frames_in_windows"] == 0 and ps["frames_per_frame_chain"] == arm + count, f"{where}: {ps}"
        stats = ctx.get_slot_ekf_stats(R * arm, R * count)
        health = ctx.get_slot_health(R * arm, R * count) if gate is not None else None
        for r, ref in enumerate(refs):
            assert stats[r::R].tolist() == ref["stats"][first:first + count], f"{where}, robot {r}: statistics"
            mu, S = dev.state(r)
            ids = ctx.fleet_get_landmark_ids(r) if fleet else ctx.get_landmark_ids()
            assert ids.tolist() == ref["ids"][k] and mu.shape == (3 + 3 * len(ref["ids"][k]),), f"{where}, robot {r}: L / landmark ids"
            if not fleet:
                gi, gx, ga = ctx.get_observations()[:3]
                assert np.stack([gi, gx, ga], 1).tolist() == [list(p) for p in ref["pops"][k]], f"{where}: pop list (id, index, action)"
            if gate is not None:
                for i, f in enumerate(range(first, first + count)):
                    check_slot_health(health[R * i + r], ref["health"][f], f"{where}, robot {r}, frame {f}")
                    if ref["health"][f]["rejected"] and name != "hG":
                        assert int(health[R * i + r]["worst_id"]) == streams[r].outliers[f], f"{where}, robot {r}, frame {f}: flagged id"
                check_track(ctx.fleet_get_health()[r] if fleet else ctx.get_track_health(), ref["track"][k], f"{where}, robot {r}")
            mu_r, S_r = ref["states"][k]
            e_mu, e_S = float(np.abs(mu - mu_r).max()), rel_err(S, S_r)
            a_dev, a_ref = asymmetry(S), asymmetry(S_r)
            eig_dev, eig_ref = min_eig(S), min_eig(S_r)
            f_mu, f_S = tails[r].get(k, (0.0, 0.0))
            print(f"{where}, robot {r}: |dmu| {e_mu:.3g} (floor {f_mu:.3g}), Sigma {e_S:.3g} (floor {f_S:.3g}), asymmetry {a_dev:.3g} (reference "
                  f"{a_ref:.3g}), smallest eigenvalue {eig_dev:.3g} (reference {eig_ref:.3g}, max|Sigma| {np.abs(S_r).max():.3g})")
            assert np.allclose(mu, mu_r, rtol=1e-9, atol=1e-11), f"{where}, robot {r}: mu differs by {e_mu}"
            assert e_S <= 1e-9, f"{where}, robot {r}: Sigma differs by {e_S} (relative)"
            if tol is not None:
                assert e_mu <= tol[0] and e_S <= tol[1], f"{where}, robot {r}: |dmu| {e_mu}, Sigma {e_S} above the measured bounds {tol[:2]}"
                assert a_dev <= tol[2], f"{where}, robot {r}: Sigma's asymmetry {a_dev} above the measured bound {tol[2]}"
            assert a_dev <= 1e-9, f"{where}, robot {r}: Sigma's asymmetry {a_dev}"
            assert eig_ref <= EIG_REL * np.abs(S_r).max() or eig_dev > 0.0, f"{where}, robot {r}: smallest eigenvalue {eig_dev} (reference {eig_ref})"
            for key, v in (("mu", e_mu), ("S", e_S), ("asym", a_dev), ("asym_ref", a_ref), ("floor_mu", f_mu), ("floor_S", f_S)):
                worst[key] = max(worst[key], v)
        if twin is not None:
            twin.call(k, first, count, reset=True)
            ran = ekf_kernels_run(twin.ctx.profile_get())
            assert ran == CHAIN_KERNELS[c["chain"]], f"{where}: the per-frame twin ran {sorted(ran)}"
            (mu, S), (mu_t, S_t) = dev.state(0), twin.state(0)
            assert mu.shape == mu_t.shape
            t_mu, t_S = float(np.abs(mu - mu_t).max() / np.abs(mu_t).max()), rel_err(S, S_t)
            print(f"{where}: against the per-frame consistent twin mu {t_mu:.3g}, Sigma {t_S:.3g} relative")
            assert t_mu <= TWIN_TOL and t_S <= TWIN_TOL, f"{where}: differs from the per-frame twin ({t_mu}, {t_S})"
            twin_diff[k] = max(t_mu, t_S)
        if windows:
            ps = ctx.plan_stats()
            assert ps["frames_in_windows"] + ps["frames_per_frame_chain"] == 1 + first + count, f"{where}: {ps}"      # (1: the arming sample)
            if k > k_complete and count > 1:
                assert ps["windows"] > windows_before, f"{where}: no window formed ({ps})"
            if k > k_complete and ps["frames_in_windows"] - in_before == count:     # the whole call ran inside windows
                wraps_inside += [w for w in streams[0].wraps if first <= w < first + count]
            windows_before, in_before = ps["windows"], ps["frames_in_windows"]
            if k == k_complete:
                plan_at_complete, frames_at_complete = ps, first + count
    if windows:
        later = frames - frames_at_complete
        inside = ps["frames_in_windows"] - plan_at_complete["frames_in_windows"]
        assert later > 0 and inside >= 0.9 * later, f"{name}: {inside} of the {later} frames behind the map build ran inside windows ({ps})"
        prof = ctx.profile_get()
        assert prof["k_ekf_win_step"][0] == ps["windows"] > 0, f"{name}: {prof['k_ekf_win_step'][0]} k_ekf_win_step launches, {ps}"
        handed = prof["k_ekf_win_next"][0]
        # D's sets slide: a call of 64 frames needs more than one set, and the second window starts from the first one's accumulators
        assert handed > 0 or not (c.get("slides") and frames >= GPU_FRAMES), f"{name}: no window was handed over to the next"
        # the window's mu_0 snapshot across a heading wrap: the prefix's one wrap (frame 79) lies no later than the call that completes the map
        assert wraps_inside or frames < GPU_FRAMES, f"{name}: no frame that wraps the heading ran inside a window"
        print(f"{name}: planner {ps}, {handed} hand-overs, {inside} of {later} frames behind the map build inside windows; wrap frames inside "
              f"windows: {wraps_inside}")
    if twin_diff:
        ks = sorted(k for k in twin_diff if k > k_complete)
        q = max(1, len(ks) // 4)
        worst["twin_first"], worst["twin_last"] = max(twin_diff[k] for k in ks[:q]), max(twin_diff[k] for k in ks[-q:])
        print(f"{name}: twin difference, largest in the first quarter of the calls behind the map build {worst['twin_first']:.3g}, in the last "
              f"{worst['twin_last']:.3g}")
        twin.ctx.close()
    print(f"{name}: {frames} frames in {len(batches)} calls, {dev.seconds:.2f} s inside them: worst |dmu| {worst['mu']:.3g} (floor {worst['floor_mu']:.3g}), "
          f"Sigma {worst['S']:.3g} (floor {worst['floor_S']:.3g}), asymmetry {worst['asym']:.3g} (reference {worst['asym_ref']:.3g})")
    ctx.close()
    return worst


def test_references_without_a_device():
    """200 frames of stream A: the gated consistent literal at +inf is the ungated one bit for bit, and with consistent = False the new
    runs are reference_run / gated_reference_run bit for bit"""
    batches = batches_of(EMU_FRAMES)
    s = ring_stream(12, 4, EMU_FRAMES, 1)
    plain, gated = consistent_reference_run(s, 12, 24, batches), consistent_gated_reference_run(s, batches, math.inf)

    def same(a, b, keys):
        for key in keys:
            if key == "states":
                assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a[key], b[key])), key
                assert len(a[key]) == len(b[key])
            else:
                assert a[key] == b[key], key

    shared = ("states", "ids", "mask", "pops", "stats", "complete")
    same(plain, gated, shared)
    assert not gated["rejected"] and all(h["attempted"] == h["accepted"] for h in gated["health"])
    same(consistent_reference_run(s, 12, 24, batches, consistent=False), reference_run(s, 12, 24, batches), shared)
    so = ring_stream(12, 4, EMU_FRAMES, 1, 0.0, OUTLIER_EVERY)
    old = gated_reference_run(so, batches, 1.0)
    assert old["rejected"], "no rejection in the gated stream: the comparison shows nothing of the gate"
    same(consistent_gated_reference_run(so, batches, 1.0, consistent=False), old, shared + ("health", "track", "rejected"))
    # and the switch is not a no-op in the reference
    assert np.abs(plain["states"][-1][0] - reference_run(s, 12, 24, batches)["states"][-1][0]).max() > SWITCH_MIN
    # the R argument leaves the draws alone
    sh = ring_stream(12, 4, EMU_FRAMES, 1, R=HONEST_R)
    assert all(np.array_equal(a[2], b[2]) and a[0] == b[0] for (_, oa), (_, ob) in zip(s, sh) for a, b in zip(oa, ob))
    assert s != sh and tuple(sh[0][1][0][3]) == HONEST_R and tuple(s[0][1][0][3]) == RDIAG


@pytest.mark.parametrize("name", sorted(CASES))
def test_long_run_consistent_prefix(name):
    run_long(name, EMU_FRAMES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_long_run_consistent_on_gpu(name, on_emulation):
    assert not on_emulation
    run_long(name, GPU_FRAMES)


# ---- localization laps ------------------------------------------------------------------------------------------------------------------

LOC_FRAMES = 320                                     # two laps, two heading wraps
LOC_L, LOC_M, LOC_SEED = 12, 4, 1
LOC_STARTS = (0.0, 0.7, 1.9)                         # F's phases, as starting headings in the one world
LOC_KINDS = ("fixed", "uncertain", "fleet", "gated")
LOC_R = {"stock": RDIAG, "honest": HONEST_R}
# With stock R the consistent and the frozen localizer come within 1e-6 of each other at the end of some call in (a), (b) and (c)
# (smallest pose difference 4.3e-7, 9.0e-7 and 4.3e-7; honest R: 1.1e-4, 5.0e-4, 4.8e-5), so those keep the honest-R variant only;
# (d) passes the condition with either R (stock 2.0e-6, where no planted outlier reaches the gate; honest 7.0e-5, where all five do
# and the true sightings of frames 282 and 318 are rejected as well)
LOC_CASES = [("fixed", "honest"), ("uncertain", "honest"), ("fleet", "honest"), ("gated", "stock"), ("gated", "honest")]


@pytest.fixture(params=["session", pytest.param("gfx950", marks=pytest.mark.gpu)])
def library(request):
    if request.param == "gfx950":
        assert capi.lib_path().endswith("libaruco_slam_hip.so"), "the gpu cases must run the native gfx950 library"
    return request.param


class Snap:
    """what close() reads of a localizer, kept at the end of a call"""

    def __init__(self, ref):
        self.mu, self.P = np.array(ref.mu, float), np.array(ref.P, float)


@functools.lru_cache(maxsize=None)
def loc_reference(kind, rname):
    """the streams, the map and, per robot, the consistent reference's records of every frame and its state at the end of every call;
    asserts the conditions on the references alone"""
    Rd = LOC_R[rname]
    starts = LOC_STARTS if kind == "fleet" else (0.0,)
    streams = [ring_stream(LOC_L, LOC_M, LOC_FRAMES, LOC_SEED, 0.0, OUTLIER_EVERY if kind == "gated" else 0, Rd, st) for st in starts]
    ids, xyth = streams[0].ids, streams[0].world
    assert all(np.array_equal(s.world, xyth) for s in streams), "the robots share one world"
    for s in streams:
        assert sum(1 for w in s.wraps) >= 2, "two heading wraps"
    batches = batches_of(LOC_FRAMES)
    gate = dict(gate_d2=DEFAULTS["gate_d2"]) if kind == "gated" else None
    C = spd_blocks(np.random.RandomState(LOC_L), LOC_L, 0.03) if kind == "uncertain" else None
    robots = []
    for st, s in zip(starts, streams):
        pose0 = np.array([0.0, 0.0, st])
        if kind == "uncertain":
            ref, frozen = ConsistentUmapLocalizer(ids, xyth, C, pose0, SIG0, gate), UncertainMapLocalizer(ids, xyth, C, pose0, SIG0, gate)
        else:
            ref = ConsistentLocalizer(ids, xyth, pose0, SIG0, gate)
            frozen = GatedLocalizer(ids, xyth, pose0, SIG0, gate if gate is not None else dict(gate_d2=math.inf))
        for m in (ref, frozen):
            m.add_encoder(0.0, 0.0, 0.0)                             # the arming sample
            m.add_observations([])
        recs, ends, sep = [], [], []
        for first, count in batches:
            for f in range(first, first + count):
                (wl, wr, dt), obs = s[f]
                for m in (ref, frozen):
                    m.add_encoder(wl, wr, dt)
                    m.add_observations(obs)
                recs.append(dict(stats=list(ref.stats), health=dict(ref.health), log=ref.log_array()))
                assert not ref.track["lost"], f"{kind} {rname}: the reference loses its track in frame {f}"
            ends.append(dict(ref=copy.deepcopy(ref) if kind == "uncertain" else Snap(ref), track=dict(ref.track)))
            sep.append(float(np.abs(np.asarray(ref.mu, float) - np.asarray(frozen.mu, float)).max()))
        ref.assert_margins()
        print(f"{kind} {rname}, start {st}: the consistent and the frozen localizer differ in the pose by {min(sep):.3g} .. {max(sep):.3g}")
        assert min(sep) > SWITCH_MIN, f"{kind} {rname}, start {st}: the switch changes the pose by {min(sep)} only"
        if kind == "gated":
            rej = {f for f, rec in enumerate(recs) if rec["health"]["rejected"]}
            print(f"{kind} {rname}: {len(s.outliers)} planted outliers, rejections in frames {sorted(rej)}")
            if rname == "honest":
                assert set(s.outliers) <= rej, "a planted outlier passes the gate"
        robots.append(dict(pose0=pose0, recs=recs, ends=ends))
    return streams, ids, xyth, C, batches, robots


@pytest.mark.parametrize("kind,rname", LOC_CASES, ids=[f"{k}-{r}" for k, r in LOC_CASES])
def test_localization_laps(library, kind, rname):
    streams, ids, xyth, C, batches, robots = loc_reference(kind, rname)
    R = len(streams)
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=(MAX_BATCH + 1) * R, persistent_waves=4, max_landmarks=LOC_L)
    if kind == "gated":
        ctx.set_innovation_gate()
    ctx.set_consistent_innovations(True)
    if kind == "fleet":
        ctx.fleet_begin([CAM] * R, ids, xyth, [rob["pose0"] for rob in robots], [SIG0] * R)
    elif kind == "uncertain":
        ctx.localize_begin_uncertain(ids, xyth, C, robots[0]["pose0"], SIG0)
    else:
        ctx.localize_begin(ids, xyth, robots[0]["pose0"], SIG0)
    assert ctx.get_consistent_innovations(), "the switch survives the begin"
    ctx.profile_enable(True)
    ctx.profile_reset()
    steps = "k_fleet_steps" if kind == "fleet" else "k_loc_steps"
    for k, (first, count) in enumerate(batches):
        where = f"{kind} {rname}, call {k} (frames {first} .. {first + count - 1})"
        arm = 1 if k == 0 else 0
        order = list(range(R)) * (arm + count)
        enc = [(0.0, 0.0, 0.0)] * (R * arm) + [streams[r][f][0] for f in range(first, first + count) for r in range(R)]
        ctx.stage_encoders([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc])
        for s in range(R * arm):
            inject_loc(ctx, s, [])
        for i, f in enumerate(range(first, first + count)):
            for r in range(R):
                inject_loc(ctx, R * (arm + i) + r, streams[r][f][1])
        if kind == "fleet":
            ctx.fleet_run_staged(0, order, with_ekf=2)
        else:
            ctx.run_staged(0, arm + count, with_ekf=2)
        ctx.sync()
        prof = ctx.profile_get()
        assert prof[steps][0] == k + 1 and not ekf_kernels_run(prof), f"{where}: {prof[steps][0]} {steps} launches, SLAM kernels {sorted(ekf_kernels_run(prof))}"
        stats = ctx.get_slot_ekf_stats(R * arm, R * count)
        for r, rob in enumerate(robots):
            recs, end = rob["recs"][first:first + count], rob["ends"][k]
            assert stats[r::R].tolist() == [rec["stats"] for rec in recs], f"{where}, robot {r}: statistics"
            if kind == "fleet":
                poses, sigs = ctx.fleet_get_poses()
                close(poses[r], sigs[r], end["ref"], f"{where}, robot {r}")
                e = float(np.abs(poses[r] - end["ref"].mu).max())
            else:
                gi, gx, ga, _, _ = ctx.get_observations()
                assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), recs[-1]["log"]), f"{where}: pops / actions differ"
                mu, S = ctx.get_state()
                e = float(np.abs(mu[:3] - end["ref"].mu).max())
                if kind == "uncertain":
                    check_single(ctx, end["ref"], where)
                else:
                    close(mu[:3], S[:3, :3], end["ref"], where)
            print(f"{where}, robot {r}: pose differs by {e:.3g}")
            if kind == "gated":
                health = ctx.get_slot_health(arm, count)
                for i, rec in enumerate(recs):
                    check_loc_health(health[i], rec["health"], f"{where}, frame {first + i}")
                check_loc_track(ctx.get_track_health(), end["track"], where)
    ctx.close()
