"""Runs of thousands of frames on small worlds, every SLAM chain, against the literal reference after every call.

The world, its streams and the references are in tests/long_run_world.py.  Every case starts from the empty map, so the map that is
corrected for thousands of frames is the one the device built (augment with float trig), the heading wraps once per lap, and slots,
rings and the window planner's tables are reused call after call: the calls cycle through batch lengths (1, 7, 64, 33, 2, 50).

  case  chain                                        cap  windows  L   m   max_landmarks
  A     fast (k_ekf_mid, k_ekf_apply)                24   off      12  4   12
  B     windows, SP 64                               24   on       12  4   12     (A's stream)
  C     mid (k_ekf_mid64, k_ekf_T, k_ekf_update_mfma) 64  off      40  26  40     (N = 123)
  D     windows, SP 128                              64   on       48  26  49     (ld = 150: no multiple of 64, N < ld)
  E     general (k_ekf_gather, k_ekf_small, ...)     128  off      48  33  49
  F     fleet SLAM, 3 robots, mid chain              64   -        40  26  40     (robot 0 has C's stream; seeds and phases differ)
  G     windows under the SLAM gate (gate_d2 = 1)    24   on       12  4   12     (A's stream, an outlier every 53rd frame)

D's sets: the sightings are contiguous in bearing, so a window's set grows by one landmark every few frames; it starts at 26
landmarks (SP 128) and the planner closes a window of 16 frames or more rather than widen it to SP 192, so SP 192 does not occur.
F: 3 robots x 64 frames do not fit into max_batch = 64 slots; the fleet context has 3 x 65 slots, so that every robot runs the shared
schedule and the references are shared with the single contexts.  Fleets keep no pop list (aslam_get_observations describes the
single filter): F compares everything else.

After EVERY call (a heading error is forgotten within a lap, and a comparison per call names the call): L and
the landmark ids, the statistics of every slot of the call, the overflow mask, the pop list of the call's last frame, the set of
EKF kernels (cases without windows), the planner's statistics (B, D, G), the slot and track records (G) with ==; mu at rtol 1e-9 /
atol 1e-11 and Sigma at 1e-9 relative (the
project's bar for f64 state against a literal reference); then the tighter per-case bounds below on |dmu|, Sigma and on the
asymmetry max |Sigma - Sigma^T| / max |Sigma|; and the smallest eigenvalue of (Sigma + Sigma^T) / 2 is positive wherever the
reference's exceeds 1e-7.  Before the device runs, every case asserts on the reference that the map was complete within the first
lap, that every later frame fused exactly m corrections (G: m less the planted outlier) and that the eigenvalue condition holds.

Lengths.  Marked gpu: 2 000 frames.  On the session's library (the emulation without a GPU): the first EMU_FRAMES = 200 frames, which
hold the whole map build (complete after frame 105 at the latest), one full lap and the first heading wrap (frame 79); on an idle
machine the emulation takes 2 s (A), 1 s (B), 6 s (C), 9 s (D), 10 s (E), 10 s (F) and 1 s (G) for them, references included.

Measured worst values over all 78 calls of 2 000 frames, seed as committed (|dmu| / Sigma relative / asymmetry of the device's Sigma;
floor = the double reference against long_double_tail, |dmu| / Sigma; the reference's own asymmetry; seconds inside the calls on the
MI355X).  The emulation ran the 2 000 frames once, outside the suite.  TOL is 10 x the larger of the two measured values.

  case  emulation                       MI355X                          floor                reference asym.  MI355X s
  A     1.51e-14 / 9.38e-15 / 1.88e-16  1.51e-14 / 9.57e-15 / 3.71e-16  1.48e-14 / 8.39e-15  7.18e-15         0.10
  B     1.15e-14 / 1.26e-14 / 1.47e-14  1.15e-14 / 1.31e-14 / 1.55e-14  1.48e-14 / 8.39e-15  7.18e-15         0.02
  C     4.88e-14 / 3.02e-14 / 2.72e-14  4.88e-14 / 3.01e-14 / 2.69e-14  5.05e-14 / 2.34e-14  2.76e-14         0.26
  D     2.58e-14 / 4.17e-14 / 6.93e-14  2.62e-14 / 4.24e-14 / 7.04e-14  5.98e-14 / 3.51e-14  2.69e-14         0.10
  E     5.60e-14 / 4.30e-14 / 3.82e-14  5.60e-14 / 4.33e-14 / 3.81e-14  5.50e-14 / 3.28e-14  3.73e-14         3.62
  F     6.62e-14 / 3.78e-14 / 3.60e-14  6.57e-14 / 3.78e-14 / 3.60e-14  5.05e-14 / 2.34e-14  2.76e-14         0.28
  G     1.29e-14 / 1.03e-14 / 7.77e-15  1.33e-14 / 9.68e-15 / 6.93e-15  2.16e-14 / 7.29e-15  6.93e-15         0.03

Every error is within 2 x its floor: what separates the device from the literal reference is the reference's own rounding.  (F's
floor is robot 0's, the stream of C.)  The floors of C .. F at 2 000 frames take a minute of long double each and are not computed
in the suite: the test prints a floor for every call of the prefix and of A, B and G, and 0 otherwise.  The windows (B, D) leave
Sigma less symmetric than the per-frame chains (A: 3.7e-16, the chains write both triangles from one product) and than the reference
itself, by a factor below 3.  With two other seeds (every seed + 100, + 200) the emulation stays inside TOL: all cases at 200 frames,
A, B and G at 2 000 (worst 1.9e-14 / 1.3e-14 / 1.4e-14).  The smallest eigenvalue of the reference's Sigma stays between 9.5e-7 and
1.3e-5 behind the map build.
"""
import os
import time

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from ekf_reference import CHAIN_KERNELS, ekf_kernels_run, rel_err
from long_run_world import (LAP, MAX_BATCH, OUTLIER_FROM, asymmetry, batches_of, first_complete_batch, gated_reference_run, long_double_tail, min_eig,
                            reference_run, ring_stream)
from slam_gate_reference import check_slot_health, check_track

GPU_FRAMES, EMU_FRAMES = 2000, 200
GATE = 1.0
OUTLIER_EVERY = 53
EIG_FLOOR = 1e-7
CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))

# streams = (seed, phase) per robot
CASES = {
    "A": dict(chain="fast", cap=24, windows=False, L=12, m=4, ML=12, streams=((1, 0.0),)),
    "B": dict(chain="fast", cap=24, windows=True, L=12, m=4, ML=12, streams=((1, 0.0),)),
    "C": dict(chain="mid", cap=64, windows=False, L=40, m=26, ML=40, streams=((2, 0.0),)),
    "D": dict(chain="mid", cap=64, windows=True, L=48, m=26, ML=49, streams=((3, 0.0),), slides=True),
    "E": dict(chain="general", cap=128, windows=False, L=48, m=33, ML=49, streams=((3, 0.0),)),
    "F": dict(chain="mid", cap=64, windows=False, L=40, m=26, ML=40, streams=((2, 0.0), (12, 0.7), (22, 1.9)), fleet=True),
    "G": dict(chain="fast", cap=24, windows=True, L=12, m=4, ML=12, streams=((1, 0.0),), gate=True),
}

# Bounds on the worst error over all calls: (|dmu|, Sigma relative, asymmetry of the device's Sigma), 10 x the larger of the two
# values measured at 2 000 frames (the table above); all far below the project's 1e-9, which is asserted as well
TOL = {"A": (1.5e-13, 9.5e-14, 3.7e-15), "B": (1.1e-13, 1.3e-13, 1.5e-13), "C": (4.8e-13, 3.0e-13, 2.7e-13), "D": (2.6e-13, 4.2e-13, 7.0e-13),
       "E": (5.6e-13, 4.3e-13, 3.8e-13), "F": (6.6e-13, 3.7e-13, 3.6e-13), "G": (1.3e-13, 1.0e-13, 7.7e-14)}


def context(c):
    kw = dict(max_rows=64, max_cols=64, max_batch=(MAX_BATCH + 1) * len(c["streams"]) if c.get("fleet") else MAX_BATCH, persistent_waves=4,
              max_landmarks=c["ML"], max_updates_per_frame=c["cap"])
    if c["windows"] or c.get("fleet"):
        return capi.Context(**kw)
    os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        return capi.Context(**kw)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)


def inject(ctx, slot, obs):
    ctx.inject_observations(slot, [o[0] for o in obs], [o[1] for o in obs], np.array([o[2] for o in obs]).reshape(-1, 3),
                            np.array([o[3] for o in obs]).reshape(-1, 3))


def references(name, frames):
    """the case's streams, batches and references, with the setup assertions on the references alone"""
    c = CASES[name]
    batches = batches_of(frames)
    streams = [ring_stream(c["L"], c["m"], frames, seed, phase, OUTLIER_EVERY if c.get("gate") else 0) for seed, phase in c["streams"]]
    refs = [gated_reference_run(s, batches, GATE) if c.get("gate") else reference_run(s, c["ML"], c["cap"], batches) for s in streams]
    for s, ref in zip(streams, refs):
        assert ref["complete"] is not None and ref["complete"] < LAP, f"{name}: the map is not complete within the first lap"
        assert sum(st[1] for st in ref["stats"]) == c["L"] and all(st[3] == 0 for st in ref["stats"]) and not any(ref["mask"])
        for f in range(ref["complete"] + 1, frames):
            assert ref["stats"][f] == [c["m"], 0, c["m"] - (f in s.outliers), 0], f"{name}: frame {f} fused {ref['stats'][f]}"
        if c.get("gate"):
            assert len(s.outliers) == sum(1 for f in range(OUTLIER_FROM, frames) if f % OUTLIER_EVERY == 0) >= 2 and min(s.outliers) > ref["complete"]
            assert ref["rejected"] == {f: [i] for f, i in s.outliers.items()}, f"{name}: the reference rejects {ref['rejected']}"
        k0 = first_complete_batch(ref, batches)
        eig = [min_eig(S) for _, S in ref["states"][k0:]]
        assert len(eig) > 1 and min(eig) > EIG_FLOOR, f"{name}: the reference's smallest eigenvalue is {min(eig)}: nothing to hold the device's against"
    return c, batches, streams, refs


def run_long(name, frames, on_emulation):
    c, batches, streams, refs = references(name, frames)
    floor = frames <= EMU_FRAMES or c["L"] <= 12         # (long double at N = 150 over 2 000 frames takes a minute: measured apart, see the table)
    R = len(streams)
    fleet, gate, windows = bool(c.get("fleet")), bool(c.get("gate")), c["windows"]
    tails = [long_double_tail(s, c["ML"], c["cap"], batches, GATE if gate else None) if floor else {} for s in streams]
    ctx = context(c)
    if gate:
        ctx.set_slam_gate(gate_d2=GATE)
        ctx.set_slam_gate_windows(True)
    if fleet:
        ctx.fleet_slam_begin([CAM] * R)
    ctx.profile_enable(True)
    ctx.profile_reset()
    tol = TOL[name]
    worst = dict(mu=0.0, S=0.0, asym=0.0, asym_ref=0.0, floor_mu=0.0, floor_S=0.0)
    k_complete = max(first_complete_batch(ref, batches) for ref in refs)
    plan_at_complete = frames_at_complete = None
    windows_before, seconds = 0, 0.0
    for k, (first, count) in enumerate(batches):
        where = f"{name}, call {k} (frames {first} .. {first + count - 1})"
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
        if not windows:
            ctx.profile_reset()                                    # (the planner's statistics count from the last reset)
        t0 = time.perf_counter()
        if fleet:
            ctx.fleet_run_staged(0, order, with_ekf=2)
        else:
            ctx.run_staged(0, arm + count, with_ekf=2)
        ctx.sync()                                                 # raises on an overflow mask: the reference's is 0
        seconds += time.perf_counter() - t0
        if not windows:
            ran = ekf_kernels_run(ctx.profile_get())
            assert ran == CHAIN_KERNELS[c["chain"]], f"{where}: ran {sorted(ran)}"
        stats = ctx.get_slot_ekf_stats(R * arm, R * count)
        for r, ref in enumerate(refs):
            assert stats[r::R].tolist() == ref["stats"][first:first + count], f"{where}, robot {r}: statistics"
            mu, S = ctx.fleet_get_state(r) if fleet else ctx.get_state()
            ids = ctx.fleet_get_landmark_ids(r) if fleet else ctx.get_landmark_ids()
            assert ids.tolist() == ref["ids"][k] and mu.shape == (3 + 3 * len(ref["ids"][k]),), f"{where}, robot {r}: L / landmark ids"
            if not fleet:
                gi, gx, ga = ctx.get_observations()[:3]
                assert np.stack([gi, gx, ga], 1).tolist() == [list(p) for p in ref["pops"][k]], f"{where}: pop list (id, index, action)"
            if gate:
                health = ctx.get_slot_health(arm, count)
                for i, f in enumerate(range(first, first + count)):
                    check_slot_health(health[i], ref["health"][f], f"{where}, frame {f}")
                    if ref["health"][f]["rejected"]:
                        assert int(health[i]["worst_id"]) == streams[r].outliers[f], f"{where}, frame {f}: flagged id"
                check_track(ctx.get_track_health(), ref["track"][k], where)
            mu_r, S_r = ref["states"][k]
            e_mu, e_S = float(np.abs(mu - mu_r).max()), rel_err(S, S_r)
            a_dev, a_ref = asymmetry(S), asymmetry(S_r)
            eig_dev, eig_ref = min_eig(S), min_eig(S_r)
            f_mu, f_S = tails[r].get(k, (0.0, 0.0))
            print(f"{where}, robot {r}: |dmu| {e_mu:.3g} (floor {f_mu:.3g}), Sigma {e_S:.3g} (floor {f_S:.3g}), asymmetry {a_dev:.3g} (reference "
                  f"{a_ref:.3g}), smallest eigenvalue {eig_dev:.3g} (reference {eig_ref:.3g})")
            assert np.allclose(mu, mu_r, rtol=1e-9, atol=1e-11), f"{where}, robot {r}: mu differs by {e_mu}"
            assert e_S <= 1e-9, f"{where}, robot {r}: Sigma differs by {e_S} (relative)"
            assert e_mu <= tol[0] and e_S <= tol[1], f"{where}, robot {r}: |dmu| {e_mu}, Sigma {e_S} above the measured bounds {tol[:2]}"
            assert a_dev <= tol[2], f"{where}, robot {r}: Sigma's asymmetry {a_dev} above the measured bound {tol[2]}"
            assert eig_ref <= EIG_FLOOR or eig_dev > 0.0, f"{where}, robot {r}: smallest eigenvalue {eig_dev} (reference {eig_ref})"
            for key, v in (("mu", e_mu), ("S", e_S), ("asym", a_dev), ("asym_ref", a_ref), ("floor_mu", f_mu), ("floor_S", f_S)):
                worst[key] = max(worst[key], v)
        if windows:
            ps = ctx.plan_stats()
            assert ps["frames_in_windows"] + ps["frames_per_frame_chain"] == 1 + first + count, f"{where}: {ps}"      # (1: the arming sample)
            if k > k_complete and count > 1:
                assert ps["windows"] > windows_before, f"{where}: no window formed ({ps})"
            windows_before = ps["windows"]
            if k == k_complete:
                plan_at_complete, frames_at_complete = ps, first + count
    if windows:
        later = frames - frames_at_complete
        inside = ps["frames_in_windows"] - plan_at_complete["frames_in_windows"]
        assert later > 0 and inside >= 0.9 * later, f"{name}: {inside} of the {later} frames behind the map build ran inside windows ({ps})"
        handed = ctx.profile_get()["k_ekf_win_next"][0]
        # D's sets slide: a call of 64 frames needs more than one set, and the second window starts from the first one's accumulators
        assert handed > 0 or not (c.get("slides") and frames >= GPU_FRAMES), f"{name}: no window was handed over to the next"
        print(f"{name}: planner {ps}, {handed} hand-overs, {inside} of {later} frames behind the map build inside windows")
    print(f"{name}: {frames} frames in {len(batches)} calls, {seconds:.2f} s inside them: worst |dmu| {worst['mu']:.3g} (floor {worst['floor_mu']:.3g}), Sigma {worst['S']:.3g} (floor "
          f"{worst['floor_S']:.3g}), asymmetry {worst['asym']:.3g} (reference {worst['asym_ref']:.3g})")
    ctx.close()
    return worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_long_run_prefix(name, on_emulation):
    run_long(name, EMU_FRAMES, on_emulation)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_long_run_on_gpu(name, on_emulation):
    assert not on_emulation
    run_long(name, GPU_FRAMES, on_emulation)
