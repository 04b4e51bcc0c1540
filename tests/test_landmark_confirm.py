"""Landmark confirmation (aslam_set_landmark_confirmation, csrc/landmark_confirm.h).

Confirmation is a filter on a slot's observation list in front of everything that reads the list, and a withheld sighting is a
sighting with valid = 0.  So nothing here has a tolerance and every comparison is np.array_equal:
  * the rule itself against tests/confirm_reference.py (flags read back, slot records, tentative lists), slot by slot;
  * a context with confirmation on against a twin with confirmation off that is fed the same stream with the reference's withheld
    sightings already marked valid = 0, on every path that runs an EKF step of a SLAM filter.  A stage that judged behind the window
    planner's copy, or inside a chain, could not pass the twins: the planner, the last-observed list and the pop list would differ.
Contexts are small (64 x 64 frames, 8 - 16 slots, 16 - 40 landmarks); lists are injected, except in the end-to-end test, which renders
240 x 320 frames and runs the detector.  Everything runs on the session's library: the CPU emulation without a GPU, the gfx950
library on one; the tests marked gpu repeat the twins and the end-to-end run so that `-m gpu` covers the feature."""
import os

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from confirm_reference import ConfirmTable
from long_run_world import ring_stream

E_INVALID, E_STATE = -1, -5
WL, WR, DT = 2.0, 2.3, 1 / 30.0
RD = np.array([0.05, 0.05, 0.01])
CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
REC_FIELDS = ("judged", "tentative", "withheld", "promoted")


def context(ML, batch=8, windows=False, cap=24):
    kw = dict(max_rows=64, max_cols=64, max_batch=batch, persistent_waves=4, max_landmarks=ML, max_updates_per_frame=cap)
    if windows:
        return capi.Context(**kw)
    os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        return capi.Context(**kw)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)


def sighting(rng, lid, valid=1):
    return (int(lid), int(valid), np.array([rng.uniform(0.5, 2), rng.uniform(-1, 1), rng.uniform(-3, 3)]), RD)


def inject(ctx, slot, obs, valid=None):
    """obs: [(id, valid, z, Rdiag)]; valid: other flags than the list's own"""
    ctx.inject_observations(slot, [o[0] for o in obs], [o[1] for o in obs] if valid is None else valid,
                            np.array([o[2] for o in obs]).reshape(-1, 3), np.array([o[3] for o in obs]).reshape(-1, 3))


def state_of(ctx, robot=None):
    if robot is None:
        return (*ctx.get_state(), ctx.get_landmark_ids())
    return (*ctx.fleet_get_state(robot), ctx.fleet_get_landmark_ids(robot))


def assert_same(a, b, where):
    assert np.array_equal(a[2], b[2]), f"{where}: landmark ids {a[2].tolist()} against {b[2].tolist()}"
    assert np.array_equal(a[0], b[0]), f"{where}: mu"
    assert np.array_equal(a[1], b[1]), f"{where}: Sigma"
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all(), f"{where}: not finite"


def check_record(rec, want, where):
    for k in REC_FIELDS:
        assert int(rec[k]) == want[k], f"{where}: {k} {int(rec[k])}, reference {want[k]}"
    assert np.array_equal(rec["withheld_mask"], np.array(want["withheld_mask"], np.uint32)), f"{where}: withheld mask"


def check_tentative(got, table, where):
    for g, w, name in zip(got, table.tentative(), ("ids", "counts", "ages")):
        assert np.array_equal(g, np.array(w, np.int32)), f"{where}: tentative {name} {g.tolist()}, reference {w}"


def judge_call(ctx, table, lists, where, first=0, predict=True):
    """one run_staged(with_ekf = 2) call over `lists`, one list per slot from `first`: the flags the slots are left with, the slot
    records and (after the call) the tentative list against the reference"""
    n = len(lists)
    enc = [WL if predict else 0.0] * (first + n), [WR if predict else 0.0] * (first + n), [DT if predict else 0.0] * (first + n)
    ctx.stage_encoders(*enc)
    for s, obs in enumerate(lists):
        inject(ctx, first + s, obs)
    ctx.run_staged(first, n, with_ekf=2)
    ctx.sync()
    recs = ctx.get_slot_confirm(first, n)
    for s, obs in enumerate(lists):
        want_valid, want_rec = table.judge([o[0] for o in obs], [o[1] for o in obs])
        ids, valid, z, R = ctx.get_slot_raw_observations(first + s)
        assert np.array_equal(ids, np.array([o[0] for o in obs], np.int32)), f"{where}, slot {first + s}: ids moved"
        assert np.array_equal(valid, np.array(want_valid, np.int32)), f"{where}, slot {first + s}: valid {valid.tolist()}, reference {want_valid}"
        if obs:
            assert np.array_equal(z, np.array([o[2] for o in obs])) and np.array_equal(R, np.array([o[3] for o in obs])), f"{where}: z / R touched"
        check_record(recs[s], want_rec, f"{where}, slot {first + s}")
    check_tentative(ctx.get_tentative(), table, where)


# ---- 1. rule edges, device against reference -------------------------------------------------------------------------------------------

def armed(ML=16, batch=8, cap=24, **prm):
    ctx = context(ML, batch, cap=cap)
    ctx.set_landmark_confirmation(**prm)
    table = ConfirmTable(prm["min_sightings"], prm["max_gap"])
    judge_call(ctx, table, [[]], "arming", predict=False)          # an empty slot advances t
    assert table.t == 1
    return ctx, table


def test_two_sightings_confirm():
    rng = np.random.RandomState(1)
    ctx, table = armed(min_sightings=2, max_gap=5)
    judge_call(ctx, table, [[sighting(rng, 7)]], "K = 2, first")
    assert ctx.get_landmark_ids().tolist() == [] and table.tentative() == ([7], [1], [0])
    judge_call(ctx, table, [[sighting(rng, 7)]], "K = 2, second")
    assert ctx.get_landmark_ids().tolist() == [7] and table.tentative() == ([], [], [])
    judge_call(ctx, table, [[sighting(rng, 7)]], "K = 2, confirmed")
    assert ctx.get_slot_ekf_stats(0, 1)[0].tolist() == [1, 0, 1, 0]


def test_127_sightings_confirm():
    rng = np.random.RandomState(2)
    ctx, table = armed(batch=16, min_sightings=127, max_gap=1000000)
    for k in range(0, 126, 14):                                    # slot ranges that move: 9 calls of 14 slots, counts carried across
        judge_call(ctx, table, [[sighting(rng, 1023)] for _ in range(14)], f"K = 127, sightings {k} ..", first=k % 3)
    assert table.tentative()[1] == [126] and ctx.get_landmark_ids().tolist() == []
    judge_call(ctx, table, [[sighting(rng, 1023)]], "K = 127, the last one")
    assert ctx.get_landmark_ids().tolist() == [1023]


def test_runs_across_the_gap():
    rng = np.random.RandomState(3)
    G = 3
    ctx, table = armed(min_sightings=5, max_gap=G)
    judge_call(ctx, table, [[sighting(rng, 40), sighting(rng, 41)]], "gap: first sightings")
    judge_call(ctx, table, [[]] * (G - 1) + [[sighting(rng, 40)]], "gap: G frames later")        # t - last == G: the run survives
    assert table.tentative() == ([40, 41], [2, 1], [0, G]), "41 is G frames old: still listed"
    judge_call(ctx, table, [[sighting(rng, 41)]], "gap: G + 1 frames later")                      # t - last == G + 1: restarts at 1
    assert table.tentative() == ([40, 41], [2, 1], [1, 0])
    judge_call(ctx, table, [[]] * G, "gap: empty slots age the list")
    assert table.tentative() == ([41], [1], [G])


def test_twice_in_one_slot_counts_once_and_both_pass():
    rng = np.random.RandomState(4)
    ctx, table = armed(min_sightings=3, max_gap=5)
    two = lambda: [sighting(rng, 9), sighting(rng, 500), sighting(rng, 9)]
    judge_call(ctx, table, [two()], "twice, first")
    assert table.tentative() == ([9, 500], [1, 1], [0, 0])
    judge_call(ctx, table, [two(), two()], "twice, promoted in the second slot of a call")
    # both sightings of 9 pass, and the step treats them as it treats an id twice in a frame without confirmation: two augments
    assert ctx.get_slot_ekf_stats(1, 1)[0].tolist() == [3, 3, 0, 0] and ctx.get_landmark_ids().tolist() == [9, 500, 9]


def test_invalid_and_out_of_range_sightings():
    rng = np.random.RandomState(5)
    ctx, table = armed(min_sightings=2, max_gap=5)
    judge_call(ctx, table, [[sighting(rng, 3, valid=0), sighting(rng, 4)]], "valid = 0 never counts")
    judge_call(ctx, table, [[sighting(rng, 3, valid=0), sighting(rng, 4, valid=7)]], "valid = 0 never counts, any other value does")
    assert ctx.get_landmark_ids().tolist() == [4] and table.tentative() == ([], [], [])
    wild = [sighting(rng, -1), sighting(rng, 1024), sighting(rng, 5000), sighting(rng, 6)]
    judge_call(ctx, table, [wild], "ids outside the table pass untouched")
    assert ctx.get_slot_ekf_stats(0, 1)[0].tolist() == [4, 3, 0, 0] and ctx.get_landmark_ids().tolist() == [4, -1, 1024, 5000]


def test_full_lists():
    rng = np.random.RandomState(6)
    ctx, table = armed(ML=40, cap=128, min_sightings=3, max_gap=5)
    distinct = lambda: [sighting(rng, (5 * k + 1) % 1024) for k in range(128)]
    judge_call(ctx, table, [distinct(), distinct()], "128 distinct tentative ids")
    assert len(table.tentative()[0]) == 128 and ctx.get_landmark_ids().tolist() == []
    ctx.set_landmark_confirmation(min_sightings=2, max_gap=5)      # (a reseed: the 128 counts go)
    table = ConfirmTable(2, 5)
    same = lambda: [sighting(rng, 77) for _ in range(128)]
    judge_call(ctx, table, [same()], "128 sightings of one id")
    assert table.tentative() == ([77], [1], [0])
    judge_call(ctx, table, [same()[:30]], "30 sightings of one id, promoted: all pass")     # (each an augment: max_landmarks = 40)
    assert ctx.get_slot_ekf_stats(0, 1)[0].tolist() == [30, 30, 0, 0] and ctx.get_landmark_ids().tolist() == [77] * 30


def fleet_slots_in_ascending_order():
    rng = np.random.RandomState(7)
    ctx = context(16, batch=8)
    ctx.set_landmark_confirmation(min_sightings=3, max_gap=1)
    ctx.fleet_slam_begin([CAM] * 3)
    tables = [ConfirmTable(3, 1) for _ in range(3)]
    robots = [1, 0, 1, 2, 1, 0, 2, 1]                              # robot 1 in slots 0, 2, 4 and 7
    # robot 1 sees id 30 in its 2nd, 3rd and 4th slot (promoted in slot 7); taken in any other order the run would break (G = 1)
    lists = [[], [], [sighting(rng, 30)], [], [sighting(rng, 30), sighting(rng, 31)], [sighting(rng, 8)], [sighting(rng, 8)], [sighting(rng, 30)]]
    ctx.stage_encoders([0.0] * 8, [0.0] * 8, [0.0] * 8)
    for s, obs in enumerate(lists):
        inject(ctx, s, obs)
    ctx.fleet_run_staged(0, robots, with_ekf=2)
    ctx.sync()
    recs = ctx.get_slot_confirm(0, 8)
    for s, obs in enumerate(lists):
        want_valid, want_rec = tables[robots[s]].judge([o[0] for o in obs], [o[1] for o in obs])
        assert np.array_equal(ctx.get_slot_raw_observations(s)[1], np.array(want_valid, np.int32)), f"fleet slot {s}: valid"
        check_record(recs[s], want_rec, f"fleet slot {s}")
    assert int(recs[7]["promoted"]) == 1 and ctx.fleet_get_landmark_ids(1).tolist() == [30]
    for r in range(3):
        check_tentative(ctx.fleet_get_tentative(r), tables[r], f"robot {r}")
    assert tables[0].tentative() == ([8], [1], [0]) and tables[2].tentative() == ([8], [1], [0]) and tables[1].tentative() == ([31], [1], [1])


def test_fleet_slots_in_ascending_order():
    fleet_slots_in_ascending_order()


# ---- 2. twin equality ----------------------------------------------------------------------------------------------------------------------

K_TWIN, G_TWIN = 3, 6
FRAMES = 48
GHOST_EVERY = 3


def ghosted(stream, seed, first_ghost=600):
    """the stream's frames (lists only) with one single-frame ghost sighting, a fresh id each time, in every third frame"""
    rng = np.random.RandomState(seed)
    world = {o[0] for _, obs in stream for o in obs}
    out, g = [], first_ghost
    for f, (_, obs) in enumerate(stream):
        obs = list(obs)
        if f % GHOST_EVERY == 1:
            while g in world:
                g += 1
            obs.insert(int(rng.randint(0, len(obs) + 1)), sighting(rng, g))
            g += 1
        out.append(obs)
    return out


def single_twin(cap, windows, gate=False, L=12, m=4, batch=16, schedule=(1, 6, 16, 3, 16, 9)):
    """A: confirmation on, the raw stream.  B: confirmation off, the reference's withheld sightings injected with valid = 0."""
    stream = ring_stream(L, m, FRAMES, 11)
    lists = [[]] + ghosted(stream, 12)                             # the arming sample's empty list first
    enc = [(0.0, 0.0, 0.0)] + [e for e, _ in stream]
    table = ConfirmTable(K_TWIN, G_TWIN)
    flags = [table.judge([o[0] for o in obs], [o[1] for o in obs])[0] for obs in lists]
    assert sum(len(f) - sum(f) for f in flags) > FRAMES // GHOST_EVERY, "the reference withholds the ghosts and the first sightings of true ids"
    a, b = context(L + 4, batch, windows, cap), context(L + 4, batch, windows, cap)
    a.set_landmark_confirmation(min_sightings=K_TWIN, max_gap=G_TWIN)
    for ctx in (a, b):
        if gate:
            ctx.set_slam_gate(gate_d2=9.0)
            ctx.set_slam_gate_windows(windows)
    f, k = 0, 0
    while f < len(lists):
        n = min(schedule[k % len(schedule)], len(lists) - f)
        where = f"frames {f} .. {f + n - 1}"
        for ctx, fl in ((a, None), (b, flags)):
            ctx.stage_encoders(*[[e[c] for e in enc[f:f + n]] for c in range(3)])
            for s in range(n):
                inject(ctx, s, lists[f + s], None if fl is None else fl[f + s])
            ctx.run_staged(0, n, with_ekf=2)
        a.sync(); b.sync()
        assert_same(state_of(a), state_of(b), where)
        assert np.array_equal(a.get_slot_ekf_stats(0, n), b.get_slot_ekf_stats(0, n)), f"{where}: EKF statistics"
        for ga, gb in zip(a.get_observations(), b.get_observations()):
            assert np.array_equal(ga, gb), f"{where}: pop list"
        for s in range(n):
            assert np.array_equal(a.get_slot_raw_observations(s)[1], np.array(flags[f + s], np.int32)), f"{where}: flags of slot {s}"
        f += n; k += 1
    world = sorted({o[0] for _, obs in stream for o in obs})
    assert set(a.get_landmark_ids().tolist()) <= set(world) and len(a.get_landmark_ids()) >= m, "no ghost in the map, true ids in it"
    if windows:
        pa, pb = a.plan_stats(), b.plan_stats()
        assert pa == pb and pa["windows"] > 0 and pa["frames_in_windows"] > 0, f"windows were not formed in both twins: {pa}, {pb}"
    if gate:
        assert np.array_equal(a.get_slot_health(0, n), b.get_slot_health(0, n)) and a.get_track_health() == b.get_track_health()


def rig_twin():
    L, m, C, batch = 12, 4, 2, 8
    stream = ring_stream(L, m, FRAMES, 21)
    lists = [[]] + ghosted(stream, 22)
    enc = [(0.0, 0.0, 0.0)] + [e for e, _ in stream]
    table = ConfirmTable(K_TWIN, G_TWIN)
    # camera 0 takes the first two sightings of a step, camera 1 the rest and a second sighting of camera 0's first id
    rng = np.random.RandomState(23)
    cams = [(obs[:2], obs[2:] + ([sighting(rng, obs[0][0])] if obs and s % 5 == 2 else [])) for s, obs in enumerate(lists)]
    flags = []
    for c0, c1 in cams:
        fl = table.judge([o[0] for o in c0 + c1], [o[1] for o in c0 + c1])[0]          # the merged list: camera 0's, then camera 1's
        flags.append((fl[:len(c0)], fl[len(c0):]))
    a, b = context(L + 4, batch), context(L + 4, batch)
    a.set_landmark_confirmation(min_sightings=K_TWIN, max_gap=G_TWIN)
    for ctx in (a, b):
        ctx.set_camera_rig([CAM, CAM])
    steps = batch // C
    for f in range(0, len(lists), steps):
        n = min(steps, len(lists) - f)
        for ctx, use in ((a, False), (b, True)):
            ctx.stage_encoders(*[[e[c] for e in enc[f:f + n] for _ in range(C)] for c in range(3)])
            for s in range(n):
                for c in range(C):
                    inject(ctx, C * s + c, cams[f + s][c], flags[f + s][c] if use else None)
            ctx.run_staged_rig(0, n, with_ekf=2)
        a.sync(); b.sync()
        where = f"rig steps {f} .. {f + n - 1}"
        assert_same(state_of(a), state_of(b), where)
        assert np.array_equal(a.get_rig_step_ekf_stats(0, n), b.get_rig_step_ekf_stats(0, n)), f"{where}: EKF statistics"
        for ga, gb in zip(a.get_rig_observations(), b.get_rig_observations()):
            assert np.array_equal(ga, gb), f"{where}: pop list"
        recs = a.get_slot_confirm(batch, n)                          # a rig step's EKF slot: max_batch + step
        for s in range(n):
            assert int(recs[s]["withheld"]) == sum(len(x) - sum(x) for x in flags[f + s]), f"{where}: step {s} withheld"
            for c in range(C):                                       # the cameras' own lists are left as they were
                assert a.get_slot_raw_observations(C * s + c)[1].all() or not cams[f + s][c]
    assert len(a.get_landmark_ids()) >= m


def fleet_twin():
    L, m, R, batch = 12, 4, 3, 16
    streams = [ring_stream(L, m, FRAMES, 31 + r, 0.7 * r) for r in range(R)]
    lists = [[[]] + ghosted(s, 41 + r, 600 + 100 * r) for r, s in enumerate(streams)]
    enc = [[(0.0, 0.0, 0.0)] + [e for e, _ in s] for s in streams]
    tables = [ConfirmTable(K_TWIN, G_TWIN) for _ in range(R)]
    flags = [[tables[r].judge([o[0] for o in obs], [o[1] for o in obs])[0] for obs in lists[r]] for r in range(R)]
    a, b = context(L + 4, batch, windows=True), context(L + 4, batch, windows=True)
    a.set_landmark_confirmation(min_sightings=K_TWIN, max_gap=G_TWIN)
    for ctx in (a, b):
        ctx.fleet_slam_begin([CAM] * R)
    pattern = [0, 1, 2, 0, 1, 0, 0, 2, 1, 0, 0]                     # uneven: robot 0 six times a call, robot 1 three times, robot 2 twice
    at = [0] * R
    call = 0
    while at[0] < len(lists[0]):
        frames, taken = [], list(at)
        for r in pattern:
            if taken[r] < len(lists[r]):
                frames.append((r, taken[r])); taken[r] += 1
        for ctx, use in ((a, False), (b, True)):
            ctx.stage_encoders(*[[enc[r][f][c] for r, f in frames] for c in range(3)])
            for s, (r, f) in enumerate(frames):
                inject(ctx, s, lists[r][f], flags[r][f] if use else None)
            ctx.fleet_run_staged(0, [r for r, _ in frames], with_ekf=2)
        a.sync(); b.sync()
        where = f"fleet call {call}"
        for r in range(R):
            assert_same(state_of(a, r), state_of(b, r), f"{where}, robot {r}")
        assert np.array_equal(a.get_slot_ekf_stats(0, len(frames)), b.get_slot_ekf_stats(0, len(frames))), f"{where}: EKF statistics"
        at = taken
        call += 1
    assert call > 5 and all(len(a.fleet_get_landmark_ids(r)) >= m for r in range(R))
    for r in range(R):
        world = {o[0] for _, obs in streams[r] for o in obs}
        assert set(a.fleet_get_landmark_ids(r).tolist()) <= world, f"robot {r}: a ghost in the map"


TWINS = {
    "fast": lambda: single_twin(24, False),
    "general": lambda: single_twin(40, False, L=14, m=6),
    "windows": lambda: single_twin(24, True),
    "rig": rig_twin,
    "fleet": fleet_twin,
    "gate": lambda: single_twin(24, False, gate=True),
    "gate_windows": lambda: single_twin(24, True, gate=True),
}


@pytest.mark.parametrize("name", sorted(TWINS))
def test_twin(name):
    TWINS[name]()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TWINS))
def test_gpu_twin(name, on_emulation):
    assert not on_emulation
    TWINS[name]()


# ---- 3. end to end with the detector ------------------------------------------------------------------------------------------------------

def end_to_end(windows):
    """a blank arming frame and four renderings of one static 3-marker scene: with K = 3 the markers enter the map in slot 3"""
    rows, cols, n = 240, 320, 5
    ids, poses, K = synth.simple_scene(rows, cols, 300.0, 3, seed=2, tz=(0.9, 1.4))
    kw = dict(max_rows=rows, max_cols=cols, max_batch=8, persistent_waves=4, max_landmarks=16)
    if not windows:
        os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        a, b = capi.Context(**kw), capi.Context(**kw)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)
    enc = [0.0] + [0.4] * (n - 1), [0.0] + [0.5] * (n - 1), [0.0] + [DT] * (n - 1)
    for ctx in (a, b):
        ctx.set_camera(K, np.zeros(5))
        ctx.synth_render(0, rows, cols, K, [], np.zeros((0, 12)), seed=1, download=False)
        for s in range(1, n):
            ctx.synth_render(s, rows, cols, K, ids, poses, noise_amp=2, seed=10 + s, download=False)
        ctx.stage_encoders(*enc)
    a.set_landmark_confirmation(min_sightings=3, max_gap=5)
    a.run_staged(0, n, with_ekf=1)
    a.sync()
    b.run_staged(0, n, with_ekf=0)
    b.sync()
    table = ConfirmTable(3, 5)
    for s in range(n):
        i_, v_, z_, r_ = b.get_slot_raw_observations(s)
        assert sorted(i_.tolist()) == (sorted(ids.tolist()) if s else []) and v_.all(), f"slot {s}: the detector's list"
        fl, _ = table.judge(i_, v_)
        b.inject_observations(s, i_, fl, z_, r_)
        assert np.array_equal(a.get_slot_raw_observations(s)[1], np.array(fl, np.int32)), f"slot {s}: flags"
    b.run_staged(0, n, with_ekf=2)
    b.sync()
    assert_same(state_of(a), state_of(b), "end to end")
    stats = a.get_slot_ekf_stats(0, n)
    assert np.array_equal(stats, b.get_slot_ekf_stats(0, n))
    assert stats[:, 1].tolist() == [0, 0, 0, 3, 0] and stats[4].tolist() == [3, 0, 3, 0], f"augments per slot: {stats.tolist()}"
    assert sorted(a.get_landmark_ids().tolist()) == sorted(ids.tolist())


@pytest.mark.parametrize("windows", [True, False])
def test_end_to_end_with_the_detector(windows):
    end_to_end(windows)


@pytest.mark.gpu
@pytest.mark.parametrize("windows", [True, False])
def test_gpu_end_to_end_with_the_detector(windows, on_emulation):
    assert not on_emulation
    end_to_end(windows)


# ---- 4. seeding ---------------------------------------------------------------------------------------------------------------------------

def seeded_state(rng, ids):
    N = 3 + 3 * len(ids)
    A = rng.uniform(-1, 1, (N, N))
    return np.concatenate([np.zeros(3), rng.uniform(-3, 3, N - 3)]), 0.02 * (A @ A.T) / N + 0.05 * np.eye(N), np.array(ids, np.int32)


def expect_reseeded(ctx, rng, known, K, G, where):
    """the table is `known` confirmed, every count 0, t = 0: a known id passes, a new one is withheld for K - 1 frames"""
    table = ConfirmTable(K, G, known)
    check_tentative(ctx.get_tentative(), table, where)
    fresh = next(i for i in range(900, 1024) if i not in known)
    for k in range(K):
        judge_call(ctx, table, [[sighting(rng, i) for i in list(known)[:2]] + [sighting(rng, fresh)]], f"{where}, frame {k}")
        assert (fresh in ctx.get_landmark_ids().tolist()) == (k == K - 1), f"{where}: the new id entered after frame {k}"
    return table


def test_set_state_and_load_state_reseed(tmp_path):
    rng = np.random.RandomState(8)
    ctx, table = armed(min_sightings=3, max_gap=4)
    judge_call(ctx, table, [[sighting(rng, 5)], [sighting(rng, 5), sighting(rng, 6)]], "before the seat")
    assert table.tentative()[0] == [5, 6]
    ctx.set_state(*seeded_state(rng, [50, 51, 6]))
    table = expect_reseeded(ctx, rng, [50, 51, 6], 3, 4, "set_state")
    judge_call(ctx, table, [[sighting(rng, 60)]], "a count to lose")
    path = str(tmp_path / "state.bin")
    ctx.save_state(path)
    ctx.load_state(path)
    expect_reseeded(ctx, rng, ctx.get_landmark_ids().tolist(), 3, 4, "load_state")


def test_localize_end_reseeds():
    rng = np.random.RandomState(9)
    ctx, table = armed(min_sightings=2, max_gap=4)
    judge_call(ctx, table, [[sighting(rng, 5)]], "before localizing")
    ctx.localize_begin([70, 71], rng.uniform(-2, 2, (2, 3)), np.zeros(3), 0.01 * np.eye(3))
    with pytest.raises(capi.AslamError) as e:
        ctx.get_tentative()
    assert e.value.code == E_STATE
    ctx.localize_end()
    expect_reseeded(ctx, rng, [70, 71], 2, 4, "localize_end")


def test_remove_landmarks_reseeds():
    rng = np.random.RandomState(10)
    ctx = context(16)
    ctx.set_state(*seeded_state(rng, [20, 21, 22]))
    ctx.set_landmark_confirmation(min_sightings=3, max_gap=4)      # switched on in mid-run: the current map is confirmed
    table = expect_reseeded(ctx, rng, [20, 21, 22], 3, 4, "switched on in mid-run")
    judge_call(ctx, table, [[sighting(rng, 30)]], "a count to lose")
    assert table.tentative()[0] == [30]
    assert ctx.remove_landmarks([21]) == 1
    table = ConfirmTable(3, 4, ctx.get_landmark_ids().tolist())
    check_tentative(ctx.get_tentative(), table, "remove_landmarks: tentative counts restart")
    for k in range(3):                                             # the removed id is withheld again for K - 1 frames
        judge_call(ctx, table, [[sighting(rng, 21), sighting(rng, 20)]], f"removed id, frame {k}")
        assert (21 in ctx.get_landmark_ids().tolist()) == (k == 2)


def test_off_and_on_again_clears_counts():
    rng = np.random.RandomState(11)
    ctx, table = armed(min_sightings=3, max_gap=4)
    judge_call(ctx, table, [[sighting(rng, 5)], [sighting(rng, 5)]], "two of three")
    ctx.set_landmark_confirmation(None)
    assert ctx.get_landmark_confirmation() is None
    ctx.set_landmark_confirmation(min_sightings=3, max_gap=4)
    assert ctx.get_landmark_confirmation() == dict(min_sightings=3, max_gap=4)
    expect_reseeded(ctx, rng, [], 3, 4, "off and on again")


def test_fleet_seats_reseed():
    rng = np.random.RandomState(12)
    ctx = context(16, batch=8)
    ctx.set_landmark_confirmation(min_sightings=2, max_gap=4)
    ctx.fleet_slam_begin([CAM] * 2)
    tables = [ConfirmTable(2, 4), ConfirmTable(2, 4)]

    def call(lists, robots, where):
        ctx.stage_encoders([0.0] * len(lists), [0.0] * len(lists), [0.0] * len(lists))
        for s, obs in enumerate(lists):
            inject(ctx, s, obs)
        ctx.fleet_run_staged(0, robots, with_ekf=2)
        ctx.sync()
        for s, obs in enumerate(lists):
            fl, _ = tables[robots[s]].judge([o[0] for o in obs], [o[1] for o in obs])
            assert np.array_equal(ctx.get_slot_raw_observations(s)[1], np.array(fl, np.int32)), f"{where}, slot {s}"
        for r in range(2):
            check_tentative(ctx.fleet_get_tentative(r), tables[r], f"{where}, robot {r}")

    call([[], [], [sighting(rng, 5)], [sighting(rng, 5)]], [0, 1, 0, 1], "fleet: first sightings")
    ctx.fleet_set_state(1, *seeded_state(rng, [80, 81]))
    tables[1] = ConfirmTable(2, 4, [80, 81])                       # robot 1 reseeded, robot 0 keeps its count
    call([[sighting(rng, 5)], [sighting(rng, 5), sighting(rng, 80)]], [0, 1], "fleet_set_state")
    assert ctx.fleet_get_landmark_ids(0).tolist() == [5] and ctx.fleet_get_landmark_ids(1).tolist() == [80, 81]
    call([[sighting(rng, 9)], [sighting(rng, 5)]], [0, 1], "counts to lose")
    assert ctx.fleet_remove_landmarks([5], robots=[0]) .tolist() == [1]
    tables[0] = ConfirmTable(2, 4, [])                             # robot 0 alone: 5 must earn its place again, 9's count restarts
    call([[sighting(rng, 5), sighting(rng, 9)], [sighting(rng, 5)]], [0, 1], "fleet_remove_landmarks")
    assert ctx.fleet_get_landmark_ids(0).tolist() == [] and ctx.fleet_get_landmark_ids(1).tolist() == [80, 81, 5]
    ctx.fleet_slam_begin([CAM] * 2)                                # every robot anew
    tables[:] = [ConfirmTable(2, 4), ConfirmTable(2, 4)]
    call([[], []], [0, 1], "fleet_slam_begin")


# ---- 5. off means off -------------------------------------------------------------------------------------------------------------------

def test_off_means_off():
    L, m = 12, 4
    stream = ring_stream(L, m, 24, 51)
    lists = [[]] + ghosted(stream, 52)
    enc = [(0.0, 0.0, 0.0)] + [e for e, _ in stream]

    def run(ctx):
        ctx.profile_enable(True)
        ctx.profile_reset()
        out = []
        for f in range(0, len(lists), 8):
            n = min(8, len(lists) - f)
            ctx.stage_encoders(*[[e[c] for e in enc[f:f + n]] for c in range(3)])
            for s in range(n):
                inject(ctx, s, lists[f + s])
            ctx.run_staged(0, n, with_ekf=2)
            ctx.sync()
            out.append((ctx.get_state(), ctx.get_slot_ekf_stats(0, n), [ctx.get_slot_raw_observations(s)[1] for s in range(n)]))
        assert ctx.profile_get()["confirm"][0] == 0, "k_confirm ran"
        return out

    never = run(context(40))
    cleared = context(40)
    cleared.set_landmark_confirmation(min_sightings=2, max_gap=3)
    cleared.set_landmark_confirmation(None)
    got = run(cleared)
    for (sa, ta, va), (sb, tb, vb) in zip(never, got):
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and np.array_equal(ta, tb)
        assert all(np.array_equal(x, y) and x.all() for x, y in zip(va, vb))
    assert never[-1][0][0].size > 3 + 3 * L, "the untouched library took ghosts into the map"
    # localizing: the switch is set and nothing is judged
    rng = np.random.RandomState(53)
    world = rng.uniform(-2, 2, (3, 3))
    res = []
    for on in (False, True):
        ctx = context(16)
        if on:
            ctx.set_landmark_confirmation(min_sightings=2, max_gap=3)
        ctx.localize_begin([1, 2, 3], world, np.zeros(3), 0.01 * np.eye(3))
        ctx.profile_enable(True)
        ctx.profile_reset()
        r2 = np.random.RandomState(54)
        ctx.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
        inject(ctx, 0, [])
        inject(ctx, 1, [sighting(r2, 1), sighting(r2, 99), sighting(r2, 3)])
        ctx.run_staged(0, 2, with_ekf=2)
        ctx.sync()
        assert ctx.profile_get()["confirm"][0] == 0 and ctx.get_slot_raw_observations(1)[1].all()
        res.append(ctx.get_state())
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def refused(code, fn, *args, **kw):
    with pytest.raises(capi.AslamError) as e:
        fn(*args, **kw)
    assert e.value.code == code, f"{fn.__name__}{args}{kw}: {e.value}"


def test_refusals_leave_everything_untouched():
    rng = np.random.RandomState(13)
    ctx = context(16)
    for getter in (lambda: ctx.get_slot_confirm(0, 1), ctx.get_tentative, lambda: ctx.fleet_get_tentative(0)):
        refused(E_STATE, getter)                                   # the switch is off
    for bad in (dict(min_sightings=1), dict(min_sightings=128), dict(max_gap=0), dict(max_gap=1000001)):
        refused(E_INVALID, ctx.set_landmark_confirmation, **bad)
    assert ctx.get_landmark_confirmation() is None
    lib = capi.load()
    assert lib.aslam_set_landmark_confirmation(None, None) == E_INVALID and lib.aslam_get_slot_confirm(None, 0, 1, None) == E_INVALID
    assert lib.aslam_get_tentative(None, 0, None, None, None, None) == E_INVALID
    assert lib.aslam_fleet_get_tentative(None, 0, 0, None, None, None, None) == E_INVALID
    ctx.set_landmark_confirmation(min_sightings=3, max_gap=4)
    table = ConfirmTable(3, 4)
    judge_call(ctx, table, [[], [sighting(rng, 5), sighting(rng, 6)]], "a table to keep")
    before = (state_of(ctx), ctx.get_tentative(), ctx.get_slot_confirm(0, 16))
    for bad in (dict(min_sightings=1), dict(max_gap=0)):
        refused(E_INVALID, ctx.set_landmark_confirmation, **bad)
    for first, count in ((-1, 1), (0, 0), (0, 17), (16, 1), (10, 7)):
        refused(E_INVALID, ctx.get_slot_confirm, first, count)     # EKF slots are [0, 2 max_batch) = [0, 16)
    refused(E_STATE, ctx.fleet_get_tentative, 0)                   # not a SLAM fleet
    assert ctx.get_landmark_confirmation() == dict(min_sightings=3, max_gap=4)
    after = (state_of(ctx), ctx.get_tentative(), ctx.get_slot_confirm(0, 16))
    assert_same(before[0], after[0], "refusals")
    assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1])) and np.array_equal(before[2], after[2])
    check_tentative(after[1], table, "refusals")
    ctx.fleet_slam_begin([CAM] * 2)
    refused(E_STATE, ctx.get_tentative)                            # a fleet mode
    refused(E_INVALID, ctx.fleet_get_tentative, 2)
    refused(E_INVALID, ctx.fleet_get_tentative, -1)
    assert all(len(x) == 0 for x in ctx.fleet_get_tentative(1))
    ctx.fleet_end()
    ctx.fleet_begin([CAM], [1, 2], rng.uniform(-2, 2, (2, 3)), [np.zeros(3)], [0.01 * np.eye(3)])
    refused(E_STATE, ctx.get_tentative)
    refused(E_STATE, ctx.fleet_get_tentative, 0)                   # a localization fleet


# ---- 7. what it is for --------------------------------------------------------------------------------------------------------------------

def test_ghosts_stay_out_of_the_map():
    L, m, slots, G = 10, 4, 200, 10
    stream = ring_stream(L, m, slots, 61)
    world = sorted({o[0] for _, obs in stream for o in obs})
    assert len(world) == L
    rng = np.random.RandomState(62)
    fresh = iter(rng.permutation([i for i in range(1024) if i not in world]))       # a ghost id is never repeated at all
    lists = [[]]
    for f, (_, obs) in enumerate(stream):
        lists.append(list(obs) + ([sighting(rng, next(fresh))] if f % 3 == 0 else []))
    enc = [(0.0, 0.0, 0.0)] + [e for e, _ in stream]
    maps = {}
    for on in (True, False):
        ctx = context(40, batch=16)
        if on:
            ctx.set_landmark_confirmation(min_sightings=3, max_gap=G)
        try:
            for f in range(0, len(lists), 16):
                n = min(16, len(lists) - f)
                ctx.stage_encoders(*[[e[c] for e in enc[f:f + n]] for c in range(3)])
                for s in range(n):
                    inject(ctx, s, lists[f + s])
                ctx.run_staged(0, n, with_ekf=2)
                ctx.sync()
        except capi.AslamError as e:
            assert not on and e.code == -4, f"confirmation {on}: {e}"                # max_landmarks overflows on the ghosts
        maps[on] = ctx.get_landmark_ids().tolist()
    assert sorted(maps[True]) == world, f"with confirmation the map is {sorted(maps[True])}"
    assert set(maps[False]) - set(world), "without it the ghosts are landmarks"
