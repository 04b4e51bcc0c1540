"""Landmark removal on the device (aslam_remove_landmarks / aslam_fleet_remove_landmarks, csrc/map_edit.h).

Marginalising a landmark out of the filter deletes its rows and columns of mu and Sigma and computes nothing, so every comparison
in this file is np.array_equal: against numpy (`mu[sel]`, `sigma[np.ix_(sel, sel)]`) for the state, and against a twin context that
took the host route (get_state, delete on the host, set_state) for everything the filter does afterwards.  States come from
aslam_set_state and injected observations only.  Runs on the session's library: the CPU emulation without a GPU and, in the twins
marked gpu, the gfx950 library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from aruco_slam_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_CAPACITY, E_STATE = -1, -4, -5
WL, WR, DT = 2.0, 2.3, 1 / 30.0
MAP_DTYPE = np.dtype([("id", "<i4"), ("index", "<i4"), ("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("S", "<f8", (9,))])


def context(ML, batch=8, windows=False, cap=24):
    kw = dict(max_rows=64, max_cols=64, max_batch=batch, persistent_waves=4, max_landmarks=ML, max_updates_per_frame=cap)
    if windows:
        return capi.Context(**kw)
    os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        return capi.Context(**kw)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)


def inject(ctx, slot, obs):
    """obs: [(id, (x, y, theta), (r0, r1, r2))]"""
    ctx.inject_observations(slot, [o[0] for o in obs], [1] * len(obs), np.array([o[1] for o in obs]).reshape(-1, 3),
                            np.array([o[2] for o in obs]).reshape(-1, 3))


def observation(rng, lid):
    return (int(lid), np.array([rng.uniform(0.5, 2), rng.uniform(-1, 1), rng.uniform(-3, 3)]), rng.uniform(0.02, 0.2, 3))


def marked_state(L):
    """mu and a Sigma that is not symmetric, every entry distinct: a swap of the row and column maps or a stale read shows"""
    N = 3 + 3 * L
    i = np.arange(N, dtype=np.float64)
    return 0.125 + 0.25 * i, i[:, None] * 4096 + i[None, :] + 0.5


def spd_state(rng, L):
    N = 3 + 3 * L
    A = rng.uniform(-1, 1, (N, N))
    S = 0.02 * (A @ A.T) / N + 0.05 * np.eye(N)
    mu = np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-3, 3, 3 * L)])
    return mu, S


def removed_reference(mu, S, ids, remove):
    """numpy: the kept landmarks' entries"""
    ids = np.asarray(ids)
    keep = [i for i in range(len(ids)) if int(ids[i]) not in set(int(r) for r in remove)]
    sel = [0, 1, 2] + [3 + 3 * i + c for i in keep for c in range(3)]
    return mu[sel], S[np.ix_(sel, sel)], ids[keep].astype(np.int32), len(ids) - len(keep)


def state_of(ctx):
    mu, S = ctx.get_state()
    return mu, S, ctx.get_landmark_ids()


def assert_same(a, b, where):
    assert a[0].shape == b[0].shape, f"{where}: N {a[0].shape} against {b[0].shape}"
    assert np.array_equal(a[2], b[2]), f"{where}: landmark ids"
    assert np.array_equal(a[0], b[0]), f"{where}: mu"
    assert np.array_equal(a[1], b[1]), f"{where}: Sigma"
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all(), f"{where}: not finite"


# ---- 1. data movement --------------------------------------------------------------------------------------------------------------

# max_landmarks, L.  N = 93 of ld = 123: several row strips of k_map_cols, the last one partial; N = 603 = ld: a full map, two batches
# of columns in k_map_cols; N = 1053: two batches of rows in k_map_rows (1024 rows each) whenever N' > 1024
SHAPES = {"N93": (40, 30), "N603": (200, 200), "N1053": (350, 350)}


def landmark_ids(L):
    return ((7 * np.arange(L) + 3) % 1021).astype(np.int32)          # distinct, not in index order


def removal_sets(ids):
    L = len(ids)
    absent = int(next(i for i in range(1023, 0, -1) if i not in set(ids.tolist())))
    return {
        "none": [],
        "first": [ids[0]],
        "last": [ids[-1]],
        "every_second": list(ids[::2]),
        "middle_block": list(ids[L // 3: 2 * L // 3]),
        "all_but_one": [i for k, i in enumerate(ids) if k != L // 2],
        "all": list(ids),
        "untidy": sorted([ids[5], ids[5], absent, ids[9], ids[2], ids[L - 2]], reverse=True),
    }


SET_NAMES = list(removal_sets(landmark_ids(30)))
_SEEDS = {}


def seed(shape):
    if shape not in _SEEDS:
        ML, L = SHAPES[shape]
        _SEEDS[shape] = (*marked_state(L), landmark_ids(L))
    return _SEEDS[shape]


def data_movement(shape, name):
    ML, L = SHAPES[shape]
    mu, S, ids = seed(shape)
    remove = removal_sets(ids)[name]
    want = removed_reference(mu, S, ids, remove)
    ctx = context(ML)
    ctx.set_state(mu, S, ids)
    removed = ctx.remove_landmarks(remove)
    where = f"{shape}, {name}"
    assert removed == want[3], f"{where}: removed"
    got = state_of(ctx)
    assert_same(got, want[:3], where)
    rec = np.frombuffer(ctx.export_map(), dtype=MAP_DTYPE)
    Lk = len(want[2])
    assert np.array_equal(rec["id"][:Lk], want[2]) and np.array_equal(rec["index"][:Lk], np.arange(Lk)) and (rec["id"][Lk:] == -1).all(), \
        f"{where}: exported records"
    assert np.array_equal(rec["x"][:Lk], want[0][3::3]) and np.array_equal(rec["S"][:Lk, 1], np.array([want[1][3 + 3 * i, 4 + 3 * i] for i in range(Lk)]))
    fresh = context(ML)
    fresh.set_state(*got)
    assert_same(state_of(fresh), got, f"{where}: re-seeded")


@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_data_movement(shape, name):
    data_movement(shape, name)


def padding_is_zeroed():
    """what the removal vacates must read as the never-used part of a seeded filter does: the next augment builds on it"""
    ML, L = 40, 30
    rng = np.random.RandomState(5)
    mu, S = spd_state(rng, L)
    ids = landmark_ids(L)
    remove = list(ids[1::2])
    frame = [observation(rng, 900), observation(rng, ids[4])]
    out = []
    for route in ("device", "host"):
        ctx = context(ML)
        ctx.set_state(mu, S, ids)
        if route == "device":
            assert ctx.remove_landmarks(remove) == len(remove)
        else:
            ctx.set_state(*removed_reference(mu, S, ids, remove)[:3])
        ctx.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
        inject(ctx, 0, [])
        inject(ctx, 1, frame)
        ctx.run_staged(0, 2, with_ekf=2)
        ctx.sync()
        assert ctx.get_slot_ekf_stats(1, 1)[0].tolist() == [2, 1, 1, 0]
        out.append(state_of(ctx))
    assert out[0][0].size == 3 + 3 * (L - len(remove) + 1)
    assert_same(out[0], out[1], "augment after a removal")


def test_padding_is_zeroed():
    padding_is_zeroed()


def ids_seeded_twice():
    rng = np.random.RandomState(6)
    ids = np.array([5, 9, 5, 11, 9, 13], np.int32)
    mu, S = spd_state(rng, len(ids))
    ctx = context(10)
    ctx.set_state(mu, S, ids)
    assert ctx.remove_landmarks([5]) == 2, "both landmarks seeded with id 5 go"
    want = removed_reference(mu, S, ids, [5])
    assert_same(state_of(ctx), want[:3], "id seeded twice")
    assert want[2].tolist() == [9, 11, 9, 13]
    ctx.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
    inject(ctx, 0, [])
    inject(ctx, 1, [observation(rng, 9), observation(rng, 5)])
    ctx.run_staged(0, 2, with_ekf=2)
    ctx.sync()
    gi, gx, ga, _, _ = ctx.get_observations()
    pops = sorted(zip(gi.tolist(), gx.tolist(), ga.tolist()))
    # (the pop list reports a new observation with index -1; where it went shows in the landmark ids)
    assert pops == [(5, -1, 0), (9, 0, 1)], "the kept id is looked up at its first landmark; the removed one is new again"
    assert ctx.get_landmark_ids().tolist() == [9, 11, 9, 13, 5], "the removed id seen again is appended at index L'"


def test_ids_seeded_twice():
    ids_seeded_twice()


# ---- 2. workgroup order ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_removal_does_not_depend_on_the_workgroup_order(order, on_emulation):
    if not on_emulation:
        pytest.skip("a property of the CPU emulation build")
    env = dict(os.environ, HIPEMU_ORDER=order)
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_remove_landmarks.py"),
           "-k", "test_data_movement or test_padding_is_zeroed or test_ids_seeded_twice"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert f"{len(SHAPES) * len(SET_NAMES) + 2} passed" in out.stdout, out.stdout[-500:]


# ---- 3. the filter goes on ---------------------------------------------------------------------------------------------------------

def snapshot(ctx, slot):
    gi, gx, ga, gz, gR = ctx.get_observations()
    return (*state_of(ctx), gi, gx, ga, ctx.get_slot_ekf_stats(slot, 1)[0])


def filter_goes_on(windows, one_call=False):
    """a 12-landmark map built by augments, a few frames of updates, 3 ids removed, then 6 frames that see kept ids, a removed id
    again and a new id; the twin removes by the host route.  one_call: the 6 frames in one staged call (with windows on the host
    planner then plans them from the tables it reads back)"""
    rng = np.random.RandomState(11)
    ids = [101, 7, 55, 300, 12, 999, 64, 65, 400, 3, 250, 18]
    gone, new = [55, 12, 3], 777
    kept = [i for i in ids if i not in gone]
    before = [[]] + [[observation(rng, i) for i in ids]] + [[observation(rng, i) for i in rng.permutation(ids)[:7]] for _ in range(4)]
    after = [[observation(rng, i) for i in rng.permutation(kept)[:5]],
             [observation(rng, i) for i in [kept[0], gone[0], kept[3]]],
             [observation(rng, i) for i in [kept[1], new, kept[2]]],
             [observation(rng, i) for i in [gone[0], kept[4], new]],
             [observation(rng, i) for i in rng.permutation(kept)[:6]],
             [observation(rng, i) for i in rng.permutation(kept + [gone[0], new])[:8]]]
    nb, na = len(before), len(after)
    runs = []
    for route in ("device", "host"):
        ctx = context(40, batch=nb + na, windows=windows)
        ctx.stage_encoders([0.0] + [WL] * (nb + na - 1), [0.0] + [WR] * (nb + na - 1), [0.0] + [DT] * (nb + na - 1))
        for s, obs in enumerate(before + after):
            inject(ctx, s, obs)
        ctx.run_staged(0, nb, with_ekf=2)
        ctx.sync()
        order = ctx.get_landmark_ids().tolist()              # the heap order of the 12 equal keys decided the indices
        assert sorted(order) == sorted(ids)
        if route == "device":
            assert ctx.remove_landmarks(gone) == 3
        else:
            mu, S, lids = state_of(ctx)
            ctx.set_state(*removed_reference(mu, S, lids, gone)[:3])
        snaps = []
        if one_call:
            ctx.run_staged(nb, na, with_ekf=2)
            ctx.sync()
            snaps.append((*snapshot(ctx, nb + na - 1), ctx.get_slot_ekf_stats(nb, na)))
        else:
            for f in range(na):
                ctx.run_staged(nb + f, 1, with_ekf=2)
                ctx.sync()
                snaps.append(snapshot(ctx, nb + f))
        runs.append(snaps)
    dev, host = runs
    left = [i for i in order if i not in gone]
    if not one_call:
        gi, gx, ga = dev[1][3:6]
        assert (gone[0], -1, 0) in zip(gi.tolist(), gx.tolist(), ga.tolist()) and dev[1][2].tolist() == left + [gone[0]], \
            "a removed id comes back as a new landmark (action 0, reported with index -1) at index L'"
        assert dev[2][6].tolist() == [3, 1, 2, 0] and dev[3][6].tolist() == [3, 0, 3, 0]
    assert dev[-1][2].tolist() == left + [gone[0], new]
    for f, (a, b) in enumerate(zip(dev, host)):
        assert_same(a[:3], b[:3], f"frame {f} after the removal (windows {windows})")
        for k, what in ((3, "ids"), (4, "indices"), (5, "actions"), (6, "statistics")):
            assert np.array_equal(a[k], b[k]), f"frame {f} after the removal: {what} of the pop list"
        if one_call:
            assert np.array_equal(a[7], b[7])
    return ctx


def test_filter_goes_on_per_frame_chain():
    filter_goes_on(windows=False)


def test_filter_goes_on_with_windows():
    filter_goes_on(windows=True)
    ctx = filter_goes_on(windows=True, one_call=True)
    assert ctx.plan_stats()["frames_device_planned"] == 0, "the host planner did not follow the removal"


# ---- 4. last-observed list -----------------------------------------------------------------------------------------------------------

def last_observed_list():
    rng = np.random.RandomState(21)
    ids = np.array([40, 41, 42, 43], np.int32)
    A, B = 41, 43
    mu, S = spd_state(rng, 4)
    oA, oB = observation(rng, A), observation(rng, B)
    out = {}
    for route in ("device", "host", "device, empty frame"):
        ctx = context(8)
        ctx.set_state(mu, S, ids)
        ctx.stage_encoders([0.0, WL, WL], [0.0, WR, WR], [0.0, DT, DT])
        inject(ctx, 0, [])
        inject(ctx, 1, [oA, oB])
        inject(ctx, 2, [] if "empty" in route else [oA])
        ctx.run_staged(0, 2, with_ekf=2)
        ctx.sync()
        assert ctx.get_observations()[2].tolist() == [1, 1]
        if route == "host":
            ctx.set_state(*removed_reference(*state_of(ctx), [B])[:3])
        else:
            assert ctx.remove_landmarks([B]) == 1
        ctx.run_staged(2, 1, with_ekf=2)
        ctx.sync()
        out[route] = (state_of(ctx), ctx.get_observations()[2].tolist(), ctx.get_slot_ekf_stats(2, 1)[0].tolist())
    assert out["device"][1] == [2] and out["device"][2] == [1, 0, 0, 1], "the kept marker seen at the same place is the stationary no-op"
    assert_same(out["device"][0], out["device, empty frame"][0], "a stationary frame corrects nothing")
    assert out["host"][1] == [1] and out["host"][2] == [1, 0, 1, 0], "the host route empties the list: the same frame is an update"


def test_last_observed_list():
    last_observed_list()


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------------------

def capacity():
    rng = np.random.RandomState(31)
    ids = np.arange(10, 18, dtype=np.int32)
    mu, S = spd_state(rng, 8)
    frame = [observation(rng, 500), observation(rng, 12), observation(rng, 501), observation(rng, 15)]
    ctx = context(8)
    ctx.set_state(mu, S, ids)
    ctx.stage_encoders([0.0, WL, WL], [0.0, WR, WR], [0.0, DT, DT])
    inject(ctx, 0, [])
    inject(ctx, 1, frame)
    inject(ctx, 2, [(i, z + 0.05, r) for i, z, r in frame])
    ctx.run_staged(0, 2, with_ekf=2)
    with pytest.raises(capi.AslamError) as e:
        ctx.sync()
    assert e.value.code == E_CAPACITY and "mask 0x20" in str(e.value)
    gi, gx, ga, _, _ = ctx.get_observations()
    assert sorted(zip(gi.tolist(), gx.tolist(), ga.tolist())) == [(12, 2, 1), (15, 5, 1), (500, -1, 0), (501, -1, 0)]
    assert ctx.get_slot_ekf_stats(1, 1)[0].tolist() == [4, 0, 2, 0] and ctx.get_landmark_ids().tolist() == ids.tolist()
    assert ctx.remove_landmarks([10, 16]) == 2
    ctx.run_staged(2, 1, with_ekf=2)
    ctx.sync()
    gi, gx, ga, _, _ = ctx.get_observations()
    pops = sorted(zip(gi.tolist(), gx.tolist(), ga.tolist()))
    assert pops[:2] == [(12, 1, 1), (15, 4, 1)] and [p[0] for p in pops[2:]] == [500, 501] and all(p[2] == 0 for p in pops[2:])
    assert ctx.get_slot_ekf_stats(2, 1)[0].tolist() == [4, 2, 2, 0]
    lids = ctx.get_landmark_ids().tolist()
    assert lids[:6] == [11, 12, 13, 14, 15, 17] and sorted(lids[6:]) == [500, 501], "the two vacated places take the two new landmarks"


def test_capacity():
    capacity()


# ---- 6. fleet SLAM ---------------------------------------------------------------------------------------------------------------------

def fleet():
    rng = np.random.RandomState(41)
    ML, R = 12, 4
    maps = [[1, 2, 3, 4, 5, 6, 30], [2, 3, 7, 8, 1], [20, 21, 22], [4, 2, 3]]       # robot 2 has none of the ids, robot 3 loses its map
    remove = [2, 3, 4, 9]
    states = [(*spd_state(rng, len(m)), np.array(m, np.int32)) for m in maps]
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    fl = capi.Context(max_rows=64, max_cols=64, max_batch=R, persistent_waves=4, max_landmarks=ML, max_updates_per_frame=24)
    fl.fleet_slam_begin([cam] * R)
    singles = []
    for r, st in enumerate(states):
        fl.fleet_set_state(r, *st)
        one = context(ML, batch=2)
        one.set_state(*st)
        singles.append(one)

    def robot(r):
        return (*fl.fleet_get_state(r), fl.fleet_get_landmark_ids(r))

    listed = [3, 0, 2]
    removed = fl.fleet_remove_landmarks(remove, listed)
    assert removed.tolist() == [singles[r].remove_landmarks(remove) for r in listed] == [3, 3, 0]
    for r in listed:
        assert_same(robot(r), state_of(singles[r]), f"robot {r}")
        assert_same(robot(r), removed_reference(*states[r], remove)[:3], f"robot {r} against numpy")
    assert_same(robot(1), states[1], "robot 1 was not listed")
    assert robot(3)[0].size == 3
    removed = fl.fleet_remove_landmarks(remove)
    assert removed.tolist() == [0, singles[1].remove_landmarks(remove), 0, 0] == [0, 2, 0, 0]
    for r in range(R):
        assert_same(robot(r), state_of(singles[r]), f"robot {r}, second call")
    # one tick: every robot sees something it kept (if any), a removed id and a new one
    frames = [[observation(rng, i) for i in ([m[-1]] if r != 3 else []) + [2, 600 + r]] for r, m in enumerate(maps)]
    for f in range(2):
        for r in range(R):
            inject(fl, r, frames[r] if f else [])
        fl.stage_encoders(*[[v if f else 0.0] * R for v in (WL, WR, DT)])
        fl.fleet_run_staged(0, list(range(R)), with_ekf=2)
        fl.sync()
    stats = fl.get_slot_ekf_stats(0, R)
    for r, one in enumerate(singles):
        one.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
        inject(one, 0, [])
        inject(one, 1, frames[r])
        one.run_staged(0, 2, with_ekf=2)
        one.sync()
        assert_same(robot(r), state_of(one), f"robot {r} after a tick")
        assert stats[r].tolist() == one.get_slot_ekf_stats(1, 1)[0].tolist() == [len(frames[r]), 2, len(frames[r]) - 2, 0]
    merged = fl.fleet_merge_maps(anchor=0, min_common=2)[0].tolist()
    assert 2 in merged and not {3, 4} & set(merged), "a removed id that was not seen again is in no robot's map"
    assert fl.fleet_remove_landmarks([2]).tolist() == [1] * R
    assert 2 not in fl.fleet_merge_maps(anchor=0, min_common=2)[0].tolist()


def test_fleet():
    fleet()


# ---- 7. errors and modes -----------------------------------------------------------------------------------------------------------------

def code_of(call):
    with pytest.raises(capi.AslamError) as e:
        call()
    return e.value.code


def errors_and_modes():
    rng = np.random.RandomState(51)
    ids = np.array([1, 2, 3, 4, 5], np.int32)
    st = (*spd_state(rng, 5), ids)
    ctx = context(8)
    ctx.set_state(*st)
    lib, h = ctx.lib, ctx.h
    two = (capi.C.c_int * 2)(1, 2)
    n_removed = capi.C.c_int(-7)
    assert lib.aslam_remove_landmarks(None, 1, two, None) == E_INVALID
    assert lib.aslam_remove_landmarks(h, -1, two, capi.C.byref(n_removed)) == E_INVALID
    assert lib.aslam_remove_landmarks(h, 2, None, None) == E_INVALID
    for bad in (-1, 1024, 5000):
        assert code_of(lambda: ctx.remove_landmarks([1, bad])) == E_INVALID
    assert_same(state_of(ctx), st, "after the refused calls")
    assert ctx.remove_landmarks([]) == 0 and lib.aslam_remove_landmarks(h, 0, None, None) == 0
    assert_same(state_of(ctx), st, "after an empty removal")
    assert code_of(lambda: ctx.fleet_remove_landmarks([1])) == E_STATE, "the fleet call on a single filter"
    ctx.localize_begin(ids, st[0][3:].reshape(-1, 3), st[0][:3], 0.01 * np.eye(3))
    assert code_of(lambda: ctx.remove_landmarks([1])) == E_STATE, "while localizing the map is the caller's"
    ctx.localize_end()
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    ctx.fleet_begin([cam] * 2, ids, st[0][3:].reshape(-1, 3), np.zeros((2, 3)), np.stack([0.01 * np.eye(3)] * 2))
    assert code_of(lambda: ctx.remove_landmarks([1])) == E_STATE and code_of(lambda: ctx.fleet_remove_landmarks([1])) == E_STATE
    ctx.fleet_slam_begin([cam] * 3)
    assert code_of(lambda: ctx.remove_landmarks([1])) == E_STATE, "the single call in a SLAM fleet"
    for r in range(3):
        ctx.fleet_set_state(r, *st)
    one = (capi.C.c_int * 1)(1)
    for robots in ([0, 3], [-1], [1, 1], [0, 1, 0]):
        assert code_of(lambda: ctx.fleet_remove_landmarks([1], robots)) == E_INVALID, robots
    assert lib.aslam_fleet_remove_landmarks(h, 1, one, -1, one, None) == E_INVALID
    assert lib.aslam_fleet_remove_landmarks(h, -1, one, 1, one, None) == E_INVALID
    assert lib.aslam_fleet_remove_landmarks(h, 1, None, 1, one, None) == E_INVALID
    assert code_of(lambda: ctx.fleet_remove_landmarks([1024], [0])) == E_INVALID
    assert ctx.fleet_remove_landmarks([1], []).tolist() == [] and ctx.fleet_remove_landmarks([], [2, 0]).tolist() == [0, 0]
    for r in range(3):
        assert_same((*ctx.fleet_get_state(r), ctx.fleet_get_landmark_ids(r)), st, f"robot {r} after the refused calls")
    assert ctx.fleet_remove_landmarks([5, 1], [1]).tolist() == [2]
    assert ctx.fleet_get_landmark_ids(1).tolist() == [2, 3, 4] and ctx.fleet_get_landmark_ids(0).tolist() == ids.tolist()


def test_errors_and_modes():
    errors_and_modes()


def pending_batch_and_saved_state(tmp_path):
    """a staged call with windows on leaves its EKF work pending until the next call or sync: the removal finalises it first"""
    rng = np.random.RandomState(61)
    ids = np.arange(100, 110, dtype=np.int32)
    mu, S = spd_state(rng, 10)
    frames = [[]] + [[observation(rng, i) for i in ids[[1, 4, 7, 8]]] for _ in range(5)]
    got = []
    for sync_first in (False, True):
        ctx = context(16, batch=len(frames), windows=True)
        ctx.set_state(mu, S, ids)
        ctx.stage_encoders([0.0] + [WL] * 5, [0.0] + [WR] * 5, [0.0] + [DT] * 5)
        for s, obs in enumerate(frames):
            inject(ctx, s, obs)
        ctx.run_staged(0, len(frames), with_ekf=2)
        if sync_first:
            ctx.sync()
        assert ctx.remove_landmarks([104, 100, 109]) == 3
        got.append(state_of(ctx))
    assert_same(got[0], got[1], "removal behind a pending batch")
    assert not np.array_equal(got[0][0][:3], mu[:3]) and got[0][2].tolist() == [101, 102, 103, 105, 106, 107, 108]
    path = str(tmp_path / "state.bin")
    ctx.save_state(path)
    other = context(16)
    other.load_state(path)
    assert_same(state_of(other), got[0], "saved and loaded after a removal")


def test_pending_batch_and_saved_state(tmp_path):
    pending_batch_and_saved_state(tmp_path)


# ---- the same on the real library ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_data_movement_on_gpu(shape, name):
    data_movement(shape, name)


@pytest.mark.gpu
def test_padding_and_ids_seeded_twice_on_gpu():
    padding_is_zeroed()
    ids_seeded_twice()


@pytest.mark.gpu
def test_filter_goes_on_on_gpu():
    filter_goes_on(windows=False)
    filter_goes_on(windows=True)
    filter_goes_on(windows=True, one_call=True)


@pytest.mark.gpu
def test_last_observed_list_and_capacity_on_gpu():
    last_observed_list()
    capacity()


@pytest.mark.gpu
def test_fleet_on_gpu():
    fleet()


@pytest.mark.gpu
def test_errors_modes_pending_batch_and_saved_state_on_gpu(tmp_path):
    errors_and_modes()
    pending_batch_and_saved_state(tmp_path)
