"""Fleet SLAM: R robots, one camera and one complete EKF-SLAM filter each, in one context (aslam_fleet_slam_begin, the chain kernels'
EkfFleet instantiations, ekf_fleet_slam.h).

Every robot must produce bit for bit what one SLAM context produces on the same frames (aslam_set_camera_rig with that robot's one
camera, the same aslam_init, windows off, aslam_run_staged_rig), and stay within rounding of a windowed context and of the
references."""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from oracle import pyoracle as orc
from tests.test_fleet import MOUNTS4, ring_cams, render_fleet, same_dets
from tests.test_localize import E_INVALID, E_STATE, _Injected, emu_context, inject, make_sequence, random_map, ring_1280, small_ring

E_CAPACITY = -4


def no_windows_context(**kw):
    os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        return capi.Context(**kw)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)


def run_single(w, cam, frames, batch, windows, **kw):
    """one SLAM context (C = 1 rig) on frames = [(img, Frame)] in calls of `batch` steps: mu, Sigma, ids, per-step stats, detections"""
    cfg = w.cfg
    kw = dict(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=batch, **kw)
    ctx = capi.Context(**kw) if windows else no_windows_context(**kw)
    synth.apply_detector(cfg, ctx=ctx)
    ctx.set_camera_rig([cam])
    stats, dets = [], []
    for f0 in range(0, len(frames), batch):
        chunk = frames[f0:f0 + batch]
        ctx.stage_frames(np.stack([im for im, _ in chunk]))
        ctx.stage_encoders([fr.wl for _, fr in chunk], [fr.wr for _, fr in chunk], [fr.dt for _, fr in chunk])
        ctx.run_staged_rig(0, len(chunk), with_ekf=True)
        ctx.sync()
        stats += ctx.get_rig_step_ekf_stats(0, len(chunk)).tolist()
        dets += [ctx.get_slot_detections(s) for s in range(len(chunk))]
    mu, S = ctx.get_state()
    return mu, S, ctx.get_landmark_ids(), np.array(stats), dets


def fleet_state(ctx, r):
    mu, S = ctx.fleet_get_state(r)
    return mu, S, ctx.fleet_get_landmark_ids(r)


def assert_close(a, b, where, tol=1e-9):
    assert a[0].shape == b[0].shape and np.array_equal(a[2], b[2]), f"{where}: map size / landmark ids differ"
    assert np.abs(a[0] - b[0]).max() <= tol, f"{where}: mu differs by {np.abs(a[0] - b[0]).max()}"
    assert np.abs(a[1] - b[1]).max() <= tol * np.abs(b[1]).max(), f"{where}: Sigma differs"


# ---- CPU emulation -----------------------------------------------------------------------------------------------------------------

_FRAMES = {}


def small_fleet():
    """R = 3 robots at different phases of the 240 x 320 ring, cameras differing in f and mount (one rear-facing, one distorted),
    13 ticks rendered once per session"""
    if not _FRAMES:
        w = synth.RingWorld(small_ring())
        cams = ring_cams(w, [260.0, 240.0, 280.0], [(0.12, 0.02, 0.0), (-0.15, -0.03, math.pi), (0.0, 0.1, math.pi / 2)])
        cams[1] = (cams[1][0], np.array([0.01, -0.004, 0.0, 0.0, 0.0]), cams[1][2])
        r = capi.Context(max_rows=w.cfg.rows, max_cols=w.cfg.cols, max_batch=1, persistent_waves=4)
        _FRAMES.update(w=w, cams=cams, frames=render_fleet(r, w, cams, [0, 40, 80], 13))
    return _FRAMES["w"], _FRAMES["cams"], _FRAMES["frames"]


@pytest.mark.parametrize("cap", [24, 64, 128])
def test_fleet_slam_equals_independent_contexts(cap):
    """one staged call from a nonzero slot (the robots' slots interleaved) and one aslam_fleet_add_images per tick both equal three
    windows-off SLAM contexts bit for bit, and a default (windowed) context to 1e-9; cap selects the chain (24 fast, 64 medium, 128
    general), so every chain kernel runs in its fleet instantiation"""
    w, cams, frames = small_fleet()
    cfg = w.cfg
    R, T = 3, len(frames)
    kw = dict(max_landmarks=w.L + 8, persistent_waves=4, max_updates_per_frame=cap)
    F0 = 5
    staged = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=F0 + R * T, **kw)
    staged.fleet_slam_begin(cams)
    assert staged.is_fleet() == R and staged.is_fleet_slam()
    robots = [r for t in range(T) for r in range(R)]
    staged.stage_frames(np.stack([frames[t][r][0] for t in range(T) for r in range(R)]), slot0=F0)
    staged.stage_encoders(*[[getattr(frames[t][r][1], k) for t in range(T) for r in range(R)] for k in ("wl", "wr", "dt")], slot0=F0)
    staged.fleet_run_staged(F0, robots)
    staged.sync()
    st_stats = staged.get_slot_ekf_stats(F0, R * T)
    st_dets = [staged.get_slot_detections(F0 + s) for s in range(R * T)]

    tick = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=R, **kw)
    tick.fleet_slam_begin(cams)
    tk_stats, tk_dets = [], []
    for t in range(T):
        tick.fleet_add_images(range(R), [frames[t][r][0] for r in range(R)],
                              *[[getattr(frames[t][r][1], k) for r in range(R)] for k in ("wl", "wr", "dt")])
        tk_stats += tick.get_slot_ekf_stats(0, R).tolist()
        tk_dets += [tick.get_slot_detections(r) for r in range(R)]
    tk_stats = np.array(tk_stats)
    poses, sigs = staged.fleet_get_poses()

    for r in range(R):
        own = [frames[t][r] for t in range(T)]
        mu, S, ids, stats, dets = run_single(w, cams[r], own, T, windows=False, **kw)
        for name, ctx in (("staged", staged), ("per tick", tick)):
            fm, fS, fids = fleet_state(ctx, r)
            assert np.array_equal(fm, mu) and np.array_equal(fS, S), f"robot {r}: {name} fleet != single context"
            assert np.array_equal(fids, ids), f"robot {r}: {name} landmark ids"
        assert np.array_equal(st_stats[r::R], stats) and np.array_equal(tk_stats[r::R], stats), f"robot {r}: slot stats"
        for t in range(T):
            assert same_dets(st_dets[t * R + r], dets[t]) and same_dets(tk_dets[t * R + r], dets[t]), f"robot {r} tick {t}: detections"
        assert np.array_equal(poses[r], mu[:3]) and np.array_equal(sigs[r], S[:3, :3]), f"robot {r}: fleet_get_poses"
        assert stats[:, 1].sum() >= 3 and stats[:, 2].sum() >= T, f"robot {r}: too little appended / fused ({stats.sum(0)})"
        win = run_single(w, cams[r], own, T, windows=True, **kw)
        assert_close((mu, S, ids), win[:3], f"robot {r}: windowed context")


def test_out_of_order_arrival_equals_own_subsequence():
    """calls carrying changing subsets of robots, one robot several times in a call: each robot equals a windows-off single context fed
    its own subsequence (injected observations), and a robot's bits do not depend on which other robots run beside it"""
    rng = np.random.RandomState(7)
    ids, xyth = random_map(rng, 12)
    seqs = [make_sequence(70 + r, 9, ids, xyth) for r in range(3)]
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    calls = [(2, [1, 0, 1, 1]), (0, [2, 1, 0]), (3, [0, 2, 2, 1]), (1, [0, 0, 0])]      # (first slot, robot of each slot)

    def run(present):
        fleet = emu_context(8, max_landmarks=40)
        fleet.fleet_slam_begin([cam] * 3)
        done, sub = [0, 0, 0], [[], [], []]
        for first, order in calls:
            order = [r for r in order if r in present]
            if not order:
                continue
            frs = []
            for r in order:
                frs.append(seqs[r][done[r]])
                sub[r].append(seqs[r][done[r]])
                done[r] += 1
            for s, fr in enumerate(frs):
                inject(fleet, first + s, fr[3])
            fleet.stage_encoders([f[0] for f in frs], [f[1] for f in frs], [f[2] for f in frs], slot0=first)
            fleet.fleet_run_staged(first, order, with_ekf=2)
            fleet.sync()
        return fleet, sub

    fleet, sub = run({0, 1, 2})
    for r in range(3):
        one = no_windows_context(max_rows=64, max_cols=64, max_batch=8, persistent_waves=4, max_landmarks=40)
        for s, fr in enumerate(sub[r]):
            inject(one, s, fr[3])
        one.stage_encoders([f[0] for f in sub[r]], [f[1] for f in sub[r]], [f[2] for f in sub[r]])
        one.run_staged(0, len(sub[r]), with_ekf=2)
        mu, S = one.get_state()
        fm, fS, fids = fleet_state(fleet, r)
        assert np.array_equal(fm, mu) and np.array_equal(fS, S) and np.array_equal(fids, one.get_landmark_ids()), f"robot {r}"
        assert fm.size > 3
    alone, _ = run({1})
    for a, b in zip(fleet_state(fleet, 1), fleet_state(alone, 1)):
        assert np.array_equal(a, b), "robot 1 changed with the robots beside it"


def test_injected_against_literal_reference():
    """with_ekf = 2 per robot against oracle/ekf_literal.py: new ids, repeated ids in one frame, gated observations, stationary no-ops,
    maps of different sizes per robot, robots interleaved in one staged call per half"""
    rng = np.random.RandomState(21)
    ids, xyth = random_map(rng, 30, id_pool=500)
    R, T = 4, 12
    seqs = [make_sequence(90 + r, T, ids[: 6 + 6 * r], xyth[: 6 + 6 * r]) for r in range(R)]       # different maps per robot
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    fleet = emu_context(R * T, max_landmarks=64)
    fleet.fleet_slam_begin([cam] * R)
    refs = [_Injected() for _ in range(R)]
    tnow = [0.0] * R
    seen = dict(new=0, dup=0, gated=0, stationary=0)
    for half in range(2):
        t0, t1 = half * T // 2, (half + 1) * T // 2
        order = [r for t in range(t0, t1) for r in range(R)]
        frs = [seqs[r][t] for t in range(t0, t1) for r in range(R)]
        for s, fr in enumerate(frs):
            inject(fleet, s, fr[3])
        fleet.stage_encoders([f[0] for f in frs], [f[1] for f in frs], [f[2] for f in frs])
        fleet.fleet_run_staged(0, order, with_ekf=2)
        stats = fleet.get_slot_ekf_stats(0, len(order))
        for s, (r, fr) in enumerate(zip(order, frs)):
            tnow[r] += fr[2]
            refs[r].add_encoder(fr[0], fr[1], tnow[r])
            refs[r]._obs = fr[3]
            k = len(fr[3])
            refs[r].add_poses(list(range(k)), np.zeros((k, 8)), np.zeros((k, 3)), np.zeros((k, 3)))
            acts = [a for _, _, a in refs[r].log]
            assert stats[s].tolist() == [k, acts.count(0), acts.count(1), acts.count(2)], f"slot {s} (robot {r})"
            seen["new"] += acts.count(0)
            seen["stationary"] += acts.count(2)
            seen["gated"] += sum(1 for o in fr[3] if not o[1])
            vid = [o[0] for o in fr[3] if o[1]]
            seen["dup"] += len(vid) != len(set(vid))
        for r in range(R):
            mu, S, lids = fleet_state(fleet, r)
            ref = refs[r]
            assert mu.shape == ref.mu.shape, f"robot {r}, half {half}: map size"
            assert np.abs(mu - ref.mu).max() <= 1e-9, f"robot {r}, half {half}: mu"
            assert np.abs(S - ref.sigma).max() <= 1e-9 * np.abs(ref.sigma).max(), f"robot {r}, half {half}: Sigma"
            assert lids.size == (mu.size - 3) // 3 and set(lids.tolist()) == set(ref.id_map), f"robot {r}: landmark ids"
    sizes = [fleet_state(fleet, r)[0].size for r in range(R)]
    assert len(set(sizes)) >= 3, sizes
    assert all(v > 0 for v in seen.values()), seen


def test_mode_and_argument_rules(tmp_path):
    ctx = emu_context(4, max_landmarks=4)
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    fresh_mu, fresh_S = ctx.get_state()
    ids = np.array([3, 7, 9], np.int32)
    xyth = np.array([[1.0, 0.0, 3.1], [0.0, 1.0, -1.5], [-1.0, -1.0, 0.7]])
    pose0, sig0 = np.array([0.1, -0.2, 0.3]), np.diag([0.02, 0.03, 0.01])

    def refused(code, fn, *a):
        with pytest.raises(capi.AslamError) as e:
            fn(*a)
        assert e.value.code == code, (fn, e.value)

    # the per-robot calls outside fleet SLAM: no fleet, then a localization fleet
    assert not ctx.is_fleet_slam()
    for fn, a in [(ctx.fleet_get_state, (0,)), (ctx.fleet_set_state, (0, fresh_mu, fresh_S, [])), (ctx.fleet_get_landmark_ids, (0,))]:
        refused(E_STATE, fn, *a)
    # begin: robot count, cameras, localizing
    refused(E_INVALID, ctx.fleet_slam_begin, [cam] * 5)                                   # R > max_batch
    refused(E_INVALID, ctx.fleet_slam_begin, [])
    big = emu_context(300, max_landmarks=2)
    refused(E_INVALID, big.fleet_slam_begin, [cam] * 257)                                  # R > ASLAM_MAX_ROBOTS
    big.close()
    refused(E_INVALID, ctx.fleet_slam_begin, [(cam[0], np.zeros(6), (0.0, 0.0, 0.0))])
    refused(E_INVALID, ctx.fleet_slam_begin, [(cam[0], np.zeros(5), (0.0, 0.0, -math.pi))])
    refused(E_INVALID, ctx.fleet_slam_begin, [(cam[0], np.zeros(5), (np.nan, 0.0, 0.0))])
    loc = emu_context(2, max_landmarks=6)
    loc.localize_begin(ids, xyth, pose0, sig0)
    refused(E_STATE, loc.fleet_slam_begin, [cam])
    assert ctx.is_fleet() == 0
    ctx.fleet_begin([cam], ids, xyth, [pose0], [sig0])
    refused(E_STATE, ctx.fleet_get_state, 0)

    # a SLAM fleet replaces the localization fleet
    ctx.fleet_slam_begin([cam, cam])
    assert ctx.is_fleet() == 2 and ctx.is_fleet_slam()
    assert ctx.get_landmark_ids().size == 0
    for r in range(2):
        mu, S, lids = fleet_state(ctx, r)
        assert np.array_equal(mu, fresh_mu) and np.array_equal(S, fresh_S) and lids.size == 0
    refused(E_STATE, ctx.fleet_set_pose, 0, pose0, sig0)
    for fn, a in [(ctx.fleet_get_state, (2,)), (ctx.fleet_get_state, (-1,)), (ctx.fleet_get_landmark_ids, (2,)),
                  (ctx.fleet_set_state, (2, fresh_mu, fresh_S, [])), (ctx.fleet_run_staged, (0, [0, 2], 2))]:
        refused(E_INVALID, fn, *a)
    refused(E_CAPACITY, ctx.fleet_set_state, 0, np.zeros(18), np.eye(18), [1, 2, 3, 4, 5])   # 5 landmarks > max_landmarks 4
    img = np.full((64, 64), 128, np.uint8)
    dev_buf = np.zeros(64, np.uint8)

    def comm_gather():
        ctx._ck(ctx.lib.aslam_comm_gather_maps(ctx.h, dev_buf.ctypes.data, 0))
    for fn, a in [(ctx.add_encoder, (1.0, 1.0, 0.1)), (ctx.add_image, (img,)), (ctx.add_images, ([img],)),
                  (ctx.run_staged, (0, 1, True)), (ctx.run_staged, (0, 1, 2)), (ctx.run_staged_rig, (0, 1, True)),
                  (ctx.stream_open, (64, 64, 1, 1)), (ctx.stream_slot, (64, 64)), (ctx.stream_commit, (1.0, 1.0, 0.05)),
                  (ctx.stream_push, (img, 1.0, 1.0, 0.05)), (ctx.stream_flush, ()), (ctx.export_map_async, (dev_buf.ctypes.data, 0)),
                  (comm_gather, ()), (ctx.localize_begin, (ids, xyth, pose0, sig0)), (ctx.localize_end, ()),
                  (ctx.get_state, ()), (ctx.set_state, (fresh_mu, fresh_S, [])), (ctx.save_state, (str(tmp_path / "s.bin"),)),
                  (ctx.load_state, (str(tmp_path / "s.bin"),)), (ctx.pose_msg, ()), (ctx.map_markers, ()), (ctx.detected_markers, ()),
                  (ctx.draw_detected_markers, (np.zeros((64, 64, 3), np.uint8),)), (ctx.get_observations, ()),
                  (ctx.get_rig_observations, ()), (ctx.export_map, ()), (ctx.set_camera, (cam[0], np.zeros(5))),
                  (ctx.set_camera_rig, ([cam],))]:
        refused(E_STATE, fn, *a)
    assert not (tmp_path / "s.bin").exists()

    # set_state: that robot only, its last-observed list emptied, its armed flag kept
    mu1 = np.array([0.5, 0.1, 0.2, 1.0, 2.0, 0.3])
    S1 = np.diag([0.01, 0.02, 0.03, 0.1, 0.1, 0.05])
    refused(E_INVALID, ctx.fleet_set_state, 1, mu1, S1, [1024])
    ctx.fleet_set_state(1, mu1, S1, [7])
    m, S, lids = fleet_state(ctx, 1)
    assert np.array_equal(m, mu1) and np.array_equal(S, S1) and lids.tolist() == [7]
    assert fleet_state(ctx, 0)[0].size == 3
    ctx.stage_encoders([1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.05, 0.05, 0.05])
    z7 = (7, 1, np.array([0.5, 1.0, -1.9]), np.full(3, 0.02))
    inject(ctx, 0, [z7])
    inject(ctx, 1, [z7])
    inject(ctx, 2, [z7, (8, 1, np.array([1.0, 0.0, 0.0]), np.full(3, 0.02))])
    ctx.fleet_run_staged(0, [1, 1, 0], with_ekf=2)                  # robot 1 arms and corrects id 7, then "stationary"; robot 0 arms
    assert ctx.get_slot_ekf_stats(0, 3).tolist() == [[1, 0, 1, 0], [1, 0, 0, 1], [2, 2, 0, 0]]
    assert fleet_state(ctx, 0)[2].tolist() == [7, 8] and fleet_state(ctx, 1)[2].tolist() == [7]
    ctx.fleet_set_state(1, mu1, S1, [7])                               # armed stays: the next frame predicts; list emptied: no "stationary"
    inject(ctx, 0, [z7])
    ctx.fleet_run_staged(0, [1], with_ekf=2)
    assert ctx.get_slot_ekf_stats(0, 1).tolist() == [[1, 0, 1, 0]]
    assert not np.array_equal(ctx.fleet_get_poses()[0][1], mu1[:3])

    # a robot that overflows its map: ASLAM_E_CAPACITY at the next sync, the other robot exact
    before = fleet_state(ctx, 1)
    inject(ctx, 0, [(20 + k, 1, np.array([1.0 + k, 0.5, 0.1]), np.full(3, 0.02)) for k in range(4)])   # robot 0 holds 2: room for 2
    inject(ctx, 1, [])
    ctx.stage_encoders([1.0, 1.0], [2.0, 2.0], [0.05, 0.05])
    ctx.fleet_run_staged(0, [0, 1], with_ekf=2)
    refused(E_CAPACITY, ctx.sync)
    lids = fleet_state(ctx, 0)[2].tolist()
    assert lids[:2] == [7, 8] and len(lids) == 4 and set(lids[2:]) < {20, 21, 22, 23}      # new ids pop in heap order
    one = no_windows_context(max_rows=64, max_cols=64, max_batch=1, persistent_waves=4, max_landmarks=4)
    one.stage_encoders([1.0], [2.0], [0.05])
    inject(one, 0, [])
    one.run_staged(0, 1, with_ekf=2)                                   # arms it, as robot 1 is armed
    one.set_state(*before[:2], before[2])
    one.run_staged(0, 1, with_ekf=2)
    mu, S = one.get_state()
    assert np.array_equal(fleet_state(ctx, 1)[0], mu) and np.array_equal(fleet_state(ctx, 1)[1], S)

    # back to a localization fleet, then to the single filter as aslam_create leaves it
    ctx.fleet_begin([cam], ids, xyth, [pose0], [sig0])
    assert ctx.is_fleet() == 1 and not ctx.is_fleet_slam()
    refused(E_STATE, ctx.fleet_get_landmark_ids, 0)
    ctx.fleet_slam_begin([cam])
    ctx.fleet_end()
    assert ctx.is_fleet() == 0 and not ctx.is_fleet_slam()
    refused(E_STATE, ctx.fleet_get_state, 0)
    mu, S = ctx.get_state()
    assert np.array_equal(mu, fresh_mu) and np.array_equal(S, fresh_S) and ctx.get_landmark_ids().size == 0
    inject(ctx, 0, [(42, 1, np.array([1.0, 0.0, 0.0]), np.full(3, 0.02))])
    ctx.stage_encoders([1.0], [2.0], [0.05])
    ctx.run_staged(0, 1, with_ekf=2)                                    # the first sample arms, the new id is appended
    ctx.sync()
    assert ctx.get_landmark_ids().tolist() == [42]


# ---- on the MI355X at 1280 x 720 ---------------------------------------------------------------------------------------------------

FRONT8 = [(0.20, 0.0, 0.0), (0.15, 0.05, 0.0), (0.10, -0.05, 0.0), (0.25, 0.0, 0.0)] * 2


def gpu_fleet(w, cams, batch):
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=batch, max_landmarks=w.L + 8)
    synth.apply_detector(cfg, ctx=ctx)
    ctx.fleet_slam_begin(cams)
    return ctx


@pytest.mark.gpu
def test_gpu_fleet_slam_lap_equals_independent_contexts():
    """R = 8 robots, front cameras of two focal lengths at different mounts, one lap in staged calls of 40 slots: each robot == a
    windows-off single context, and within 1e-9 of the C++ oracle (oracle/pyoracle.py Slam) on its frames"""
    w = synth.RingWorld(ring_1280(80))
    cfg = w.cfg
    R, B = 8, 40
    cams = ring_cams(w, [cfg.f] * 4 + [0.9 * cfg.f] * 4, FRONT8)
    L = w.lap_length()
    phases = [(r * L) // R for r in range(R)]
    fleet = gpu_fleet(w, cams, B)
    per = B // R
    singles = []
    for r in range(R):
        s = no_windows_context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=per, max_landmarks=w.L + 8)
        synth.apply_detector(cfg, ctx=s)
        s.set_camera_rig([cams[r]])
        singles.append(s)
    own = [[] for _ in range(R)]
    for t0 in range(0, L, per):
        nt = min(per, L - t0)
        frames = render_fleet(fleet, w, cams, phases, nt, t0)
        fleet.stage_frames(np.stack([frames[t][r][0] for t in range(nt) for r in range(R)]))
        fleet.stage_encoders(*[[getattr(frames[t][r][1], k) for t in range(nt) for r in range(R)] for k in ("wl", "wr", "dt")])
        fleet.fleet_run_staged(0, [r for t in range(nt) for r in range(R)])
        fleet.sync()
        stats = fleet.get_slot_ekf_stats(0, nt * R)
        for r in range(R):
            s = singles[r]
            s.stage_frames(np.stack([frames[t][r][0] for t in range(nt)]))
            s.stage_encoders(*[[getattr(frames[t][r][1], k) for t in range(nt)] for k in ("wl", "wr", "dt")])
            s.run_staged_rig(0, nt, with_ekf=True)
            s.sync()
            assert np.array_equal(stats[r::R], s.get_rig_step_ekf_stats(0, nt)), f"robot {r}, ticks from {t0}"
            own[r] += [frames[t][r] for t in range(nt)]
    for r in range(R):
        mu, S = singles[r].get_state()
        fm, fS, fids = fleet_state(fleet, r)
        assert np.array_equal(fm, mu) and np.array_equal(fS, S) and np.array_equal(fids, singles[r].get_landmark_ids()), f"robot {r}"
        assert fids.size >= w.L // 2, f"robot {r}: {fids.size} landmarks"

    def oracle(r):
        o = orc.Slam(literal=False, r2c_tx=cams[r][2][0], r2c_ty=cams[r][2][1])
        synth.apply_detector(cfg, oracle=o)
        o.set_camera(cams[r][0], cams[r][1])
        t = 0.0
        for img, fr in own[r]:
            t += fr.dt
            o.add_encoder(fr.wl, fr.wr, t)
            o.add_image(img)
        return o.get_state() + (o.landmark_ids(),)

    with ThreadPoolExecutor(8) as ex:
        refs = list(ex.map(oracle, range(R)))
    for r, (mu_o, S_o, ids_o) in enumerate(refs):
        fm, fS, fids = fleet_state(fleet, r)
        assert mu_o.shape == fm.shape and np.array_equal(ids_o, fids), f"robot {r}: map {fm.size} vs oracle {mu_o.size}, or its ids"
        assert np.abs(mu_o - fm).max() < 1e-9, f"robot {r}: mu differs from the oracle by {np.abs(mu_o - fm).max()}"
        assert np.abs(S_o - fS).max() < 1e-9 * np.abs(S_o).max(), f"robot {r}: Sigma differs from the oracle"


@pytest.mark.gpu
def test_gpu_many_robots_ticks_equal_staged():
    """R = 64 robots, 20 ticks through aslam_fleet_add_images == the same frames staged, two ticks per staged call"""
    w = synth.RingWorld(ring_1280(200))
    cfg = w.cfg
    R, T = 64, 20
    cams = ring_cams(w, [cfg.f * (1.0 - 0.1 * (r % 2)) for r in range(R)], [MOUNTS4[r % 4] for r in range(R)])
    phases = [(r * 3) % w.lap_length() for r in range(R)]
    a = gpu_fleet(w, cams, R)
    b = gpu_fleet(w, cams, 2 * R)
    fused, pend = 0, []
    for t in range(T):
        frs = [w.rig_frame(phases[r] + t, [cams[r][2]])[0] for r in range(R)]
        imgs = [a.synth_render(0, cfg.rows, cfg.cols, cams[r][0], fr.ids, fr.poses, noise_amp=2, seed=1000 * r + t) for r, fr in enumerate(frs)]
        enc = [[getattr(fr, k) for fr in frs] for k in ("wl", "wr", "dt")]
        a.fleet_add_images(range(R), imgs, *enc)
        sa = a.get_slot_ekf_stats(0, R)
        fused += int(sa[:, 2].sum())
        pend.append((imgs, enc, sa))
        if len(pend) == 2:
            b.stage_frames(np.stack(pend[0][0] + pend[1][0]))
            b.stage_encoders(*[pend[0][1][k] + pend[1][1][k] for k in range(3)])
            b.fleet_run_staged(0, list(range(R)) * 2)
            b.sync()
            sb = b.get_slot_ekf_stats(0, 2 * R)
            assert np.array_equal(sb, np.concatenate([pend[0][2], pend[1][2]])), f"ticks {t - 1}, {t}"
            pend = []
    for r in range(R):
        for x, y in zip(fleet_state(a, r), fleet_state(b, r)):
            assert np.array_equal(x, y), f"robot {r}"
    pa, sa_ = a.fleet_get_poses()
    pb, sb_ = b.fleet_get_poses()
    assert np.array_equal(pa, pb) and np.array_equal(sa_, sb_)
    assert fused > R * T
