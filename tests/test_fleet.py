"""Fleet localization: R robots, one camera and one pose filter each, on one shared frozen map (aslam_fleet_*, k_fleet_steps,
k_pose's camera-table instantiation).

Every robot must produce bit for bit what a single localizing context produces on the same frames (aslam_set_camera_rig with that
robot's one camera, aslam_localize_begin, aslam_run_staged_rig), and its pose must follow test_localize.FrozenMapLocalizer."""
import math

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from oracle.ekf_literal import norm_angle
from tests.test_localize import (E_INVALID, E_STATE, FrozenMapLocalizer, POSE0, SIG0, emu_context, inject, make_sequence, random_map,
                                 ring_1280, small_ring)

SIG_START = np.diag([1e-4, 1e-4, 1e-5])


def ring_cams(w, fs, mounts):
    rows, cols = w.cfg.rows, w.cfg.cols
    return [(synth.camera_matrix(rows, cols, f), np.zeros(5), m) for f, m in zip(fs, mounts)]


def render_fleet(ctx, w, cams, phases, ticks, t0=0):
    """per tick t0 .. t0 + ticks - 1 and robot r: (image, Frame) of robot r at lap index phases[r] + t, seen by its one camera"""
    cfg = w.cfg
    out = []
    for t in range(t0, t0 + ticks):
        row = []
        for r, (K, _, m) in enumerate(cams):
            fr = w.rig_frame(phases[r] + t, [m])[0]
            img = ctx.synth_render(0, cfg.rows, cfg.cols, K, fr.ids, fr.poses, noise_amp=2, seed=1000 * r + t)
            row.append((img, fr))
        out.append(row)
    return out


def single_localizer(w, cam, pose, batch, **kw):
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=batch, max_landmarks=w.L + 8, **kw)
    ctx.set_camera_rig([cam])
    ctx.localize_begin(w.ids, w.world, pose, SIG_START)
    return ctx


def run_single(w, cam, pose, frames, batch, **kw):
    """one localizing context (C = 1 rig) on frames = [(img, Frame)], staged in calls of `batch` steps: poses, Sigma, per-step stats,
    per-step detections"""
    ctx = single_localizer(w, cam, pose, batch, **kw)
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
    return mu[:3], S[:3, :3], stats, dets


def same_dets(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- CPU emulation -----------------------------------------------------------------------------------------------------------------

def test_fleet_equals_independent_localizers():
    """R = 3 robots at different phases of the 240 x 320 ring, cameras differing in f and mount (one rear-facing), 12 ticks: one
    staged call and one aslam_fleet_add_images per tick both equal three single localizing contexts, bit for bit"""
    w = synth.RingWorld(small_ring())
    cfg = w.cfg
    R, T = 3, 12
    cams = ring_cams(w, [260.0, 240.0, 280.0], [(0.12, 0.02, 0.0), (-0.15, -0.03, math.pi), (0.0, 0.1, math.pi / 2)])
    cams[1] = (cams[1][0], np.array([0.01, -0.004, 0.0, 0.0, 0.0]), cams[1][2])
    phases = [0, 40, 80]
    poses0 = np.array([w.pose[p] for p in phases])
    F0 = 5                                                     # the staged call starts past slot 0: absolute slots everywhere
    staged = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=F0 + R * T, max_landmarks=w.L + 8, persistent_waves=4)
    frames = render_fleet(staged, w, cams, phases, T)
    staged.fleet_begin(cams, w.ids, w.world, poses0, [SIG_START] * R)
    assert staged.is_fleet() == R
    robots = [r for t in range(T) for r in range(R)]
    staged.stage_frames(np.stack([frames[t][r][0] for t in range(T) for r in range(R)]), slot0=F0)
    staged.stage_encoders(*[[getattr(frames[t][r][1], k) for t in range(T) for r in range(R)] for k in ("wl", "wr", "dt")], slot0=F0)
    staged.fleet_run_staged(F0, robots)
    staged.sync()
    st_stats = staged.get_slot_ekf_stats(F0, R * T)
    st_dets = [staged.get_slot_detections(F0 + s) for s in range(R * T)]
    st_pose, st_sig = staged.fleet_get_poses()

    tick = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=R, max_landmarks=w.L + 8, persistent_waves=4)
    tick.fleet_begin(cams, w.ids, w.world, poses0, [SIG_START] * R)
    tk_stats, tk_dets = [], []
    for t in range(T):
        tick.fleet_add_images(range(R), [frames[t][r][0] for r in range(R)], *[[getattr(frames[t][r][1], k) for r in range(R)]
                                                                               for k in ("wl", "wr", "dt")])
        tk_stats += tick.get_slot_ekf_stats(0, R).tolist()
        tk_dets += [tick.get_slot_detections(r) for r in range(R)]
    tk_pose, tk_sig = tick.fleet_get_poses()

    n_fused = 0
    for r in range(R):
        mu, S, stats, dets = run_single(w, cams[r], poses0[r], [frames[t][r] for t in range(T)], T, persistent_waves=4)
        assert np.array_equal(st_pose[r], mu) and np.array_equal(st_sig[r], S), f"robot {r}: staged fleet != single localizer"
        assert np.array_equal(tk_pose[r], mu) and np.array_equal(tk_sig[r], S), f"robot {r}: per-tick fleet != single localizer"
        assert np.array_equal(st_stats[r::R], np.array(stats)) and np.array_equal(np.array(tk_stats[r::R]), np.array(stats))
        for t in range(T):
            assert same_dets(st_dets[t * R + r], dets[t]) and same_dets(tk_dets[t * R + r], dets[t]), f"robot {r} tick {t}: detections"
        assert not np.array_equal(mu, poses0[r])
        n_fused += sum(s[2] for s in stats)
    assert n_fused >= 2 * R * T, n_fused


def test_asynchronous_arrival_equals_own_subsequence():
    """one staged call: robot 1 three times, robot 2 absent, robot 0 once; then all three.  Each robot equals a single localizing
    context fed its own subsequence (injected observations, bit for bit) and the numpy reference"""
    rng = np.random.RandomState(4)
    ids, xyth = random_map(rng, 9)
    seqs = [make_sequence(30 + r, 8, ids, xyth) for r in range(3)]
    poses0 = np.array([POSE0, POSE0 + 0.1, POSE0 - 0.05])
    fleet = emu_context(8)
    fleet.fleet_begin([(synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))] * 3, ids, xyth, poses0, [SIG0] * 3)
    calls = [(2, [1, 0, 1, 1]), (0, [2, 1, 0]), (3, [0, 2, 2, 1])]        # (first slot, robot of each slot)
    sub = [[], [], []]
    done = [0, 0, 0]
    for first, order in calls:
        frames = []
        for r in order:
            frames.append(seqs[r][done[r]])
            sub[r].append(seqs[r][done[r]])
            done[r] += 1
        for s, fr in enumerate(frames):
            inject(fleet, first + s, fr[3])
        fleet.stage_encoders([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], slot0=first)
        fleet.fleet_run_staged(first, order, with_ekf=2)
        fleet.sync()
    poses, sigs = fleet.fleet_get_poses()
    for r in range(3):
        one = emu_context(8)
        one.localize_begin(ids, xyth, poses0[r], SIG0)
        for s, fr in enumerate(sub[r]):
            inject(one, s, fr[3])
        one.stage_encoders([f[0] for f in sub[r]], [f[1] for f in sub[r]], [f[2] for f in sub[r]])
        one.run_staged(0, len(sub[r]), with_ekf=2)
        mu, S = one.get_state()
        assert np.array_equal(poses[r], mu[:3]) and np.array_equal(sigs[r], S[:3, :3]), f"robot {r}"
        ref = FrozenMapLocalizer(ids, xyth, poses0[r], SIG0)
        for fr in sub[r]:
            ref.add_encoder(*fr[:3])
            ref.add_observations(fr[3])
        assert np.abs(poses[r] - ref.mu).max() <= 1e-9 and np.abs(sigs[r] - ref.P).max() <= 1e-9 * np.abs(ref.P).max()


def test_injected_against_reference():
    """with_ekf = 2 per robot against the numpy reference: unknown ids, a repeated id, gated and stationary observations, 128
    observations in one slot, empty slots, re-seating (arming again) and two robots given identical observations in interleaved
    slots, neither of them "stationary" because of the other"""
    rng = np.random.RandomState(12)
    n = 100
    ids, xyth = random_map(rng, n, id_pool=600)
    R, T = 4, 10
    seqs = [make_sequence(50 + r, T, ids, xyth) for r in range(R)]
    seqs[3] = [tuple(f) for f in seqs[2]]                       # robots 2 and 3: identical observations
    big = [(int(ids[k % n]), 1, np.array([0.5 + 0.01 * k, -0.2, 0.1]), np.full(3, 0.03)) for k in range(127)]
    big.append((777, 1, np.zeros(3), np.full(3, 0.02)))        # unknown id among 128
    seqs[0][4] = (seqs[0][4][0], seqs[0][4][1], seqs[0][4][2], big)
    seqs[1][2] = (seqs[1][2][0], seqs[1][2][1], seqs[1][2][2], [])
    seqs[1][5] = (seqs[1][5][0], seqs[1][5][1], seqs[1][5][2], [])
    poses0 = np.array([POSE0 + 0.02 * min(r, 2) for r in range(R)])   # robots 2 and 3 start alike: they must stay alike
    fleet = emu_context(R * T, max_landmarks=n)
    fleet.fleet_begin([(synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))] * R, ids, xyth, poses0, [SIG0] * R)
    refs = [FrozenMapLocalizer(ids, xyth, poses0[r], SIG0) for r in range(R)]
    reseat = (np.array([0.3, 0.1, -0.4]), np.diag([0.01, 0.02, 0.005]))
    seen = dict(stationary=0, big=0, empty=0)
    for half in range(2):
        t0, t1 = half * T // 2, (half + 1) * T // 2
        order = [r for t in range(t0, t1) for r in range(R)]
        frames = [seqs[r][t] for t in range(t0, t1) for r in range(R)]
        for s, fr in enumerate(frames):
            inject(fleet, s, fr[3])
        fleet.stage_encoders([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames])
        fleet.fleet_run_staged(0, order, with_ekf=2)
        stats = fleet.get_slot_ekf_stats(0, len(order))
        for s, (r, fr) in enumerate(zip(order, frames)):
            refs[r].add_encoder(*fr[:3])
            refs[r].add_observations(fr[3])
            assert np.array_equal(stats[s], np.array(refs[r].stats)), f"slot {s} (robot {r})"
            seen["stationary"] += refs[r].stats[3]
            seen["big"] += len(fr[3]) == 128
            seen["empty"] += len(fr[3]) == 0
        poses, sigs = fleet.fleet_get_poses()
        for r in range(R):
            assert np.abs(poses[r] - refs[r].mu).max() <= 1e-9, f"robot {r}, half {half}"
            assert np.abs(sigs[r] - refs[r].P).max() <= 1e-9 * np.abs(refs[r].P).max()
        assert np.array_equal(poses[2], poses[3]) and np.array_equal(sigs[2], sigs[3])
        if half == 0:                                          # re-seat robot 1: its next frame only arms
            fleet.fleet_set_pose(1, *reseat)
            refs[1] = FrozenMapLocalizer(ids, xyth, reseat[0], reseat[1])
            p, s_ = fleet.fleet_get_poses()
            assert np.array_equal(p[1], reseat[0]) and np.array_equal(s_[1], reseat[1])
    assert all(v > 0 for v in seen.values()), seen


def test_mode_and_argument_rules(tmp_path):
    ctx = emu_context(4, max_landmarks=6)
    ids = np.array([3, 7, 9], np.int32)
    xyth = np.array([[1.0, 0.0, 3.1], [0.0, 1.0, -1.5], [-1.0, -1.0, 0.7]])
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    fresh_mu, fresh_S = ctx.get_state()

    def refused(code, fn, *a):
        with pytest.raises(capi.AslamError) as e:
            fn(*a)
        assert e.value.code == code, (fn, e.value)

    # outside fleet mode the fleet calls refuse
    assert ctx.is_fleet() == 0
    refused(E_STATE, ctx.fleet_run_staged, 0, [0], 2)
    refused(E_STATE, ctx.fleet_get_poses)
    refused(E_STATE, ctx.fleet_set_pose, 0, POSE0, SIG0)
    refused(E_STATE, ctx.fleet_end)
    refused(E_STATE, ctx.fleet_add_images, [0], [np.zeros((64, 64), np.uint8)], [0.0], [0.0], [0.05])
    # arguments
    refused(E_INVALID, ctx.fleet_begin, [cam] * 5, ids, xyth, [POSE0] * 5, [SIG0] * 5)              # R > max_batch
    big = emu_context(300, max_landmarks=6)
    refused(E_INVALID, big.fleet_begin, [cam] * 257, ids, xyth, [POSE0] * 257, [SIG0] * 257)        # R > ASLAM_MAX_ROBOTS
    big.fleet_begin([cam] * 256, ids, xyth, [POSE0] * 256, [SIG0] * 256)
    assert big.is_fleet() == 256
    refused(E_INVALID, ctx.fleet_begin, [cam], np.array([3, 3], np.int32), xyth[:2], [POSE0], [SIG0])
    refused(E_INVALID, ctx.fleet_begin, [cam], np.array([3, 1024], np.int32), xyth[:2], [POSE0], [SIG0])
    refused(E_INVALID, ctx.fleet_begin, [cam], ids, np.where(np.eye(3) > 0, np.nan, xyth), [POSE0], [SIG0])
    asym = SIG0.copy()
    asym[0, 1] += 1e-6
    refused(E_INVALID, ctx.fleet_begin, [cam, cam], ids, xyth, [POSE0, POSE0], [SIG0, asym])
    refused(E_INVALID, ctx.fleet_begin, [cam], ids, xyth, [[0.0, np.inf, 0.0]], [SIG0])
    refused(E_INVALID, ctx.fleet_begin, [(cam[0], np.zeros(6), (0.0, 0.0, 0.0))], ids, xyth, [POSE0], [SIG0])
    refused(E_INVALID, ctx.fleet_begin, [(cam[0], np.zeros(5), (0.0, 0.0, -math.pi))], ids, xyth, [POSE0], [SIG0])
    assert ctx.is_fleet() == 0

    ctx.set_camera(cam[0], np.zeros(5))
    ctx.fleet_begin([cam, cam], ids, xyth, [POSE0, POSE0 + 0.1], [SIG0, SIG0])
    assert ctx.is_fleet() == 2
    refused(E_INVALID, ctx.fleet_run_staged, 0, [0, 2], 2)                                          # robot outside the fleet
    refused(E_INVALID, ctx.fleet_run_staged, 0, [-1], 2)
    refused(E_INVALID, ctx.fleet_set_pose, 2, POSE0, SIG0)
    refused(E_INVALID, ctx.fleet_set_pose, 0, POSE0, asym)
    img = np.full((64, 64), 128, np.uint8)
    refused(E_INVALID, ctx.fleet_add_images, [1, 1], [img, img], [0.0, 0.0], [0.0, 0.0], [0.05, 0.05])   # one robot twice
    refused(E_INVALID, ctx.fleet_add_images, [0, 5], [img, img], [0.0, 0.0], [0.0, 0.0], [0.05, 0.05])
    # every entry point on the single filter or camera refuses (the map gather through the C-ABI: no communicator is needed to be
    # refused; the export target is never written)
    K = cam[0]
    dev_buf = np.zeros(64, np.uint8)

    def comm_gather():
        ctx._ck(ctx.lib.aslam_comm_gather_maps(ctx.h, dev_buf.ctypes.data, 0))
    for fn, a in [(ctx.add_encoder, (1.0, 1.0, 0.1)), (ctx.add_image, (img,)), (ctx.add_images, ([img],)),
                  (ctx.run_staged, (0, 1, True)), (ctx.run_staged, (0, 1, 2)), (ctx.run_staged_rig, (0, 1, True)),
                  (ctx.stream_open, (64, 64, 1, 1)), (ctx.stream_slot, (64, 64)), (ctx.stream_commit, (1.0, 1.0, 0.05)),
                  (ctx.stream_push, (img, 1.0, 1.0, 0.05)), (ctx.stream_flush, ()), (ctx.export_map_async, (dev_buf.ctypes.data, 0)),
                  (comm_gather, ()), (ctx.localize_begin, (ids, xyth, POSE0, SIG0)), (ctx.localize_end, ()),
                  (ctx.get_state, ()), (ctx.set_state, (fresh_mu, fresh_S, [])), (ctx.save_state, (str(tmp_path / "s.bin"),)),
                  (ctx.load_state, (str(tmp_path / "s.bin"),)), (ctx.pose_msg, ()), (ctx.map_markers, ()), (ctx.detected_markers, ()),
                  (ctx.draw_detected_markers, (np.zeros((64, 64, 3), np.uint8),)), (ctx.get_observations, ()),
                  (ctx.get_rig_observations, ()), (ctx.export_map, ()), (ctx.set_camera, (K, np.zeros(5))),
                  (ctx.set_camera_rig, ([cam],))]:
        refused(E_STATE, fn, *a)
    assert not (tmp_path / "s.bin").exists()
    # detection-only calls and detector changes stay allowed; the fleet slots' getters work
    ctx.stage_frames(np.stack([img, img]))
    ctx.run_staged(0, 2, with_ekf=False)
    ctx.fleet_run_staged(0, [1, 0], with_ekf=0)
    ctx.sync()
    ctx.set_detector_params(minMarkerPerimeterRate=0.04)
    assert ctx.get_slot_detections(0)[0].size == 0 and ctx.get_slot_raw_observations(1)[0].size == 0
    # a known id corrects robot 1 only, after it was armed; an unknown one is dropped
    ctx.stage_encoders([1.0, 1.0], [2.0, 2.0], [0.05, 0.05])
    inject(ctx, 0, [(7, 1, np.array([0.5, 1.0, -1.9]), np.full(3, 0.02)), (42, 1, np.array([1.0, 0.0, 0.0]), np.full(3, 0.02))])
    inject(ctx, 1, [(7, 1, np.array([0.5, 1.0, -1.9]), np.full(3, 0.02))])
    ctx.fleet_run_staged(0, [1, 1], with_ekf=2)
    p, s = ctx.fleet_get_poses()
    assert np.array_equal(p[0], POSE0) and np.array_equal(s[0], SIG0)
    assert not np.array_equal(p[1], POSE0 + 0.1)
    assert ctx.get_slot_ekf_stats(0, 2).tolist() == [[2, 0, 1, 0], [1, 0, 0, 1]]   # the same observation again: robot 1 stationary
    assert ctx.get_landmark_ids().tolist() == [3, 7, 9]
    # localize_begin is refused during a fleet, fleet_begin while localizing
    other = emu_context(2, max_landmarks=6)
    other.localize_begin(ids, xyth, POSE0, SIG0)
    refused(E_STATE, other.fleet_begin, [cam], ids, xyth, [POSE0], [SIG0])
    # leaving: the single filter as after aslam_create
    ctx.fleet_end()
    assert ctx.is_fleet() == 0
    mu, S = ctx.get_state()
    assert np.array_equal(mu, fresh_mu) and np.array_equal(S, fresh_S)
    assert ctx.get_landmark_ids().size == 0
    inject(ctx, 0, [(42, 1, np.array([1.0, 0.0, 0.0]), np.full(3, 0.02))])
    ctx.stage_encoders([1.0], [2.0], [0.05])
    ctx.run_staged(0, 1, with_ekf=2)                       # a SLAM step again: the first sample arms, the new id is appended
    ctx.sync()
    assert ctx.get_landmark_ids().tolist() == [42]
    ctx.set_camera_rig([cam])


# ---- on the MI355X at 1280 x 720 ---------------------------------------------------------------------------------------------------

def gpu_fleet(w, cams, poses0, batch):
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=batch, max_landmarks=w.L + 8)
    synth.apply_detector(cfg, ctx=ctx)
    ctx.fleet_begin(cams, w.ids, w.world, poses0, [SIG_START] * len(cams))
    return ctx


MOUNTS4 = [(0.20, 0.0, 0.0), (-0.22, 0.0, math.pi), (0.0, 0.15, math.pi / 2), (0.0, -0.15, -math.pi / 2)]


@pytest.mark.gpu
def test_gpu_fleet_lap_equals_independent_localizers():
    """R = 8 robots, front / rear / left / right mounts and two sets of intrinsics, one lap in staged calls of max_batch slots"""
    w = synth.RingWorld(ring_1280(100))
    cfg = w.cfg
    R, B = 8, 40
    cams = ring_cams(w, [cfg.f] * 4 + [0.9 * cfg.f] * 4, MOUNTS4 * 2)
    L = w.lap_length()
    phases = [(r * L) // R for r in range(R)]
    poses0 = np.array([w.pose[p] for p in phases])
    fleet = gpu_fleet(w, cams, poses0, B)
    singles = []
    for r in range(R):
        s = single_localizer(w, cams[r], poses0[r], B // R)
        synth.apply_detector(cfg, ctx=s)
        singles.append(s)
    per = B // R
    worst = [0.0] * R
    for t0 in range(0, L, per):
        nt = min(per, L - t0)
        frames = render_fleet(fleet, w, cams, phases, nt, t0)
        robots = [r for t in range(nt) for r in range(R)]
        fleet.stage_frames(np.stack([frames[t][r][0] for t in range(nt) for r in range(R)]))
        fleet.stage_encoders(*[[getattr(frames[t][r][1], k) for t in range(nt) for r in range(R)] for k in ("wl", "wr", "dt")])
        fleet.fleet_run_staged(0, robots)
        fleet.sync()
        stats = fleet.get_slot_ekf_stats(0, nt * R)
        poses, sigs = fleet.fleet_get_poses()
        for r in range(R):
            s = singles[r]
            s.stage_frames(np.stack([frames[t][r][0] for t in range(nt)]))
            s.stage_encoders(*[[getattr(frames[t][r][1], k) for t in range(nt)] for k in ("wl", "wr", "dt")])
            s.run_staged_rig(0, nt, with_ekf=True)
            s.sync()
            mu, S = s.get_state()
            assert np.array_equal(poses[r], mu[:3]) and np.array_equal(sigs[r], S[:3, :3]), f"robot {r}, ticks from {t0}"
            assert np.array_equal(stats[r::R], s.get_rig_step_ekf_stats(0, nt)), f"robot {r}, ticks from {t0}"
            tp = frames[-1][r][1].true_pose
            worst[r] = max(worst[r], math.hypot(mu[0] - tp[0], mu[1] - tp[1]))
            assert abs(norm_angle(mu[2] - tp[2])) < 0.05, f"robot {r}: heading error"
    print("fleet lap: worst position error per robot", np.round(worst, 4))
    assert max(worst) < 0.1


@pytest.mark.gpu
def test_gpu_many_robots_add_images_equals_staged():
    """R = 64 robots, 20 ticks through aslam_fleet_add_images == the same ticks staged"""
    w = synth.RingWorld(ring_1280(200))
    cfg = w.cfg
    R, T = 64, 20
    cams = ring_cams(w, [cfg.f * (1.0 - 0.1 * (r % 2)) for r in range(R)], [MOUNTS4[r % 4] for r in range(R)])
    phases = [(r * 3) % w.lap_length() for r in range(R)]
    poses0 = np.array([w.pose[p] for p in phases])
    a = gpu_fleet(w, cams, poses0, R)
    b = gpu_fleet(w, cams, poses0, R)
    fused = 0
    for t in range(T):
        frs = [w.rig_frame(phases[r] + t, [cams[r][2]])[0] for r in range(R)]
        imgs = [a.synth_render(0, cfg.rows, cfg.cols, cams[r][0], fr.ids, fr.poses, noise_amp=2, seed=1000 * r + t) for r, fr in enumerate(frs)]
        enc = [[getattr(fr, k) for fr in frs] for k in ("wl", "wr", "dt")]
        a.fleet_add_images(range(R), imgs, *enc)
        sa = a.get_slot_ekf_stats(0, R)
        b.stage_frames(np.stack(imgs))
        b.stage_encoders(*enc)
        b.fleet_run_staged(0, list(range(R)))
        b.sync()
        assert np.array_equal(sa, b.get_slot_ekf_stats(0, R)), f"tick {t}"
        fused += int(sa[:, 2].sum())
    pa, sa_ = a.fleet_get_poses()
    pb, sb_ = b.fleet_get_poses()
    assert np.array_equal(pa, pb) and np.array_equal(sa_, sb_)
    assert fused > R * T
