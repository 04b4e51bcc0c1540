"""Localization against a frozen, known marker map (aslam_localize_begin / _end, k_loc_steps).

The reference for every check is FrozenMapLocalizer below: the reference's addEncoder / addImage arithmetic (aruco_slam.cpp:21-74,
88-207) on the 3-state pose block alone, which is what the reference's dense update reduces to when Sigma_ll = 0 and Sigma_xl = 0.
It is first pinned against the dense literal transcription (oracle.ekf_literal.LiteralSlam) started from [pose, map] with
blockdiag(Sigma_xx, 0); then injected observation sequences, camera rigs and (on the MI355X) whole rendered laps are replayed
through the device and compared with it."""
import math
import os

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from oracle.ekf_literal import LiteralSlam, _Heap, norm_angle

E_INVALID, E_STATE = -1, -5


class FrozenMapLocalizer:
    """pose mu (3) and Sigma_xx (3 x 3) of the reference's filter on a frozen map; observations are (id, valid, z, Rdiag)"""

    def __init__(self, ids, xyth, pose, pose_sigma, Q_k=0.01, kl=0.05, kr=0.05, b=0.09):
        self.index = {}
        for i, lid in enumerate(ids):
            self.index.setdefault(int(lid), i)
        self.xyth = np.asarray(xyth, float).reshape(-1, 3)
        self.mu = np.asarray(pose, float).copy()
        self.P = np.asarray(pose_sigma, float).reshape(3, 3).copy()
        self.Q_k, self.kl, self.kr, self.b = Q_k, kl, kr, b
        self.is_init = False
        self.last = []                                  # (id, last_observation_ or NaN)
        self.log = []
        self.stats = None

    def predict(self, wl, wr, dt):                      # aruco_slam.cpp:35-73 on the pose block
        delta_sl, delta_sr = self.kl * (dt * wl), self.kr * (dt * wr)
        delta_theta = (delta_sr - delta_sl) / (2 * self.b)
        delta_s = 0.5 * (delta_sr + delta_sl)
        tmp = self.mu[2] + 0.5 * delta_theta
        c, s = math.cos(tmp), math.sin(tmp)
        self.mu[0] += delta_s * c
        self.mu[1] += delta_s * s
        self.mu[2] = norm_angle(self.mu[2] + delta_theta)
        H = np.array([[1.0, 0.0, -delta_s * s], [0.0, 1.0, delta_s * c], [0.0, 0.0, 1.0]])
        wkh = (0.5 * self.kl * dt) * np.array([[c, c], [s, s], [1 / self.b, -1 / self.b]])
        Q = wkh @ np.diag([self.Q_k * abs(wl), self.Q_k * abs(wr)]) @ wkh.T
        self.P = H @ self.P @ H.T + Q

    def add_encoder(self, wl, wr, dt):                  # the first sample only arms the filter (aruco_slam.cpp:24-29)
        if not self.is_init:
            self.is_init = True
            return
        self.predict(wl, wr, dt)

    def add_observations(self, obs):
        q = _Heap()
        for k, (lid, valid, z, r) in enumerate(obs):
            if valid and int(lid) in self.index:        # gated and unknown ids never enter the queue
                q.push(dict(id=int(lid), index=self.index[int(lid)], z=np.asarray(z, float), R=np.diag(r), det=k))
        x, y, th = self.mu
        s, c = math.sin(th), math.cos(th)
        self.log, nxt, nupd, nstat = [], [], 0, 0
        while q.c:
            ob = q.pop()
            mx, my, mth = self.xyth[ob["index"]]
            last = next((l for l in self.last if l[0] == ob["id"]), None)
            if last is not None and np.linalg.norm(last[1] - ob["z"]) < 0.01:
                act = 2
                nstat += 1
                nxt.append((ob["id"], np.full(3, np.nan)))
            else:
                act = 1
                nupd += 1
                gdx, gdy = mx - x, my - y
                gdth = norm_angle(mth - th)
                ze = ob["z"] - np.array([gdx * c + gdy * s, -gdx * s + gdy * c, gdth])
                ze[2] = norm_angle(ze[2])
                H = np.array([[-c, -s, -gdx * s + gdy * c], [s, -c, -gdx * c - gdy * s], [0.0, 0.0, -1.0]])
                K = self.P @ H.T @ np.linalg.inv(H @ self.P @ H.T + ob["R"])
                self.mu = self.mu + K @ ze
                self.P = (np.eye(3) - K @ H) @ self.P
                nxt.append((ob["id"], ob["z"].copy()))
            self.log.append((ob["id"], ob["index"], act))
        self.last = nxt
        self.stats = [len(obs), 0, nupd, nstat]

    def log_array(self):
        return np.array(self.log, np.int32).reshape(-1, 3)


def random_map(rng, n, id_pool=400):
    ids = rng.permutation(np.arange(1, id_pool))[:n].astype(np.int32)
    xyth = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-math.pi, math.pi, n)], 1)
    return ids, xyth


def observe(pose, lm, rng, noise=0.01):
    x, y, th = pose
    c, s = math.cos(th), math.sin(th)
    dx, dy = lm[0] - x, lm[1] - y
    return np.array([dx * c + dy * s + rng.normal(0, noise), -dx * s + dy * c + rng.normal(0, noise),
                     norm_angle(lm[2] - th + rng.normal(0, noise))])


def make_sequence(seed, n_frames, ids, xyth, unknown=True, dup=True, gated=True, stationary=True):
    """frames of (wl, wr, dt, obs); obs = [(id, valid, z, Rdiag)] in detection order, mixing known ids, unknown ids, one id twice,
    repeated observations (the "stationary" rule) and gated observations"""
    rng = np.random.RandomState(seed)
    n = len(ids)
    pose = np.array([0.1, -0.2, 0.3])
    frames, prev = [], {}
    for f in range(n_frames):
        wl, wr = rng.uniform(1, 4), rng.uniform(1, 4)
        dt = 0.05
        pose = pose + np.array([0.02 * math.cos(pose[2]), 0.02 * math.sin(pose[2]), 0.01])
        sel = rng.permutation(n)[: rng.randint(0, min(n, 7) + 1)]
        obs = []
        for li in sel:
            z = observe(pose, xyth[li], rng)
            if stationary and f % 4 == 3 and int(ids[li]) in prev:
                z = prev[int(ids[li])].copy()                       # the same observation as last frame: a no-op
            obs.append((int(ids[li]), 1, z, rng.uniform(0.01, 0.05, 3)))
        if unknown and f % 3 == 1:
            obs.insert(rng.randint(0, len(obs) + 1), (int(500 + f), 1, rng.normal(0, 1, 3), np.full(3, 0.02)))
        if dup and f % 5 == 2 and len(obs) > 0:
            lid = obs[0][0]
            if lid < 500:
                li = int(np.nonzero(ids == lid)[0][0])
                obs.append((lid, 1, observe(pose, xyth[li], rng), rng.uniform(0.01, 0.05, 3)))
        if gated and f % 4 == 1 and len(sel) > 0:
            li = sel[0]
            obs.append((int(ids[li]), 0, np.zeros(3), np.ones(3)))
        prev = {o[0]: o[2] for o in obs if o[1]}
        frames.append((wl, wr, dt, obs))
    return frames


def inject(ctx, slot, obs):
    ctx.inject_observations(slot, [o[0] for o in obs], [o[1] for o in obs], np.array([o[2] for o in obs]).reshape(-1, 3),
                            np.array([o[3] for o in obs]).reshape(-1, 3))


def emu_context(n_frames, max_landmarks=16, **kw):
    return capi.Context(max_rows=64, max_cols=64, max_batch=n_frames, persistent_waves=4, max_landmarks=max_landmarks, **kw)


POSE0 = np.array([0.1, -0.2, 0.3])
SIG0 = np.array([[0.02, 0.001, 0.0], [0.001, 0.03, -0.002], [0.0, -0.002, 0.01]])


def check_against(ctx, ref, L, xyth, where, tol=1e-9):
    mu, S = ctx.get_state()
    assert mu.shape == (3 + 3 * L,)
    e_mu = np.abs(mu[:3] - ref.mu).max()
    e_S = np.abs(S[:3, :3] - ref.P).max() / np.abs(ref.P).max()
    assert e_mu <= tol and e_S <= tol, f"{where}: pose differs by {e_mu}, Sigma_xx by {e_S}"
    assert np.array_equal(mu[3:], xyth.reshape(-1)), f"{where}: the map moved"
    assert np.array_equal(S[3:, :], np.zeros((3 * L, 3 + 3 * L))) and np.array_equal(S[:, 3:], np.zeros((3 + 3 * L, 3 * L))), \
        f"{where}: a landmark block is not zero"


# ---- CPU: the numpy reference against the dense literal transcription -----------------------------------------------------

class _Injected(LiteralSlam):
    """LiteralSlam whose add_poses takes ready observations (index k of the current frame's list)"""

    def make_observation(self, k, corners, rvec, tvec):
        lid, valid, z, r = self._obs[k]
        if not valid:
            return None
        return dict(id=int(lid), index=self.id_map.get(int(lid), -1), z=np.asarray(z, float), R=np.diag(r), last=np.full(3, np.nan))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_frozen_map_localizer_equals_literal_dense_update(seed):
    rng = np.random.RandomState(seed)
    n = 4 + 2 * seed                                           # <= 10 landmarks: the dense N x N literal stays cheap
    ids, xyth = random_map(rng, n)
    frames = make_sequence(seed, 30, ids, xyth)
    lit = _Injected()
    lit.mu = np.concatenate([POSE0, xyth.reshape(-1)])
    lit.sigma = np.zeros((3 + 3 * n, 3 + 3 * n))
    lit.sigma[:3, :3] = SIG0
    lit.id_map = {int(i): k for k, i in enumerate(ids)}
    ref = FrozenMapLocalizer(ids, xyth, POSE0, SIG0)
    t, n_stat = 0.0, 0
    for f, (wl, wr, dt, obs) in enumerate(frames):
        t += dt if f else 0.0
        lit.add_encoder(wl, wr, t)
        ref.add_encoder(wl, wr, dt)
        known = [o for o in obs if o[0] in lit.id_map]             # unknown ids filtered out before add_poses
        lit._obs = known
        k = len(known)
        lit.add_poses(list(range(k)), np.zeros((k, 8)), np.zeros((k, 3)), np.zeros((k, 3)))
        ref.add_observations(obs)
        assert lit.mu.size == 3 + 3 * n, "the literal appended a landmark"
        assert [tuple(e) for e in lit.log] == ref.log, f"frame {f}: pop order / actions differ"
        assert np.abs(lit.mu[:3] - ref.mu).max() <= 1e-12, f"frame {f}"
        assert np.abs(lit.sigma[:3, :3] - ref.P).max() <= 1e-12, f"frame {f}"
        assert np.array_equal(lit.mu[3:], xyth.reshape(-1))
        assert np.array_equal(lit.sigma[3:, :], np.zeros((3 * n, 3 + 3 * n))) and np.array_equal(lit.sigma[:, 3:], np.zeros((3 + 3 * n, 3 * n)))
        n_stat += ref.stats[3]
    assert n_stat > 0

# ---- CPU emulation of k_loc_steps: injected replays ------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [1, 3, 17])
def test_injected_replay_against_reference(batch):
    rng = np.random.RandomState(11)
    n = 9
    ids, xyth = random_map(rng, n)
    frames = make_sequence(5, 34, ids, xyth)
    ctx = emu_context(len(frames))
    ctx.stage_encoders([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames])
    for s, fr in enumerate(frames):
        inject(ctx, s, fr[3])
    ctx.localize_begin(ids, xyth, POSE0, SIG0)
    assert ctx.is_localizing()
    ref = FrozenMapLocalizer(ids, xyth, POSE0, SIG0)
    seen = dict(stationary=0, dup=0, unknown=0, gated=0)
    for f0 in range(0, len(frames), batch):
        nb = min(batch, len(frames) - f0)
        ctx.run_staged(f0, nb, with_ekf=2)
        ctx.sync()
        want = []
        for f in range(f0, f0 + nb):
            wl, wr, dt, obs = frames[f]
            ref.add_encoder(wl, wr, dt)
            ref.add_observations(obs)
            want.append(ref.stats)
            seen["stationary"] += ref.stats[3]
            seen["unknown"] += sum(o[0] >= 500 for o in obs)
            seen["gated"] += sum(o[1] == 0 for o in obs)
            ks = [o[0] for o in obs if o[1]]
            seen["dup"] += len(ks) != len(set(ks))
        check_against(ctx, ref, n, xyth, f"batch at frame {f0}")
        gi, gx, ga, _, _ = ctx.get_observations()
        assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), ref.log_array()), f"batch at frame {f0}: pops differ"
        assert np.array_equal(ctx.get_slot_ekf_stats(f0, nb), np.array(want)), f"batch at frame {f0}: stats differ"
    assert all(v > 0 for v in seen.values()), seen
    assert np.array_equal(ctx.get_landmark_ids(), ids)
    assert ctx.plan_stats() == dict(frames_in_windows=0, frames_per_frame_chain=0, windows=0, frames_device_planned=0)


@pytest.mark.parametrize("windows", [True, False])
def test_equals_slam_path_on_known_markers(windows):
    """SLAM from [pose, map] with blockdiag(Sigma_xx, 0) and only known markers in view gives the localization's pose"""
    rng = np.random.RandomState(21)
    n = 8
    ids, xyth = random_map(rng, n)
    frames = make_sequence(8, 30, ids, xyth, unknown=False, dup=False)
    S0 = np.zeros((3 + 3 * n, 3 + 3 * n))
    S0[:3, :3] = SIG0
    mu0 = np.concatenate([POSE0, xyth.reshape(-1)])
    if not windows:
        os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        slam = emu_context(len(frames), max_updates_per_frame=24)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)
    loc = emu_context(len(frames))
    for ctx in (slam, loc):
        ctx.stage_encoders([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames])
        for s, fr in enumerate(frames):
            inject(ctx, s, fr[3])
    slam.set_state(mu0, S0, ids)
    loc.localize_begin(ids, xyth, POSE0, SIG0)
    for f0 in range(0, len(frames), 6):
        nb = min(6, len(frames) - f0)
        for ctx in (slam, loc):
            ctx.run_staged(f0, nb, with_ekf=2)
            ctx.sync()
        (ma, Sa), (mb, Sb) = slam.get_state(), loc.get_state()
        assert ma.shape == mb.shape
        assert np.abs(ma[:3] - mb[:3]).max() <= 1e-9, f"frame {f0}: pose differs by {np.abs(ma[:3] - mb[:3]).max()}"
        assert np.abs(Sa[:3, :3] - Sb[:3, :3]).max() <= 1e-9 * np.abs(Sb[:3, :3]).max()
        for x, y in zip(slam.get_observations()[:3], loc.get_observations()[:3]):
            assert np.array_equal(x, y), f"frame {f0}: popped order / actions differ"
        sa, sb = slam.get_slot_ekf_stats(f0, nb), loc.get_slot_ekf_stats(f0, nb)
        assert np.array_equal(sa, sb)


# ---- CPU emulation: a two-camera rig at 240 x 320 ---------------------------------------------------------------------------

def small_ring(lap=120):
    return synth.SceneConfig(kind="ring", rows=240, cols=320, f=260.0, grid=(2, 2), n_panels=8, ring_radius=1.8,
                             ring_robot_radius=0.2, ring_lap_frames=lap)


def raw_step_obs(ctx, slots):
    """the device's own observation lists of a rig step's frame slots, concatenated in camera order"""
    out = []
    for s in slots:
        i, v, z, r = ctx.get_slot_raw_observations(s)
        out += [(int(i[k]), int(v[k]), z[k], r[k]) for k in range(len(i))]
    return out


@pytest.mark.parametrize("mode", ["images", "staged"])
def test_two_camera_rig_against_reference(mode):
    w = synth.RingWorld(small_ring())
    cfg = w.cfg
    K2 = synth.camera_matrix(240, 320, 240.0)
    cams = [(w.K, np.zeros(5), (0.12, 0.02, 0.0)), (K2, np.array([0.01, -0.004, 0.0, 0.0, 0.0]), (-0.15, -0.03, math.pi))]
    mounts = [m for _, _, m in cams]
    C, n_steps, bs = 2, 16, 4
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=C * bs, max_landmarks=w.L + 8, persistent_waves=4)
    ctx.set_camera_rig(cams)
    sig0 = np.diag([1e-4, 1e-4, 1e-5])
    ctx.localize_begin(w.ids, w.world, w.pose[0], sig0)
    ref = FrozenMapLocalizer(w.ids, w.world, w.pose[0], sig0)
    t_now, n_obs = 0.0, []
    for s0 in range(0, n_steps, bs):
        steps = [w.rig_frame(s0 + s, mounts) for s in range(bs)]
        imgs = [[ctx.synth_render(s * C + c, cfg.rows, cfg.cols, cams[c][0], fr.ids, fr.poses, noise_amp=2, seed=(s0 + s) * C + c)
                 for c, fr in enumerate(frs)] for s, frs in enumerate(steps)]
        if mode == "staged":
            ctx.stage_encoders([steps[i // C][0].wl for i in range(bs * C)], [steps[i // C][0].wr for i in range(bs * C)],
                               [steps[i // C][0].dt for i in range(bs * C)])
            ctx.run_staged_rig(0, bs, with_ekf=True)
            ctx.sync()
        for s in range(bs):
            fr0 = steps[s][0]
            if mode == "images":
                t_now += fr0.dt
                ctx.add_encoder(fr0.wl, fr0.wr, t_now)
                ctx.add_images(imgs[s])
            ref.add_encoder(fr0.wl, fr0.wr, fr0.dt)
            obs = raw_step_obs(ctx, range(C) if mode == "images" else range(s * C, s * C + C))
            ref.add_observations(obs)
            n_obs.append(ref.stats[2])
            if mode == "images":
                check_against(ctx, ref, w.L, w.world, f"step {s0 + s}")
        check_against(ctx, ref, w.L, w.world, f"steps from {s0}")
        gi, gx, ga, gc, _, _ = ctx.get_rig_observations()
        assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), ref.log_array())
        assert set(gc.tolist()) == {0, 1}
    assert min(n_obs) >= 3 and np.mean(n_obs) >= 5, n_obs
    mu, _ = ctx.get_state()
    print("2-camera rig, emulation: pose error", np.abs(mu[:2] - w.pose[n_steps - 1][:2]).max())


# ---- mode rules ---------------------------------------------------------------------------------------------------------------

def test_mode_rules(tmp_path):
    ctx = emu_context(4, max_landmarks=6)
    ids = np.array([3, 7, 9], np.int32)
    xyth = np.array([[1.0, 0.0, 3.1], [0.0, 1.0, -1.5], [-1.0, -1.0, 0.7]])
    bad = [
        (np.zeros(0, np.int32), np.zeros((0, 3))),             # n = 0
        (np.arange(7, dtype=np.int32), np.zeros((7, 3))),      # n > max_landmarks
        (np.array([3, 7, 3], np.int32), xyth),                 # duplicate id
        (np.array([3, 7, 1024], np.int32), xyth),              # id >= 1024
        (np.array([3, -1, 9], np.int32), xyth),                # id < 0
        (ids, np.where(np.arange(9).reshape(3, 3) == 4, np.nan, xyth)),
    ]
    for i, x in bad:
        with pytest.raises(capi.AslamError) as e:
            ctx.localize_begin(i, x, POSE0, SIG0)
        assert e.value.code == E_INVALID
    with pytest.raises(capi.AslamError) as e:
        ctx.localize_begin(ids, xyth, [0.0, float("nan"), 0.0], SIG0)
    assert e.value.code == E_INVALID
    asym = SIG0.copy()
    asym[0, 1] += 1e-6
    for P in (asym, np.where(np.eye(3) > 0, np.inf, SIG0)):
        with pytest.raises(capi.AslamError) as e:
            ctx.localize_begin(ids, xyth, POSE0, P)
        assert e.value.code == E_INVALID
    assert not ctx.is_localizing()

    ctx.save_state(str(tmp_path / "s.bin"))
    ctx.localize_begin(ids, xyth, POSE0, SIG0)
    assert ctx.is_localizing()
    mu, S = ctx.get_state()
    assert np.array_equal(mu, np.concatenate([POSE0, xyth.reshape(-1)]))
    assert np.array_equal(S[:3, :3], SIG0) and not S[3:, :].any() and not S[:, 3:].any()
    with pytest.raises(capi.AslamError) as e:
        ctx.set_state(mu, S, ids)
    assert e.value.code == E_STATE
    with pytest.raises(capi.AslamError) as e:
        ctx.load_state(str(tmp_path / "s.bin"))
    assert e.value.code == E_STATE
    ctx.save_state(str(tmp_path / "loc.bin"))                 # the state getters work unchanged

    # before arming: an image call is a no-op
    K = synth.camera_matrix(64, 64, 60.0)
    ctx.set_camera(K, np.zeros(5))
    ctx.add_image(np.full((64, 64), 128, np.uint8))
    assert np.array_equal(ctx.get_state()[0], mu)
    # after arming: a known id corrects the pose, an unknown id is ignored
    ctx.stage_encoders([1.0, 1.0], [2.0, 2.0], [0.05, 0.05])
    inject(ctx, 0, [(7, 1, np.array([0.5, 1.0, -1.9]), np.full(3, 0.02)), (42, 1, np.array([1.0, 0.0, 0.0]), np.full(3, 0.02))])
    inject(ctx, 1, [(42, 1, np.array([1.0, 0.0, 0.0]), np.full(3, 0.02))])
    ctx.run_staged(0, 2, with_ekf=2)
    m2, _ = ctx.get_state()
    assert m2.size == mu.size and not np.array_equal(m2[:3], mu[:3]) and np.array_equal(m2[3:], mu[3:])
    assert ctx.get_slot_ekf_stats(0, 2).tolist() == [[2, 0, 1, 0], [1, 0, 0, 0]]

    # leaving: the state stays, later steps are SLAM steps and a new id is appended again
    ctx.localize_end()
    assert not ctx.is_localizing()
    assert np.array_equal(ctx.get_state()[0], m2)
    inject(ctx, 0, [(42, 1, np.array([1.0, 0.0, 0.0]), np.full(3, 0.02))])
    ctx.run_staged(0, 1, with_ekf=2)
    ctx.sync()
    assert ctx.get_landmark_ids().tolist() == [3, 7, 9, 42]
    assert ctx.get_slot_ekf_stats(0, 1).tolist() == [[1, 1, 0, 0]]
    ctx.set_state(*ctx.get_state(), ctx.get_landmark_ids())    # allowed again


# ---- landmarks_from_markers ------------------------------------------------------------------------------------------------------

MAP_TXT = """# id    length	x	y	z	roll_x	pitch_y	yaw_z
0   0.27	5.1 0       0.3     0    -1.5708   0
1	0.27	-2.0 1.5    0.3     0    1.5708   0
3	0.27	4   0.6025 0.3 	1.5708 	-0	0
5	0.27	4 	-4.09375 0.3 	-1.5708	-0	0
8	0.27	1 	2 0.3 	0	0	0.5
"""


def test_landmarks_from_markers(tmp_path):
    lines = MAP_TXT.splitlines()
    (tmp_path / "ok.txt").write_text("\n".join(lines[:5]) + "\n")
    ids, xyth = capi.known_map_from_txt(tmp_path / "ok.txt")
    assert ids.tolist() == [0, 1, 3, 5]
    assert np.array_equal(xyth[:, :2], np.array([[5.1, 0.0], [-2.0, 1.5], [4.0, 0.6025], [4.0, -4.09375]]))
    # pitch -pi/2 turns +z to -x (heading -pi), pitch +pi/2 to +x (0); roll +pi/2 turns +z to -y (-pi/2), roll -pi/2 to +y (+pi/2)
    want = np.array([-math.pi, 0.0, -math.pi / 2, math.pi / 2])
    assert np.abs(xyth[:, 2] - want).max() < 1e-5, xyth[:, 2]
    assert xyth[0, 2] < 0                                       # normAngle: +pi wraps to -pi
    # the same through the marker messages of a context-free load
    ids2, xyth2 = capi.landmarks_from_markers(capi.load_map_txt(tmp_path / "ok.txt"))
    assert np.array_equal(ids, ids2) and np.array_equal(xyth, xyth2)
    # a marker lying flat (roll = pitch = 0: +z is vertical) has no heading: refused, naming the id
    (tmp_path / "flat.txt").write_text("\n".join(lines[:3] + [lines[5]]) + "\n")
    with pytest.raises(capi.AslamError) as e:
        capi.known_map_from_txt(tmp_path / "flat.txt")
    assert e.value.code == E_INVALID and "marker 8" in str(e.value)


# ---- on the MI355X at 1280 x 720 ------------------------------------------------------------------------------------------------

def ring_1280(lap=500):
    cfg = synth.CONFIGS["cfg2_sliding"]
    return synth.SceneConfig(**{**cfg.__dict__, "ring_lap_frames": lap})


SIG_START = np.diag([1e-4, 1e-4, 1e-5])


def render_frames(ctx, w, f0, n, slot0=0):
    cfg = w.cfg
    frs = [w.frame(f0 + i) for i in range(n)]
    imgs = [ctx.synth_render(slot0 + i, cfg.rows, cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=f0 + i) for i, fr in enumerate(frs)]
    return frs, imgs


def gpu_context(w, batch, **kw):
    cfg = w.cfg
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=batch, max_landmarks=w.L + 8, **kw)
    ctx.set_camera(w.K, np.zeros(5))
    synth.apply_detector(cfg, ctx=ctx)
    return ctx


@pytest.mark.gpu
def test_gpu_lap_run_staged_against_reference():
    w = synth.RingWorld(ring_1280())
    B = 50
    ctx = gpu_context(w, B)
    ctx.localize_begin(w.ids, w.world, w.pose[0], SIG_START)
    ref = FrozenMapLocalizer(w.ids, w.world, w.pose[0], SIG_START)
    worst_ref, worst_pos, worst_th, nupd = 0.0, 0.0, 0.0, []
    for f0 in range(0, w.lap_length(), B):
        frs, _ = render_frames(ctx, w, f0, B)
        ctx.stage_frames(np.stack(_))
        ctx.stage_encoders([fr.wl for fr in frs], [fr.wr for fr in frs], [fr.dt for fr in frs])
        ctx.run_staged(0, B, with_ekf=True)
        ctx.sync()
        for i, fr in enumerate(frs):
            ref.add_encoder(fr.wl, fr.wr, fr.dt)
            i_, v_, z_, r_ = ctx.get_slot_raw_observations(i)
            ref.add_observations([(int(i_[k]), int(v_[k]), z_[k], r_[k]) for k in range(len(i_))])
            nupd.append(ref.stats[2])
        mu, S = ctx.get_state()
        e = max(np.abs(mu[:3] - ref.mu).max(), np.abs(S[:3, :3] - ref.P).max() / np.abs(ref.P).max())
        worst_ref = max(worst_ref, e)
        assert e <= 1e-9, f"frames from {f0}: {e}"
        assert np.array_equal(mu[3:], w.world.reshape(-1))
        tp = frs[-1].true_pose
        worst_pos = max(worst_pos, math.hypot(mu[0] - tp[0], mu[1] - tp[1]))
        worst_th = max(worst_th, abs(norm_angle(mu[2] - tp[2])))
    print(f"localize lap: max |device - reference| {worst_ref:.3g}, pose error vs true pose: {worst_pos:.4f} m, {worst_th:.4f} rad, "
          f"corrections per frame {np.mean(nupd):.1f}")
    assert np.mean(nupd) > 15
    assert worst_pos < 0.1 and worst_th < 0.05


@pytest.mark.gpu
def test_gpu_add_image_equals_run_staged_equals_stream():
    w = synth.RingWorld(ring_1280())
    n = 48
    a = gpu_context(w, 16)
    b = gpu_context(w, 16)
    c = gpu_context(w, 16)
    for ctx in (a, b, c):
        ctx.localize_begin(w.ids, w.world, w.pose[0], SIG_START)
    frames = [w.frame(i) for i in range(n)]
    imgs = [a.synth_render(0, w.cfg.rows, w.cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=i) for i, fr in enumerate(frames)]
    t = np.cumsum([0.0] + [fr.dt for fr in frames[1:]]).tolist()
    dts = [0.0] + [t[i] - t[i - 1] for i in range(1, n)]   # what aslam_add_encoder computes from the time stamps
    for i, fr in enumerate(frames):                            # add_encoder + add_image
        a.add_encoder(fr.wl, fr.wr, t[i])
        a.add_image(imgs[i])
    for f0 in range(0, n, 16):                                 # staged batches of 16
        b.stage_frames(np.stack(imgs[f0:f0 + 16]))
        b.stage_encoders([fr.wl for fr in frames[f0:f0 + 16]], [fr.wr for fr in frames[f0:f0 + 16]], dts[f0:f0 + 16])
        b.run_staged(0, 16, with_ekf=True)
        b.sync()
    c.stream_open(w.cfg.rows, w.cfg.cols, 1, 8)                # host-fed stream
    for i, fr in enumerate(frames):
        c.stream_push(imgs[i], fr.wl, fr.wr, dts[i])
    c.stream_flush()
    sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y), "add_image and run_staged differ"
    for x, y in zip(sa, sc):
        assert np.array_equal(x, y), "add_image and the host-fed stream differ"
    assert a.get_observations()[0].size > 15


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["staged", "images"])
def test_gpu_four_camera_rig_lap(mode):
    w = synth.RingWorld(ring_1280(100))
    cfg = w.cfg
    mounts = [(0.20, 0.0, 0.0), (-0.22, 0.0, math.pi), (0.0, 0.15, math.pi / 2), (0.0, -0.15, -math.pi / 2)]
    C, bs = 4, 10
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=C * bs, max_landmarks=w.L + 8)
    ctx.set_camera_rig([(w.K, np.zeros(5), m) for m in mounts])
    synth.apply_detector(cfg, ctx=ctx)
    ctx.localize_begin(w.ids, w.world, w.pose[0], SIG_START)
    ref = FrozenMapLocalizer(w.ids, w.world, w.pose[0], SIG_START)
    n_steps = w.lap_length() if mode == "staged" else 30
    t_now, fused = 0.0, []
    for s0 in range(0, n_steps, bs):
        steps = [w.rig_frame(s0 + s, mounts) for s in range(bs)]
        imgs = [[ctx.synth_render(s * C + c, cfg.rows, cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=(s0 + s) * C + c)
                 for c, fr in enumerate(frs)] for s, frs in enumerate(steps)]
        if mode == "staged":
            ctx.stage_encoders([steps[i // C][0].wl for i in range(bs * C)], [steps[i // C][0].wr for i in range(bs * C)],
                               [steps[i // C][0].dt for i in range(bs * C)])
            ctx.run_staged_rig(0, bs, with_ekf=True)
            ctx.sync()                                         # raises on ASLAM_E_CAPACITY
            got = ctx.get_rig_step_ekf_stats(0, bs)
        for s in range(bs):
            fr0 = steps[s][0]
            if mode == "images":
                t_now += fr0.dt
                ctx.add_encoder(fr0.wl, fr0.wr, t_now)
                ctx.add_images(imgs[s])
                got_s = ctx.get_rig_step_ekf_stats(0, 1)[0]
            ref.add_encoder(fr0.wl, fr0.wr, fr0.dt)
            slots = range(C) if mode == "images" else range(s * C, s * C + C)
            obs = []
            for sl in slots:
                i_, v_, z_, r_ = ctx.get_slot_raw_observations(sl)
                obs += [(int(i_[k]), int(v_[k]), z_[k], r_[k]) for k in range(len(i_))]
            ref.add_observations(obs)
            fused.append(ref.stats[2])
            assert np.array_equal(got[s] if mode == "staged" else got_s, np.array(ref.stats))
        mu, S = ctx.get_state()
        e = max(np.abs(mu[:3] - ref.mu).max(), np.abs(S[:3, :3] - ref.P).max() / np.abs(ref.P).max())
        assert e <= 1e-9, f"steps from {s0}: {e}"
        assert np.array_equal(mu[3:], w.world.reshape(-1))
    print(f"4-camera localize ({mode}): corrections per step {np.mean(fused):.1f} (min {min(fused)})")
    assert min(fused) >= 70
