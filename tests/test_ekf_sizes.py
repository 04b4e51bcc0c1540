"""Every EKF correction path at the edges of its sizes, against a long-double restatement of the reference (tests/ekf_reference.py).

Per-frame chains (capi.hip: run_ekf_frame, chosen by max_updates_per_frame = the cap): fast (cap <= 24), mid (cap <= 64), general
(cap > 64; k_ekf_small takes its LDS Gauss-Jordan for m <= 32 fused corrections and ekf_small_general above).  Each case is one
arming sample and one predict + update frame on an injected dense state: the kernels that ran, the pop order and the branches,
mu and Sigma at 1e-9.  Windows (ekf_window.hip) at the set sizes where the image widens (20 / 21, 41 / 42) and at the largest set
and frame (63), against the literal transcription and the per-frame chain.  Localization (k_loc_steps) at the widths of its two
waves.  Runs on the emulation build without a GPU; the GPU runs matter most, the emulation cannot show an LDS race."""
import functools
import math

import numpy as np
import pytest

from aruco_slam_amd import capi
from ekf_reference import (CHAIN_CAP, CHAIN_KERNELS, LD, ekf_kernels_run, observe, predicted_pose, random_state, reference_step,
                           rel_err, wrap_once)
from oracle.ekf_literal import LiteralSlam
from test_ekf_window import make_case, run_device
from test_localize import FrozenMapLocalizer, inject, random_map

E_INVALID, E_CAPACITY = -1, -4
WL, WR, DT = 2.0, 2.3, 1 / 30.0
ID_TABLE = 1024                                    # kIdTableSize: marker ids 0 .. 1023


def landmark_ids(rng, L):
    """ids of L landmarks and the indices observable by id.  Above 1024 landmarks the first L - 1023 share id 0 (the id table
    maps it to index 0), so that index 0 and the last 1023 indices, the edges of the state, are observable."""
    if L <= ID_TABLE:
        return rng.permutation(ID_TABLE)[:L].astype(np.int32), np.arange(L)
    ids = np.zeros(L, np.int32)
    ids[L - (ID_TABLE - 1):] = 1 + rng.permutation(ID_TABLE - 1)
    return ids, np.concatenate([[0], np.arange(L - (ID_TABLE - 1), L)])


def pick(rng, observable, m):
    """m landmark indices, ascending; the first and the last observable index are always among them"""
    if m == 1:
        return np.array([observable[-1]])
    mid = rng.choice(observable[1:-1], m - 2, replace=False) if m > 2 else np.zeros(0, int)
    return np.sort(np.concatenate([[observable[0], observable[-1]], mid])).astype(int)


def context(cap, ML, batch=2, waves=4):
    return capi.Context(max_rows=64, max_cols=64, max_batch=batch, persistent_waves=waves, max_landmarks=ML, max_updates_per_frame=cap)


def run_one_frame(chain, m, L, ML, seed, dtype=LD, waves=4, cap=None):
    """one arming sample, then predict + m corrections of known landmarks (detection order shuffled); returns the errors"""
    cap = CHAIN_CAP[chain] if cap is None else cap
    rng = np.random.RandomState(seed)
    mu, S = random_state(rng, L)
    ids, observable = landmark_ids(rng, L)
    seen = pick(rng, observable, m)
    obs = observe(rng, mu, seen, post_predict=predicted_pose(mu, WL, WR, DT))
    det = rng.permutation(m)
    ctx = context(cap, ML, waves=waves)
    ctx.set_state(mu, S, ids)
    ctx.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
    ctx.inject_observations(0, [], [], np.zeros((0, 3)), np.zeros((0, 3)))
    ctx.inject_observations(1, ids[seen[det]], [1] * m, np.array([obs[i][1] for i in det]), np.array([obs[i][2] for i in det]))
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.run_staged(0, 2, with_ekf=2)
    ctx.sync()
    ran = ekf_kernels_run(ctx.profile_get())
    assert ran == CHAIN_KERNELS[chain], f"cap {cap}: ran {sorted(ran)}"
    gi, gx, ga, _, _ = ctx.get_observations()
    assert np.array_equal(gx, seen) and np.array_equal(gi, ids[seen]) and (ga == 1).all(), "pop order / branches differ"
    assert ctx.get_slot_ekf_stats(1, 1)[0].tolist() == [m, 0, m, 0]
    mu_g, S_g = ctx.get_state()
    mu_r, S_r = reference_step(mu, S, WL, WR, DT, obs, dtype=dtype)
    assert mu_g.shape == mu_r.shape
    e_mu, e_S = float(np.abs(mu_g - mu_r).max()), rel_err(S_g, S_r)
    print(f"{chain} cap {cap} m {m} L {L} max_landmarks {ML} (ld {3 + 3 * ML}): |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert np.allclose(mu_g, mu_r, rtol=1e-9, atol=1e-11), f"mu differs by {e_mu}"
    assert e_S <= 1e-9, f"Sigma differs by {e_S} (relative)"
    return e_mu, e_S


def _above(L, r):
    """the smallest max_landmarks > L with max_landmarks = r (mod 64)"""
    return L + 1 + (r - (L + 1)) % 64


# max_landmarks = 63, 42, 20 (mod 64) give a leading dimension ld = 3 + 3 max_landmarks = 0, 1, 63 (mod 64)
LD_RESIDUES = (63, 42, 20)
SIZES = {"fast": (1, 2, 23, 24), "mid": (25, 32, 33, 48, 63, 64), "general": (1, 32, 33, 64, 65, 96, 127, 128)}
CASES = []
for _chain, _ms in SIZES.items():
    for _m in _ms:
        for _L in (_m, _m + 19):
            for _ML in (_L, _above(_L, LD_RESIDUES[len(CASES) % 3])):
                CASES.append((_chain, _m, _L, _ML))


@pytest.mark.parametrize("chain,m,L,ML", CASES, ids=[f"{c}-m{m}-L{L}-ml{ml}" for c, m, L, ml in CASES])
def test_per_frame_chain_against_long_double_reference(chain, m, L, ML):
    run_one_frame(chain, m, L, ML, seed=1000 * m + L + ML)


def test_sizes_cover_every_leading_dimension_residue():
    assert {(3 + 3 * ml) % 64 for _, _, _, ml in CASES} >= {0, 1, 63}


@pytest.mark.parametrize("chain", ["fast", "mid"])
def test_one_correction_over_the_cap_is_reported(chain):
    cap = CHAIN_CAP[chain]
    with pytest.raises(capi.AslamError) as e:
        run_one_frame(chain, cap + 1, cap + 1, cap + 1, seed=7, cap=cap)
    assert e.value.code == E_CAPACITY


def test_general_cap_is_the_frame_list():
    """cap 128 = kMarkerMax: a cap above it is refused, and so is a 129th observation in a frame"""
    with pytest.raises(capi.AslamError) as e:
        context(129, 8)
    assert e.value.code == E_INVALID
    ctx = context(128, 8)
    with pytest.raises(capi.AslamError) as e:
        ctx.inject_observations(1, np.arange(129), [1] * 129, np.zeros((129, 3)), np.ones((129, 3)))
    assert e.value.code == E_INVALID


class _Injected(LiteralSlam):
    """LiteralSlam whose add_poses takes ready observations (index k of the frame's list)"""

    def make_observation(self, k, corners, rvec, tvec):
        lid, z, r = self._obs[k]
        return dict(id=int(lid), index=self.id_map.get(int(lid), -1), z=np.asarray(z, float), R=np.diag(r), last=np.full(3, np.nan))


def test_mixed_frame_on_the_general_chain():
    """known ids (more than 32 corrections: ekf_small_general), new ids and one id twice, through the device's own plan"""
    rng = np.random.RandomState(5)
    L, n_known, n_new = 50, 40, 12
    mu, S = random_state(rng, L)
    ids = rng.permutation(ID_TABLE)[:L + n_new].astype(np.int32)
    seen = np.sort(rng.choice(L, n_known, replace=False))
    obs = [(int(ids[i]), z, r) for i, z, r in observe(rng, mu, seen, post_predict=predicted_pose(mu, WL, WR, DT))]
    obs += [(int(ids[L + k]), np.array([rng.uniform(0.5, 2), rng.uniform(-1, 1), rng.uniform(-3, 3)]), rng.uniform(0.02, 0.2, 3))
            for k in range(n_new)]
    dup = obs[3]
    obs.append((dup[0], dup[1] + rng.normal(0, 0.02, 3), rng.uniform(0.02, 0.2, 3)))
    obs = [obs[i] for i in rng.permutation(len(obs))]
    lit = _Injected()
    lit.mu, lit.sigma = mu.copy(), S.copy()
    lit.id_map = {int(i): k for k, i in enumerate(ids[:L])}
    lit.add_encoder(0.0, 0.0, 0.0)
    lit.add_encoder(WL, WR, DT)
    lit._obs = obs
    lit.add_poses(list(range(len(obs))), np.zeros((len(obs), 8)), np.zeros((len(obs), 3)), np.zeros((len(obs), 3)))
    ctx = context(128, 64)
    ctx.set_state(mu, S, ids[:L])
    ctx.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
    ctx.inject_observations(0, [], [], np.zeros((0, 3)), np.zeros((0, 3)))
    ctx.inject_observations(1, [o[0] for o in obs], [1] * len(obs), np.array([o[1] for o in obs]), np.array([o[2] for o in obs]))
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.run_staged(0, 2, with_ekf=2)
    ctx.sync()
    assert ekf_kernels_run(ctx.profile_get()) == CHAIN_KERNELS["general"]
    lg = np.array(lit.log, np.int32).reshape(-1, 3)
    assert (lg[:, 2] == 0).sum() == n_new and (lg[:, 2] == 1).sum() == n_known + 1
    gi, gx, ga, _, _ = ctx.get_observations()
    assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), lg), "pop order / branches differ"
    mu_g, S_g = ctx.get_state()
    assert mu_g.shape == lit.mu.shape == (3 + 3 * (L + n_new),)
    e_mu, e_S = float(np.abs(mu_g - lit.mu).max()), rel_err(S_g, lit.sigma)
    print(f"mixed frame: |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert np.allclose(mu_g, lit.mu, rtol=1e-9, atol=1e-11) and e_S <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("chain,m,L,ML", CASES, ids=[f"{c}-m{m}-L{L}-ml{ml}" for c, m, L, ml in CASES])
def test_per_frame_chain_on_gpu(chain, m, L, ML):
    run_one_frame(chain, m, L, ML, seed=1000 * m + L + ML)


@pytest.mark.gpu
def test_mixed_frame_and_caps_on_gpu():
    test_mixed_frame_on_the_general_chain()
    for chain in ("fast", "mid"):
        test_one_correction_over_the_cap_is_reported(chain)


# the update kernel k_ekf_update_mfma<5> runs for 938 <= max_landmarks <= 1065, <4> for every other size
GPU_CASES = [(L, chain, cap, m) for L in (937, 938, 1000, 1065, 1066) for chain, cap, m in (("mid", 64, 64), ("general", 128, 100))]


@pytest.mark.gpu
@pytest.mark.parametrize("L,chain,cap,m", GPU_CASES, ids=[f"{c}-m{m}-L{L}" for L, c, _, m in GPU_CASES])
def test_update_tile_widths_on_gpu(L, chain, cap, m):
    """both tile widths of the update kernel and the edges of their tiles (double reference: long double takes minutes here)"""
    run_one_frame(chain, m, L, L, seed=L + m, dtype=np.float64, waves=64)


# ---- windows -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _window_case(n, frames_in_window, seed):
    """arming frame, the frame that maps n landmarks, then frames_in_window frames that see all n (seeds where no gate drops one),
    with the per-frame chain's result (ASLAM_WIN_PIECE does not reach it)"""
    frames, exp = make_case(seed, [(frames_in_window + 2, list(range(n)), False)], n)
    for e in exp[2:]:
        assert (e["log"][:, 2] == 1).sum() == n, "a gate dropped an observation: the case does not test m = |S|"
    (mu2, S2), prof2, _ = run_device(frames, exp, batch=len(frames), windows=False, max_landmarks=n + 3, max_updates=64)
    assert prof2["k_ekf_win_step"][0] == 0
    return frames, exp, mu2, S2


def _window_run(n, frames_in_window, seed):
    """the window against the literal transcription (1e-9, in run_device) and against the per-frame chain (1e-10)"""
    frames, exp, mu2, S2 = _window_case(n, frames_in_window, seed)
    (mu, S), prof, worst = run_device(frames, exp, batch=len(frames), max_landmarks=n + 3, max_updates=64)
    e = rel_err(S, S2)
    print(f"|S| = {n}, {frames_in_window} window frames: literal {worst:.3g}, per-frame chain |dmu| {np.abs(mu - mu2).max():.3g} "
          f"Sigma {e:.3g} relative")
    assert np.allclose(mu, mu2, rtol=1e-10, atol=1e-12) and e <= 1e-10
    return prof


WIN_SETS = (20, 21, 41, 42, 62, 63)


@pytest.mark.parametrize("piece", [1, 8])
@pytest.mark.parametrize("n", WIN_SETS)
def test_window_set_size_edges(n, piece, monkeypatch):
    monkeypatch.setenv("ASLAM_WIN_PIECE", str(piece))
    prof = _window_run(n, 9, seed=n)                   # 9 frames: a piece of 8 and one of 1 with the default pieces
    assert prof["k_ekf_win_step"][0] > 0, "no window was formed"


@pytest.mark.parametrize("k", [2, 16, 17, 64, 65])
def test_window_lengths(k):
    prof = _window_run(12, k, seed=12)
    assert prof["k_ekf_win_step"][0] > 0, "no window was formed"


@pytest.mark.parametrize("case", ["set_of_64", "frame_of_64"])
def test_no_window_past_63(case):
    """a set of 64 landmarks (frames of 63 alternating between two sets) and a frame of 64 corrections stay on the per-frame chain"""
    if case == "set_of_64":
        groups = [(1, list(range(63)), False), (1, list(range(1, 64)), False)] + [(1, list(range(i % 2, 63 + i % 2)), False) for i in range(6)]
    else:
        groups = [(6, list(range(64)), False)]
    frames, exp = make_case(64, groups, 64)
    (mu, S), prof, worst = run_device(frames, exp, batch=len(frames), max_landmarks=66, max_updates=64)
    assert prof["k_ekf_win_step"][0] == 0, "a window was formed"
    print(f"{case}: literal {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [1, 8])
@pytest.mark.parametrize("n", WIN_SETS)
def test_window_set_size_edges_on_gpu(n, piece, monkeypatch):
    monkeypatch.setenv("ASLAM_WIN_PIECE", str(piece))
    prof = _window_run(n, 9, seed=n)
    assert prof["k_ekf_win_step"][0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 16, 17, 64, 65])
def test_window_lengths_on_gpu(k):
    prof = _window_run(12, k, seed=12)
    assert prof["k_ekf_win_step"][0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["set_of_64", "frame_of_64"])
def test_no_window_past_63_on_gpu(case):
    test_no_window_past_63(case)


# ---- localization --------------------------------------------------------------------------------------------------------------

LOC_M = (1, 63, 64, 65, 127, 128)


def _localize_full_width(m):
    """m known markers in each of three frames (the third repeats some of the second: "stationary" no-ops), detection order
    shuffled, against the frozen-map reference"""
    rng = np.random.RandomState(m)
    n = m + 5
    ids, xyth = random_map(rng, n, id_pool=ID_TABLE)
    pose0 = np.array([0.1, -0.2, math.pi - 0.003])
    sig0 = np.array([[0.02, 0.001, 0.0], [0.001, 0.03, -0.002], [0.0, -0.002, 0.01]])
    frames, prev = [], {}
    for f in range(3):
        sel = rng.permutation(n)[:m]
        obs = []
        for li in sel:
            dx, dy = xyth[li, 0] - pose0[0], xyth[li, 1] - pose0[1]
            c, s = math.cos(pose0[2]), math.sin(pose0[2])
            z = np.array([dx * c + dy * s, -dx * s + dy * c, float(wrap_once(LD(xyth[li, 2] - pose0[2])))]) + rng.normal(0, 0.01, 3)
            if f == 2 and int(ids[li]) in prev and rng.rand() < 0.3:
                z = prev[int(ids[li])].copy()
            obs.append((int(ids[li]), 1, z, rng.uniform(0.01, 0.05, 3)))
        prev = {o[0]: o[2] for o in obs}
        frames.append((rng.uniform(1, 4), rng.uniform(1, 4), 0.05, obs))
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=3, persistent_waves=4, max_landmarks=n)
    ctx.stage_encoders([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames])
    for s, fr in enumerate(frames):
        inject(ctx, s, fr[3])
    ctx.localize_begin(ids, xyth, pose0, sig0)
    ref = FrozenMapLocalizer(ids, xyth, pose0, sig0)
    ctx.profile_enable(True)
    ctx.profile_reset()
    worst = 0.0
    for f, (wl, wr, dt, obs) in enumerate(frames):
        ctx.run_staged(f, 1, with_ekf=2)
        ctx.sync()
        ref.add_encoder(wl, wr, dt)
        ref.add_observations(obs)
        mu, S = ctx.get_state()
        e = max(np.abs(mu[:3] - ref.mu).max(), np.abs(S[:3, :3] - ref.P).max() / np.abs(ref.P).max())
        worst = max(worst, e)
        assert e <= 1e-9, f"frame {f}: pose / Sigma_xx differ by {e}"
        assert np.array_equal(mu[3:], xyth.reshape(-1)) and not S[3:, :].any() and not S[:, 3:].any()
        gi, gx, ga, _, _ = ctx.get_observations()
        assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), ref.log_array()), f"frame {f}: pops differ"
        assert ctx.get_slot_ekf_stats(f, 1)[0].tolist() == ref.stats
    assert ctx.profile_get()["k_loc_steps"][0] == 3
    print(f"localize m = {m}: worst {worst:.3g}")


@pytest.mark.parametrize("m", LOC_M)
def test_localize_full_width(m):
    _localize_full_width(m)


@pytest.mark.gpu
@pytest.mark.parametrize("m", LOC_M)
def test_localize_full_width_on_gpu(m):
    _localize_full_width(m)
