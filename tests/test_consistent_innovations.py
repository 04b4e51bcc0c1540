"""Consistent innovations (aslam_set_consistent_innovations): every correction of a frame is formed at the mean the
previous one left, e_i = ze_i - H_i (mu_{i-1} - mu_0), against the sequential references of tests/consistent_reference.py.

Inputs: random_state / observe of tests/ekf_reference.py (noise 0.03); an outlier is a true sighting displaced by OUTLIER of
slam_gate_reference.py; gate_d2 = 1.0 on the SLAM chains.  Every case asserts on its own inputs, before it compares anything discrete,
that no d2 lies within 1e-6 (relative) of the gate, no ||ze|| within 1e-6 of 1, and that the reference alone gives the planted verdicts.
Tolerances, the project's: mu rtol 1e-9 / atol 1e-11, Sigma 1e-9 relative, nis_sum and d2_max 1e-9 relative; counts, ids, actions, flags
and worst_id exact.  Contexts as in test_slam_gate.py: 64 x 64 images, max_batch 2, injected observations, with_ekf = 2.  Every device
case runs on the session's library (the emulation without a GPU) and again under -m gpu (the `library` fixture)."""
import functools
import math

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from consistent_reference import ConsistentLiteral, ConsistentLocalizer, ConsistentUmapLocalizer, consistent_step, joint_mean
from ekf_reference import CHAIN_CAP, CHAIN_KERNELS, LD, ekf_kernels_run, observe, predicted_pose, random_state, rel_err
from slam_gate_reference import DEFAULTS, OUTLIER, TRACK_ZERO, advance_track, assert_margins, check_slot_health, check_track
from test_ekf_sizes import DT, ID_TABLE, WL, WR, landmark_ids, pick
from test_slam_gate import CAM, FINISH, context, inject, no_obs, outlier_positions, patterns_for, same_bytes, stage_case
from tests.gate_reference import GatedLocalizer
from tests.gate_reference import check_slot_health as check_loc_health
from tests.gate_reference import check_track as check_loc_track
from tests.test_innovation_gate import close, fleet_call, fleet_context, h_of
from tests.test_localize import POSE0, SIG0, FrozenMapLocalizer, emu_context, random_map
from tests.test_localize import inject as inject_loc
from tests.test_uncertain_map import check_robot, check_single, spd_blocks, staged

E_INVALID = -1
INF = float("inf")
GATE = 1.0


@pytest.fixture(params=["session", pytest.param("gfx950", marks=pytest.mark.gpu)])
def library(request):
    if request.param == "gfx950":
        assert capi.lib_path().endswith("libaruco_slam_hip.so"), "the gpu cases must run the native gfx950 library"
    return request.param


# (chain, m, L): both sides of the fast chain's m x m mapping, of k_ekf_mid64's blocks per thread, of kSmallMax (3m = 96) and the
# general path above it; L > m where the gathered rows and columns are not the whole state
SHAPES = [("fast", 1, 1), ("fast", 2, 2), ("fast", 24, 24), ("fast", 24, 43),
          ("mid", 24, 43), ("mid", 25, 25), ("mid", 64, 64),
          ("general", 2, 2), ("general", 32, 32), ("general", 33, 52), ("general", 65, 65), ("general", 128, 128)]
SHAPE_IDS = [f"{c}-m{m}-L{L}" for c, m, L in SHAPES]


@functools.lru_cache(maxsize=None)
def frame_case(m, L, pattern="none", nan_at=None, gate=INF):
    """a dense state, m sightings of known landmarks in pop order with the pattern's outliers planted (nan_at: that pop position's z[0]
    is NaN), a detection order, and the long-double consistent step on them under `gate`.  Computed once, shared with the GPU twin."""
    rng = np.random.RandomState(1000 * m + L)
    mu, S = random_state(rng, L)
    ids, observable = landmark_ids(rng, L)
    seen = pick(rng, observable, m)
    out = outlier_positions(pattern, m)
    obs = []
    for k, (i, z, r) in enumerate(observe(rng, mu, seen, post_predict=predicted_pose(mu, WL, WR, DT))):
        z = z + OUTLIER if k in out else z
        if k == nan_at:
            z = z.copy()
            z[0] = math.nan
        obs.append((i, z, r))
    det = rng.permutation(m)
    mu_r, S_r, info = consistent_step(mu, S, WL, WR, DT, obs, gate, ids=ids)
    want_rej = [math.isfinite(gate) and (k in out or k == nan_at) for k in range(m)]
    assert_margins(gate, info["d2"], info["norms"])
    assert info["rejected"] == want_rej, "the reference alone does not separate the planted outliers from the true sightings"
    case = dict(mu=mu, S=S, ids=ids, seen=seen, obs=obs, det=det, mu_ref=mu_r, S_ref=S_r, info=info, rejected=want_rej)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def run_frame(chain, case, ML, consistent, gate=None, windows=True):
    """the case's frame on a fresh context; returns the context, synchronised, and its profile"""
    ctx = context(CHAIN_CAP[chain], ML, windows=windows)
    if gate is not None:
        ctx.set_slam_gate(gate_d2=gate)
    if consistent:
        ctx.set_consistent_innovations(True)
    stage_case(ctx, case)
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.run_staged(0, 2, with_ekf=2)
    ctx.sync()
    return ctx, ctx.profile_get()


def check_state(ctx, case, where):
    mu_g, S_g = ctx.get_state()
    assert np.isfinite(mu_g).all() and np.isfinite(S_g).all()
    e_mu, e_S = float(np.abs(mu_g - case["mu_ref"]).max()), rel_err(S_g, case["S_ref"])
    print(f"{where}: |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert np.allclose(mu_g, case["mu_ref"], rtol=1e-9, atol=1e-11), f"{where}: mu differs by {e_mu}"
    assert e_S <= 1e-9, f"{where}: Sigma differs by {e_S} (relative)"
    return mu_g, S_g


# ---- 1. the reference itself (CPU only) ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,L", [(1, 1), (2, 2), (24, 43), (64, 64), (128, 128)])
def test_sequential_consistent_mean_is_the_joint_update(m, L):
    case = frame_case(m, L)
    mu_j = joint_mean(case["info"]["mu0"], case["info"]["S0"], case["obs"])
    d = float(np.abs(mu_j - case["mu_ref"]).max())
    print(f"m {m} L {L}: sequential - joint {d:.3g}")
    assert d <= 1e-12


def test_frozen_reference_is_the_gated_reference_step():
    from slam_gate_reference import gated_reference_step
    case = frame_case(24, 43, "third", gate=GATE)
    a = gated_reference_step(case["mu"], case["S"], WL, WR, DT, case["obs"], GATE, ids=case["ids"])
    b = consistent_step(case["mu"], case["S"], WL, WR, DT, case["obs"], GATE, ids=case["ids"], consistent=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["d2"] == b[2]["d2"]


# ---- 2. SLAM chains, ungated ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chain,m,L", SHAPES, ids=SHAPE_IDS)
def test_ungated_chain(library, chain, m, L):
    case = frame_case(m, L)
    ML = L + (m % 3)
    on, prof = run_frame(chain, case, ML, True)
    assert ekf_kernels_run(prof) == CHAIN_KERNELS[chain], f"ran {sorted(ekf_kernels_run(prof))}"
    mu_on, S_on = check_state(on, case, f"{chain} m {m} L {L}")
    assert on.get_slot_ekf_stats(1, 1)[0].tolist() == [m, 0, m, 0]
    off, _ = run_frame(chain, case, ML, False, windows=False)
    mu_off, S_off = off.get_state()
    assert np.array_equal(S_on, S_off), "Sigma does not depend on the innovation: it must keep its bits"
    d = float(np.abs(mu_on - mu_off).max())
    print(f"{chain} m {m}: |mu_on - mu_off| {d:.3g}")
    if m >= 2:
        assert d > 1e-3, "the switch changed nothing"
    else:
        assert np.array_equal(mu_on, mu_off), "one correction: e_0 = ze_0"


# ---- 3. SLAM chains, gated ------------------------------------------------------------------------------------------------------------

GATED = [(c, m, L, p) for c, m, L in SHAPES for p in patterns_for(m)]
NAN_CASES = [(c, m, L, w) for c, m, L in (("fast", 7, 9), ("mid", 30, 33), ("general", 7, 9), ("general", 40, 45)) for w in ("first", "middle", "last")]


def run_gated(chain, m, L, pattern, nan_at=None, gate=GATE):
    case = frame_case(m, L, pattern, nan_at, gate)
    ctx, prof = run_frame(chain, case, L + 1, True, gate=gate)
    where = f"{chain} m {m} L {L} {pattern} nan {nan_at} gate {gate}"
    assert ekf_kernels_run(prof) == CHAIN_KERNELS[chain] | {FINISH}, f"ran {sorted(ekf_kernels_run(prof))}"
    rej = np.array(case["rejected"])
    gi, gx, ga, _, _ = ctx.get_observations()
    assert np.array_equal(gx, case["seen"]) and np.array_equal(gi, case["ids"][case["seen"]]), "pop order differs"
    assert np.array_equal(ga, np.where(rej, 3, 1)), f"actions {ga.tolist()}"
    assert ctx.get_slot_ekf_stats(1, 1)[0].tolist() == [m, 0, int((~rej).sum()), 0]
    check_slot_health(ctx.get_slot_health(1, 1)[0], case["info"]["health"], where)
    track = dict(TRACK_ZERO)
    advance_track(track, dict(attempted=0, accepted=0, rejected=0), {**DEFAULTS})
    advance_track(track, case["info"]["health"], {**DEFAULTS})
    check_track(ctx.get_track_health(), track, where)
    if math.isfinite(gate) or nan_at is None:
        check_state(ctx, case, where)
    return ctx, case


@pytest.mark.parametrize("chain,m,L,pattern", GATED, ids=[f"{c}-m{m}-L{L}-{p}" for c, m, L, p in GATED])
def test_gated_chain(library, chain, m, L, pattern):
    _, case = run_gated(chain, m, L, pattern)
    if pattern == "third" and m >= 3:
        d2 = np.array(case["info"]["d2"]); rej = np.array(case["rejected"])
        print(f"true d2 <= {d2[~rej].max():.3g}, outlier d2 >= {d2[rej].min():.3g}")


@pytest.mark.parametrize("chain,m,L,where", NAN_CASES)
def test_nan_sighting_is_rejected(library, chain, m, L, where):
    nan_at = {"first": 0, "middle": m // 2, "last": m - 1}[where]
    _, case = run_gated(chain, m, L, "none", nan_at=nan_at)
    obs = [o for k, o in enumerate(case["obs"]) if k != nan_at]          # the reference with the NaN sighting equals the one without
    mu_r, S_r, _ = consistent_step(case["mu"], case["S"], WL, WR, DT, obs, GATE, ids=case["ids"])
    assert np.array_equal(mu_r, case["mu_ref"]) and np.array_equal(S_r, case["S_ref"])


@pytest.mark.parametrize("chain,m,L", [("fast", 24, 43), ("mid", 25, 25), ("general", 32, 32), ("general", 65, 65)])
def test_gate_at_infinity_is_the_ungated_result_with_records(library, chain, m, L):
    ctx, case = run_gated(chain, m, L, "third", gate=INF)
    plain = frame_case(m, L, "third")
    assert np.array_equal(plain["mu_ref"], case["mu_ref"])
    ungated, _ = run_frame(chain, plain, L + 1, True)
    mu_u, S_u = ungated.get_state()
    mu_g, S_g = ctx.get_state()
    assert np.allclose(mu_g, mu_u, rtol=1e-9, atol=1e-11) and rel_err(S_g, S_u) <= 1e-9
    assert ctx.get_slot_health(1, 1)[0]["rejected"] == 0 and ctx.get_slot_health(1, 1)[0]["attempted"] == m


# ---- 4. fleet SLAM and rigs -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fleet_case(cap, R):
    """R robots on maps of their own, one arming frame and two stepping frames each; the middle robot of three is absent from the last round"""
    rng = np.random.RandomState(60 + cap + R)
    m = {24: 9, 64: 27}[cap]
    robots = []
    for r in range(R):
        L = m + 2 + r
        mu, S = random_state(rng, L, heading=0.3 * r - 0.5)
        ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
        wl, wr, dt = WL + 0.25 * r, WR + 0.4 * r, DT * (1 + 0.1 * r)
        pose, frames = mu[:3], []
        for f in range(2):
            pose = predicted_pose(np.concatenate([pose, mu[3:]]), wl, wr, dt)
            seen = np.sort(rng.choice(L, m, replace=False))
            out = outlier_positions("third", m) if r % 2 == 0 else set()
            obs = [(i, z + (OUTLIER if k in out else 0.0), rd) for k, (i, z, rd) in enumerate(observe(rng, mu, seen, post_predict=pose))]
            frames.append((wl, wr, dt, obs, [int(k) for k in rng.permutation(len(obs))]))
        robots.append(dict(mu=mu, S=S, ids=ids, frames=frames))
    return robots


@pytest.mark.parametrize("cap,R", [(24, 1), (24, 3), (64, 3)])
def test_fleet_slam_rounds(library, cap, R):
    robots = fleet_case(cap, R)
    ML = max(len(r["ids"]) for r in robots) + 1
    ctx = context(cap, ML, batch=3 * R)
    ctx.set_slam_gate(gate_d2=GATE)
    ctx.set_consistent_innovations(True)
    ctx.fleet_slam_begin([CAM] * R)
    assert ctx.get_consistent_innovations(), "the switch survives a fleet begin"
    for r, rob in enumerate(robots):
        ctx.fleet_set_state(r, rob["mu"], rob["S"], rob["ids"])
    last = [r for r in range(R) if not (R == 3 and r == 1)]                 # robot 1 of three is absent from the last round
    order = list(range(R)) + list(range(R)) + last
    enc = np.zeros((len(order), 3))
    for s, r in enumerate(order):
        f = s // R - 1
        if f < 0:
            ctx.inject_observations(s, *no_obs())
        else:
            fr = robots[r]["frames"][f]
            enc[s] = fr[:3]
            inject(ctx, s, [(int(robots[r]["ids"][fr[3][k][0]]), fr[3][k][1], fr[3][k][2]) for k in fr[4]])
    ctx.stage_encoders(enc[:, 0], enc[:, 1], enc[:, 2])
    ctx.fleet_run_staged(0, order[:2 * R], with_ekf=2)
    ctx.fleet_run_staged(2 * R, last, with_ekf=2)
    ctx.sync()
    slots = ctx.get_slot_health(0, len(order))
    for r, rob in enumerate(robots):
        mu, S = rob["mu"], rob["S"]
        nf = 2 if r in last else 1
        for f in range(nf):
            fr = rob["frames"][f]
            mu, S, info = consistent_step(mu, S, fr[0], fr[1], fr[2], fr[3], GATE, ids=rob["ids"])
            assert_margins(GATE, info["d2"], info["norms"])
            assert info["rejected"] == [r % 2 == 0 and k in outlier_positions("third", len(fr[3])) for k in range(len(fr[3]))]
            slot = R + r if f == 0 else 2 * R + last.index(r)
            check_slot_health(slots[slot], info["health"], f"robot {r} frame {f}")
        mu_g, S_g = ctx.fleet_get_state(r)
        e_S = rel_err(S_g, S)
        assert np.allclose(mu_g, mu, rtol=1e-9, atol=1e-11) and e_S <= 1e-9, f"robot {r}: {np.abs(mu_g - mu).max()}, {e_S}"
        # a single consistent context on the same frames: bit for bit
        one = context(cap, ML, batch=3)
        one.set_slam_gate(gate_d2=GATE)
        one.set_consistent_innovations(True)
        one.set_state(rob["mu"], rob["S"], rob["ids"])
        one.stage_encoders([0.0] + [f[0] for f in rob["frames"]], [0.0] + [f[1] for f in rob["frames"]], [0.0] + [f[2] for f in rob["frames"]])
        one.inject_observations(0, *no_obs())
        for f in range(nf):
            fr = rob["frames"][f]
            inject(one, 1 + f, [(int(rob["ids"][fr[3][k][0]]), fr[3][k][1], fr[3][k][2]) for k in fr[4]])
        one.run_staged(0, 1 + nf, with_ekf=2)
        one.sync()
        mu_1, S_1 = one.get_state()
        assert np.array_equal(mu_g, mu_1) and np.array_equal(S_g, S_1), f"robot {r}: fleet != single consistent context"


def test_rig_step(library):
    rng = np.random.RandomState(3)
    L, batch = 12, 4
    mu, S = random_state(rng, L, heading=-0.7)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    seen = [0, 2, 3, 5, 8, 9, 11]
    obs = [(i, z + (OUTLIER if i in (2, 8) else 0.0), r) for i, z, r in observe(rng, mu, seen, post_predict=predicted_pose(mu, WL, WR, DT))]
    named = [(int(ids[i]), z, r) for i, z, r in obs]
    ctx = context(24, L + 1, batch=batch)
    ctx.set_slam_gate(gate_d2=GATE)
    ctx.set_consistent_innovations(True)
    ctx.set_camera_rig([CAM, CAM])
    ctx.set_state(mu, S, ids)
    ctx.stage_encoders([0.0, 0.0, WL, WL], [0.0, 0.0, WR, WR], [0.0, 0.0, DT, DT])
    ctx.inject_observations(0, *no_obs())
    ctx.inject_observations(1, *no_obs())
    inject(ctx, 2, named[:3])
    inject(ctx, 3, named[3:])
    ctx.run_staged_rig(0, 2, with_ekf=2)
    ctx.sync()
    mu_r, S_r, info = consistent_step(mu, S, WL, WR, DT, obs, GATE, ids=ids)
    assert_margins(GATE, info["d2"], info["norms"])
    assert info["rejected"] == [i in (2, 8) for i in seen]
    check_slot_health(ctx.get_slot_health(batch + 1, 1)[0], info["health"], "rig step 1")
    assert ctx.get_rig_observations()[2].tolist() == [3 if i in (2, 8) else 1 for i in seen]
    check_state(ctx, dict(mu_ref=mu_r, S_ref=S_r), "rig step")


# ---- 5. localization ------------------------------------------------------------------------------------------------------------------

def loc_sight(pose, ids, xyth, sel, rng, moved=()):
    obs = []
    for k, li in enumerate(sel):
        r = rng.uniform(0.01, 0.05, 3)
        z = h_of(pose, xyth[li]) + rng.normal(0, 1, 3) * np.sqrt(r)
        if k in moved:
            z = z + np.array([1.5, -1.0, 0.8])
        z[2] = float(np.arctan2(np.sin(z[2]), np.cos(z[2])))
        obs.append((int(ids[li]), 1, z, r))
    return obs


@functools.lru_cache(maxsize=None)
def loc_frames(m, seed):
    """a map of max(m, 12) + 4 landmarks and four frames from a moving truth: m sightings (every fifth displaced when m >= 5, the last
    one when 2 <= m < 5), then the same list again with the first sighting repeated identically (a stationary no-op between
    corrections) and, for m < 128, one id twice (the heap path), then two more plain frames"""
    rng = np.random.RandomState(seed)
    n = max(m, 12) + 4
    ids, xyth = random_map(rng, n, id_pool=600)
    truth = FrozenMapLocalizer(ids, xyth, POSE0, np.zeros((3, 3)))
    frames = []
    for f in range(4):
        wl, wr, dt = rng.uniform(1, 4), rng.uniform(1, 4), 0.05
        if f:
            truth.predict(wl, wr, dt)
        sel = np.sort(rng.permutation(n)[:m])
        moved = tuple(range(4, m, 5)) if m >= 5 else ((m - 1,) if m >= 2 and f == 0 else ())
        obs = loc_sight(truth.mu, ids, xyth, sel, rng, moved)
        if f == 0:
            again = obs[0]                                                     # pop position 0 is never displaced
        if f == 1:
            obs = [o for o in obs if o[0] != again[0]]
            obs.insert(len(obs) // 2, again)                                   # the previous frame's accepted sighting again: stationary
            if m < 128 and len(obs) > 1:
                li = int(np.nonzero(ids == obs[0][0])[0][0])
                obs.append(loc_sight(truth.mu, ids, xyth, [li], rng)[0])       # one id twice
            obs = obs[:128]
        frames.append((wl, wr, dt, [obs[k] for k in rng.permutation(len(obs))]))
    return ids, xyth, frames


def loc_reference(ids, xyth, C, frames, gate, pose0=POSE0):
    ref = (ConsistentUmapLocalizer(ids, xyth, C, pose0, SIG0, gate) if C is not None else ConsistentLocalizer(ids, xyth, pose0, SIG0, gate))
    out = []
    for fr in frames:
        ref.add_encoder(*fr[:3])
        ref.add_observations(fr[3])
        out.append(dict(stats=list(ref.stats), health=dict(ref.health), track=dict(ref.track), log=ref.log_array()))
    ref.assert_margins()
    return ref, out


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("umap", [False, True], ids=["fixed", "uncertain"])
@pytest.mark.parametrize("m", [1, 2, 12, 128])
def test_localization_single_and_fleet(library, m, umap, gated):
    ids, xyth, frames = loc_frames(m, 300 + m)
    n = len(ids)
    C = spd_blocks(np.random.RandomState(m), n, 0.03) if umap else None
    gate = dict(gate_d2=DEFAULTS["gate_d2"]) if gated else None
    ref, want = loc_reference(ids, xyth, C, frames, gate)
    acts = [a for w in want for a in w["log"][:, 2].tolist()]
    assert 2 in acts, "no stationary no-op in the frames"
    if gated and m >= 2:
        assert 3 in acts and 1 in acts, "the reference alone does not show both verdicts"
    if m in (2, 12):
        lg = want[1]["log"][:, 0].tolist()
        assert len(set(lg)) < len(lg), "no id twice"
    frozen, _ = (None, None) if umap else GatedLocalizerRun(ids, xyth, frames, gate)
    # the single filter: frame by frame
    one = emu_context(len(frames), max_landmarks=n)
    if gated:
        one.set_innovation_gate(**gate)
    one.set_consistent_innovations(True)
    (one.localize_begin_uncertain(ids, xyth, C, POSE0, SIG0) if umap else one.localize_begin(ids, xyth, POSE0, SIG0))
    assert one.get_consistent_innovations(), "the switch survives aslam_localize_begin"
    staged(one, frames)
    one.profile_enable(True)
    one.profile_reset()
    for s, w in enumerate(want):
        one.run_staged(s, 1, with_ekf=2)
        assert one.get_slot_ekf_stats(s, 1)[0].tolist() == w["stats"], f"frame {s}"
        gi, gx, ga, _, _ = one.get_observations()
        assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), w["log"]), f"frame {s}: pops / actions differ"
        if gated:
            check_loc_health(one.get_slot_health(s, 1)[0], w["health"], f"frame {s}")
            check_loc_track(one.get_track_health(), w["track"], f"frame {s}")
    prof = one.profile_get()
    assert prof["k_loc_steps"][0] == len(frames) and not ekf_kernels_run(prof)
    mu_1, S_1 = one.get_state()
    if umap:
        check_single(one, ref, f"m {m}")
    else:
        close(mu_1[:3], S_1[:3, :3], ref, f"m {m}")
        if m >= 2 and not gated:
            assert np.abs(mu_1[:3] - frozen.mu).max() > 1e-6, "the switch changed nothing"
    # fleets of 1, 2 and 5 robots in a call, every robot on the same frames: each equals the single filter bit for bit
    for R in (1, 2, 5):
        fleet = emu_context(R * len(frames), max_landmarks=n)
        if gated:
            fleet.set_innovation_gate(**gate)
        fleet.set_consistent_innovations(True)
        if umap:
            fleet.fleet_begin_uncertain([CAM] * R, ids, xyth, C, [POSE0] * R, [SIG0] * R)
        else:
            fleet.fleet_begin([CAM] * R, ids, xyth, [POSE0] * R, [SIG0] * R)
        assert fleet.get_consistent_innovations(), "the switch survives a fleet begin"
        order = [r for _ in frames for r in range(R)]
        fleet_call(fleet, order, [fr for fr in frames for _ in range(R)])
        poses, sigs = fleet.fleet_get_poses()
        for r in range(R):
            assert np.array_equal(poses[r], mu_1[:3]) and np.array_equal(sigs[r], S_1[:3, :3]), f"R {R} robot {r}: fleet != single"
            if umap:
                assert np.array_equal(fleet.fleet_get_cross(r), S_1[:3, 3:]), f"R {R} robot {r}: cross strip bits"
        if gated:
            health = fleet.get_slot_health(0, len(order))
            for s, w in enumerate(want):
                check_loc_health(health[s * R + R - 1], w["health"], f"R {R} frame {s}")
            check_loc_track(fleet.fleet_get_health()[R - 1], want[-1]["track"], f"R {R}")


def GatedLocalizerRun(ids, xyth, frames, gate):
    """the frozen-mean reference on the same frames"""
    ref = GatedLocalizer(ids, xyth, POSE0, SIG0, gate if gate is not None else dict(gate_d2=INF))
    for fr in frames:
        ref.add_encoder(*fr[:3])
        ref.add_observations(fr[3])
    return ref, None


# ---- 6. what it is for ----------------------------------------------------------------------------------------------------------------

def ring_map(n=12, radius=2.5):
    a = 2 * math.pi * np.arange(n) / n
    xyth = np.stack([radius * np.cos(a), radius * np.sin(a), np.arctan2(-np.sin(a), -np.cos(a))], 1)
    return (10 + 3 * np.arange(n)).astype(np.int32), xyth


def one_frame_run(consistent, gate):
    """5 cm off in x, Sigma = 1e-2 I, 12 exact sightings at R = 1e-6: returns the position error and the slot's health record"""
    ids, xyth = ring_map()
    truth = np.array([0.2, -0.1, 0.4])
    obs = [(int(ids[k]), 1, h_of(truth, xyth[k]), np.full(3, 1e-6)) for k in range(12)]
    ctx = emu_context(2, max_landmarks=12)
    if gate:
        ctx.set_innovation_gate()
    ctx.set_consistent_innovations(consistent)
    ctx.localize_begin(ids, xyth, truth + [0.05, 0.0, 0.0], 1e-2 * np.eye(3))
    ctx.stage_encoders([0.0], [0.0], [0.0])
    inject_loc(ctx, 0, obs)
    ctx.run_staged(0, 1, with_ekf=2)
    mu, _ = ctx.get_state()
    return float(np.hypot(*(mu[:2] - truth[:2]))), (ctx.get_slot_health(0, 1)[0] if gate else None)


def test_one_frame_of_exact_sightings(library):
    err_on, _ = one_frame_run(True, False)
    err_off, _ = one_frame_run(False, False)
    print(f"position error: consistent {err_on:.3g} m, frozen {err_off:.3g} m")
    assert err_on <= 1e-4
    assert err_off > 0.05, "the parent's behaviour"
    _, h_on = one_frame_run(True, True)
    _, h_off = one_frame_run(False, True)
    assert int(h_on["accepted"]) == 12 and int(h_on["rejected"]) == 0
    assert int(h_off["rejected"]) >= 1


LAP_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
SIGMA = 0.01


@functools.lru_cache(maxsize=None)
def lap_case(seed):
    """40 frames of 12 sightings with R = sigma^2; the truth is driven with the filter's own wheel noise (Q_k |w| on each wheel)"""
    rng = np.random.RandomState(9000 + seed)
    ids, xyth = ring_map()
    kl = kr = 0.05; b = 0.09; Qk = 0.01
    pose = np.array([0.1, -0.2, 0.3])
    frames = []
    for f in range(40):
        wl, wr, dt = rng.uniform(20, 40), rng.uniform(20, 40), 0.05            # 5 to 10 cm a frame: no sighting repeats within 0.01
        if f:
            # the filter's motion model, then its own process noise: F n with F = (kl dt / 2) [[c, c], [s, s], [1/b, -1/b]], n ~ N(0, Q_k |w|)
            dsl, dsr = kl * dt * wl, kr * dt * wr
            dth, ds = (dsr - dsl) / (2 * b), 0.5 * (dsr + dsl)
            th = pose[2] + 0.5 * dth
            c, s = math.cos(th), math.sin(th)
            nl, nr = rng.normal(0, math.sqrt(Qk * abs(wl))), rng.normal(0, math.sqrt(Qk * abs(wr)))
            g = 0.5 * kl * dt
            pose = pose + np.array([ds * c + g * c * (nl + nr), ds * s + g * s * (nl + nr), dth + g / b * (nl - nr)])
            pose[2] = math.atan2(math.sin(pose[2]), math.cos(pose[2]))
        obs = []
        for k in range(12):
            z = h_of(pose, xyth[k]) + rng.normal(0, SIGMA, 3)
            z[2] = math.atan2(math.sin(z[2]), math.cos(z[2]))
            obs.append((int(ids[k]), 1, z, np.full(3, SIGMA ** 2)))
        frames.append((wl, wr, dt, obs))
    ref = ConsistentLocalizer(ids, xyth, np.array([0.1, -0.2, 0.3]), 1e-4 * np.eye(3), dict(gate_d2=INF))
    nis = att = 0
    for fr in frames:
        ref.add_encoder(*fr[:3])
        ref.add_observations(fr[3])
        nis += ref.health["nis_sum"]; att += ref.health["accepted"]
    return ids, xyth, frames, nis, att


def test_forty_frames_have_a_chi_square_nis(library):
    tot = n = 0
    for seed in LAP_SEEDS:
        ids, xyth, frames, nis_ref, att_ref = lap_case(seed)
        # (a sighting that repeats the previous frame's within 0.01 is a no-op, not a correction: a few of the 480 may be)
        assert att_ref >= 470 and 2.5 <= nis_ref / att_ref <= 3.5, f"seed {seed}: the reference alone gives {nis_ref / att_ref} over {att_ref}"
        ctx = emu_context(len(frames), max_landmarks=12)
        ctx.set_innovation_gate(gate_d2=INF)
        ctx.set_consistent_innovations(True)
        ctx.localize_begin(ids, xyth, np.array([0.1, -0.2, 0.3]), 1e-4 * np.eye(3))
        staged(ctx, frames)
        ctx.run_staged(0, len(frames), with_ekf=2)
        h = ctx.get_slot_health(0, len(frames))
        nis, acc = float(h["nis_sum"].sum()), int(h["accepted"].sum())
        print(f"seed {seed}: mean d2 {nis / acc:.4f} (reference {nis_ref / att_ref:.4f})")
        assert acc == att_ref and 2.5 <= nis / acc <= 3.5, f"seed {seed}: mean d2 {nis / acc}"
        tot += nis; n += acc
    ref_pooled = sum(lap_case(s)[3] for s in LAP_SEEDS) / sum(lap_case(s)[4] for s in LAP_SEEDS)
    assert 2.8 <= ref_pooled <= 3.2, f"the reference alone gives a pooled mean of {ref_pooled}"
    print(f"pooled mean d2 {tot / n:.4f} over {n} corrections (reference {ref_pooled:.4f})")
    assert n >= 3800 and 2.8 <= tot / n <= 3.2


# ---- 7. switch off ----------------------------------------------------------------------------------------------------------------------

def everything(ctx, fleet=False):
    out = list(ctx.get_state()) + list(ctx.get_observations()) + [ctx.get_slot_ekf_stats(0, 2), ctx.get_landmark_ids()]
    return out


def touched(ctx):
    ctx.set_consistent_innovations(True)
    assert ctx.get_consistent_innovations()
    ctx.set_consistent_innovations(False)
    assert not ctx.get_consistent_innovations()


@pytest.mark.parametrize("chain", ["fast", "mid", "general"])
def test_switch_off_slam_is_untouched(library, chain):
    m, L = {"fast": (9, 12), "mid": (30, 33), "general": (40, 45)}[chain]
    case = frame_case(m, L)
    res = []
    for touch in (False, True):
        ctx = context(CHAIN_CAP[chain], L + 1, windows=False)
        if touch:
            touched(ctx)
        stage_case(ctx, case)
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.run_staged(0, 2, with_ekf=2)
        ctx.sync()
        assert ekf_kernels_run(ctx.profile_get()) == CHAIN_KERNELS[chain]
        res.append(everything(ctx))
    for x, y in zip(*res):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "setting and clearing the switch changed a result"


def test_switch_off_fleet_slam_rig_and_localization_are_untouched(library):
    robots = fleet_case(24, 3)
    ids, xyth, frames = loc_frames(12, 312)
    res = []
    for touch in (False, True):
        got = []
        # fleet SLAM
        ctx = context(24, 16, batch=6)
        if touch:
            touched(ctx)
        ctx.fleet_slam_begin([CAM] * 3)
        for r, rob in enumerate(robots):
            ctx.fleet_set_state(r, rob["mu"], rob["S"], rob["ids"])
            ctx.inject_observations(r, *no_obs())
            fr = rob["frames"][0]
            inject(ctx, 3 + r, [(int(rob["ids"][fr[3][k][0]]), fr[3][k][1], fr[3][k][2]) for k in fr[4]])
        ctx.stage_encoders([0.0] * 3 + [r["frames"][0][0] for r in robots], [0.0] * 3 + [r["frames"][0][1] for r in robots],
                           [0.0] * 3 + [r["frames"][0][2] for r in robots])
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.fleet_run_staged(0, [0, 1, 2, 0, 1, 2], with_ekf=2)
        ctx.sync()
        assert ekf_kernels_run(ctx.profile_get()) == CHAIN_KERNELS["fast"]
        for r in range(3):
            got += list(ctx.fleet_get_state(r))
        got.append(ctx.get_slot_ekf_stats(0, 6))
        # rig SLAM
        rig = context(24, 16, batch=4)
        if touch:
            touched(rig)
        rob = robots[0]
        rig.set_camera_rig([CAM, CAM])
        rig.set_state(rob["mu"], rob["S"], rob["ids"])
        fr = rob["frames"][0]
        named = [(int(rob["ids"][i]), z, r) for i, z, r in fr[3]]
        rig.stage_encoders([0.0, 0.0, fr[0], fr[0]], [0.0, 0.0, fr[1], fr[1]], [0.0, 0.0, fr[2], fr[2]])
        rig.inject_observations(0, *no_obs())
        rig.inject_observations(1, *no_obs())
        inject(rig, 2, named[:4])
        inject(rig, 3, named[4:])
        rig.run_staged_rig(0, 2, with_ekf=2)
        rig.sync()
        got += list(rig.get_state()) + [rig.get_rig_observations()[2]]
        # localization and fleet localization, gated
        loc = emu_context(len(frames), max_landmarks=len(ids))
        if touch:
            touched(loc)
        loc.set_innovation_gate()
        loc.localize_begin(ids, xyth, POSE0, SIG0)
        staged(loc, frames)
        loc.profile_enable(True)
        loc.profile_reset()
        loc.run_staged(0, len(frames), with_ekf=2)
        loc.sync()
        assert loc.profile_get()["k_loc_steps"][0] == 1
        got += list(loc.get_state()) + list(loc.get_observations()) + [loc.get_slot_health(0, len(frames)), loc.get_track_health()]
        fl = fleet_context(2, 2 * len(frames), ids, xyth, [POSE0, POSE0 + 0.01], gate=dict(gate_d2=DEFAULTS["gate_d2"]))
        if touch:
            touched(fl)
        fleet_call(fl, [r for _ in frames for r in range(2)], [fr for fr in frames for _ in range(2)])
        got += list(fl.fleet_get_poses()) + [fl.get_slot_health(0, 2 * len(frames)), fl.fleet_get_health()]
        res.append(got)
    for x, y in zip(*res):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "setting and clearing the switch changed a result"


# ---- 8. windows -----------------------------------------------------------------------------------------------------------------------

def test_no_window_is_planned_while_the_switch_is_on(library):
    rng = np.random.RandomState(5)
    L, nf = 10, 3
    mu, S = random_state(rng, L, heading=0.4)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    seen = [1, 3, 4, 6, 8, 9]
    pose, frames = mu[:3], []
    for f in range(2):
        pose = predicted_pose(np.concatenate([pose, mu[3:]]), WL, WR, DT)
        frames.append(observe(rng, mu, seen, post_predict=pose))

    def run(consistent):
        ctx = context(24, L + 2, batch=nf)                       # a default context: windows enabled
        ctx.set_consistent_innovations(consistent)
        ctx.set_state(mu, S, ids)
        ctx.stage_encoders([0.0, WL, WL], [0.0, WR, WR], [0.0, DT, DT])
        ctx.inject_observations(0, *no_obs())
        for f in range(2):
            inject(ctx, 1 + f, [(int(ids[i]), z, r) for i, z, r in frames[f]])
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.run_staged(0, nf, with_ekf=2)
        ctx.sync()
        return ctx, ctx.profile_get(), ctx.plan_stats()

    _, prof, stats = run(False)
    assert stats["windows"] >= 1 and prof["k_ekf_win_step"][0] > 0, "the planner does not window this batch: the case shows nothing"
    ctx, prof, stats = run(True)
    assert not any(k.startswith("k_ekf_win") and v[0] > 0 for k, v in prof.items()), "a window kernel ran under consistent innovations"
    assert ekf_kernels_run(prof) == CHAIN_KERNELS["fast"] and prof["k_ekf_mid"][0] == nf
    assert stats["windows"] == 0 and stats["frames_in_windows"] == 0 and stats["frames_per_frame_chain"] == nf
    mu_r, S_r = mu, S
    for f in range(2):
        mu_r, S_r, _ = consistent_step(mu_r, S_r, WL, WR, DT, frames[f])
    check_state(ctx, dict(mu_ref=mu_r, S_ref=S_r), "two per-frame steps")


# ---- 9. arguments and persistence -------------------------------------------------------------------------------------------------------

def test_arguments_and_persistence(library):
    ctx = emu_context(2, max_landmarks=4)
    assert ctx.get_consistent_innovations() is False, "off by default"
    for bad in (-1, 2, 7):
        assert ctx.lib.aslam_set_consistent_innovations(ctx.h, bad) == E_INVALID
        assert ctx.get_consistent_innovations() is False, "a refused call changes nothing"
    assert ctx.lib.aslam_set_consistent_innovations(None, 1) == E_INVALID
    assert ctx.lib.aslam_get_consistent_innovations(ctx.h, None) == E_INVALID
    assert ctx.lib.aslam_get_consistent_innovations(None, None) == E_INVALID
    ctx.set_consistent_innovations(True)
    assert ctx.get_consistent_innovations() is True
    ids, xyth = random_map(np.random.RandomState(1), 4)
    ctx.localize_begin(ids, xyth, POSE0, SIG0)
    assert ctx.get_consistent_innovations() is True
    ctx.set_consistent_innovations(False)                           # settable while localizing
    ctx.set_consistent_innovations(True)
    ctx.localize_end()
    assert ctx.get_consistent_innovations() is True
    ctx.fleet_begin([CAM] * 2, ids, xyth, [POSE0] * 2, [SIG0] * 2)
    assert ctx.get_consistent_innovations() is True
    ctx.fleet_end()
    ctx.fleet_slam_begin([CAM] * 2)
    assert ctx.get_consistent_innovations() is True
    ctx.fleet_end()
    assert ctx.get_consistent_innovations() is True
    ctx.set_consistent_innovations(False)
    assert ctx.get_consistent_innovations() is False


# ---- 10. rendered frames (GPU only) -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_rendered_ring_slam_equals_the_reference_sequence():
    from tests.test_localize import small_ring
    from tests.test_uncertain_map import raw_obs
    from tests.test_localize import gpu_context, render_frames
    w = synth.RingWorld(small_ring())
    n = 8
    ctx = gpu_context(w, n, persistent_waves=4)
    ctx.set_consistent_innovations(True)
    frs, imgs = render_frames(ctx, w, 0, n)
    ctx.stage_frames(np.stack(imgs))
    ctx.stage_encoders([f.wl for f in frs], [f.wr for f in frs], [f.dt for f in frs])
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.run_staged(0, n, with_ekf=True)
    ctx.sync()
    prof = ctx.profile_get()
    assert not any(k.startswith("k_ekf_win") and v[0] > 0 for k, v in prof.items())
    mu_g, S_g = ctx.get_state()
    ids_g = ctx.get_landmark_ids()
    assert ids_g.size >= 2, "the ring showed no markers"
    # the same raw observations through a second context with the switch on, frame by frame, and through the reference's sequence
    lit = ConsistentLiteral()
    t = 0.0
    for i, f in enumerate(frs):
        t += f.dt
        lit.add_encoder(f.wl, f.wr, t)
        lit.add_frame(raw_obs(ctx, i))
    assert np.array_equal(ids_g, np.array(sorted(lit.id_map, key=lit.id_map.get), np.int32))
    e_S = rel_err(S_g, lit.sigma)
    print(f"rendered ring: |dmu| {np.abs(mu_g - lit.mu).max():.3g}, Sigma {e_S:.3g}, {ids_g.size} landmarks")
    assert np.allclose(mu_g, lit.mu, rtol=1e-9, atol=1e-11) and e_S <= 1e-9

