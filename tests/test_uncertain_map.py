"""Localization on an uncertain map: Schmidt-Kalman steps, single filter and fleet (aslam_localize_begin_uncertain,
aslam_fleet_begin_uncertain, k_loc_steps_umap[_gated], k_fleet_steps_umap[_gated]) against tests/umap_reference.py.

Every device case runs on the session's library (the CPU emulation of the kernel sources without a GPU) and again, marked gpu, on the
gfx950 library.  All inputs are injected observations (with_ekf = 2) except the two rendered runs at the end.

Tolerances (the project's bar, not a measurement): 1e-9 on poses, 1e-9 of max|Sigma| on the strip [Sigma_xx | Sigma_xl], 1e-9 relative
on nis_sum / d2_max; counts, ids, actions and flags exact.  The kernels take 128 lanes, so the map sizes of the replay are 1, 2, the
three sizes around 3 + 3L = 384 = 3 * 128 (L = 126, 127, 128; at L = 128 the 3L landmark columns are a multiple of the block too) and
max_landmarks."""
import math

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from oracle.ekf_literal import norm_angle
from tests.gate_reference import DEFAULTS, TRACK_ZERO, check_slot_health, check_track
from tests.test_innovation_gate import CAM, Truth, fleet_call, gate_scenarios, refused, sight
from tests.test_localize import (E_INVALID, E_STATE, FrozenMapLocalizer, POSE0, SIG0, _Injected, emu_context, inject, make_sequence, random_map,
                                 small_ring)
from tests.umap_reference import UncertainMapLocalizer, sym_blocks

INF = float("inf")
BLOCK = 128                                                 # lanes of the uncertain-map kernels
MAP_DTYPE = np.dtype([("id", "<i4"), ("index", "<i4"), ("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("S", "<f8", (9,))])


@pytest.fixture(params=["session", pytest.param("gfx950", marks=pytest.mark.gpu)])
def library(request):
    if request.param == "gfx950":
        assert capi.lib_path().endswith("libaruco_slam_hip.so"), "the gpu cases must run the native gfx950 library"
    return request.param


def spd_blocks(rng, n, scale=0.05, zero=()):
    """n seeded 3 x 3 SPD blocks of standard deviations around `scale`, the ones in `zero` all zero (what a merge gives for n_seen = 0)"""
    A = rng.normal(0, scale, (n, 3, 3))
    C = A @ A.transpose(0, 2, 1) + 1e-6 * np.eye(3)
    for i in zero:
        C[i] = 0.0
    return C


def staged(ctx, frames, first=0):
    ctx.stage_encoders(*[[f[k] for f in frames] for k in range(3)], slot0=first)
    for s, fr in enumerate(frames):
        inject(ctx, first + s, fr[3])


def strip_of(S):
    return S[:3, :]


def check_single(ctx, ref, where, tol=1e-9):
    """the single filter against the reference: pose, strip, and the fixed parts of the state bit for bit"""
    mu, S = ctx.get_state()
    L = ref.L
    assert mu.shape == (3 + 3 * L,) and S.shape == (3 + 3 * L, 3 + 3 * L)
    want = ref.full_sigma()
    e_mu = np.abs(mu[:3] - ref.mu).max()
    e_X = np.abs(strip_of(S) - strip_of(want)).max() / np.abs(want).max()
    assert e_mu <= tol and e_X <= tol, f"{where}: pose differs by {e_mu}, the strip by {e_X} of max|Sigma|"
    # the full matrix is symmetric: the strip is mirrored bit for bit (Sigma_xx is as symmetric as the chain's rounding leaves it)
    assert np.array_equal(S[:3, 3:], S[3:, :3].T) and np.array_equal(S[3:, 3:], S[3:, 3:].T), f"{where}: Sigma is not symmetric"
    assert np.abs(S[:3, :3] - S[:3, :3].T).max() <= tol * np.abs(want).max(), f"{where}: Sigma_xx is not symmetric"
    assert np.array_equal(mu[3:], ref.xyth.reshape(-1)), f"{where}: the map moved"
    ll = S[3:, 3:].copy()
    for i in range(L):
        assert np.array_equal(ll[3 * i:3 * i + 3, 3 * i:3 * i + 3], ref.C[i]), f"{where}: C_{i} changed"
        ll[3 * i:3 * i + 3, 3 * i:3 * i + 3] = 0.0
    assert not ll.any(), f"{where}: landmarks became correlated"
    return e_mu, e_X


def check_robot(fleet, r, ref, where, poses=None, tol=1e-9):
    poses, sigs = poses if poses is not None else fleet.fleet_get_poses()
    X = np.concatenate([sigs[r], fleet.fleet_get_cross(r)], 1)
    want = ref.full_sigma()
    e_mu = np.abs(poses[r] - ref.mu).max()
    e_X = np.abs(X - strip_of(want)).max() / np.abs(want).max()
    assert e_mu <= tol and e_X <= tol, f"{where}: pose differs by {e_mu}, the strip by {e_X} of max|Sigma|"


def pops(ctx):
    gi, gx, ga, _, _ = ctx.get_observations()
    return np.stack([gi, gx, ga], 1).reshape(-1, 3)


# ---- 1. the reference itself (CPU only) ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2])
def test_reference_with_zero_covariances_is_the_frozen_map_filter(seed):
    rng = np.random.RandomState(seed)
    n = 12
    ids, xyth = random_map(rng, n)
    frames = make_sequence(seed, 30, ids, xyth)
    ref = UncertainMapLocalizer(ids, xyth, np.zeros((n, 9)), POSE0, SIG0)
    frozen = FrozenMapLocalizer(ids, xyth, POSE0, SIG0)
    for f, fr in enumerate(frames):
        for m in (ref, frozen):
            m.add_encoder(*fr[:3])
            m.add_observations(fr[3])
        assert ref.log == frozen.log and ref.stats == frozen.stats, f"frame {f}"
        assert np.abs(ref.mu - frozen.mu).max() <= 1e-12 and np.abs(ref.P - frozen.P).max() <= 1e-12, f"frame {f}"
        assert not ref.cross.any()


def test_reference_keeps_the_pose_covariance_from_collapsing():
    """one landmark sighted in 30 consecutive frames: Sigma_xx ends strictly above the frozen-map filter's, and above a filter that only
    inflates R by Hl C Hl^T and carries no cross term (so the cross term is live)"""
    rng = np.random.RandomState(4)
    ids, xyth = np.array([17], np.int32), np.array([[1.5, 0.4, -2.0]])
    C = spd_blocks(rng, 1, 0.03)
    truth = Truth(ids, xyth, POSE0)
    umap = UncertainMapLocalizer(ids, xyth, C, POSE0, SIG0)
    no_cross = UncertainMapLocalizer(ids, xyth, C, POSE0, SIG0, cross=False)
    frozen = FrozenMapLocalizer(ids, xyth, POSE0, SIG0)
    for f in range(30):
        wl, wr, dt = rng.uniform(1, 4), rng.uniform(1, 4), 0.05
        obs = sight(truth.step(wl, wr, dt), ids, xyth, [0], rng)
        for m in (umap, no_cross, frozen):
            m.add_encoder(wl, wr, dt)
            m.add_observations(obs)
            assert m.stats[2] == 1, f"frame {f}: the sighting must be fused"
    lo = lambda P: np.linalg.eigvalsh(0.5 * (P + P.T))[0]
    assert np.abs(umap.cross).max() > 0
    assert lo(umap.P - frozen.P) > 0, (lo(umap.P), lo(frozen.P))
    assert lo(umap.P - no_cross.P) > 0, (lo(umap.P), lo(no_cross.P))
    assert lo(umap.P) > lo(no_cross.P) > lo(frozen.P) > 0
    # the smallest eigenvalue of Sigma_xx cannot fall below what the landmark's own uncertainty leaves: it stops shrinking
    print("Sigma_xx smallest eigenvalue after 30 sightings: frozen", lo(frozen.P), "R inflated", lo(no_cross.P), "uncertain map", lo(umap.P))


# ---- 2. replay against the reference, single context --------------------------------------------------------------------------------

COUNTS = (0, 1, 63, 64, 65, 128)


def replay_frames(seed, ids, xyth):
    """make_sequence's frames (unknown ids, one id twice, stationary repeats, gated observations), then one frame per observation count
    in COUNTS: true sightings of as many distinct landmarks as the map has, one of them sighted twice, the rest unknown ids; then a
    frame that repeats three observations of the one before (stationary no-ops beside corrections)"""
    rng = np.random.RandomState(seed)
    n = len(ids)
    frames = make_sequence(seed, 6, ids, xyth)
    truth = Truth(ids, xyth, POSE0)
    for k in COUNTS:
        wl, wr, dt = rng.uniform(1, 4), rng.uniform(1, 4), 0.05
        pose = truth.step(wl, wr, dt)
        sel = rng.permutation(n)[:min(n, max(k - 1, 1))].tolist() if k else []
        if k >= 2:
            sel.append(sel[0])                              # one id twice: the heap replay
        obs = sight(pose, ids, xyth, sel, rng)
        obs += [(600 + j, 1, rng.normal(0, 1, 3), np.full(3, 0.02)) for j in range(k - len(obs))]
        order = rng.permutation(len(obs))
        frames.append((wl, wr, dt, [obs[i] for i in order]))
    wl, wr, dt = 2.0, 2.5, 0.05
    pose = truth.step(wl, wr, dt)
    known = [o for o in frames[-1][3] if o[0] < 600]
    again = known[:3] + sight(pose, ids, xyth, list(range(min(n, 2))), rng)
    frames.append((wl, wr, dt, again))
    return frames


@pytest.mark.parametrize("L", [1, 2, 126, 127, 128, "max"])
def test_replay_against_reference(library, L):
    max_landmarks = 150
    L = max_landmarks if L == "max" else L
    assert (3 + 3 * 126) < 3 * BLOCK == 3 + 3 * 127 < 3 + 3 * 128 and (3 * 128) % BLOCK == 0
    rng = np.random.RandomState(100 + L)
    ids, xyth = random_map(rng, L)
    C = spd_blocks(rng, L, 0.05, zero=(0, 2) if L > 3 else (0,) if L == 2 else ())
    frames = replay_frames(20 + L, ids, xyth)
    ctx = emu_context(len(frames), max_landmarks=max_landmarks)
    ctx.localize_begin_uncertain(ids, xyth, C, POSE0, SIG0)
    assert ctx.is_localizing() and ctx.is_map_uncertain()
    ref = UncertainMapLocalizer(ids, xyth, C, POSE0, SIG0)
    check_single(ctx, ref, "begin")
    staged(ctx, frames)
    seen = dict(stationary=0, dup=0, unknown=0, corrections=0)
    worst = [0.0, 0.0]
    calls = [(0, 1), (1, 3), (4, 2)] + [(f, 1) for f in range(6, 6 + len(COUNTS))] + [(6 + len(COUNTS), len(frames) - 6 - len(COUNTS))]
    for f0, nb in calls:                                    # several slots in one call, several calls: the strip persists between launches
        want = []
        for f in range(f0, f0 + nb):
            ref.add_encoder(*frames[f][:3])
            ref.add_observations(frames[f][3])
            want.append(list(ref.stats))
            seen["stationary"] += ref.stats[3]
            seen["corrections"] += ref.stats[2]
            seen["unknown"] += sum(o[0] >= 500 for o in frames[f][3])
            ks = [o[0] for o in frames[f][3] if o[1] and o[0] < 500]
            seen["dup"] += len(ks) != len(set(ks))
        ctx.run_staged(f0, nb, with_ekf=2)
        e = check_single(ctx, ref, f"frames from {f0}")
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert np.array_equal(pops(ctx), ref.log_array()), f"frames from {f0}: pops / actions differ"
        assert ctx.get_slot_ekf_stats(f0, nb).tolist() == want, f"frames from {f0}: stats differ"
    assert all(v > 0 for v in seen.values()), seen
    if L > 2:
        assert np.abs(ref.cross).max() > 0
    # single steps: aslam_add_encoder predicts the whole strip, an image without markers is a step without corrections, then one
    # injected step whose own encoder sample does not move
    wl, wr, dt = 3.0, 1.5, 0.05
    ctx.set_camera(CAM[0], CAM[1])
    ctx.add_encoder(wl, wr, dt)                              # (the context's clock still stands at 0: staged calls do not move it)
    ctx.add_image(np.full((64, 64), 128, np.uint8))
    ref.predict(wl, wr, dt)
    ref.add_observations([])
    check_single(ctx, ref, "aslam_add_encoder + aslam_add_image")
    obs = sight(ref.mu, ids, xyth, list(range(min(L, 3))), rng)
    staged(ctx, [(0.0, 0.0, dt, obs)])
    ctx.run_staged(0, 1, with_ekf=2)
    ref.add_encoder(0.0, 0.0, dt)
    ref.add_observations(obs)
    check_single(ctx, ref, "single injected step")
    assert np.array_equal(pops(ctx), ref.log_array())
    print(f"L = {L}: {seen['corrections']} corrections, worst pose error {worst[0]:.2e}, worst strip error {worst[1]:.2e} of max|Sigma|")


# ---- 3. zero covariances ---------------------------------------------------------------------------------------------------------------

def test_zero_covariances_follow_the_fixed_map_filter(library):
    rng = np.random.RandomState(8)
    n = 40
    ids, xyth = random_map(rng, n)
    frames = make_sequence(9, 20, ids, xyth)
    a, b = emu_context(len(frames), max_landmarks=n), emu_context(len(frames), max_landmarks=n)
    a.localize_begin(ids, xyth, POSE0, SIG0)
    b.localize_begin_uncertain(ids, xyth, np.zeros((n, 3, 3)), POSE0, SIG0)
    for f0, nb in ((0, 1), (1, 7), (8, 12)):
        for ctx in (a, b):
            if f0 == 0:
                staged(ctx, frames)
            ctx.run_staged(f0, nb, with_ekf=2)
        (ma, Sa), (mb, Sb) = a.get_state(), b.get_state()
        assert np.abs(ma[:3] - mb[:3]).max() <= 1e-9 and np.abs(Sa[:3, :3] - Sb[:3, :3]).max() <= 1e-9 * np.abs(Sa).max(), f"frames from {f0}"
        assert not Sb[:3, 3:].any() and not Sb[3:, :].any(), "the cross strip of an exact map must stay exactly 0.0"
        assert np.array_equal(pops(a), pops(b)) and np.array_equal(a.get_slot_ekf_stats(f0, nb), b.get_slot_ekf_stats(f0, nb))
    # ... and so does a fleet's
    fleet = emu_context(4, max_landmarks=n)
    fleet.fleet_begin_uncertain([CAM] * 2, ids, xyth, np.zeros((n, 9)), [POSE0] * 2, [SIG0] * 2)
    fleet_call(fleet, [0, 1, 0, 1], [frames[0], frames[0], frames[1], frames[1]])
    for r in range(2):
        assert not fleet.fleet_get_cross(r).any()


# ---- 4. fleet ---------------------------------------------------------------------------------------------------------------------------

def single_twin(ids, xyth, C, pose, frames, gate=None, max_landmarks=None):
    """a single uncertain-map context run on one robot's frames, all in one call"""
    one = emu_context(max(len(frames), 1), max_landmarks=max_landmarks or len(ids))
    if gate is not None:
        one.set_innovation_gate(**gate)
    one.localize_begin_uncertain(ids, xyth, C, pose, SIG0)
    if frames:
        staged(one, frames)
        one.run_staged(0, len(frames), with_ekf=2)
    return one


def test_fleet_of_16_permuted_equals_single_contexts_and_reference(library):
    rng = np.random.RandomState(21)
    n, R, T = 40, 16, 6
    ids, xyth = random_map(rng, n, id_pool=600)
    C = spd_blocks(rng, n, 0.04, zero=(3,))
    seqs = [make_sequence(70 + r, T, ids, xyth) for r in range(R)]
    poses0 = POSE0 + rng.uniform(-0.03, 0.03, (R, 3))
    fleet = emu_context(R * 2, max_landmarks=n)
    fleet.fleet_begin_uncertain([CAM] * R, ids, xyth, C, poses0, [SIG0] * R)
    assert fleet.is_map_uncertain() and fleet.is_fleet() == R
    refs = [UncertainMapLocalizer(ids, xyth, C, poses0[r], SIG0) for r in range(R)]
    done = [0] * R

    def call(order):
        frames = []
        for r in order:
            fr = seqs[r][done[r]]
            done[r] += 1
            refs[r].add_encoder(*fr[:3])
            refs[r].add_observations(fr[3])
            frames.append(fr)
        fleet_call(fleet, order, frames)

    perm = [int(r) for r in rng.permutation(R)]
    call(perm + perm[::-1])                                 # every robot twice in one staged call, in a permuted order
    idle = [r for r in range(R) if r % 3 == 0]
    before = {r: fleet.fleet_get_cross(r).tobytes() for r in idle}
    busy = [r for r in perm if r % 3]
    call(busy + busy[:5] + busy)                            # a subset, some of them three times
    for r in idle:
        assert fleet.fleet_get_cross(r).tobytes() == before[r], f"robot {r} was not in the call"
    call(perm)
    poses = fleet.fleet_get_poses()
    for r in range(R):
        one = single_twin(ids, xyth, C, poses0[r], seqs[r][:done[r]])
        mu, S = one.get_state()
        assert np.array_equal(poses[0][r], mu[:3]) and np.array_equal(poses[1][r], S[:3, :3]), f"robot {r}: pose / Sigma_xx bits"
        assert np.array_equal(fleet.fleet_get_cross(r), S[:3, 3:]), f"robot {r}: cross strip bits"
        check_robot(fleet, r, refs[r], f"robot {r}", poses)
        assert np.abs(refs[r].cross).max() > 0


def test_256_robots_on_12_landmarks(library):
    rng = np.random.RandomState(33)
    n, R = 12, 256
    ids, xyth = random_map(rng, n, id_pool=600)
    C = spd_blocks(rng, n, 0.04)
    poses0 = POSE0 + rng.uniform(-0.05, 0.05, (R, 3))
    lists = [sight(poses0[r], ids, xyth, rng.permutation(n)[:1 + r % n].tolist(), rng) for r in range(R)]
    perm = [int(r) for r in rng.permutation(R)]
    fleet = emu_context(R, max_landmarks=n)
    fleet.fleet_begin_uncertain([CAM] * R, ids, xyth, C, poses0, [SIG0] * R)
    fleet_call(fleet, perm, [(0.0, 0.0, 0.05, lists[r]) for r in perm])
    poses, sigs = fleet.fleet_get_poses()
    stats = fleet.get_slot_ekf_stats(0, R)
    one = emu_context(1, max_landmarks=n)
    one.stage_encoders([0.0], [0.0], [0.05])
    for s, r in enumerate(perm):
        one.localize_begin_uncertain(ids, xyth, C, poses0[r], SIG0)
        inject(one, 0, lists[r])
        one.run_staged(0, 1, with_ekf=2)
        mu, S = one.get_state()
        assert np.array_equal(poses[r], mu[:3]) and np.array_equal(sigs[r], S[:3, :3]), f"robot {r}"
        assert np.array_equal(fleet.fleet_get_cross(r), S[:3, 3:]), f"robot {r}"
        assert np.array_equal(stats[s], one.get_slot_ekf_stats(0, 1)[0]) and stats[s][2] == 1 + r % n
    for r in (0, 100, 255):
        ref = UncertainMapLocalizer(ids, xyth, C, poses0[r], SIG0)
        ref.add_encoder(0.0, 0.0, 0.05)
        ref.add_observations(lists[r])
        check_robot(fleet, r, ref, f"robot {r}", (poses, sigs))


def test_fleet_at_the_id_table_limit(library):
    """L = 1024, every id of the table: the strip takes 73.7 KB of dynamic LDS, above the 64 KB a kernel may use unasked"""
    rng = np.random.RandomState(44)
    n, R = 1024, 2
    ids = rng.permutation(n).astype(np.int32)
    xyth = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-math.pi, math.pi, n)], 1)
    C = spd_blocks(rng, n, 0.04)
    poses0 = np.array([POSE0, POSE0 + 0.05])
    fleet = emu_context(6, max_landmarks=n)
    fleet.set_innovation_gate()
    fleet.fleet_begin_uncertain([CAM] * R, ids, xyth, C, poses0, [SIG0] * R)
    refs = [UncertainMapLocalizer(ids, xyth, C, poses0[r], SIG0, dict(DEFAULTS)) for r in range(R)]
    truth = [Truth(ids, xyth, poses0[r]) for r in range(R)]
    order, frames = [], []
    for t in range(3):
        for r in range(R):
            wl, wr = rng.uniform(1, 4), rng.uniform(1, 4)
            sel = [0, 1023] + rng.permutation(n)[:10].tolist()           # the first and the last block of the strip among them
            fr = (wl, wr, 0.05, sight(truth[r].step(wl, wr, 0.05), ids, xyth, sel, rng, moved=(3,)))
            refs[r].add_encoder(*fr[:3])
            refs[r].add_observations(fr[3])
            refs[r].assert_margins()
            order.append(r)
            frames.append(fr)
    fleet_call(fleet, order, frames)
    track = fleet.fleet_get_health()
    for r in range(R):
        check_robot(fleet, r, refs[r], f"robot {r}")
        check_track(track[r], refs[r].track, f"robot {r}")
        assert refs[r].track["rejected_total"] >= 1 and np.abs(refs[r].cross[:, -3:]).max() > 0


# ---- 5. gate ----------------------------------------------------------------------------------------------------------------------------

def test_monitor_only_gate_is_bit_equal_to_the_ungated_kernels(library):
    ids, xyth, scen = gate_scenarios()
    C = spd_blocks(np.random.RandomState(2), len(ids), 0.04, zero=(9,))
    frames = scen["edges"][:8] + scen["counts"]              # (the NaN observation of edges[8] would make every later comparison vacuous)
    a, b = (emu_context(len(frames), max_landmarks=len(ids)) for _ in range(2))
    b.set_innovation_gate(gate_d2=INF)
    for ctx in (a, b):
        ctx.localize_begin_uncertain(ids, xyth, C, POSE0, SIG0)
        staged(ctx, frames)
    for f0, nb in ((0, 1), (1, 6), (7, len(frames) - 7)):
        for ctx in (a, b):
            ctx.run_staged(f0, nb, with_ekf=2)
        for x, y in zip(a.get_state() + a.get_observations(), b.get_state() + b.get_observations()):
            assert np.array_equal(x, y, equal_nan=True), f"frames from {f0}: the monitor changed the filter"
        assert np.array_equal(a.get_slot_ekf_stats(f0, nb), b.get_slot_ekf_stats(f0, nb))
    R = 3
    fa, fb = (emu_context(len(frames), max_landmarks=len(ids)) for _ in range(2))
    fb.set_innovation_gate(gate_d2=INF)
    order = [s % R for s in range(len(frames))]
    for f in (fa, fb):
        f.fleet_begin_uncertain([CAM] * R, ids, xyth, C, [POSE0] * R, [SIG0] * R)
        fleet_call(f, order, frames)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(fa.fleet_get_poses(), fb.fleet_get_poses()))
    for r in range(R):
        assert np.array_equal(fa.fleet_get_cross(r), fb.fleet_get_cross(r), equal_nan=True)


@pytest.mark.parametrize("gate_d2", [DEFAULTS["gate_d2"], INF])
def test_gate_against_reference(library, gate_d2):
    ids, xyth, scen = gate_scenarios()
    C = spd_blocks(np.random.RandomState(2), len(ids), 0.04, zero=(9,))
    gate = dict(gate_d2=gate_d2)
    scen = dict(scen, edges=scen["edges"][:8])
    want, refs = {}, {}
    for name, frames in scen.items():
        ref = UncertainMapLocalizer(ids, xyth, C, POSE0, SIG0, gate)
        ctx = emu_context(len(frames), max_landmarks=len(ids))
        ctx.set_innovation_gate(**gate)
        ctx.localize_begin_uncertain(ids, xyth, C, POSE0, SIG0)
        staged(ctx, frames)
        want[name] = []
        for s, fr in enumerate(frames):
            ref.add_encoder(*fr[:3])
            ref.add_observations(fr[3])
            ref.assert_margins()                            # §19's margin, before any discrete comparison
            ctx.run_staged(s, 1, with_ekf=2)
            where = f"{name} frame {s}"
            check_single(ctx, ref, where)
            assert np.array_equal(pops(ctx), ref.log_array()), f"{where}: pops / actions differ"
            assert ctx.get_slot_ekf_stats(s, 1)[0].tolist() == ref.stats, where
            check_slot_health(ctx.get_slot_health(s, 1)[0], ref.health, where)
            check_track(ctx.get_track_health(), ref.track, where)
            want[name].append((dict(ref.health), list(ref.stats)))
        refs[name] = ref
    acts = sum(ref.track["rejected_total"] for ref in refs.values())
    assert (acts > 10) if math.isfinite(gate_d2) else (acts == 0)
    # the same as a fleet, every scenario one robot, all slots in one call
    names = list(scen)
    order = [r for r, k in enumerate(names) for _ in scen[k]]
    frames = [fr for k in names for fr in scen[k]]
    fleet = emu_context(len(frames), max_landmarks=len(ids))
    fleet.set_innovation_gate(**gate)
    fleet.fleet_begin_uncertain([CAM] * len(names), ids, xyth, C, [POSE0] * len(names), [SIG0] * len(names))
    fleet_call(fleet, order, frames)
    health, stats, track = fleet.get_slot_health(0, len(frames)), fleet.get_slot_ekf_stats(0, len(frames)), fleet.fleet_get_health()
    s = 0
    for r, k in enumerate(names):
        for f, (h, st) in enumerate(want[k]):
            check_slot_health(health[s], h, f"fleet {k} frame {f}")
            assert stats[s].tolist() == st
            s += 1
        check_robot(fleet, r, refs[k], f"fleet {k}")
        check_track(track[r], refs[k].track, f"fleet {k}")


def test_a_poorly_known_landmark_is_gated_against_its_own_covariance(library):
    """a sighting 1.4 m off a landmark whose C_i says half a metre: the fixed-map filter rejects it, the uncertain-map filter fuses it;
    no observation goes the other way; and a frame of rejections only leaves the strip's bits"""
    rng = np.random.RandomState(6)
    n = 8
    ids, xyth = random_map(rng, n)
    C = spd_blocks(rng, n, 0.01)
    C[5] = np.diag([0.25, 0.25, 0.04])
    obs = sight(POSE0, ids, xyth, [1, 3, 5, 6], rng)
    obs[2] = (obs[2][0], 1, obs[2][2] + np.array([1.2, -0.8, 0.1]), obs[2][3])
    frame = (0.0, 0.0, 0.05, obs)
    fixed, umap = emu_context(2, max_landmarks=n), emu_context(2, max_landmarks=n)
    for ctx in (fixed, umap):
        ctx.set_innovation_gate()
    sig = np.diag([1e-3, 1e-3, 1e-4])
    fixed.localize_begin(ids, xyth, POSE0, sig)
    umap.localize_begin_uncertain(ids, xyth, C, POSE0, sig)
    ref = UncertainMapLocalizer(ids, xyth, C, POSE0, sig, dict(DEFAULTS))
    ref.add_encoder(*frame[:3])
    ref.add_observations(obs)
    ref.assert_margins()
    for ctx in (fixed, umap):
        staged(ctx, [frame])
        ctx.run_staged(0, 1, with_ekf=2)
    pf, pu = pops(fixed), pops(umap)
    assert np.array_equal(pu, ref.log_array()) and np.array_equal(pf[:, :2], pu[:, :2])
    assert pf[:, 2].tolist() == [1, 1, 3, 1] and pu[:, 2].tolist() == [1, 1, 1, 1], (pf, pu)
    assert not ((pf[:, 2] == 1) & (pu[:, 2] == 3)).any()
    check_single(umap, ref, "the accepted sighting")
    # every sighting displaced: all rejected, pose and strip keep their bits (the frame's own encoder sample does not move)
    before = umap.get_state()
    assert np.abs(before[1][:3, 3:]).max() > 0
    far = [(o[0], 1, o[2] + np.array([3.0, -2.0, 1.0]), o[3]) for o in sight(POSE0, ids, xyth, [0, 2, 4], rng)]
    staged(umap, [(0.0, 0.0, 0.05, far)], first=1)
    umap.run_staged(1, 1, with_ekf=2)
    h = umap.get_slot_health(1, 1)[0]
    assert (int(h["attempted"]), int(h["rejected"])) == (3, 3)
    for x, y in zip(before, umap.get_state()):
        assert np.array_equal(x, y), "a rejected correction moved the state"


# ---- 6. reseat --------------------------------------------------------------------------------------------------------------------------

def test_every_seat_zeroes_the_cross_strip_and_nothing_else(library):
    rng = np.random.RandomState(14)
    n, R = 20, 3
    ids, xyth = random_map(rng, n, id_pool=600)
    C = spd_blocks(rng, n, 0.03)
    truth = [Truth(ids, xyth, POSE0) for _ in range(R)]
    frames = []
    for t in range(3):
        for r in range(R):
            wl, wr = rng.uniform(1, 4), rng.uniform(1, 4)
            frames.append((wl, wr, 0.05, sight(truth[r].step(wl, wr, 0.05), ids, xyth, rng.permutation(n)[:4].tolist(), rng)))
    order = [r for _ in range(3) for r in range(R)]
    fleet = emu_context(len(frames), max_landmarks=n)
    fleet.fleet_begin_uncertain([CAM] * R, ids, xyth, C, [POSE0] * R, [SIG0] * R)
    fleet_call(fleet, order, frames)
    snap = lambda: (fleet.fleet_get_poses(), [fleet.fleet_get_cross(r) for r in range(R)])
    (p0, s0), x0 = snap()
    assert all(np.abs(x).max() > 0 for x in x0)
    seat = (np.array([0.3, 0.1, -0.4]), np.diag([0.01, 0.02, 0.005]))
    fleet.fleet_set_pose(1, *seat)
    (p1, s1), x1 = snap()
    assert not x1[1].any() and np.array_equal(p1[1], seat[0]) and np.array_equal(s1[1], seat[1])
    for r in (0, 2):
        assert np.array_equal(x1[r], x0[r]) and np.array_equal(p1[r], p0[r]) and np.array_equal(s1[r], s0[r]), f"robot {r}"
    inject(fleet, 0, [])
    assert fleet.fleet_relocalize(0, [2])[0]["status"] == 1                      # unsolved: as it was
    inject(fleet, 0, frames[-1][3])
    assert fleet.fleet_relocalize(0, [2], apply=False, tol_xy=1.0, tol_th=0.6)[0]["status"] == 0   # solved, not applied: as it was
    (p2, s2), x2 = snap()
    assert all(np.array_equal(a, b) for a, b in zip(x1 + [p1, s1], x2 + [p2, s2]))
    res = fleet.fleet_relocalize(0, [2], tol_xy=1.0, tol_th=0.6)[0]
    assert res["status"] == 0
    (p3, s3), x3 = snap()
    assert not x3[2].any() and np.array_equal(p3[2], res["pose"]) and np.array_equal(s3[2].reshape(-1), res["sigma"].reshape(-1))
    assert np.array_equal(x3[0], x0[0]) and not x3[1].any() and np.array_equal(p3[:2], p1[:2])
    # the reseated robots go on against the reference from their seats
    refs = {1: UncertainMapLocalizer(ids, xyth, C, *seat), 2: UncertainMapLocalizer(ids, xyth, C, res["pose"], np.asarray(res["sigma"]).reshape(3, 3))}
    more = [(0.0, 0.0, 0.05, sight(p3[r], ids, xyth, [1, 5, 9], rng)) for r in (1, 2) for _ in range(2)]
    for r, fr in zip((1, 1, 2, 2), more):
        refs[r].add_encoder(*fr[:3])
        refs[r].add_observations(fr[3])
    fleet_call(fleet, [1, 1, 2, 2], more)
    for r in (1, 2):
        check_robot(fleet, r, refs[r], f"reseated robot {r}")
        assert fleet.fleet_get_cross(r).any()

    # the single filter: aslam_relocalize
    one = emu_context(4, max_landmarks=n)
    one.localize_begin_uncertain(ids, xyth, C, POSE0, SIG0)
    mine = [frames[i] for i in (0, 3, 6)]
    staged(one, mine)
    one.run_staged(0, 3, with_ekf=2)
    mu0, S0 = one.get_state()
    assert np.abs(S0[:3, 3:]).max() > 0
    inject(one, 3, [])
    assert one.relocalize(3)["status"] == 1
    inject(one, 3, mine[-1][3])
    assert one.relocalize(3, apply=False, tol_xy=1.0, tol_th=0.6)["status"] == 0
    assert all(np.array_equal(a, b) for a, b in zip((mu0, S0), one.get_state()))
    res = one.relocalize(3, tol_xy=1.0, tol_th=0.6)
    assert res["status"] == 0
    mu1, S1 = one.get_state()
    assert not S1[:3, 3:].any() and not S1[3:, :3].any()
    assert np.array_equal(S1[3:, 3:], S0[3:, 3:]) and np.array_equal(mu1[3:], mu0[3:])
    assert np.array_equal(mu1[:3], res["pose"]) and np.array_equal(S1[:3, :3].reshape(-1), np.asarray(res["sigma"]).reshape(-1))
    assert one.is_map_uncertain()


# ---- 7. modes and arguments -------------------------------------------------------------------------------------------------------------

def test_arguments_and_modes(library, tmp_path):
    ids = np.array([3, 7, 9], np.int32)
    xyth = np.array([[1.0, 0.0, 3.1], [0.0, 1.0, -1.5], [-1.0, -1.0, 0.7]])
    C = spd_blocks(np.random.RandomState(1), 3, 0.05, zero=(1,))        # an all-zero block is legal
    ctx = emu_context(4, max_landmarks=6)
    assert not ctx.is_map_uncertain()
    state0 = ctx.get_state()

    def bad_blocks():
        for v in (np.nan, np.inf):
            c = C.copy(); c[2, 0, 1] = v
            yield c, "9"
        c = C.copy(); c[0, 1, 1] = -1e-9
        yield c, "3"
        c = C.copy(); c[2] = np.array([[1.0, 1.1, 0.0], [1.1, 1.0, 0.0], [0.0, 0.0, 1.0]])
        yield c, "9"
        c = C.copy(); c[0] = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.1], [0.0, 0.1, 1.0]])      # a covariance beside a zero variance
        yield c, "3"

    for begin in ("single", "fleet"):
        for c, who in bad_blocks():
            with pytest.raises(capi.AslamError) as e:
                if begin == "single":
                    ctx.localize_begin_uncertain(ids, xyth, c, POSE0, SIG0)
                else:
                    ctx.fleet_begin_uncertain([CAM] * 2, ids, xyth, c, [POSE0] * 2, [SIG0] * 2)
            assert e.value.code == E_INVALID and f"landmark {who}" in str(e.value), e.value
            assert not ctx.is_localizing() and ctx.is_fleet() == 0 and not ctx.is_map_uncertain()
            assert all(np.array_equal(a, b) for a, b in zip(state0, ctx.get_state())), "a refused begin touched the state"
    # the checks of aslam_localize_begin / aslam_fleet_begin
    refused(E_INVALID, ctx.localize_begin_uncertain, np.array([3, 3, 9], np.int32), xyth, C, POSE0, SIG0)
    refused(E_INVALID, ctx.localize_begin_uncertain, ids, xyth, C, np.array([0.0, np.nan, 0.0]), SIG0)
    refused(E_INVALID, ctx.localize_begin_uncertain, ids, xyth, C, POSE0, np.array([[1.0, 0.5, 0], [0.0, 1.0, 0], [0, 0, 1.0]]))
    refused(E_INVALID, ctx.localize_begin_uncertain, np.arange(7, dtype=np.int32), np.zeros((7, 3)), np.zeros((7, 9)), POSE0, SIG0)
    refused(E_INVALID, ctx.fleet_begin_uncertain, [CAM] * 5, ids, xyth, C, [POSE0] * 5, [SIG0] * 5)       # more robots than max_batch
    assert ctx.lib.aslam_localize_begin_uncertain(ctx.h, 3, None, None, None, None, None) == E_INVALID
    assert ctx.lib.aslam_is_map_uncertain(ctx.h, None) == E_INVALID and ctx.lib.aslam_fleet_get_cross(ctx.h, 0, None, None) == E_INVALID
    # the new getter in each wrong mode
    refused(E_STATE, ctx.fleet_get_cross, 0)                                    # SLAM
    ctx.localize_begin(ids, xyth, POSE0, SIG0)
    assert not ctx.is_map_uncertain()
    refused(E_STATE, ctx.fleet_get_cross, 0)                                    # localizing on an exact map
    refused(E_STATE, ctx.fleet_begin_uncertain, [CAM] * 2, ids, xyth, C, [POSE0] * 2, [SIG0] * 2)
    ctx.localize_end()
    ctx.fleet_begin([CAM] * 2, ids, xyth, [POSE0] * 2, [SIG0] * 2)
    assert not ctx.is_map_uncertain()
    refused(E_STATE, ctx.fleet_get_cross, 0)                                    # a fleet on an exact map
    refused(E_STATE, ctx.localize_begin_uncertain, ids, xyth, C, POSE0, SIG0)
    ctx.fleet_slam_begin([CAM] * 2)
    refused(E_STATE, ctx.fleet_get_cross, 0)                                    # fleet SLAM
    ctx.fleet_begin_uncertain([CAM] * 2, ids, xyth, C, [POSE0] * 2, [SIG0] * 2)          # a begin while a fleet is active starts a new one
    assert ctx.is_map_uncertain() and ctx.is_fleet() == 2
    assert ctx.fleet_get_cross(1).shape == (3, 9) and not ctx.fleet_get_cross(1).any()
    refused(E_INVALID, ctx.fleet_get_cross, 2)
    refused(E_INVALID, ctx.fleet_get_cross, -1)
    ctx.fleet_begin([CAM] * 2, ids, xyth, [POSE0] * 2, [SIG0] * 2)              # ... and an exact one ends the uncertain one
    assert not ctx.is_map_uncertain()
    ctx.fleet_begin_uncertain([CAM] * 2, ids, xyth, C, [POSE0] * 2, [SIG0] * 2)
    ctx.fleet_end()
    assert not ctx.is_map_uncertain()
    refused(E_STATE, ctx.fleet_get_cross, 0)

    # the single filter: state layout, export, save; C = (S + S^T) / 2
    skew = C.copy()
    skew[0, 0, 1] += 2e-4
    skew[0, 1, 0] -= 2e-4
    assert np.array_equal(sym_blocks(skew)[1:], C[1:]) and not np.array_equal(skew[0], skew[0].T)
    ctx.localize_begin_uncertain(ids, xyth, skew, POSE0, SIG0)
    Cs = sym_blocks(skew)
    ref = UncertainMapLocalizer(ids, xyth, skew, POSE0, SIG0)
    assert np.array_equal(ref.C, Cs)
    check_single(ctx, ref, "begin")
    mu, S = ctx.get_state()
    want = np.zeros((12, 12))
    want[:3, :3] = SIG0
    for i in range(3):
        want[3 + 3 * i:6 + 3 * i, 3 + 3 * i:6 + 3 * i] = Cs[i]
    assert np.array_equal(S, want) and np.array_equal(mu, np.concatenate([POSE0, xyth.reshape(-1)]))
    rec = np.frombuffer(ctx.export_map(), MAP_DTYPE)[:3]
    assert rec["id"].tolist() == ids.tolist() and np.array_equal(rec["S"].reshape(3, 3, 3), Cs)
    refused(E_STATE, ctx.set_state, mu, S, ids)
    ctx.save_state(str(tmp_path / "state.bin"))
    frames = [(2.0, 3.0, 0.05, [(7, 1, np.array([0.5, 1.0, -1.9]), np.full(3, 0.02))]),
              (2.5, 2.0, 0.05, [(3, 1, np.array([1.1, -0.2, 2.7]), np.full(3, 0.03)), (42, 1, np.array([1.0, 0.0, 0.0]), np.full(3, 0.02))])]
    staged(ctx, frames)
    ctx.run_staged(0, 2, with_ekf=2)
    for fr in frames:
        ref.add_encoder(*fr[:3])
        ref.add_observations(fr[3])
    check_single(ctx, ref, "two frames")
    # leaving: a valid SLAM state, later steps are SLAM steps that append a new id and move the landmarks again
    mu, S = ctx.get_state()
    ctx.localize_end()
    assert not ctx.is_localizing() and not ctx.is_map_uncertain()
    assert all(np.array_equal(a, b) for a, b in zip((mu, S), ctx.get_state()))
    lit = _Injected()
    lit.mu, lit.sigma, lit.id_map = mu.copy(), S.copy(), {int(i): k for k, i in enumerate(ids)}
    lit.is_init, lit.last_time = True, 0.0
    slam = [(3.0, 2.0, 0.05, [(42, 1, np.array([1.0, 0.2, 0.1]), np.full(3, 0.02)), (9, 1, np.array([0.3, -1.4, 0.9]), np.full(3, 0.02))]),
            (2.0, 2.0, 0.05, [(42, 1, np.array([0.9, 0.25, 0.12]), np.full(3, 0.02)), (3, 1, np.array([1.2, -0.1, 2.6]), np.full(3, 0.03))])]
    staged(ctx, slam)
    t = 0.0
    for s, fr in enumerate(slam):
        ctx.run_staged(s, 1, with_ekf=2)
        ctx.sync()
        t += fr[2]
        lit.add_encoder(fr[0], fr[1], t)
        lit._obs = fr[3]
        k = len(fr[3])
        lit.add_poses(list(range(k)), np.zeros((k, 8)), np.zeros((k, 3)), np.zeros((k, 3)))
        m2, S2 = ctx.get_state()
        assert m2.shape == lit.mu.shape == (15,)
        assert np.abs(m2 - lit.mu).max() <= 1e-9 and np.abs(S2 - lit.sigma).max() <= 1e-9 * np.abs(lit.sigma).max(), f"SLAM frame {s}"
    assert ctx.get_landmark_ids().tolist() == [3, 7, 9, 42]
    assert not np.array_equal(m2[3:12], mu[3:]), "the landmarks must move again"


# ---- 8. the loop, end to end: survey, merge, operate on the merged map with its covariances ---------------------------------------------

def raw_obs(ctx, slot):
    i, v, z, r = ctx.get_slot_raw_observations(slot)
    return [(int(i[k]), int(v[k]), z[k], r[k]) for k in range(len(i))]


def test_survey_merge_then_localize_on_the_merged_map():
    """a 3-robot SLAM fleet on the 240 x 320 ring for 13 ticks, its maps merged, then 5 ticks of aslam_fleet_begin_uncertain on the merge's
    own ids, xyth and sigmas: poses, strips and records equal the reference on each slot's raw observations"""
    from tests.test_fleet import render_fleet, ring_cams
    w = synth.RingWorld(small_ring())
    cfg = w.cfg
    R, T1, T2 = 3, 13, 5
    cams = ring_cams(w, [260.0, 240.0, 260.0], [(0.12, 0.02, 0.0), (0.1, -0.03, 0.0), (0.12, 0.0, 0.0)])
    phases = [0, 6, 12]
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=R, max_landmarks=w.L + 8, persistent_waves=4)
    synth.apply_detector(cfg, ctx=ctx)
    ctx.fleet_slam_begin(cams)
    for row in render_fleet(ctx, w, cams, phases, T1):
        ctx.fleet_add_images(range(R), [im for im, _ in row], *[[getattr(fr, k) for _, fr in row] for k in ("wl", "wr", "dt")])
    m_ids, m_xyth, m_sig, m_seen, rounds, _ = ctx.fleet_merge_maps()
    assert m_ids.size >= 4 and rounds.min() >= 0, (m_ids, rounds)
    assert np.abs(m_sig).max() > 0
    # the robots' poses in the merged (robot 0's) frame: robot 0 started at the origin of its own map
    start = np.array([w.pose[p] for p in phases])
    c0, s0 = math.cos(start[0][2]), math.sin(start[0][2])
    def into0(p):
        d = p[:2] - start[0][:2]
        return np.array([c0 * d[0] + s0 * d[1], -s0 * d[0] + c0 * d[1], norm_angle(p[2] - start[0][2])])
    poses0 = np.array([into0(np.asarray(w.pose[(phases[r] + T1) % len(w.pose)])) for r in range(R)])
    sig = np.diag([1e-3, 1e-3, 1e-4])
    ctx.set_innovation_gate()
    ctx.fleet_begin_uncertain(cams, m_ids, m_xyth, m_sig, poses0, [sig] * R)
    refs = [UncertainMapLocalizer(m_ids, m_xyth, m_sig, poses0[r], sig, dict(DEFAULTS)) for r in range(R)]
    fused = 0
    for t, row in enumerate(render_fleet(ctx, w, cams, phases, T2, t0=T1)):
        ctx.fleet_add_images(range(R), [im for im, _ in row], *[[getattr(fr, k) for _, fr in row] for k in ("wl", "wr", "dt")])
        health, track = ctx.get_slot_health(0, R), ctx.fleet_get_health()
        for r in range(R):
            fr = row[r][1]
            refs[r].add_encoder(fr.wl, fr.wr, fr.dt)
            refs[r].add_observations(raw_obs(ctx, r))
            refs[r].assert_margins()
            check_slot_health(health[r], refs[r].health, f"tick {t} robot {r}")
            check_track(track[r], refs[r].track, f"tick {t} robot {r}")
            check_robot(ctx, r, refs[r], f"tick {t} robot {r}")
            fused += refs[r].health["accepted"]
    assert fused >= R * (T2 - 1), fused
    assert all(np.abs(ref.cross).max() > 0 for ref in refs)


# ---- 9. rendered frames on the MI355X -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_rendered_ring_on_an_uncertain_map():
    """the ring of test_innovation_gate.test_gpu_rendered_ring_records_equal_reference (4 robots, 10 ticks, default gate) on a map whose
    C_i are seeded SPD blocks: poses, strips and records against the reference on each slot's raw observations"""
    assert capi.lib_path().endswith("libaruco_slam_hip.so")
    w = synth.RingWorld(small_ring())
    cfg = w.cfg
    R, T = 4, 10
    mounts = [(0.12, 0.02, 0.0), (-0.15, -0.03, math.pi), (0.0, 0.1, math.pi / 2), (0.0, -0.1, -math.pi / 2)]
    cams = [(synth.camera_matrix(cfg.rows, cfg.cols, f), np.zeros(5), m) for f, m in zip([260.0, 240.0, 280.0, 260.0], mounts)]
    phases = [0, 30, 60, 90]
    poses0 = np.array([w.pose[p] for p in phases])
    sig = np.diag([1e-4, 1e-4, 1e-5])
    C = spd_blocks(np.random.RandomState(19), w.L, 0.02)
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=R, max_landmarks=w.L + 8)
    ctx.set_innovation_gate()
    ctx.fleet_begin_uncertain(cams, w.ids, w.world, C, poses0, [sig] * R)
    refs = [UncertainMapLocalizer(w.ids, w.world, C, poses0[r], sig, dict(DEFAULTS)) for r in range(R)]
    for t in range(T):
        frs = [w.rig_frame(phases[r] + t, [cams[r][2]])[0] for r in range(R)]
        imgs = [ctx.synth_render(0, cfg.rows, cfg.cols, cams[r][0], fr.ids, fr.poses, noise_amp=2, seed=1000 * r + t) for r, fr in enumerate(frs)]
        ctx.fleet_add_images(range(R), imgs, *[[getattr(fr, k) for fr in frs] for k in ("wl", "wr", "dt")])
        health, track = ctx.get_slot_health(0, R), ctx.fleet_get_health()
        for r in range(R):
            refs[r].add_encoder(frs[r].wl, frs[r].wr, frs[r].dt)
            refs[r].add_observations(raw_obs(ctx, r))
            refs[r].assert_margins()
            check_slot_health(health[r], refs[r].health, f"tick {t} robot {r}")
            check_track(track[r], refs[r].track, f"tick {t} robot {r}")
            check_robot(ctx, r, refs[r], f"tick {t} robot {r}")
    n_acc = sum(ref.track["accepted_total"] for ref in refs)
    assert n_acc > R * T and all(np.abs(ref.cross).max() > 0 for ref in refs)
    print("uncertain-map ring:", n_acc, "corrections fused,", sum(ref.track["rejected_total"] for ref in refs), "rejected")
