"""Fleet SLAM rounds at the edges of the chain kernels' sizes, against the long-double restatement of tests/ekf_reference.py.

tests/test_ekf_sizes.py holds the EkfSingle instantiations of the per-frame chain to every edge of their sizes; this file does the same
for the EkfFleet instantiations (ekf_fleet_slam.h), where three more things can go wrong:
  * layout: ekf_fleet_alloc packs a robot's buffers 256-byte padded into one slab, the slabs `stride` apart, so an access past ld or
    past a full map lands in the robot's own id tables, in its neighbour's mu or past the allocation (full maps, every ld residue);
  * divergent z-slices: one launch serves robots with m = 0 beside m = cap, both solvers of k_ekf_small, an appending robot beside a
    correcting one; a value read from the wrong robot shows only when the neighbours differ;
  * blockIdx.z != robot: the stepping robots are listed out of order, with bystanders between them and behind them.
Every stepping robot is held to the reference at the tolerances of test_ekf_sizes.py and, bit for bit, to a windows-off single context
on the same state, encoder sample and list; every bystander must keep the bits it was given.  Runs on the emulation build without a
GPU; the GPU twins run the gfx950 kernels."""
import functools

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from ekf_reference import (CHAIN_CAP, CHAIN_KERNELS, LD, ekf_kernels_run, observe, predicted_pose, random_state, reference_step,
                           rel_err)
from test_ekf_sizes import DT, ID_TABLE, WL, WR, _above, _Injected, landmark_ids, pick
from test_fleet_slam import no_windows_context

E_CAPACITY = -4
CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
FIRST = 3                                           # the staged calls start at a nonzero slot


def encoder_sample(r):
    """robot r's sample of the stepping frame: different per robot, each turns the heading of random_state past pi"""
    return WL + 0.25 * r, WR + 0.4 * r, DT * (1 + 0.1 * r)


def launch_order(stepping):
    """the stepping robots from the ends inwards, [0, 1, 3, 4] -> [4, 0, 3, 1]: never ascending for two robots or more"""
    s, out = sorted(stepping), []
    while s:
        out.append(s.pop())
        if s:
            out.append(s.pop(0))
    return out


def no_obs():
    return [], [], np.zeros((0, 3)), np.zeros((0, 3))


def as_lists(listed):
    """[(id, valid, z, Rdiag)] as the arguments of inject_observations"""
    return ([o[0] for o in listed], [o[1] for o in listed], np.array([o[2] for o in listed]).reshape(-1, 3),
            np.array([o[3] for o in listed]).reshape(-1, 3))


def single_twin(cap, ML, mu, S, ids, frames, waves=4):
    """a windows-off single context of the same capacity and cap on the same state: one arming sample, then
    frames = [(wl, wr, dt, listed)]; returns the context, synchronised"""
    one = no_windows_context(max_rows=64, max_cols=64, max_batch=1 + len(frames), persistent_waves=waves, max_landmarks=ML,
                             max_updates_per_frame=cap)
    one.set_state(mu, S, ids)
    one.stage_encoders([0.0] + [f[0] for f in frames], [0.0] + [f[1] for f in frames], [0.0] + [f[2] for f in frames])
    one.inject_observations(0, *no_obs())
    for s, f in enumerate(frames):
        one.inject_observations(1 + s, *as_lists(f[3]))
    one.run_staged(0, 1 + len(frames), with_ekf=2)
    one.sync()
    return one


@functools.lru_cache(maxsize=None)
def fleet_case(robots, seed, dtype):
    """per robot (m, L), m None for a bystander: a dense state and ids of its own; for a stepping robot also its encoder sample, its
    list in detection order (m = 0: three true measurements, all marked invalid) and the reference's result.  Computed once and
    shared by a test and its GPU twin; nothing modifies it."""
    rng = np.random.RandomState(seed)
    out = []
    for r, (m, L) in enumerate(robots):
        mu, S = random_state(rng, L)
        ids, observable = landmark_ids(rng, L)
        rob = dict(m=m, L=L, mu=mu, S=S, ids=ids)
        if m is not None:
            wl, wr, dt = encoder_sample(r)
            at = predicted_pose(mu, wl, wr, dt)
            if m > 0:
                seen = pick(rng, observable, m)
                obs = observe(rng, mu, seen, post_predict=at)
                det = rng.permutation(m)
                listed = [(int(ids[seen[i]]), 1, obs[i][1], obs[i][2]) for i in det]
                assert seen[-1] == observable[-1] and (m == 1 or seen[0] == observable[0])
            else:
                obs = []
                gated = observe(rng, mu, observable[-3:], post_predict=at) if L >= 3 else \
                    [(0, np.array([1.0 + k, 0.5, 0.1]), np.full(3, 0.05)) for k in range(3)]
                listed = [(int(ids[i]) if L >= 3 else 900 + k, 0, z, rd) for k, (i, z, rd) in enumerate(gated)]
            mu_r, S_r = reference_step(mu, S, wl, wr, dt, obs, dtype=dtype)
            rob.update(enc=(wl, wr, dt), listed=listed, mu_ref=mu_r, S_ref=S_r)
        for v in rob.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(rob)
    return out


def fleet_bits(ctx, r):
    mu, S = ctx.fleet_get_state(r)
    return mu, S, ctx.fleet_get_landmark_ids(r)


def run_fleet_frame(chain, ML, robots, seed, dtype=LD, waves=4, keep=True):
    """one fleet_run_staged of two rounds (an empty list that arms, then predict + m corrections) over the stepping robots of
    `robots` = ((m, L) per robot, m None for a bystander), out of order and from slot FIRST; returns the worst errors.  keep = False
    does not hold on to the case (the large ones)"""
    cap = CHAIN_CAP[chain]
    case = (fleet_case if keep else fleet_case.__wrapped__)(tuple(robots), seed, dtype)
    R = len(robots)
    order = launch_order([r for r in range(R) if robots[r][0] is not None])
    n = len(order)
    assert n < 2 or order != sorted(order)
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=FIRST + 2 * n, persistent_waves=waves, max_landmarks=ML,
                       max_updates_per_frame=cap)
    ctx.fleet_slam_begin([CAM] * R)
    for r, rob in enumerate(case):
        ctx.fleet_set_state(r, rob["mu"], rob["S"], rob["ids"])
    enc = np.zeros((2 * n, 3))
    for i, r in enumerate(order):
        enc[n + i] = case[r]["enc"]
        ctx.inject_observations(FIRST + i, *no_obs())
        ctx.inject_observations(FIRST + n + i, *as_lists(case[r]["listed"]))
    ctx.stage_encoders(enc[:, 0], enc[:, 1], enc[:, 2], slot0=FIRST)
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.fleet_run_staged(FIRST, order + order, with_ekf=2)
    ctx.sync()
    prof = ctx.profile_get()
    assert ekf_kernels_run(prof) == CHAIN_KERNELS[chain], f"cap {cap}: ran {sorted(ekf_kernels_run(prof))}"
    # one launch of each kernel per round, gridDim.z = the round's robots (capi.hip: one profile span per launch)
    assert {k: prof[k][0] for k in CHAIN_KERNELS[chain]} == {k: 2 for k in CHAIN_KERNELS[chain]}, "launches per round"
    stats = ctx.get_slot_ekf_stats(FIRST, 2 * n)
    poses, sigs = ctx.fleet_get_poses()
    worst_mu = worst_S = 0.0
    for i, r in enumerate(order):
        rob = case[r]
        m, L = rob["m"], rob["L"]
        mu_g, S_g, ids_g = fleet_bits(ctx, r)
        assert mu_g.shape == rob["mu_ref"].shape
        e_mu, e_S = float(np.abs(mu_g - rob["mu_ref"]).max()), rel_err(S_g, rob["S_ref"])
        worst_mu, worst_S = max(worst_mu, e_mu), max(worst_S, e_S)
        print(f"fleet {chain} cap {cap} robot {r} (slice {i}) m {m} L {L} max_landmarks {ML} (ld {3 + 3 * ML}): |dmu| {e_mu:.3g}, "
              f"Sigma {e_S:.3g} relative")
        assert np.allclose(mu_g, rob["mu_ref"], rtol=1e-9, atol=1e-11), f"robot {r}: mu differs by {e_mu}"
        assert e_S <= 1e-9, f"robot {r}: Sigma differs by {e_S} (relative)"
        assert np.array_equal(ids_g, rob["ids"]), f"robot {r}: landmark ids changed"
        # detections listed (the gated robot lists three and fuses none), appended, fused, stationary
        assert stats[i].tolist() == [0, 0, 0, 0] and stats[n + i].tolist() == [len(rob["listed"]), 0, m, 0], f"robot {r}: slot stats"
        assert np.array_equal(poses[r], mu_g[:3]) and np.array_equal(sigs[r], S_g[:3, :3]), f"robot {r}: fleet_get_poses"
        one = single_twin(cap, ML, rob["mu"], rob["S"], rob["ids"], [rob["enc"] + (rob["listed"],)], waves)
        mu_1, S_1 = one.get_state()
        assert np.array_equal(mu_g, mu_1) and np.array_equal(S_g, S_1), f"robot {r}: fleet != single context, bit for bit"
        one.close()
    for r in set(range(R)) - set(order):
        mu_g, S_g, ids_g = fleet_bits(ctx, r)
        rob = case[r]
        assert np.array_equal(mu_g, rob["mu"]) and np.array_equal(S_g, rob["S"]) and np.array_equal(ids_g, rob["ids"]), \
            f"bystander {r} changed"
        assert np.array_equal(poses[r], rob["mu"][:3]) and np.array_equal(sigs[r], rob["S"][:3, :3]), f"bystander {r}: fleet_get_poses"
    ctx.close()
    return worst_mu, worst_S


# ---- every chain at its caps, every leading-dimension residue ----------------------------------------------------------------------

# max_landmarks = 63, 42, 20 (mod 64) give ld = 3 + 3 max_landmarks = 0, 1, 63 (mod 64)
LD_RESIDUES = (63, 42, 20)
FLEET_M = {"fast": (0, 1, 24, 23), "mid": (0, 25, 64, 33), "general": (1, 32, 33, 128)}
STEPPERS = (0, 1, 3, 4)                             # robot 2 stands by between them, robot 5 (full) behind them
KINDS = ("seen", "some", "full")                    # L = m (every landmark seen), m + 19, max_landmarks


def _fleet_cases():
    cases = []
    for chain, ms in FLEET_M.items():
        for j, res in enumerate(LD_RESIDUES):
            ML = _above(max(ms) + 19, res)
            robots = [None] * 6
            for i, (r, m) in enumerate(zip(STEPPERS, ms)):
                robots[r] = (m, {"seen": m, "some": m + 19, "full": ML}[KINDS[(i + j) % 3]])
            robots[2] = (None, 7)
            robots[5] = (None, ML)
            cases.append((chain, ML, tuple(robots)))
    return cases


FLEET_CASES = _fleet_cases()
FLEET_IDS = [f"{c}-ml{ml}-ld{(3 + 3 * ml) % 64}" for c, ml, _ in FLEET_CASES]


@pytest.mark.parametrize("chain,ML,robots", FLEET_CASES, ids=FLEET_IDS)
def test_fleet_round_against_long_double_reference(chain, ML, robots):
    run_fleet_frame(chain, ML, robots, seed=7 * ML + len(chain))


@pytest.mark.gpu
@pytest.mark.parametrize("chain,ML,robots", FLEET_CASES, ids=FLEET_IDS)
def test_fleet_round_on_gpu(chain, ML, robots):
    run_fleet_frame(chain, ML, robots, seed=7 * ML + len(chain))


def test_fleet_cases_cover_the_edges():
    for chain, ms in FLEET_M.items():
        mine = [(ml, rb) for c, ml, rb in FLEET_CASES if c == chain]
        cap = CHAIN_CAP[chain]
        assert {(3 + 3 * ml) % 64 for ml, _ in mine} == {0, 1, 63}, chain
        assert max(ms) == cap
        full_at_cap = False
        for ml, rb in mine:
            stepping = [r for r in range(len(rb)) if rb[r][0] is not None]
            order = launch_order(stepping)
            assert sorted(rb[r][0] for r in stepping) == sorted(ms), "every case steps the whole row of sizes"
            assert order != sorted(order), "robots listed ascending"
            assert any(a < b < c and rb[b][0] is None for a in stepping for c in stepping for b in range(len(rb))), "no bystander between"
            assert rb[-1] == (None, ml), "the last robot is not a bystander with a full map"
            assert any(rb[r][0] > 0 and rb[r][1] == ml for r in stepping), "no full stepping robot that observes its last landmark"
            assert all(rb[r][1] <= ml and rb[r][1] >= rb[r][0] for r in stepping)
            full_at_cap |= any(rb[r] == (cap, ml) for r in stepping)
            sliced = [rb[r][0] for r in order]                       # m by z-slice
            if 0 in ms:
                assert any({a, b} == {0, cap} for a, b in zip(sliced, sliced[1:])), "m = 0 not beside m = cap"
        assert full_at_cap, f"{chain}: no robot at the cap with a full map"
    ms = FLEET_M["general"]
    assert any(m <= 32 for m in ms) and any(32 < m for m in ms) and {32, 33} <= set(ms), "one k_ekf_small launch takes both solvers"


# ---- appending to exactly full, beside correcting robots ---------------------------------------------------------------------------

APPEND_ML = 84                                      # ld = 255 = 63 (mod 64)
A, B, C, D = 2, 0, 3, 1                             # appends to full / corrects / sees nothing / stands by (between B and A)
APPEND_L = {A: 60, B: 50, C: 30, D: APPEND_ML}


def _literal(mu, S, ids):
    lit = _Injected()
    lit.mu, lit.sigma = mu.copy(), S.copy()
    lit.id_map = {int(i): k for k, i in enumerate(ids)}
    lit.add_encoder(0.0, 0.0, 0.0)
    return lit


def _literal_frame(lit, wl, wr, t, listed):
    """one frame of [(id, valid, z, Rdiag)] through the literal transcription; returns its log (id, index, action) in pop order"""
    lit.add_encoder(wl, wr, t)
    lit._obs = [(o[0], o[2], o[3]) for o in listed if o[1]]
    k = len(lit._obs)
    lit.add_poses(list(range(k)), np.zeros((k, 8)), np.zeros((k, 3)), np.zeros((k, 3)))
    return np.array(lit.log, np.int32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def append_case():
    """states, ids and two frames per stepping robot.  Frame 1: A sees 40 known ids (one of them twice) and the 24 new ids that fill
    its map, B corrects 35, C sees nothing.  Frame 2: A and B correct again, C sees nothing; `extra` is one further new id for A."""
    rng = np.random.RandomState(84)
    pool = rng.permutation(ID_TABLE).astype(np.int32)
    n_new = APPEND_ML - APPEND_L[A]
    st = {}
    for r in (B, D, A, C):
        mu, S = random_state(rng, APPEND_L[r])
        st[r] = dict(mu=mu, S=S, ids=pool[:APPEND_L[r]].copy(), enc=encoder_sample(r))

    def known(r, mu, k, t_enc):
        seen = np.sort(rng.choice(APPEND_L[r], k, replace=False))
        return [(int(st[r]["ids"][i]), 1, z, rd) for i, z, rd in observe(rng, mu, seen, post_predict=predicted_pose(mu, *t_enc))]

    def fresh(lid):
        return (int(lid), 1, np.array([rng.uniform(0.5, 2), rng.uniform(-1, 1), rng.uniform(-3, 3)]), rng.uniform(0.02, 0.2, 3))

    a1 = known(A, st[A]["mu"], 40, st[A]["enc"])
    a1 += [fresh(lid) for lid in pool[APPEND_L[A]:APPEND_ML]]
    a1.append((a1[3][0], 1, a1[3][2] + rng.normal(0, 0.02, 3), rng.uniform(0.02, 0.2, 3)))
    st[A]["frames"] = [[a1[i] for i in rng.permutation(len(a1))], known(A, st[A]["mu"], 9, st[A]["enc"])]
    st[B]["frames"] = [known(B, st[B]["mu"], 35, st[B]["enc"]), known(B, st[B]["mu"], 34, st[B]["enc"])]
    st[C]["frames"] = [[], []]
    assert len(st[A]["frames"][0]) == 41 + n_new
    return st, fresh(pool[APPEND_ML])


def run_append(extra):
    """the two calls on a fleet of four; returns the fleet (synchronised after frame 1 and checked there), and whether the second
    sync reported ASLAM_E_CAPACITY"""
    st, extra_obs = append_case()
    cap = CHAIN_CAP["general"]
    order = launch_order([A, B, C])
    assert order == [C, B, A] and B < D < A
    n = len(order)
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=FIRST + 2 * n, persistent_waves=4, max_landmarks=APPEND_ML,
                       max_updates_per_frame=cap)
    ctx.fleet_slam_begin([CAM] * 4)
    for r in range(4):
        ctx.fleet_set_state(r, st[r]["mu"], st[r]["S"], st[r]["ids"])
    enc = np.zeros((2 * n, 3))
    for i, r in enumerate(order):
        enc[n + i] = st[r]["enc"]
        ctx.inject_observations(FIRST + i, *no_obs())
        ctx.inject_observations(FIRST + n + i, *as_lists(st[r]["frames"][0]))
    ctx.stage_encoders(enc[:, 0], enc[:, 1], enc[:, 2], slot0=FIRST)
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.fleet_run_staged(FIRST, order + order, with_ekf=2)
    ctx.sync()                                                      # A is exactly full: no capacity error
    assert ekf_kernels_run(ctx.profile_get()) == CHAIN_KERNELS["general"]
    stats1 = ctx.get_slot_ekf_stats(FIRST + n, n)
    after1 = {r: fleet_bits(ctx, r) for r in range(4)}
    frames2 = {r: list(st[r]["frames"][1]) for r in order}
    if extra:
        frames2[A].insert(4, extra_obs)
    first2 = 1                                                       # another nonzero slot, overlapping the first call's
    for i, r in enumerate(order):
        ctx.inject_observations(first2 + i, *as_lists(frames2[r]))
    ctx.stage_encoders(enc[n:, 0], enc[n:, 1], enc[n:, 2], slot0=first2)
    ctx.fleet_run_staged(first2, order, with_ekf=2)
    overflow = False
    try:
        ctx.sync()
    except capi.AslamError as e:
        assert e.code == E_CAPACITY, e
        overflow = True
    stats2 = ctx.get_slot_ekf_stats(first2, n)
    return ctx, order, stats1, after1, stats2, overflow


def _append_to_exactly_full():
    st, _ = append_case()
    cap = CHAIN_CAP["general"]
    ctx, order, stats1, after1, stats2, overflow = run_append(extra=False)
    assert not overflow
    n_new = APPEND_ML - APPEND_L[A]
    for i, r in enumerate(order):
        s = st[r]
        wl, wr, dt = s["enc"]
        lit = _literal(s["mu"], s["S"], s["ids"])
        lg = _literal_frame(lit, wl, wr, dt, s["frames"][0])
        acts = lg[:, 2].tolist()
        mu_g, S_g, ids_g = after1[r]
        assert mu_g.shape == lit.mu.shape, f"robot {r}: map size"
        e_mu, e_S = float(np.abs(mu_g - lit.mu).max()), rel_err(S_g, lit.sigma)
        print(f"append to full, robot {r} (slice {i}), {len(s['frames'][0])} observations: |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")
        assert np.allclose(mu_g, lit.mu, rtol=1e-9, atol=1e-11) and e_S <= 1e-9, f"robot {r}: differs from the literal transcription"
        assert stats1[i].tolist() == [len(s["frames"][0]), acts.count(0), acts.count(1), acts.count(2)], f"robot {r}: stats"
        assert ids_g.tolist() == sorted(lit.id_map, key=lit.id_map.get), f"robot {r}: landmark ids / order of appending"
        # the fleet has no per-robot pop list to read: the single context's is compared with the literal log, its state with the fleet's
        frames = [(wl, wr, dt, f) for f in s["frames"]]
        one = single_twin(cap, APPEND_ML, s["mu"], s["S"], s["ids"], frames[:1])
        gi, gx, ga, _, _ = one.get_observations()
        assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), lg), f"robot {r}: pop order / branches"
        mu_1, S_1 = one.get_state()
        assert np.array_equal(mu_g, mu_1) and np.array_equal(S_g, S_1) and np.array_equal(ids_g, one.get_landmark_ids()), \
            f"robot {r}: fleet != single context, bit for bit"
        one.close()
        # the second frame (the run without the further id): corrections on the map that has just become full
        lg2 = _literal_frame(lit, wl, wr, 2 * dt, s["frames"][1])
        mu_2, S_2, ids_2 = fleet_bits(ctx, r)
        assert np.allclose(mu_2, lit.mu, rtol=1e-9, atol=1e-11) and rel_err(S_2, lit.sigma) <= 1e-9, f"robot {r}: frame 2"
        assert stats2[i].tolist() == [len(s["frames"][1]), 0, (lg2[:, 2] == 1).sum(), (lg2[:, 2] == 2).sum()], f"robot {r}: frame 2 stats"
        one = single_twin(cap, APPEND_ML, s["mu"], s["S"], s["ids"], frames)
        gi, gx, ga, _, _ = one.get_observations()
        assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), lg2), f"robot {r}: pop order / branches of frame 2"
        mu_1, S_1 = one.get_state()
        assert np.array_equal(mu_2, mu_1) and np.array_equal(S_2, S_1) and np.array_equal(ids_2, one.get_landmark_ids()), \
            f"robot {r}: fleet != single context after two frames, bit for bit"
        one.close()
        if r == A:
            assert acts.count(0) == n_new and acts.count(1) == 41 and ids_g.size == APPEND_ML, "A does not end exactly full"
        if r == B:
            assert acts.count(0) == 0 and acts.count(1) == 35 > 32
        if r == C:
            assert lg.size == 0 and not np.array_equal(mu_g[:3], s["mu"][:3]), "C predicts only"
    for got in (after1[D], fleet_bits(ctx, D)):
        assert all(np.array_equal(a, b) for a, b in zip(got, (st[D]["mu"], st[D]["S"], st[D]["ids"]))), "bystander D changed"

    # one further new id for the full robot: reported at the next sync, and nobody else notices
    ctx2, _, stats1x, after1x, stats2x, overflow = run_append(extra=True)
    assert overflow, "a new id for a full map was not reported"
    assert np.array_equal(stats1x, stats1)
    for r in range(4):
        assert all(np.array_equal(a, b) for a, b in zip(after1x[r], after1[r])), f"robot {r}: frame 1 is not reproducible"
        where = "the full robot's own corrections changed with the id it could not append" if r == A else \
            f"robot {r} changed with the overflow of robot {A}"
        assert all(np.array_equal(a, b) for a, b in zip(fleet_bits(ctx2, r), fleet_bits(ctx, r))), where
    assert fleet_bits(ctx2, A)[2].size == APPEND_ML
    ia = order.index(A)
    assert stats2x[ia].tolist() == [stats2[ia][0] + 1, 0, stats2[ia][2], stats2[ia][3]], "the id that did not fit is listed, not appended"
    assert np.array_equal(np.delete(stats2x, ia, 0), np.delete(stats2, ia, 0))
    ctx.close()
    ctx2.close()


def test_append_to_exactly_full_beside_correcting_robots():
    _append_to_exactly_full()


@pytest.mark.gpu
def test_append_to_exactly_full_on_gpu():
    _append_to_exactly_full()


# ---- both tile widths of the update kernel in a fleet (GPU only: a quarter of a minute per case on the emulation) -----------------------------------------

# k_ekf_update_mfma<5> runs for 938 <= max_landmarks <= 1065, <4> for every other size
TILE_CASES = [(ML, chain, ms) for ML in (938, 1065, 1066) for chain, ms in (("mid", (64, 40)), ("general", (100, 20)))]


@pytest.mark.gpu
@pytest.mark.parametrize("ML,chain,ms", TILE_CASES, ids=[f"{c}-ml{ml}" for ml, c, _ in TILE_CASES])
def test_fleet_update_tile_widths_on_gpu(ML, chain, ms):
    """two full robots with different m, the second listed first (double reference: long double takes minutes at these sizes, as in
    test_update_tile_widths_on_gpu)"""
    run_fleet_frame(chain, ML, tuple((m, ML) for m in ms), seed=ML + ms[0], dtype=np.float64, waves=64, keep=False)
