"""The innovation gate of SLAM, rig SLAM and fleet SLAM (aslam_set_slam_gate) against the gated references of
tests/slam_gate_reference.py.

Inputs: random_state / observe of tests/ekf_reference.py (noise 0.03); an outlier is a true sighting displaced by (2.7, -2.1, 0);
gate_d2 = 1.0.  On such inputs a long-double gated step gives every true sighting d2 <= 0.14 and every outlier d2 >= 5.8 (m = L in
{1, 2, 24, 64, 128}, (24, 43), (33, 52), 8 seeds each, every third correction an outlier), so no decision hangs on rounding; every
case asserts that again for its own inputs (no d2 within 1e-6 of the gate, no ||ze|| within 1e-6 of 1, the reference alone accepts
every true sighting and rejects every planted outlier) before it compares anything discrete.
Tolerances, the project's: mu rtol 1e-9 / atol 1e-11, Sigma 1e-9 relative, nis_sum and d2_max 1e-9 relative; counts, ids, actions,
flags and worst_id exact.  Every device case runs on the session's library (the emulation without a GPU) and again under -m gpu."""
import functools
import math

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from ekf_reference import (CHAIN_CAP, CHAIN_KERNELS, LD, ekf_kernels_run, observe, predicted_pose, random_state, rel_err)
from slam_gate_reference import (DEFAULTS, OUTLIER, TRACK_ZERO, GatedLiteralSlam, advance_track, assert_margins, check_slot_health,
                                 check_track, gated_reference_step)
from test_ekf_sizes import DT, ID_TABLE, WL, WR, _above, landmark_ids, pick
from test_fleet_slam import no_windows_context

E_INVALID, E_STATE = -1, -5
INF = float("inf")
GATE = 1.0
FINISH = "k_ekf_gate_finish"
CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))


def same_bytes(a, b):
    """two health records (or arrays of them), every byte"""
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def refused(code, fn, *a, **kw):
    with pytest.raises(capi.AslamError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (fn, e.value)


def no_obs():
    return [], [], np.zeros((0, 3)), np.zeros((0, 3))


def inject(ctx, slot, obs):
    """obs = [(id, z, Rdiag)] in detection order"""
    ctx.inject_observations(slot, [o[0] for o in obs], [1] * len(obs), np.array([o[1] for o in obs]).reshape(-1, 3),
                            np.array([o[2] for o in obs]).reshape(-1, 3))


def outlier_positions(pattern, m):
    """which pop positions of a frame of m corrections carry an outlier"""
    return {"none": set(), "all": set(range(m)), "first": {0}, "last": {m - 1}, "pair": {m // 2, min(m // 2 + 1, m - 1)},
            "third": set(range(2, m, 3))}[pattern]


def patterns_for(m):
    """the rejection patterns that differ at this m"""
    seen, out = [], []
    for p in ("none", "all", "first", "last", "pair", "third"):
        s = outlier_positions(p, m)
        if s not in seen:
            seen.append(s)
            out.append(p)
    return out


@functools.lru_cache(maxsize=None)
def frame_case(m, L, seed, pattern, nan_at=None):
    """a dense state, m sightings of known landmarks in pop order with the pattern's outliers planted (nan_at: that pop position's
    z[0] is NaN instead), a detection order, and the gated long-double step on them.  Computed once, shared with the GPU twin."""
    rng = np.random.RandomState(seed)
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
    mu_r, S_r, info = gated_reference_step(mu, S, WL, WR, DT, obs, GATE, ids=ids)
    want_rej = [k in out or k == nan_at for k in range(m)]
    assert_margins(GATE, info["d2"], info["norms"])
    assert info["rejected"] == want_rej, "the reference alone does not separate the planted outliers from the true sightings"
    free, _, info_inf = gated_reference_step(mu, S, WL, WR, DT, obs, INF, ids=ids, dtype=np.float64)
    case = dict(mu=mu, S=S, ids=ids, seen=seen, obs=obs, det=det, mu_ref=mu_r, S_ref=S_r, info=info, info_inf=info_inf, rejected=want_rej)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def stage_case(ctx, case):
    """the state, an arming sample in slot 0 and the frame in slot 1"""
    ids, seen, obs, det = case["ids"], case["seen"], case["obs"], case["det"]
    ctx.set_state(case["mu"], case["S"], ids)
    ctx.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
    ctx.inject_observations(0, *no_obs())
    inject(ctx, 1, [(ids[seen[i]], obs[i][1], obs[i][2]) for i in det])


def context(cap, ML, batch=2, windows=True):
    kw = dict(max_rows=64, max_cols=64, max_batch=batch, persistent_waves=4, max_landmarks=ML, max_updates_per_frame=cap)
    return capi.Context(**kw) if windows else no_windows_context(**kw)


def run_gated_frame(chain, m, L, ML, pattern, nan_at=None):
    case = frame_case(m, L, 1000 * m + L, pattern, nan_at)
    cap = CHAIN_CAP[chain]
    ctx = context(cap, ML)
    ctx.set_slam_gate(gate_d2=GATE)
    stage_case(ctx, case)
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.run_staged(0, 2, with_ekf=2)
    ctx.sync()
    prof = ctx.profile_get()
    ran = ekf_kernels_run(prof)
    assert ran == CHAIN_KERNELS[chain] | {FINISH}, f"cap {cap}: ran {sorted(ran)}"
    assert prof[FINISH][0] == 2, "one finish launch per frame"
    rej = np.array(case["rejected"])
    gi, gx, ga, _, _ = ctx.get_observations()
    assert np.array_equal(gx, case["seen"]) and np.array_equal(gi, case["ids"][case["seen"]]), "pop order differs"
    assert np.array_equal(ga, np.where(rej, 3, 1)), f"actions {ga.tolist()}"
    n_acc = int((~rej).sum())
    assert ctx.get_slot_ekf_stats(1, 1)[0].tolist() == [m, 0, n_acc, 0]
    h = ctx.get_slot_health(0, 2)
    check_slot_health(h[0], dict(attempted=0, accepted=0, rejected=0, ref_flagged=0, worst_id=-1, nis_sum=0.0, d2_max=0.0), "arming slot")
    check_slot_health(h[1], case["info"]["health"], f"{chain} m {m} {pattern}")
    track = dict(TRACK_ZERO)
    advance_track(track, dict(attempted=0, accepted=0, rejected=0), {**DEFAULTS})
    advance_track(track, case["info"]["health"], {**DEFAULTS})
    check_track(ctx.get_track_health(), track, f"{chain} m {m} {pattern}")
    mu_g, S_g = ctx.get_state()
    assert np.isfinite(mu_g).all() and np.isfinite(S_g).all()
    e_mu, e_S = float(np.abs(mu_g - case["mu_ref"]).max()), rel_err(S_g, case["S_ref"])
    print(f"{chain} m {m} L {L} max_landmarks {ML} {pattern} nan {nan_at}: |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert np.allclose(mu_g, case["mu_ref"], rtol=1e-9, atol=1e-11), f"mu differs by {e_mu}"
    assert e_S <= 1e-9, f"Sigma differs by {e_S} (relative)"


# the sizes at which each solver can go wrong: the fast chain's m x m thread mapping, the mid chain's blocks per thread, k_ekf_small's
# LDS Gauss-Jordan (3m <= 96) and ekf_small_general above it; L = m and m + 19; max_landmarks giving ld = 0, 1, 63 (mod 64) in turn
LD_RESIDUES = (63, 42, 20)
SIZES = {"fast": (1, 2, 23, 24), "mid": (25, 32, 33, 63, 64), "general": (1, 32, 33, 65, 127, 128)}
CASES, _n = [], 0
for _chain, _ms in SIZES.items():
    for _k, _m in enumerate(_ms):
        for _L in (_m, _m + 19):
            _ML = _L if _L == _m and _k % 2 == 0 else _above(_L, LD_RESIDUES[_n % 3])      # a full map at every other size
            _n += 1
            for _p in patterns_for(_m):
                CASES.append((_chain, _m, _L, _ML, _p))
CASE_IDS = [f"{c}-m{m}-L{L}-ml{ml}-{p}" for c, m, L, ml, p in CASES]


def test_cases_cover_every_leading_dimension_residue_and_a_full_map():
    assert {(3 + 3 * ml) % 64 for _, _, _, ml, _ in CASES} >= {0, 1, 63}
    assert any(L == ml for _, _, L, ml, _ in CASES)


@pytest.mark.parametrize("chain,m,L,ML,pattern", CASES, ids=CASE_IDS)
def test_gated_chain_against_long_double_reference(chain, m, L, ML, pattern):
    run_gated_frame(chain, m, L, ML, pattern)


@pytest.mark.gpu
@pytest.mark.parametrize("chain,m,L,ML,pattern", CASES, ids=CASE_IDS)
def test_gated_chain_on_gpu(chain, m, L, ML, pattern):
    run_gated_frame(chain, m, L, ML, pattern)


# ---- gate_d2 = inf: monitor only -----------------------------------------------------------------------------------------------

MONITOR = [("fast", 23, 30), ("mid", 33, 52), ("general", 32, 40), ("general", 65, 70)]


def _monitor_only(chain, m, L):
    """bit for bit the gate-off, windows-off context; the records equal the reference (which rejects nothing at +inf)"""
    case = frame_case(m, L, 77 * m + L, "third")
    cap = CHAIN_CAP[chain]
    res = []
    for gated in (False, True):
        ctx = context(cap, L + 2, windows=gated)                  # the gated context is a default one: the gate turns windows off
        if gated:
            ctx.set_slam_gate(gate_d2=INF)
        stage_case(ctx, case)
        ctx.run_staged(0, 2, with_ekf=2)
        ctx.sync()
        res.append(ctx.get_state() + (ctx.get_landmark_ids(),) + ctx.get_observations() + (ctx.get_slot_ekf_stats(0, 2),))
        if gated:
            check_slot_health(ctx.get_slot_health(1, 1)[0], case["info_inf"]["health"], f"monitor {chain} m {m}")
            assert ctx.get_slot_health(1, 1)[0]["rejected"] == 0 and len(outliers_of(case)) > 0
    for x, y in zip(*res):
        assert np.array_equal(x, y, equal_nan=True), f"monitor {chain} m {m}: the gate at +inf changed a result"


def outliers_of(case):
    return [k for k, r in enumerate(case["rejected"]) if r]


@pytest.mark.parametrize("chain,m,L", MONITOR)
def test_monitor_only_keeps_every_bit(chain, m, L):
    _monitor_only(chain, m, L)


@pytest.mark.gpu
@pytest.mark.parametrize("chain,m,L", MONITOR)
def test_monitor_only_keeps_every_bit_on_gpu(chain, m, L):
    _monitor_only(chain, m, L)


# ---- a NaN z at the finite gate ---------------------------------------------------------------------------------------------------

NAN_CASES = [(chain, m, L, where) for chain, m, L in (("fast", 7, 9), ("general", 7, 9), ("general", 40, 45)) for where in ("first", "last")]


def _nan_is_rejected(chain, m, L, where):
    nan_at = 0 if where == "first" else m - 1
    run_gated_frame(chain, m, L, L + 1, "none", nan_at=nan_at)
    # the reference with the NaN sighting equals the reference without it
    case = frame_case(m, L, 1000 * m + L, "none", nan_at)
    obs = [o for k, o in enumerate(case["obs"]) if k != nan_at]
    mu_r, S_r, _ = gated_reference_step(case["mu"], case["S"], WL, WR, DT, obs, GATE, ids=case["ids"])
    assert np.array_equal(mu_r, case["mu_ref"]) and np.array_equal(S_r, case["S_ref"])


@pytest.mark.parametrize("chain,m,L,where", NAN_CASES)
def test_nan_sighting_is_rejected(chain, m, L, where):
    _nan_is_rejected(chain, m, L, where)


@pytest.mark.gpu
@pytest.mark.parametrize("chain,m,L,where", NAN_CASES)
def test_nan_sighting_is_rejected_on_gpu(chain, m, L, where):
    _nan_is_rejected(chain, m, L, where)


# ---- sequences on the device's own plan --------------------------------------------------------------------------------------------

def literal_on(mu, S, ids, gate=None):
    lit = GatedLiteralSlam(gate=dict(gate_d2=GATE, **(gate or {})))
    lit.seat(mu, S, ids)
    return lit


def check_frame(ctx, lit, slot, where, single=True):
    """the last frame's pops, the slot's stats and record against the literal reference"""
    if single:
        gi, gx, ga, _, _ = ctx.get_observations()
        assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), np.array(lit.log, np.int32).reshape(-1, 3)), f"{where}: pops differ"
    assert ctx.get_slot_ekf_stats(slot, 1)[0].tolist() == lit.stats, f"{where}: stats"
    check_slot_health(ctx.get_slot_health(slot, 1)[0], lit.health, where)


def check_state(got, lit, where):
    mu_g, S_g = got
    assert mu_g.shape == lit.mu.shape, f"{where}: map size"
    e_mu, e_S = float(np.abs(mu_g - lit.mu).max()), rel_err(S_g, lit.sigma)
    print(f"{where}: |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert np.allclose(mu_g, lit.mu, rtol=1e-9, atol=1e-11) and e_S <= 1e-9, f"{where}: state differs ({e_mu}, {e_S})"


@functools.lru_cache(maxsize=None)
def sequence_case():
    """frame 1: known ids, one of them (X) an outlier; frame 2: X and an accepted sighting A repeated identically, new ids, fresh known
    ids, and one id twice whose first popped copy is an outlier; frame 3: a plain frame.  Then six frames of the same eight landmarks
    for the windows that come back once the gate is cleared."""
    rng = np.random.RandomState(11)
    L, n_new = 14, 3
    mu, S = random_state(rng, L, heading=0.4)
    ids = rng.permutation(ID_TABLE)[:L + n_new].astype(np.int32)
    at = predicted_pose(mu, WL, WR, DT)

    def sight(idx, outlier=()):
        return [(int(ids[i]), z + (OUTLIER if i in outlier else 0.0), r) for i, z, r in observe(rng, mu, idx, post_predict=at)]

    f1 = sight([1, 4, 6, 9], outlier=(4,))                       # X = landmark 4, A = landmark 6
    x_obs, a_obs = f1[1], f1[2]
    new = [(int(ids[L + k]), np.array([rng.uniform(0.5, 2), rng.uniform(-1, 1), rng.uniform(-3, 3)]), rng.uniform(0.02, 0.2, 3))
           for k in range(n_new)]
    twice_bad, twice_good = sight([11], outlier=(11,))[0], sight([11])[0]
    frames = [[], f1]
    for pair in ((twice_bad, twice_good), (twice_good, twice_bad)):     # the detection order in which the outlier copy pops first
        f2 = [x_obs, new[0], a_obs] + sight([2, 9]) + [pair[0], new[1]] + [pair[1], new[2]]
        lit = literal_on(mu, S, ids[:L])
        lit.add_encoder(0.0, 0.0, 0.0)
        for k, f in enumerate((f1, f2)):
            lit.add_encoder(WL, WR, DT * (k + 1))
            lit.add_frame(f)
        acts = [a for i, _, a in lit.log if i == twice_bad[0]]
        if acts == [3, 1]:
            break
    else:
        raise AssertionError(f"neither order pops the outlier copy first: {acts}")
    frames += [f2, sight([0, 3, 5, 13])]
    tail = [sight(range(2, 10)) for _ in range(6)]
    return dict(mu=mu, S=S, ids=ids, L=L, frames=frames, tail=tail, x_id=x_obs[0], a_id=a_obs[0], twice_id=twice_bad[0])


def _sequence():
    sc = sequence_case()
    mu, S, ids, L, frames, tail = sc["mu"], sc["S"], sc["ids"], sc["L"], sc["frames"], sc["tail"]
    nf = len(frames)
    lit = literal_on(mu, S, ids[:L])

    def fresh(windows=True):
        ctx = context(24, L + 8, batch=nf + len(tail), windows=windows)
        ctx.set_slam_gate(gate_d2=GATE)
        ctx.set_state(mu, S, ids[:L])
        ctx.stage_encoders([0.0] + [WL] * (nf - 1), [0.0] + [WR] * (nf - 1), [0.0] + [DT] * (nf - 1))
        for s, f in enumerate(frames):
            inject(ctx, s, f)
        return ctx

    # single steps, each checked against the literal reference
    one = fresh(windows=False)
    t = 0.0
    for s, f in enumerate(frames):
        one.run_staged(s, 1, with_ekf=2)
        one.sync()
        lit.add_encoder(WL if s else 0.0, WR if s else 0.0, t)
        t += DT
        lit.add_frame(f)
        check_frame(one, lit, s, f"frame {s}")
        check_state(one.get_state(), lit, f"frame {s}")
        if s == 2:
            by_id = {}
            for i, _, a in lit.log:
                by_id.setdefault(i, []).append(a)
            assert by_id[sc["x_id"]] == [3], "a rejected sighting repeated identically must be judged (and rejected) again"
            assert by_id[sc["a_id"]] == [2], "an accepted sighting repeated identically is stationary"
            assert by_id[sc["twice_id"]] == [3, 1] and sum(a == 0 for _, _, a in lit.log) == 3
    lit.assert_margins()
    assert lit.track["rejected_total"] == 3 and lit.track["frames"] == nf
    check_track(one.get_track_health(), lit.track, "single steps")
    # one batch on a default (windows-on) context: no window kernel runs, every bit equals the single steps
    ctx = fresh()
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.run_staged(0, nf, with_ekf=2)
    ctx.sync()
    prof = ctx.profile_get()
    assert not any(k.startswith("k_ekf_win") and v[0] > 0 for k, v in prof.items()), "a window kernel ran under the SLAM gate"
    assert prof[FINISH][0] == nf
    for x, y in zip(one.get_state() + one.get_observations() + (one.get_slot_ekf_stats(0, nf), one.get_landmark_ids()),
                    ctx.get_state() + ctx.get_observations() + (ctx.get_slot_ekf_stats(0, nf), ctx.get_landmark_ids())):
        assert np.array_equal(x, y, equal_nan=True), "a batch differs from single steps"
    assert same_bytes(one.get_slot_health(0, nf), ctx.get_slot_health(0, nf)) and same_bytes(one.get_track_health(), ctx.get_track_health())
    # the gate cleared: the next batch runs windows again and matches the literal transcription
    ctx.set_slam_gate(None)
    assert ctx.get_slam_gate() is None
    ctx.stage_encoders([WL] * len(tail), [WR] * len(tail), [DT] * len(tail), slot0=nf)
    for s, f in enumerate(tail):
        inject(ctx, nf + s, f)
    ctx.profile_reset()
    ctx.run_staged(nf, len(tail), with_ekf=2)
    ctx.sync()
    prof = ctx.profile_get()
    assert prof["k_ekf_win_step"][0] > 0 and prof[FINISH][0] == 0, "no window after the gate was cleared"
    lit.gate["gate_d2"] = INF
    for f in tail:
        lit.add_encoder(WL, WR, t)
        t += DT
        lit.add_frame(f)
    check_state(ctx.get_state(), lit, "windows after set_slam_gate(None)")
    gi, gx, ga, _, _ = ctx.get_observations()
    assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), np.array(lit.log, np.int32).reshape(-1, 3))


def test_sequence_on_the_device_plan():
    _sequence()


@pytest.mark.gpu
def test_sequence_on_the_device_plan_on_gpu():
    _sequence()


# ---- fleet SLAM ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fleet_case(cap):
    """six robots: m = 0, a bystander, all rejected, none rejected, mixed, a bystander; two stepping frames each"""
    rng = np.random.RandomState(40 + cap)
    kinds = ("empty", None, "all", "none", "third", None)
    m = {24: 9, 64: 27, 128: 35}[cap]
    robots = []
    for r, kind in enumerate(kinds):
        L = m + 2 + r
        mu, S = random_state(rng, L, heading=0.3 * r - 0.5)
        ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
        rob = dict(kind=kind, mu=mu, S=S, ids=ids, frames=[])
        if kind is not None:
            wl, wr, dt = WL + 0.25 * r, WR + 0.4 * r, DT * (1 + 0.1 * r)
            pose = mu[:3]
            for f in range(2):
                pose = predicted_pose(np.concatenate([pose, mu[3:]]), wl, wr, dt)
                seen = np.sort(rng.choice(L, m, replace=False)) if kind != "empty" else []
                out = outlier_positions(kind, m) if kind != "empty" else set()
                obs = [(int(ids[i]), z + (OUTLIER if k in out else 0.0), rd)
                       for k, (i, z, rd) in enumerate(observe(rng, mu, seen, post_predict=pose))]
                rob["frames"].append((wl, wr, dt, [obs[i] for i in rng.permutation(len(obs))]))
        robots.append(rob)
    return robots


def _fleet(cap):
    robots = fleet_case(cap)
    R = len(robots)
    order = [4, 0, 3, 2]                                       # out of order, bystanders 1 and 5 between and behind
    n = len(order)
    ML = max(len(r["ids"]) for r in robots) + 1
    first = 3
    ctx = context(cap, ML, batch=first + 3 * n)
    ctx.set_slam_gate(gate_d2=GATE)
    ctx.fleet_slam_begin([CAM] * R)
    for r, rob in enumerate(robots):
        ctx.fleet_set_state(r, rob["mu"], rob["S"], rob["ids"])
    enc = np.zeros((3 * n, 3))
    for i, r in enumerate(order):
        ctx.inject_observations(first + i, *no_obs())
        for f in range(2):
            enc[(1 + f) * n + i] = robots[r]["frames"][f][:3]
            inject(ctx, first + (1 + f) * n + i, robots[r]["frames"][f][3])
    ctx.stage_encoders(enc[:, 0], enc[:, 1], enc[:, 2], slot0=first)
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.fleet_run_staged(first, order + order, with_ekf=2)                      # two rounds in one call: arm, step
    ctx.sync()
    mid_health = ctx.fleet_get_health()
    ctx.fleet_run_staged(first + 2 * n, order, with_ekf=2)                      # the second step in a call of its own
    ctx.sync()
    prof = ctx.profile_get()
    chain = "fast" if cap <= 24 else "mid" if cap <= 64 else "general"
    assert ekf_kernels_run(prof) == CHAIN_KERNELS[chain] | {FINISH}
    assert prof[FINISH][0] == 3, "one finish launch per round"
    refused(E_STATE, ctx.get_track_health)
    health = ctx.fleet_get_health()
    assert health.size == R
    slots = ctx.get_slot_health(first, 3 * n)
    stats = ctx.get_slot_ekf_stats(first, 3 * n)
    for i, r in enumerate(order):
        rob = robots[r]
        # a single gated windows-off context on the same state, samples and lists: bit for bit
        one = context(cap, ML, batch=3, windows=False)
        one.set_slam_gate(gate_d2=GATE)
        one.set_state(rob["mu"], rob["S"], rob["ids"])
        one.stage_encoders([0.0] + [f[0] for f in rob["frames"]], [0.0] + [f[1] for f in rob["frames"]], [0.0] + [f[2] for f in rob["frames"]])
        one.inject_observations(0, *no_obs())
        for f in range(2):
            inject(one, 1 + f, rob["frames"][f][3])
        one.run_staged(0, 3, with_ekf=2)
        one.sync()
        mu_g, S_g = ctx.fleet_get_state(r)
        mu_1, S_1 = one.get_state()
        assert np.array_equal(mu_g, mu_1) and np.array_equal(S_g, S_1), f"robot {r}: fleet != single gated context"
        assert same_bytes(slots[i::n].copy(), one.get_slot_health(0, 3)) and np.array_equal(stats[i::n], one.get_slot_ekf_stats(0, 3))
        assert same_bytes(health[r], one.get_track_health()), f"robot {r}: track record"
        # the literal reference
        lit = literal_on(rob["mu"], rob["S"], rob["ids"])
        lit.add_encoder(0.0, 0.0, 0.0)
        lit.add_frame([])
        t = 0.0
        for f in range(2):
            t += rob["frames"][f][2]
            lit.add_encoder(rob["frames"][f][0], rob["frames"][f][1], t)
            lit.add_frame(rob["frames"][f][3])
            check_slot_health(slots[(1 + f) * n + i], lit.health, f"robot {r} frame {f}")
            assert stats[(1 + f) * n + i].tolist() == lit.stats
            if f == 0:
                check_track(mid_health[r], lit.track, f"robot {r} after the first call")
            want = {"empty": 0, "all": lit.health["attempted"], "none": 0, "third": len(outlier_positions("third", lit.health["attempted"]))}
            assert lit.health["rejected"] == want[rob["kind"]], "the reference alone does not separate the planted outliers"
        lit.assert_margins()
        check_track(health[r], lit.track, f"robot {r}")
        check_state((mu_g, S_g), lit, f"fleet cap {cap} robot {r} ({rob['kind']})")
    assert health[2]["bad_streak"] == 2 and health[3]["bad_streak"] == 0 and health[2]["rejected_total"] > 0
    for r in (1, 5):                                                            # bystanders keep their bits and an empty record
        mu_g, S_g = ctx.fleet_get_state(r)
        assert np.array_equal(mu_g, robots[r]["mu"]) and np.array_equal(S_g, robots[r]["S"]), f"bystander {r} changed"
        check_track(health[r], TRACK_ZERO, f"bystander {r}")
    # a seat clears its robot's record only
    ctx.fleet_set_state(2, robots[2]["mu"], robots[2]["S"], robots[2]["ids"])
    after = ctx.fleet_get_health()
    check_track(after[2], TRACK_ZERO, "fleet_set_state")
    assert all(same_bytes(after[r], health[r]) for r in range(R) if r != 2)
    assert list(ctx.fleet_remove_landmarks([int(robots[4]["ids"][0])], robots=[4])) == [1]
    after2 = ctx.fleet_get_health()
    check_track(after2[4], TRACK_ZERO, "fleet_remove_landmarks")
    assert all(same_bytes(after2[r], after[r]) for r in range(R) if r != 4)


@pytest.mark.parametrize("cap", [24, 64, 128])
def test_fleet_slam_rounds(cap):
    _fleet(cap)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [24, 64, 128])
def test_fleet_slam_rounds_on_gpu(cap):
    _fleet(cap)


# ---- rig SLAM ----------------------------------------------------------------------------------------------------------------------

def _rig_step():
    """one arming step and one step of two cameras; the record sits at max_batch + step"""
    rng = np.random.RandomState(3)
    L, batch = 12, 4
    mu, S = random_state(rng, L, heading=-0.7)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    obs = [(int(ids[i]), z + (OUTLIER if i in (2, 8) else 0.0), r)
           for i, z, r in observe(rng, mu, [0, 2, 3, 5, 8, 9, 11], post_predict=predicted_pose(mu, WL, WR, DT))]
    cam0, cam1 = obs[:3], obs[3:]
    ctx = context(24, L + 1, batch=batch)
    ctx.set_slam_gate(gate_d2=GATE)
    ctx.set_camera_rig([CAM, CAM])
    ctx.set_state(mu, S, ids)
    ctx.stage_encoders([0.0, 0.0, WL, WL], [0.0, 0.0, WR, WR], [0.0, 0.0, DT, DT])
    ctx.inject_observations(0, *no_obs())
    ctx.inject_observations(1, *no_obs())
    inject(ctx, 2, cam0)
    inject(ctx, 3, cam1)
    ctx.run_staged_rig(0, 2, with_ekf=2)
    ctx.sync()
    lit = literal_on(mu, S, ids)
    lit.add_encoder(0.0, 0.0, 0.0)
    lit.add_frame([])
    lit.add_encoder(WL, WR, DT)
    lit.add_frame(cam0 + cam1)
    lit.assert_margins()
    assert lit.health["rejected"] == 2 and lit.health["accepted"] == 5
    check_slot_health(ctx.get_slot_health(batch + 1, 1)[0], lit.health, "rig step 1")
    assert ctx.get_rig_step_ekf_stats(1, 1)[0].tolist() == lit.stats
    acts = ctx.get_rig_observations()[2]
    assert acts.tolist() == [a for _, _, a in lit.log]
    check_track(ctx.get_track_health(), lit.track, "rig")
    check_state(ctx.get_state(), lit, "rig step")


def test_rig_step():
    _rig_step()


@pytest.mark.gpu
def test_rig_step_on_gpu():
    _rig_step()


# ---- lost ------------------------------------------------------------------------------------------------------------------------

def _lost():
    """a filter whose pose was displaced by 1 m / 0.5 rad is lost after exactly lost_after bad frames; a one-correction frame leaves
    the streak; set_state clears the record"""
    rng = np.random.RandomState(8)
    L, lost_after = 10, 3
    mu, S = random_state(rng, L, heading=0.2)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    wrong = mu.copy()
    wrong[:3] += [0.8, 0.6, 0.5]                                # 1 m and 0.5 rad off
    gate = dict(min_attempted=2, min_accept_percent=50, lost_after=lost_after)
    nf = 6
    ctx = context(24, L, batch=nf)
    ctx.set_slam_gate(gate_d2=GATE, **gate)
    ctx.set_state(wrong, S, ids)
    lit = literal_on(wrong, S, ids, gate)
    true_pose = mu[:3].copy()
    sizes = [0, 5, 1, 5, 5, 5]                                  # arming; bad; one correction: the streak stays; bad; bad -> lost; bad
    ctx.stage_encoders([0.0] + [WL] * (nf - 1), [0.0] + [WR] * (nf - 1), [0.0] + [DT] * (nf - 1))
    t = 0.0
    for s, k in enumerate(sizes):
        if s:
            true_pose = predicted_pose(np.concatenate([true_pose, mu[3:]]), WL, WR, DT)
        seen = np.sort(rng.choice(L, k, replace=False))
        obs = [(int(ids[i]), z, r) for i, z, r in observe(rng, mu, seen, post_predict=true_pose)]
        inject(ctx, s, obs)
        ctx.run_staged(s, 1, with_ekf=2)
        lit.add_encoder(WL if s else 0.0, WR if s else 0.0, t)
        t += DT
        lit.add_frame(obs)
        tr = ctx.get_track_health()
        check_track(tr, lit.track, f"frame {s}")
        check_slot_health(ctx.get_slot_health(s, 1)[0], lit.health, f"frame {s}")
    lit.assert_margins()
    assert [lit.track["bad_streak"], lit.track["lost"]] == [4, 1]
    check_state(ctx.get_state(), lit, "lost filter")
    ctx.set_state(mu, S, ids)
    check_track(ctx.get_track_health(), TRACK_ZERO, "set_state")


def _lost_streak_by_frame():
    """the reference's streak alone, frame by frame: lost exactly when the third bad frame ends"""
    rng = np.random.RandomState(8)
    L = 10
    mu, S = random_state(rng, L, heading=0.2)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    wrong = mu.copy()
    wrong[:3] += [0.8, 0.6, 0.5]
    lit = literal_on(wrong, S, ids, dict(lost_after=3))
    true_pose, out, t = mu[:3].copy(), [], 0.0
    for s, k in enumerate([0, 5, 1, 5, 5, 5]):
        if s:
            true_pose = predicted_pose(np.concatenate([true_pose, mu[3:]]), WL, WR, DT)
        seen = np.sort(rng.choice(L, k, replace=False))
        lit.add_encoder(WL if s else 0.0, WR if s else 0.0, t)
        t += DT
        lit.add_frame([(int(ids[i]), z, r) for i, z, r in observe(rng, mu, seen, post_predict=true_pose)])
        out.append((lit.track["bad_streak"], lit.track["lost"]))
    return out


def test_lost_after_exactly_lost_after_bad_frames():
    assert _lost_streak_by_frame() == [(0, 0), (1, 0), (1, 0), (2, 0), (3, 1), (4, 1)]
    _lost()


@pytest.mark.gpu
def test_lost_on_gpu():
    _lost()


# ---- arguments and modes -----------------------------------------------------------------------------------------------------------

def _arguments_and_modes():
    ctx = context(24, 8, batch=4)
    assert ctx.get_slam_gate() is None
    for bad in (dict(gate_d2=0.0), dict(gate_d2=-1.0), dict(gate_d2=float("nan")), dict(gate_d2=-INF), dict(min_attempted=0),
                dict(min_accept_percent=-1), dict(min_accept_percent=101), dict(lost_after=0)):
        refused(E_INVALID, ctx.set_slam_gate, **bad)
        assert ctx.get_slam_gate() is None
    getters = ((ctx.get_slot_health, (0, 1)), (ctx.get_track_health, ()), (ctx.fleet_get_health, ()))
    for fn, a in getters:                                      # no gate at all
        refused(E_STATE, fn, *a)
    ctx.set_innovation_gate()                                  # only the localization gate: SLAM and fleet SLAM still refuse
    for fn, a in getters:
        refused(E_STATE, fn, *a)
    ctx.fleet_slam_begin([CAM] * 2)
    for fn, a in getters:
        refused(E_STATE, fn, *a)
    ctx.fleet_end()
    ctx.set_innovation_gate(None)
    ctx.set_slam_gate()
    assert ctx.get_slam_gate() == DEFAULTS and ctx.get_innovation_gate() is None
    ctx.set_slam_gate(gate_d2=INF, min_attempted=1, min_accept_percent=100, lost_after=7)
    assert ctx.get_slam_gate() == dict(gate_d2=INF, min_attempted=1, min_accept_percent=100, lost_after=7)
    assert ctx.get_slot_health(0, 8).size == 8 and ctx.get_track_health()["frames"] == 0      # slots [0, 2 max_batch)
    refused(E_STATE, ctx.fleet_get_health)
    refused(E_INVALID, ctx.get_slot_health, -1, 1)
    refused(E_INVALID, ctx.get_slot_health, 0, 0)
    refused(E_INVALID, ctx.get_slot_health, 7, 2)
    ctx.fleet_slam_begin([CAM] * 2)
    assert ctx.fleet_get_health().size == 2 and ctx.get_slot_health(0, 4).size == 4
    refused(E_STATE, ctx.get_track_health)
    ctx.fleet_end()
    # the localization modes: the SLAM gate alone makes nothing readable there
    ids = np.array([3, 7, 9], np.int32)
    xyth = np.array([[1.0, 0.0, 3.1], [0.0, 1.0, -1.5], [-1.0, -1.0, 0.7]])
    pose, sig = np.array([0.1, -0.2, 0.3]), np.diag([0.02, 0.03, 0.01])
    ctx.localize_begin(ids, xyth, pose, sig)
    for fn, a in getters:
        refused(E_STATE, fn, *a)
    ctx.localize_end()
    ctx.fleet_begin([CAM] * 2, ids, xyth, [pose] * 2, [sig] * 2)
    for fn, a in getters:
        refused(E_STATE, fn, *a)
    ctx.fleet_end()
    ctx.set_slam_gate(None)
    assert ctx.get_slam_gate() is None
    refused(E_STATE, ctx.get_slot_health, 0, 1)


def _localization_ignores_the_slam_gate():
    """localization and fleet localization results keep their bits with the SLAM gate set"""
    rng = np.random.RandomState(2)
    L = 6
    mu, _ = random_state(rng, L, heading=0.3)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    xyth = mu[3:].reshape(-1, 3)
    pose, sig = mu[:3], np.diag([0.02, 0.03, 0.01])
    at = predicted_pose(mu, WL, WR, DT)
    frames = [[(int(ids[i]), z + (OUTLIER if i == 2 else 0.0), r) for i, z, r in observe(rng, mu, range(L), post_predict=at)] for _ in range(3)]

    def run(gated, fleet):
        ctx = context(24, L, batch=3)
        if gated:
            ctx.set_slam_gate(gate_d2=GATE)
        if fleet:
            ctx.fleet_begin([CAM] * 2, ids, xyth, [pose] * 2, [sig] * 2)
        else:
            ctx.localize_begin(ids, xyth, pose, sig)
        ctx.stage_encoders([0.0, WL, 0.0], [0.0, WR, 0.0], [0.0, DT, 0.0])
        for s, f in enumerate(frames):
            inject(ctx, s, f)
        if fleet:
            ctx.fleet_run_staged(0, [1, 1, 0], with_ekf=2)
            ctx.sync()
            return ctx.fleet_get_poses() + (ctx.get_slot_ekf_stats(0, 3),)
        ctx.run_staged(0, 3, with_ekf=2)
        return ctx.get_state() + ctx.get_observations() + (ctx.get_slot_ekf_stats(0, 3),)

    for fleet in (False, True):
        for x, y in zip(run(False, fleet), run(True, fleet)):
            assert np.array_equal(x, y, equal_nan=True), "the SLAM gate changed a localization result"


def _gate_off_runs_the_parent_kernels():
    """with the gate off (never set, or set and cleared) a SLAM step launches the ungated chain's kernels and nothing else"""
    case = frame_case(7, 9, 5, "third")
    for cleared in (False, True):
        ctx = context(24, 10, windows=False)
        if cleared:
            ctx.set_slam_gate(gate_d2=GATE)
            ctx.set_slam_gate(None)
        stage_case(ctx, case)
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.run_staged(0, 2, with_ekf=2)
        ctx.sync()
        assert ekf_kernels_run(ctx.profile_get()) == CHAIN_KERNELS["fast"]
        assert (ctx.get_observations()[2] == 1).all()


def test_arguments_and_modes():
    _arguments_and_modes()


def test_localization_ignores_the_slam_gate():
    _localization_ignores_the_slam_gate()


def test_gate_off_runs_the_parent_kernels():
    _gate_off_runs_the_parent_kernels()


@pytest.mark.gpu
def test_arguments_modes_and_switches_on_gpu():
    _arguments_and_modes()
    _localization_ignores_the_slam_gate()
    _gate_off_runs_the_parent_kernels()


# ---- the rendered small ring, on the GPU ------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_ring_fleet_records_equal_the_reference():
    """a 3-robot SLAM fleet on the rendered 240 x 320 ring, the default gate: every slot record and every track record equals the
    literal reference run on the slot's raw observations; prints the d2 quantiles over its corrections"""
    from test_fleet_slam import small_fleet
    w, cams, frames = small_fleet()
    cfg = w.cfg
    R, T = 3, min(len(frames), 10)
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=R * T, max_landmarks=w.L + 8, persistent_waves=4)
    synth.apply_detector(cfg, ctx=ctx)
    ctx.set_slam_gate()
    ctx.fleet_slam_begin(cams)
    robots = [r for t in range(T) for r in range(R)]
    ctx.stage_frames(np.stack([frames[t][r][0] for t in range(T) for r in range(R)]))
    ctx.stage_encoders(*[[getattr(frames[t][r][1], k) for t in range(T) for r in range(R)] for k in ("wl", "wr", "dt")])
    ctx.fleet_run_staged(0, robots)
    ctx.sync()
    slots, stats, health = ctx.get_slot_health(0, R * T), ctx.get_slot_ekf_stats(0, R * T), ctx.fleet_get_health()
    d2 = []
    for r in range(R):
        lit = GatedLiteralSlam()
        t_now = 0.0
        for t in range(T):
            fr = frames[t][r][1]
            t_now += fr.dt
            lit.add_encoder(fr.wl, fr.wr, t_now)
            ids, valid, xyth, Rd = ctx.get_slot_raw_observations(t * R + r)
            lit.add_frame([(int(i), z, rd) for i, v, z, rd in zip(ids, valid, xyth, Rd) if v])
            check_slot_health(slots[t * R + r], lit.health, f"robot {r} tick {t}")
            assert stats[t * R + r, 1:].tolist() == lit.stats[1:], f"robot {r} tick {t}: stats"      # ([0] counts the invalid ones too)
        lit.assert_margins()
        check_track(health[r], lit.track, f"robot {r}")
        mu_g, S_g = ctx.fleet_get_state(r)
        check_state((mu_g, S_g), lit, f"ring robot {r}")
        d2 += lit.d2_seen
    d2 = np.array(d2)
    assert d2.size >= 3 * T
    print(f"ring fleet: {d2.size} corrections, d2 quantiles 0.5 / 0.9 / 0.99 / max: "
          + " / ".join(f"{q:.3g}" for q in (*np.quantile(d2, [0.5, 0.9, 0.99]), d2.max())))
