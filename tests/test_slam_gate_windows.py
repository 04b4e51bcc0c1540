"""The SLAM gate inside EKF windows (aslam_set_slam_gate_windows) against the gated references of
tests/slam_gate_reference.py and against a gated per-frame twin (ASLAM_NO_WINDOWS + gate).

Inputs as in tests/test_slam_gate.py: random_state / observe of tests/ekf_reference.py (noise 0.03); an outlier is a true sighting
displaced by (2.7, -2.1, 0); gate_d2 = 1.0.  Before anything discrete is compared every case asserts on the CPU that the reference
alone separates the planted outliers from the true sightings, that no d2 lies within a relative 1e-6 of the gate and no ||ze|| within
1e-6 of 1, and that repeated sightings are either identical or far from the 0.01 "stationary" threshold.
Tolerances.  Window against the reference: mu rtol 1e-9 / atol 1e-11, Sigma 1e-9 relative, nis_sum and d2_max 1e-9 relative.  Window
against the per-frame twin: mu and Sigma 1e-10 relative, nis_sum and d2_max 1e-9 relative (floating-point sums cannot be bit-equal
across the two paths).  Everything discrete is exact: pop ids / indices / actions, slot stats, the integer fields of the health
records, track records, landmark ids.  Every case not marked gpu runs on the session's library (the emulation without a GPU)."""
import ctypes
import functools
import math

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from ekf_reference import CHAIN_KERNELS, ekf_kernels_run, observe, predicted_pose, random_state, rel_err
from slam_gate_reference import (DEFAULTS, OUTLIER, TRACK_ZERO, GatedLiteralSlam, check_slot_health, check_track)
from test_ekf_sizes import DT, ID_TABLE, WL, WR
from test_fleet_slam import no_windows_context

E_INVALID = -1
INF = float("inf")
GATE = 1.0
WIN_FINISH, FRAME_FINISH = "k_ekf_win_gate_finish", "k_ekf_gate_finish"
INT_FIELDS = ("attempted", "accepted", "rejected", "ref_flagged", "worst_id")
CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))


# ---- sequences and their reference ------------------------------------------------------------------------------------------------

def make_frames(rng, mu, ids, plan, nan=(), motions=None, params=None):
    """plan = per frame the landmark indices it sees, ascending (frame 0 arms the filter and sees nothing), outliers = set of (frame,
    position): frames = [[(id, z, Rdiag)]] in a random detection order; nan: (frame, position) whose z[0] is NaN.  motions: frame f's
    (wl, wr, dt) in place of (WL, WR, DT), params: the filter's Q_k, kl, kr, b in place of the defaults"""
    pose = mu[:3].copy()
    frames, marks = [], []
    prev = {}
    for f, (seen, out) in enumerate(plan):
        if f:
            pose = predicted_pose(np.concatenate([pose, mu[3:]]), *((WL, WR, DT) if motions is None else motions[f]),
                                  **{k: v for k, v in (params or {}).items() if k != "Q_k"})
        obs = []
        for k, i in enumerate(seen):
            while True:                                            # drawn again while it lies within 0.03 of the frame before's sighting
                _, z, r = observe(rng, mu, [i], post_predict=pose)[0]
                if i not in prev or not np.linalg.norm(prev[i] - z) <= 0.03:      # (a NaN predecessor never matches)
                    break
            z = z + OUTLIER if k in out else z
            if (f, k) in nan:
                z = z.copy()
                z[0] = math.nan
            obs.append((int(ids[i]), z, r))
        prev = {i: o[1] for i, o in zip(seen, obs)}
        marks.append([k in out or (f, k) in nan for k in range(len(obs))])
        frames.append([obs[i] for i in rng.permutation(len(obs))])
    return frames, marks


def assert_repeats_decidable(frames):
    """a sighting repeated from the frame before is either identical or far from the 0.01 threshold"""
    for a, b in zip(frames, frames[1:]):
        prev = {i: z for i, z, _ in a}
        for i, z, _ in b:
            if i in prev:
                d = float(np.linalg.norm(prev[i] - z))
                assert d == 0.0 or math.isnan(d) or d > 0.02, f"a repeated sighting {d} from its predecessor"


def reference(mu, S, ids, frames, gate=None, marks=None, motions=None, params=None, cls=GatedLiteralSlam):
    """GatedLiteralSlam over the frames (frame 0 arms): per frame its pop log, stats, slot record and the track record behind it.
    motions: frame f's (wl, wr, dt) in place of (WL, WR, DT); params: the transcription's Q_k, kl, kr, b"""
    lit = cls(gate=dict(gate_d2=GATE, **(gate or {})), **(params or {}))
    lit.seat(mu, S, ids)
    per = []
    for f, obs in enumerate(frames):
        lit.last_time = 0.0                                        # (every sample's dt is DT exactly)
        lit.add_encoder(*((0.0, 0.0, 0.0) if not f else (WL, WR, DT) if motions is None else motions[f]))
        lit.add_frame(obs)
        per.append(dict(log=list(lit.log), stats=list(lit.stats), health=dict(lit.health), track=dict(lit.track)))
        if marks is not None:                                      # the reference alone separates outliers from true sightings
            want = {i for (i, _, _), k in zip(sorted(obs, key=lambda o: lit.id_map[o[0]]), marks_by_index(obs, marks[f], lit)) if k}
            got = {i for i, _, a in lit.log if a == 3}
            assert got == want, f"frame {f}: the reference rejects {sorted(got)}, planted {sorted(want)}"
    lit.assert_margins()
    return lit, per


def marks_by_index(obs, marks_f, lit):
    """the frame's outlier marks (by generation position = ascending landmark index) in the order of sorted(obs) by landmark index"""
    return marks_f                                                 # make_frames generates in ascending index order


def plan_list(ctx):
    """[frames inside windows, frames on the per-frame chain, windows, frames left to the device's own plan]"""
    return list(ctx.plan_stats().values())


class Run:
    """a context on a sequence: state seated, every frame injected, run in the given batches"""

    def __init__(self, mu, S, ids, frames, batches=None, gate=GATE, switch=True, windows=True, cap=24, ML=None, gate_kw=None, rig=0,
                 motions=None, params=None):
        n = len(frames)
        kw = dict(max_rows=64, max_cols=64, max_batch=n * max(rig, 1), persistent_waves=4, max_landmarks=ML or len(ids), max_updates_per_frame=cap,
                  **(params or {}))
        ctx = capi.Context(**kw) if windows else no_windows_context(**kw)
        if gate is not None:
            ctx.set_slam_gate(gate_d2=gate, **(gate_kw or {}))
        if switch:
            ctx.set_slam_gate_windows(True)
        if rig:
            ctx.set_camera_rig([CAM] * rig)
        ctx.set_state(mu, S, ids)
        slots = n * max(rig, 1)
        enc = np.repeat(np.array([[0.0, 0.0, 0.0]] + ([[WL, WR, DT]] * (n - 1) if motions is None else [list(m) for m in motions[1:n]])),
                        max(rig, 1), axis=0)
        ctx.stage_encoders(enc[:, 0], enc[:, 1], enc[:, 2])
        for s, obs in enumerate(frames):
            cams = [obs] if not rig else [obs[c::rig] for c in range(rig)]
            for c, part in enumerate(cams):
                ctx.inject_observations(s * max(rig, 1) + c, [o[0] for o in part], [1] * len(part), np.array([o[1] for o in part]).reshape(-1, 3),
                                        np.array([o[2] for o in part]).reshape(-1, 3))
        ctx.profile_enable(True)
        ctx.profile_reset()
        self.ctx, self.n, self.rig, self.slots = ctx, n, rig, slots
        self.pops = {}                                             # last frame of every batch: its pop list
        for first, count in ([(0, n)] if batches is None else batches):
            self.step(first, count)

    def step(self, first, count):
        ctx = self.ctx
        if self.rig:
            ctx.run_staged_rig(first * self.rig, count, with_ekf=2)
        else:
            ctx.run_staged(first, count, with_ekf=2)
        ctx.sync()
        obs = ctx.get_rig_observations() if self.rig else ctx.get_observations()
        self.pops[first + count - 1] = np.stack([obs[0], obs[1], obs[2]], 1).reshape(-1, 3)

    def results(self):
        ctx = self.ctx
        base = self.slots if self.rig else 0                       # a rig step's EKF slot is max_batch + step
        stats = ctx.get_rig_step_ekf_stats(0, self.n) if self.rig else ctx.get_slot_ekf_stats(0, self.n)
        out = dict(state=ctx.get_state(), ids=ctx.get_landmark_ids(), stats=stats, prof=ctx.profile_get(), plan=plan_list(ctx))
        if ctx.get_slam_gate() is not None:
            out.update(health=ctx.get_slot_health(base, self.n), track=ctx.get_track_health())
        return out


def check_against_reference(run, lit, per, where):
    res = run.results()
    for f, pops in run.pops.items():
        assert np.array_equal(pops, np.array(per[f]["log"], np.int32).reshape(-1, 3)), f"{where}: frame {f} pops differ"
    for f in range(run.n):                                         # every frame's stats and slot record, not only the last
        assert res["stats"][f].tolist() == per[f]["stats"], f"{where}: frame {f} stats {res['stats'][f].tolist()} != {per[f]['stats']}"
        check_slot_health(res["health"][f], per[f]["health"], f"{where} frame {f}")
    check_track(res["track"], per[-1]["track"], where)
    mu_g, S_g = res["state"]
    assert mu_g.shape == lit.mu.shape and np.isfinite(mu_g).all() and np.isfinite(S_g).all(), f"{where}: state"
    e_mu, e_S = float(np.abs(mu_g - lit.mu).max()), rel_err(S_g, lit.sigma)
    print(f"{where}: against the reference |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert np.allclose(mu_g, lit.mu, rtol=1e-9, atol=1e-11), f"{where}: mu differs by {e_mu}"
    assert e_S <= 1e-9, f"{where}: Sigma differs by {e_S} (relative)"
    return res


def check_against_twin(res, twin, where):
    """a gated per-frame run of the same sequence: discrete results exact, mu and Sigma 1e-10, the two sums 1e-9"""
    two = twin.results()
    assert not any(k.startswith("k_ekf_win") and v[0] > 0 for k, v in two["prof"].items()), "the twin ran a window kernel"
    assert np.array_equal(res["stats"], two["stats"]) and np.array_equal(res["ids"], two["ids"]), f"{where}: stats / ids differ from the twin"
    for k in INT_FIELDS:
        assert np.array_equal(res["health"][k], two["health"][k]), f"{where}: {k} differs from the twin"
    for k in ("nis_sum", "d2_max"):
        assert np.allclose(res["health"][k], two["health"][k], rtol=1e-9, atol=0.0), f"{where}: {k} differs from the twin"
    assert res["track"].tobytes() == two["track"].tobytes(), f"{where}: track record differs from the twin"
    (mu_w, S_w), (mu_t, S_t) = res["state"], two["state"]
    e_mu, e_S = float(np.abs(mu_w - mu_t).max() / np.abs(mu_t).max()), rel_err(S_w, S_t)
    print(f"{where}: against the per-frame twin mu {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert e_mu <= 1e-10 and e_S <= 1e-10, f"{where}: differs from the twin ({e_mu}, {e_S})"


# ---- 1. each width at its smallest shape --------------------------------------------------------------------------------------------

SHAPES = {4: dict(L=4, frames=6, cap=24, ML=4), 8: dict(L=25, frames=3, cap=64, ML=25), 12: dict(L=50, frames=3, cap=64, ML=55)}
PATTERNS = ("none", "frame", "first", "last", "pair", "third")


def pattern_outliers(pattern, K, m):
    """(window frame, pop position) of the outliers: none; all of one frame; the first correction of the window's first frame; the last
    of its last; two consecutive; every third correction of the window"""
    if pattern == "none":
        return set()
    if pattern == "frame":
        return {(1, a) for a in range(m)}
    if pattern == "first":
        return {(0, 0)}
    if pattern == "last":
        return {(K - 1, m - 1)}
    if pattern == "pair":
        return {(1, m // 2), (1, m // 2 + 1)}
    return {(j // m, j % m) for j in range(2, K * m, 3)}


@functools.lru_cache(maxsize=None)
def width_case(T, pattern, nan=()):
    sh = SHAPES[T]
    rng = np.random.RandomState(100 * T + PATTERNS.index(pattern) + 7 * len(nan))
    L, K = sh["L"], sh["frames"]
    mu, S = random_state(rng, L, heading=0.4)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    out = pattern_outliers(pattern, K, L)
    plan = [([], set())] + [(list(range(L)), {a for k, a in out if k == f}) for f in range(K)]
    frames, marks = make_frames(rng, mu, ids, plan, nan={(1 + k, a) for k, a in nan})
    assert_repeats_decidable(frames)
    lit, per = reference(mu, S, ids, frames, marks=marks)
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per, n_out=len(out) + len(nan))


def _width(T, pattern, nan=()):
    sh, c = SHAPES[T], width_case(T, pattern, nan)
    where = f"T {T} {pattern}" + (f" nan {nan}" if nan else "")
    run = Run(c["mu"], c["S"], c["ids"], c["frames"], cap=sh["cap"], ML=sh["ML"])
    res = check_against_reference(run, c["lit"], c["per"], where)
    assert int(res["health"]["rejected"].sum()) == c["n_out"]
    prof, K = res["prof"], sh["frames"]
    assert prof["k_ekf_win_step"][0] == 1 and prof[WIN_FINISH][0] == 1 and prof[FRAME_FINISH][0] == 1, f"{where}: ran {sorted(ekf_kernels_run(prof))}"
    assert res["plan"] == [K, 1, 1, 0]                    # the arming frame alone takes the per-frame chain
    twin = Run(c["mu"], c["S"], c["ids"], c["frames"], cap=sh["cap"], ML=sh["ML"], windows=False)
    check_against_twin(res, twin, where)
    return res


def test_shapes_select_the_three_widths():
    assert [3 + 3 * s["L"] <= 16 * T and (T == 4 or 3 + 3 * s["L"] > 16 * (T - 4)) for T, s in SHAPES.items()] == [True] * 3


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T", [4, 8, 12])
def test_gated_window_against_reference_and_twin(T, pattern):
    res = _width(T, pattern)
    # a frame whose corrections are all rejected is a lone predict in effect
    if pattern == "frame":
        assert res["stats"][2].tolist()[2] == 0 and res["health"][2]["accepted"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_widest_gated_window_on_gpu(pattern):
    _width(12, pattern)


# ---- 2. gate_d2 = inf: bit for bit the ungated window -------------------------------------------------------------------------------

def _monitor_only(T):
    sh, c = SHAPES[T], width_case(T, "third")
    got = []
    for gate in (None, INF):
        run = Run(c["mu"], c["S"], c["ids"], c["frames"], gate=gate, cap=sh["cap"], ML=sh["ML"])
        res = run.results()
        assert res["prof"]["k_ekf_win_step"][0] == 1 and res["prof"][WIN_FINISH][0] == (0 if gate is None else 1)
        got.append(res["state"] + (run.pops[run.n - 1], res["stats"], res["ids"]))
        if gate is not None:
            assert (res["health"]["rejected"] == 0).all() and c["n_out"] > 0
            assert res["health"]["attempted"].tolist() == [0] + [sh["L"]] * sh["frames"]
    for x, y in zip(*got):
        assert np.array_equal(x, y, equal_nan=True), f"T {T}: the gate at +inf changed a bit of the window's result"


@pytest.mark.parametrize("T", [4, 8, 12])
def test_monitor_only_window_keeps_every_bit(T):
    _monitor_only(T)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [4, 8, 12])
def test_monitor_only_window_keeps_every_bit_on_gpu(T):
    _monitor_only(T)


# ---- 3. a NaN z -------------------------------------------------------------------------------------------------------------------

NAN_AT = {"first_of_a_middle_frame": ((1, 0),), "last_of_the_window": ((2, 24),)}


@pytest.mark.parametrize("where", sorted(NAN_AT))
def test_nan_sighting_in_a_window_is_rejected(where):
    _width(8, "none", NAN_AT[where])


@pytest.mark.gpu
@pytest.mark.parametrize("where", sorted(NAN_AT))
def test_nan_sighting_in_a_window_is_rejected_on_gpu(where):
    _width(8, "none", NAN_AT[where])


# ---- 4. the planner rule ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planner_case(rejected):
    """frames 1..3 see landmarks 0..5; in frame 3 the sighting of X = landmark 2 is an outlier (rejected) or a true one (accepted);
    frame 4 repeats frame 3's sighting of X identically; frames 5..7 follow in a second batch, frame 5 repeating frame 4's accepted
    sighting of Y = landmark 4 identically (tested against an entry read back from the device)"""
    rng = np.random.RandomState(31 + rejected)
    L = 6
    mu, S = random_state(rng, L, heading=-0.3)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    plan = [([], set())] + [(list(range(L)), {2} if f == 3 and rejected else set()) for f in range(1, 8)]
    rs = np.random.RandomState(5)                                  # an order of our own, so that the repeats can be found again
    frames, marks = make_frames(rng, mu, ids, plan)
    by = lambda f, i: next(k for k, o in enumerate(frames[f]) if o[0] == int(ids[i]))
    frames[4][by(4, 2)] = frames[3][by(3, 2)]
    frames[5][by(5, 4)] = frames[4][by(4, 4)]
    marks[4][2] = bool(rejected)
    assert_repeats_decidable(frames)
    lit, per = reference(mu, S, ids, frames)
    act = lambda f, i: next(a for lid, _, a in per[f]["log"] if lid == int(ids[i]))
    assert act(3, 2) == (3 if rejected else 1) and act(4, 2) == (3 if rejected else 2), "the reference does not judge the repeat as planned"
    assert act(4, 4) == 1 and act(5, 4) == 2
    del rs
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per)


def _planner(rejected):
    c = planner_case(rejected)
    where = f"planner rule, predecessor {'rejected' if rejected else 'accepted'}"
    run = Run(c["mu"], c["S"], c["ids"], c["frames"], batches=[(0, 5)])
    plan = plan_list(run.ctx)
    # frames 1..3 in one window; frame 4 is undecidable on the host and left to the device
    assert plan == [3, 2, 1, 1], f"{where}: plan stats {plan}"
    prof = run.ctx.profile_get()
    assert prof["k_ekf_win_step"][0] == 1 and prof[WIN_FINISH][0] == 1 and prof[FRAME_FINISH][0] == 2
    x_act = [a for lid, _, a in run.pops[4].tolist() if lid == int(c["ids"][2])]
    assert x_act == [3 if rejected else 2], f"{where}: the repeat got action {x_act}"
    # the next batch reads the mirror back: its first frame's stationary repeat is tested against a confirmed entry and stays in its window
    run.step(5, 3)
    plan = plan_list(run.ctx)
    assert plan == [6, 2, 2, 1], f"{where}: plan stats after the second batch {plan}"
    res = check_against_reference(run, c["lit"], c["per"], where)
    assert res["stats"][5].tolist() == [6, 0, 5, 1] and res["prof"][WIN_FINISH][0] == 2


@pytest.mark.parametrize("rejected", [0, 1])
def test_planner_rule(rejected):
    _planner(rejected)


@pytest.mark.gpu
@pytest.mark.parametrize("rejected", [0, 1])
def test_planner_rule_on_gpu(rejected):
    _planner(rejected)


# ---- 5. window to window -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def two_window_case():
    rng = np.random.RandomState(52)
    L = 42
    mu, S = random_state(rng, L, heading=1.1)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    a, b = list(range(21)), list(range(21, 42))
    plan = [([], set()), (a, set()), (a, {5, 6}), (a, set()), (b, set()), (b, {0}), (b, {20})]
    frames, marks = make_frames(rng, mu, ids, plan)
    assert_repeats_decidable(frames)
    lit, per = reference(mu, S, ids, frames, marks=marks)
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per)


def _two_windows():
    c = two_window_case()
    run = Run(c["mu"], c["S"], c["ids"], c["frames"], cap=24, ML=42)
    res = check_against_reference(run, c["lit"], c["per"], "window to window")
    prof = res["prof"]
    assert res["plan"] == [6, 1, 2, 0] and prof["k_ekf_win_step"][0] == 2 and prof[WIN_FINISH][0] == 2
    assert prof["k_ekf_win_next"][0] == 1, "the second window did not start early from the first one's accumulators"
    assert res["health"]["rejected"].tolist() == [0, 0, 2, 0, 0, 1, 1]
    check_against_twin(res, Run(c["mu"], c["S"], c["ids"], c["frames"], cap=24, ML=42, windows=False), "window to window")


def test_window_to_window_under_the_gate():
    _two_windows()


@pytest.mark.gpu
def test_window_to_window_under_the_gate_on_gpu():
    _two_windows()


# ---- 6. a run longer than one window -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_case():
    rng = np.random.RandomState(6)
    L = 2
    mu, S = random_state(rng, L, heading=0.9)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    plan = [([], set())] + [([] if f == 33 else [1], {0} if f % 5 == 0 else set()) for f in range(1, 71)]
    frames, marks = make_frames(rng, mu, ids, plan)
    assert_repeats_decidable(frames)
    lit, per = reference(mu, S, ids, frames, marks=marks)
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per)


def _long_run():
    c = long_case()
    run = Run(c["mu"], c["S"], c["ids"], c["frames"])
    res = check_against_reference(run, c["lit"], c["per"], "70 frames")
    assert res["plan"] == [70, 1, 2, 0] and res["prof"][WIN_FINISH][0] == 2      # 64 frames, then 6
    assert res["track"]["rejected_total"] == 14 and res["track"]["frames"] == 71
    assert res["health"][33]["attempted"] == 0


def test_a_run_longer_than_one_window():
    _long_run()


@pytest.mark.gpu
def test_a_run_longer_than_one_window_on_gpu():
    _long_run()


# ---- 7. records: lost inside one window ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lost_case():
    """test_slam_gate's lost filter: a pose displaced by 1 m / 0.5 rad; frames of 5, 1, 5, 5, 5 sightings"""
    rng = np.random.RandomState(8)
    L = 10
    mu, S = random_state(rng, L, heading=0.2)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    wrong = mu.copy()
    wrong[:3] += [0.8, 0.6, 0.5]
    plan = [([], set())] + [(np.sort(rng.choice(L, k, replace=False)).tolist(), set()) for k in (5, 1, 5, 5, 5)]
    frames, _ = make_frames(rng, mu, ids, plan)
    assert_repeats_decidable(frames)
    gate = dict(min_attempted=2, min_accept_percent=50, lost_after=3)
    lit, per = reference(wrong, S, ids, frames, gate=gate)
    assert [(p["track"]["bad_streak"], p["track"]["lost"]) for p in per] == [(0, 0), (1, 0), (1, 0), (2, 0), (3, 1), (4, 1)]
    return dict(mu=mu, wrong=wrong, S=S, ids=ids, frames=frames, lit=lit, per=per, gate=gate)


def _lost_inside_a_window():
    c = lost_case()
    # one window of frames 1..4: lost exactly when its third bad frame ends; one frame less is not lost, and the next call goes on from there
    for last, want in ((4, (3, 1)), (3, (2, 0))):
        run = Run(c["wrong"], c["S"], c["ids"], c["frames"], batches=[(0, last + 1)], gate_kw=c["gate"])
        tr = run.ctx.get_track_health()
        assert plan_list(run.ctx) == [last, 1, 1, 0] and (int(tr["bad_streak"]), int(tr["lost"])) == want
        check_track(tr, c["per"][last]["track"], f"frames 0..{last}")
    run.step(4, 2)                                                 # frames 4, 5 as a window of their own: the record is carried into it
    assert plan_list(run.ctx) == [5, 1, 2, 0]
    check_against_reference(run, c["lit"], c["per"], "lost inside a window")
    run.ctx.set_state(c["mu"], c["S"], c["ids"])
    check_track(run.ctx.get_track_health(), TRACK_ZERO, "set_state")


def test_lost_inside_one_window_and_carried():
    _lost_inside_a_window()


@pytest.mark.gpu
def test_lost_inside_one_window_and_carried_on_gpu():
    _lost_inside_a_window()


# ---- 8. the switch and the modes -------------------------------------------------------------------------------------------------------

def _kernels(res):
    return ekf_kernels_run(res["prof"])


def _switch_and_modes(monkeypatch):
    c = width_case(4, "third")
    args = (c["mu"], c["S"], c["ids"], c["frames"])
    n = len(c["frames"])
    # default off: a gated context runs no window kernel
    off = Run(*args, switch=False)
    assert off.ctx.get_slam_gate_windows() is False
    r_off = off.results()
    assert _kernels(r_off) == CHAIN_KERNELS["fast"] | {FRAME_FINISH} and r_off["prof"][FRAME_FINISH][0] == n
    # on without a gate: the ungated window's kernels and bits
    plain, on = Run(*args, gate=None, switch=False).results(), Run(*args, gate=None).results()
    assert _kernels(on) == _kernels(plain) and WIN_FINISH not in _kernels(on) and on["prof"]["k_ekf_win_step"][0] == 1
    for x, y in zip(plain["state"] + (plain["stats"],), on["state"] + (on["stats"],)):
        assert np.array_equal(x, y)
    # on, but no windows or the piece schedule: the per-frame path
    r_nw = Run(*args, windows=False).results()
    monkeypatch.setenv("ASLAM_WIN_PIECE", "8")
    r_pc = Run(*args).results()
    monkeypatch.delenv("ASLAM_WIN_PIECE")
    for r in (r_nw, r_pc):
        assert _kernels(r) == CHAIN_KERNELS["fast"] | {FRAME_FINISH} and r["prof"][FRAME_FINISH][0] == n
        for x, y in zip(r_off["state"] + (r_off["stats"],), r["state"] + (r["stats"],)):
            assert np.array_equal(x, y)
        assert r["health"].tobytes() == r_off["health"].tobytes() and r["track"].tobytes() == r_off["track"].tobytes()
    # round trip, in any mode, persistent
    ctx = off.ctx
    for v in (True, False, True):
        ctx.set_slam_gate_windows(v)
        assert ctx.get_slam_gate_windows() is v
    ctx.fleet_slam_begin([CAM] * 2)
    assert ctx.get_slam_gate_windows() is True
    ctx.set_slam_gate_windows(False)
    ctx.fleet_end()
    assert ctx.get_slam_gate_windows() is False
    # argument errors
    lib = ctx.lib
    on_flag = ctypes.c_int(7)
    assert lib.aslam_set_slam_gate_windows(None, 1) == E_INVALID
    assert lib.aslam_get_slam_gate_windows(None, ctypes.byref(on_flag)) == E_INVALID
    assert lib.aslam_get_slam_gate_windows(ctx.h, None) == E_INVALID and on_flag.value == 7


def _setter_finalises_a_pending_batch():
    """a batch submitted with the switch on keeps its windows when the switch is cleared before anything waited for it"""
    c = width_case(4, "third")
    args = (c["mu"], c["S"], c["ids"], c["frames"])
    n = len(c["frames"])
    got = []
    for wait in (True, False):
        run = Run(*args, batches=[])
        run.ctx.run_staged(0, 4, with_ekf=2)                       # deferred: enqueued by the next call
        if wait:
            run.ctx.sync()
        run.ctx.set_slam_gate_windows(False)
        run.ctx.run_staged(4, n - 4, with_ekf=2)                   # the per-frame path
        run.ctx.sync()
        res = run.results()
        assert res["plan"] == [3, 1 + n - 4, 1, 0] and res["prof"][WIN_FINISH][0] == 1 and res["prof"][FRAME_FINISH][0] == 1 + n - 4
        got.append(res)
    a, b = got
    for x, y in zip(a["state"] + (a["stats"],), b["state"] + (b["stats"],)):
        assert np.array_equal(x, y)
    assert a["health"].tobytes() == b["health"].tobytes() and a["track"].tobytes() == b["track"].tobytes()
    for f in range(n):
        check_slot_health(a["health"][f], c["per"][f]["health"], f"frame {f}")
    check_track(a["track"], c["per"][-1]["track"], "switch cleared behind a pending batch")


def _other_modes_are_unaffected():
    """localization, fleet localization and fleet SLAM results keep their bits with the gate and the switch set"""
    rng = np.random.RandomState(2)
    L = 6
    mu, S = random_state(rng, L, heading=0.3)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    xyth = mu[3:].reshape(-1, 3)
    pose, sig = mu[:3], np.diag([0.02, 0.03, 0.01])
    at = predicted_pose(mu, WL, WR, DT)
    frames = [[(int(ids[i]), z + (OUTLIER if i == 2 else 0.0), r) for i, z, r in observe(rng, mu, range(L), post_predict=at)] for _ in range(3)]

    def run(switch, mode):
        ctx = capi.Context(max_rows=64, max_cols=64, max_batch=3, persistent_waves=4, max_landmarks=L, max_updates_per_frame=24)
        ctx.set_slam_gate(gate_d2=GATE)
        if switch:
            ctx.set_slam_gate_windows(True)
        if mode == "fleet":
            ctx.fleet_begin([CAM] * 2, ids, xyth, [pose] * 2, [sig] * 2)
        elif mode == "fleet_slam":
            ctx.fleet_slam_begin([CAM] * 2)
            for r in range(2):
                ctx.fleet_set_state(r, mu, S, ids)
        else:
            ctx.localize_begin(ids, xyth, pose, sig)
        ctx.stage_encoders([0.0, WL, 0.0], [0.0, WR, 0.0], [0.0, DT, 0.0])
        for s, f in enumerate(frames):
            ctx.inject_observations(s, [o[0] for o in f], [1] * len(f), np.array([o[1] for o in f]), np.array([o[2] for o in f]))
        if mode == "localize":
            ctx.run_staged(0, 3, with_ekf=2)
            return ctx.get_state() + ctx.get_observations() + (ctx.get_slot_ekf_stats(0, 3),)
        ctx.fleet_run_staged(0, [1, 1, 0], with_ekf=2)
        ctx.sync()
        if mode == "fleet":
            return ctx.fleet_get_poses() + (ctx.get_slot_ekf_stats(0, 3),)
        prof = ctx.profile_get()
        assert not any(k.startswith("k_ekf_win") and v[0] > 0 for k, v in prof.items())
        return ctx.fleet_get_state(0) + ctx.fleet_get_state(1) + (ctx.get_slot_ekf_stats(0, 3), ctx.get_slot_health(0, 3).view(np.uint8))

    for mode in ("localize", "fleet", "fleet_slam"):
        for x, y in zip(run(False, mode), run(True, mode)):
            assert np.array_equal(x, y, equal_nan=True), f"{mode}: the switch changed a result"


def test_switch_and_modes(monkeypatch):
    _switch_and_modes(monkeypatch)


def test_setter_finalises_a_pending_batch():
    _setter_finalises_a_pending_batch()


def test_other_modes_are_unaffected():
    _other_modes_are_unaffected()


@pytest.mark.gpu
def test_switch_modes_and_pending_batch_on_gpu(monkeypatch):
    _switch_and_modes(monkeypatch)
    _setter_finalises_a_pending_batch()
    _other_modes_are_unaffected()


# ---- 9. one rig sequence ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rig_case():
    rng = np.random.RandomState(9)
    L = 12
    mu, S = random_state(rng, L, heading=-0.7)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    seen = [0, 2, 3, 5, 8, 9, 11]
    plan = [([], set()), (seen, set()), (seen, {4}), (seen, set())]
    frames, marks = make_frames(rng, mu, ids, plan)
    assert_repeats_decidable(frames)
    # camera c of a step gets the step's observations c, c + 2, ...: the merged list is camera 0's, then camera 1's
    merged = [f[0::2] + f[1::2] for f in frames]
    lit, per = reference(mu, S, ids, merged, marks=marks)
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per)


def _rig():
    c = rig_case()
    run = Run(c["mu"], c["S"], c["ids"], c["frames"], rig=2, ML=13)
    res = check_against_reference(run, c["lit"], c["per"], "rig steps")     # (slot records read at max_batch + step)
    assert res["plan"] == [3, 1, 1, 0] and res["prof"][WIN_FINISH][0] == 1
    assert res["health"]["rejected"].tolist() == [0, 0, 1, 0]
    assert (run.ctx.get_slot_health(0, run.slots)["attempted"] == 0).all(), "a rig step's record landed in a frame slot"


def test_rig_steps_in_a_gated_window():
    _rig()


@pytest.mark.gpu
def test_rig_steps_in_a_gated_window_on_gpu():
    _rig()


# ---- 10. the rendered small ring, on the GPU -----------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_ring_lap_equals_the_per_frame_twin():
    """one robot, one lap of the rendered 240 x 320 ring in batches of 8, the default gate with the switch on, against the gated per-frame
    twin on the same raw observations"""
    from test_fleet import render_fleet, ring_cams
    from test_localize import small_ring
    w = synth.RingWorld(small_ring())
    cfg = w.cfg
    cam = ring_cams(w, [260.0], [(0.12, 0.02, 0.0)])[0]
    B, lap = 8, w.lap_length()
    kw = dict(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=B, max_landmarks=w.L + 8, persistent_waves=4)
    win, twin = capi.Context(**kw), no_windows_context(**kw)
    for ctx in (win, twin):
        synth.apply_detector(cfg, ctx=ctx)
        ctx.set_camera(cam[0], cam[1])
        ctx.set_slam_gate()
    win.set_slam_gate_windows(True)
    win.profile_enable(True)
    win.profile_reset()
    n_rej = 0
    for t0 in range(0, lap, B):
        nt = min(B, lap - t0)
        frames = render_fleet(win, w, [cam], [0], nt, t0)
        enc = [[getattr(frames[t][0][1], k) for t in range(nt)] for k in ("wl", "wr", "dt")]
        win.stage_frames(np.stack([frames[t][0][0] for t in range(nt)]))
        win.stage_encoders(*enc)
        win.run_staged(0, nt)
        win.sync()
        twin.stage_encoders(*enc)
        for s in range(nt):
            twin.inject_observations(s, *win.get_slot_raw_observations(s))
        twin.run_staged(0, nt, with_ekf=2)
        twin.sync()
        hw, ht = win.get_slot_health(0, nt), twin.get_slot_health(0, nt)
        for k in INT_FIELDS:
            assert np.array_equal(hw[k], ht[k]), f"ticks {t0}..: {k} differs from the twin"
        for k in ("nis_sum", "d2_max"):
            assert np.allclose(hw[k], ht[k], rtol=1e-9, atol=0.0), f"ticks {t0}..: {k} differs from the twin"
        assert np.array_equal(win.get_slot_ekf_stats(0, nt)[:, 1:], twin.get_slot_ekf_stats(0, nt)[:, 1:])
        for x, y in zip(win.get_observations()[:3], twin.get_observations()[:3]):
            assert np.array_equal(x, y), f"ticks {t0}..: pops differ from the twin"
        n_rej += int(hw["rejected"].sum())
    assert win.get_track_health().tobytes() == twin.get_track_health().tobytes()
    assert np.array_equal(win.get_landmark_ids(), twin.get_landmark_ids())
    plan, prof = plan_list(win), win.profile_get()
    assert plan[2] > 0 and prof[WIN_FINISH][0] == plan[2] and prof["k_ekf_win_step"][0] == plan[2], f"no gated window on the ring: {plan}"
    (mu_w, S_w), (mu_t, S_t) = win.get_state(), twin.get_state()
    e_mu, e_S = float(np.abs(mu_w - mu_t).max() / np.abs(mu_t).max()), rel_err(S_w, S_t)
    print(f"ring lap: {lap} frames, plan {plan}, {n_rej} rejected, against the twin mu {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert e_mu <= 1e-10 and e_S <= 1e-10
