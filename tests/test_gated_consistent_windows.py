"""The SLAM gate on the running innovation inside EKF windows (aslam_set_gated_consistent_windows): with a SLAM gate,
consistent innovations and both window switches on, the new switch keeps a staged batch's windows, and the gated one-launch chain
judges and applies e_i = ze_i - H_i (mu_{i-1} - mu_0).

References: consistent_reference.ConsistentLiteral (the literal transcription with the gate, the records and e in place of ze) through
test_slam_gate_windows.reference(..., cls=ConsistentLiteral), consistent_reference.consistent_step in long double where a case needs e
itself, and the per-frame gated consistent twin (ASLAM_NO_WINDOWS, the same switches).  Inputs as in tests/test_slam_gate_windows.py
(make_frames: noise 0.03, an outlier is a true sighting displaced by (2.7, -2.1, 0); gate_d2 = 1.0 unless the case says otherwise).
Before any device comparison every case asserts on the CPU reference alone that no d2 lies within a relative 1e-6 of the gate, no
||ze|| within 1e-6 of 1 (reference() asserts both), that repeated sightings are decidable and that the planted outliers are exactly
what the reference rejects.
Tolerances, the project's.  Against the reference: mu rtol 1e-9 / atol 1e-11, Sigma 1e-9 relative, nis_sum and d2_max 1e-9 relative.
Against the twin: mu and Sigma 1e-10 relative, the two sums 1e-9.  Everything discrete is exact.  Every case not marked gpu runs on the
session's library (the emulation without a GPU)."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import test_slam_gate_windows as gw
from aruco_slam_amd import capi, synth
from consistent_reference import ConsistentLiteral, _linearise, consistent_step
from ekf_reference import CHAIN_KERNELS, LD, ekf_kernels_run, random_state
from slam_gate_reference import GatedLiteralSlam, assert_margins, check_slot_health, check_track
from test_consistent_windows import CRun, bits, launches
from test_ekf_sizes import DT, ID_TABLE, WL, WR

E_INVALID = -1
INF, GATE = gw.INF, gw.GATE
WIN_FINISH, FRAME_FINISH = gw.WIN_FINISH, gw.FRAME_FINISH


class GRun(CRun):
    """CRun (gw.Run with the two consistent switches set before the first call) with a gate, the gate's window switch and the new switch"""

    def __init__(self, *a, gcw=True, **kw):
        self._gcw = gcw
        kw.setdefault("gate", GATE)
        kw.setdefault("switch", True)
        super().__init__(*a, **kw)

    def arm(self):
        if not self._armed:
            self.ctx.set_gated_consistent_windows(self._gcw)
        super().arm()


def reference(mu, S, ids, frames, marks=None, gate_d2=GATE, cls=ConsistentLiteral, motions=None):
    """gw.reference(..., cls=ConsistentLiteral) at gate 1.0; at another gate_d2 (gw.reference fixes it) the same loop: per frame the
    pop log, stats, slot record and the track record behind it, the margins asserted"""
    if gate_d2 == GATE:
        return gw.reference(mu, S, ids, frames, marks=marks, cls=cls, motions=motions)
    assert marks is None and motions is None
    lit = cls(gate=dict(gate_d2=gate_d2))
    lit.seat(mu, S, ids)
    per = []
    for f, obs in enumerate(frames):
        lit.last_time = 0.0
        lit.add_encoder(*((WL, WR, DT) if f else (0.0, 0.0, 0.0)))
        lit.add_frame(obs)
        per.append(dict(log=list(lit.log), stats=list(lit.stats), health=dict(lit.health), track=dict(lit.track)))
    lit.assert_margins()
    return lit, per


def window_launches(res, windows=1):
    prof = res["prof"]
    assert prof["k_ekf_win_step"][0] == windows and prof[WIN_FINISH][0] == windows, f"ran {launches(prof)}"


# ---- 1. three widths x six outlier patterns; 4. NaN sightings --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def width_case(T, pattern, nan=(), gate=GATE):
    """gw.width_case (the same draw) under the consistent reference"""
    sh = gw.SHAPES[T]
    rng = np.random.RandomState(100 * T + gw.PATTERNS.index(pattern) + 7 * len(nan))
    L, K = sh["L"], sh["frames"]
    mu, S = random_state(rng, L, heading=0.4)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    out = gw.pattern_outliers(pattern, K, L)
    plan = [([], set())] + [(list(range(L)), {a for k, a in out if k == f}) for f in range(K)]
    frames, marks = gw.make_frames(rng, mu, ids, plan, nan={(1 + k, a) for k, a in nan})
    gw.assert_repeats_decidable(frames)
    lit, per = reference(mu, S, ids, frames, marks=marks if math.isfinite(gate) else None, gate_d2=gate)
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per, n_out=len(out) + len(nan))


def _width(T, pattern, nan=()):
    sh, c = gw.SHAPES[T], width_case(T, pattern, nan)
    where = f"T {T} {pattern}" + (f" nan {nan}" if nan else "")
    args, kw = (c["mu"], c["S"], c["ids"], c["frames"]), dict(cap=sh["cap"], ML=sh["ML"])
    run = GRun(*args, **kw)
    res = gw.check_against_reference(run, c["lit"], c["per"], where)
    assert int(res["health"]["rejected"].sum()) == c["n_out"]
    assert res["plan"] == [sh["frames"], 1, 1, 0], f"{where}: plan {res['plan']}"      # the arming frame alone takes the per-frame chain
    window_launches(res)
    assert res["prof"][FRAME_FINISH][0] == 1
    gw.check_against_twin(res, GRun(*args, windows=False, **kw), where)
    return res


@pytest.mark.parametrize("pattern", gw.PATTERNS)
@pytest.mark.parametrize("T", [4, 8, 12])
def test_gated_consistent_window_against_reference_and_twin(T, pattern):
    res = _width(T, pattern)
    if pattern == "frame":                                         # a frame whose corrections are all rejected is a lone predict in effect
        assert res["stats"][2].tolist()[2] == 0 and res["health"][2]["accepted"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", gw.PATTERNS)
def test_widest_gated_consistent_window_on_gpu(pattern):
    _width(12, pattern)


def nan_positions(T):
    """the first, a middle and the last correction of the window: (window frame, pop position)"""
    L, K = gw.SHAPES[T]["L"], gw.SHAPES[T]["frames"]
    return {"first": ((0, 0),), "middle": ((K // 2, L // 2),), "last": ((K - 1, L - 1),)}


@pytest.mark.parametrize("at", ["first", "middle", "last"])
@pytest.mark.parametrize("T", [4, 12])
def test_nan_sighting_is_rejected_and_spreads_nowhere(T, at):
    res = _width(T, "none", nan_positions(T)[at])                  # (check_against_reference asserts a finite state)
    k, a = nan_positions(T)[at][0]
    h = res["health"][1 + k]
    assert h["rejected"] == 1 and np.isfinite(h["nis_sum"]) and np.isfinite(h["d2_max"])


@pytest.mark.gpu
@pytest.mark.parametrize("at", ["first", "middle", "last"])
def test_nan_sighting_is_rejected_and_spreads_nowhere_on_gpu(at):
    _width(12, "none", nan_positions(12)[at])


# ---- 2. the verdict is on e, not on ze ----------------------------------------------------------------------------------------------------
# All-true sightings.  The reference at gate +inf, once consistent and once frozen: the first-frame correction whose two d2 differ most
# (relatively) gives the gate, their geometric mean, so that the two filters part at that correction at the latest.  Asserted on the
# reference alone: the two rejection lists differ, the margins hold.

@functools.lru_cache(maxsize=None)
def verdict_case(T):
    sh = gw.SHAPES[T]
    L, K = sh["L"], sh["frames"]
    rng = np.random.RandomState(100 * T + 3)
    mu, S = random_state(rng, L, heading=0.4)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    frames, _ = gw.make_frames(rng, mu, ids, [([], set())] + [(list(range(L)), set())] * K)
    gw.assert_repeats_decidable(frames)
    lc, _ = reference(mu, S, ids, frames, gate_d2=INF)
    lf, _ = reference(mu, S, ids, frames, gate_d2=INF, cls=GatedLiteralSlam)
    dc, df = np.array(lc.d2_seen[:L]), np.array(lf.d2_seen[:L])
    a = int(np.argmax(np.abs(np.log(dc / df))))
    gate = float(np.sqrt(dc[a] * df[a]))
    lit, per = reference(mu, S, ids, frames, gate_d2=gate)                                # (asserts its margins)
    frozen, per_f = reference(mu, S, ids, frames, gate_d2=gate, cls=GatedLiteralSlam)
    rej = lambda p: [[i for i, _, act in f["log"] if act == 3] for f in p]
    assert rej(per) != rej(per_f), f"T {T}: gate {gate} does not tell e from ze"
    print(f"T {T}: gate {gate:.6g}, rejections per frame {[len(r) for r in rej(per)]} (e) against {[len(r) for r in rej(per_f)]} (ze)")
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per, gate=gate)


def _verdict(T):
    sh, c = gw.SHAPES[T], verdict_case(T)
    args, kw = (c["mu"], c["S"], c["ids"], c["frames"]), dict(cap=sh["cap"], ML=sh["ML"], gate=c["gate"])
    run = GRun(*args, **kw)
    res = gw.check_against_reference(run, c["lit"], c["per"], f"verdict on e, T {T}")
    assert res["plan"] == [sh["frames"], 1, 1, 0]
    window_launches(res)
    gw.check_against_twin(res, GRun(*args, windows=False, **kw), f"verdict on e, T {T}")


@pytest.mark.parametrize("T", [4, 8, 12])
def test_the_verdict_is_on_e(T):
    _verdict(T)


@pytest.mark.gpu
def test_the_verdict_is_on_e_on_gpu():
    _verdict(12)


# ---- 3. ref_flagged is on ze ----------------------------------------------------------------------------------------------------------------
# One frame sees every landmark (an empty frame at rest behind it, so that the planner makes a window of the two) from a seated pose displaced by (1.3, -0.4, 0) with diag(4, 4, 0) added to Sigma_xx: every ||ze|| >= 1,
# the first correction pulls the pose back, so ||e|| >= 1 for the first correction only, and the wide Sigma keeps every d2 under the gate.

@functools.lru_cache(maxsize=None)
def flag_case(T):
    sh = gw.SHAPES[T]
    L = sh["L"]
    rng = np.random.RandomState(100 * T + 5)
    mu, S = random_state(rng, L, heading=0.4)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    motions = [None, (WL, WR, DT), (0.0, 0.0, DT)]
    frames, _ = gw.make_frames(rng, mu, ids, [([], set()), (list(range(L)), set()), ([], set())], motions=motions)
    off, wide = mu.copy(), S.copy()
    off[:3] += [1.3, -0.4, 0.0]
    wide[0, 0] += 4.0
    wide[1, 1] += 4.0
    lit, per = reference(off, wide, ids, frames, motions=motions)
    # e of every correction, from the long-double step on the prefixes of the frame's pop order (ascending landmark index)
    index = {int(i): k for k, i in enumerate(ids)}
    fused = sorted(((index[i], z, r) for i, z, r in frames[1]), key=lambda o: o[0])
    mu0 = consistent_step(off, wide, WL, WR, DT, [])[2]["mu0"]
    e_norm = []
    for a, (k, z, _) in enumerate(fused):
        mu_a = consistent_step(off, wide, WL, WR, DT, fused[:a])[0]
        ze, G, cols = _linearise(mu0, k, z, LD)
        e_norm.append(float(np.linalg.norm(ze - G @ (mu_a[cols] - mu0[cols]))))
    norms, d2 = lit.norms_seen, lit.d2_seen
    assert len(norms) == L and min(norms) >= 1.0, f"T {T}: ||ze|| {min(norms)}"
    assert e_norm[0] >= 1.0 and max(e_norm[1:]) < 1.0, f"T {T}: ||e|| {e_norm[:3]}"
    assert max(d2) < GATE and per[1]["health"]["rejected"] == 0 and per[1]["health"]["ref_flagged"] == L
    assert_margins(GATE, d2, norms + e_norm, rel=1e-6)
    print(f"T {T}: ||ze|| >= {min(norms):.3g}, ||e|| {e_norm[0]:.3g} then <= {max(e_norm[1:]):.3g}, d2 <= {max(d2):.3g}")
    return dict(mu=off, S=wide, ids=ids, frames=frames, lit=lit, per=per, motions=motions)


def _flag(T):
    sh, c = gw.SHAPES[T], flag_case(T)
    run = GRun(c["mu"], c["S"], c["ids"], c["frames"], cap=sh["cap"], ML=sh["ML"], motions=c["motions"])
    res = gw.check_against_reference(run, c["lit"], c["per"], f"ref_flagged on ze, T {T}")
    assert res["plan"] == [2, 1, 1, 0]
    window_launches(res)
    h = res["health"][1]
    assert h["ref_flagged"] == sh["L"] and h["accepted"] == sh["L"] and h["rejected"] == 0


@pytest.mark.parametrize("T", [4, 8, 12])
def test_ref_flagged_is_on_ze(T):
    _flag(T)


@pytest.mark.gpu
def test_ref_flagged_is_on_ze_on_gpu():
    _flag(12)


# ---- 5. the gate at +inf: bit for bit the ungated consistent window -------------------------------------------------------------------------

def _monitor_only(T):
    sh, c = gw.SHAPES[T], width_case(T, "third", gate=INF)
    args, kw = (c["mu"], c["S"], c["ids"], c["frames"]), dict(cap=sh["cap"], ML=sh["ML"])
    plain_run, run = CRun(*args, **kw), GRun(*args, gate=INF, **kw)
    plain, res = plain_run.results(), run.results()
    assert plain["prof"]["k_ekf_win_step"][0] == 1 and plain["prof"][WIN_FINISH][0] == 0 and plain["plan"] == res["plan"] == [sh["frames"], 1, 1, 0]
    window_launches(res)
    assert np.array_equal(plain["state"][0], res["state"][0]), f"T {T}: the gate at +inf changed a bit of mu"
    assert bits(plain, plain_run) == bits(res, run), f"T {T}: the gate at +inf changed a bit of Sigma, the ids, the pops or the slot statistics"
    # the records: nothing rejected, nis_sum from e
    assert (res["health"]["rejected"] == 0).all() and c["n_out"] > 0
    for f in range(run.n):
        check_slot_health(res["health"][f], c["per"][f]["health"], f"T {T} frame {f}")
    check_track(res["track"], c["per"][-1]["track"], f"T {T}")
    frozen, _ = reference(*args, gate_d2=INF, cls=GatedLiteralSlam)
    assert abs(frozen.health["nis_sum"] - c["per"][-1]["health"]["nis_sum"]) > 1e-6 * frozen.health["nis_sum"], "nis_sum does not tell e from ze"


@pytest.mark.parametrize("T", [4, 8, 12])
def test_gate_at_infinity_is_the_ungated_consistent_window(T):
    _monitor_only(T)


@pytest.mark.gpu
def test_gate_at_infinity_is_the_ungated_consistent_window_on_gpu():
    _monitor_only(12)


# ---- 6. mu_R and the hand-overs -------------------------------------------------------------------------------------------------------------
# large_state: 30 landmarks, 4 of them in the window's set, one of the four rejected in every frame: the 26 means outside move through
# psi, from the accepted steps only.  three_windows: three batches, a window each, handed over.  empty_frames: a window with an empty
# frame at its start, in its middle and at its end.  single: m = 1 frames, one of them rejected.

SEQUENCES = {
    "large_state": dict(L=30, seed=61, plan=[([3, 11, 18, 27], {f % 4}) for f in range(4)], batches=[(0, 5)], windows=1),
    "three_windows": dict(L=6, seed=62, plan=[(list(range(6)), {f} if f % 2 else set()) for f in range(9)], batches=[(0, 4), (4, 3), (7, 3)], windows=3),
    "empty_frames": dict(L=5, seed=63, plan=[([], set()), (list(range(5)), {1}), ([], set()), (list(range(5)), set()), ([], set())],
                         batches=[(0, 6)], windows=1),
    "single": dict(L=4, seed=64, plan=[([2], {0} if f == 2 else set()) for f in range(5)], batches=[(0, 6)], windows=1),
}


@functools.lru_cache(maxsize=None)
def sequence_case(name):
    q = SEQUENCES[name]
    rng = np.random.RandomState(q["seed"])
    mu, S = random_state(rng, q["L"], heading=-0.2)
    ids = rng.permutation(ID_TABLE)[:q["L"]].astype(np.int32)
    frames, marks = gw.make_frames(rng, mu, ids, [([], set())] + q["plan"])
    gw.assert_repeats_decidable(frames)
    lit, per = reference(mu, S, ids, frames, marks=marks)
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per)


def _sequence(name):
    q, c = SEQUENCES[name], sequence_case(name)
    args, kw = (c["mu"], c["S"], c["ids"], c["frames"]), dict(ML=q["L"], batches=[])
    run, twin = GRun(*args, **kw), GRun(*args, windows=False, **kw)
    for first, count in q["batches"]:                              # against the twin behind every call
        run.step(first, count)
        twin.step(first, count)
        (mu_w, S_w), (mu_t, S_t) = run.ctx.get_state(), twin.ctx.get_state()
        e_mu, e_S = float(np.abs(mu_w - mu_t).max() / np.abs(mu_t).max()), gw.rel_err(S_w, S_t)
        assert e_mu <= 1e-10 and e_S <= 1e-10, f"{name}: behind frame {first + count - 1} differs from the twin ({e_mu}, {e_S})"
        assert np.array_equal(run.pops[first + count - 1], twin.pops[first + count - 1]), f"{name}: pops behind frame {first + count - 1}"
        assert run.ctx.get_track_health().tobytes() == twin.ctx.get_track_health().tobytes(), f"{name}: track record behind frame {first + count - 1}"
    res = gw.check_against_reference(run, c["lit"], c["per"], name)
    assert res["plan"] == [run.n - 1, 1, q["windows"], 0], f"{name}: plan {res['plan']}"
    window_launches(res, q["windows"])
    gw.check_against_twin(res, twin, name)
    return res, c


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_hand_overs_and_the_means_outside(name):
    res, c = _sequence(name)
    if name == "large_state":
        # the means outside the set moved, and not as the frozen gated window moves them
        outside = [x for x in range(c["mu"].size) if x >= 3 and (x - 3) // 3 not in (3, 11, 18, 27)]
        frozen = gw.Run(c["mu"], c["S"], c["ids"], c["frames"], ML=30).results()
        assert np.abs(res["state"][0][outside] - c["mu"][outside]).max() > 1e-6
        assert np.abs(res["state"][0][outside] - frozen["state"][0][outside]).max() > 1e-7, "the means outside did not see e"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_hand_overs_and_the_means_outside_on_gpu(name):
    _sequence(name)


# ---- 7. the planner's tail rule -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planner_case(rejected):
    """gw.planner_case under the consistent reference: frame 4 repeats frame 3's sighting of landmark 2 (an outlier, or a true one)
    identically, which the host cannot decide under the gate: the window closes behind frame 3"""
    rng = np.random.RandomState(31 + rejected)
    L = 6
    mu, S = random_state(rng, L, heading=-0.3)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    plan = [([], set())] + [(list(range(L)), {2} if f == 3 and rejected else set()) for f in range(1, 8)]
    frames, marks = gw.make_frames(rng, mu, ids, plan)
    by = lambda f, i: next(k for k, o in enumerate(frames[f]) if o[0] == int(ids[i]))
    frames[4][by(4, 2)] = frames[3][by(3, 2)]
    frames[5][by(5, 4)] = frames[4][by(4, 4)]
    gw.assert_repeats_decidable(frames)
    lit, per = reference(mu, S, ids, frames)
    act = lambda f, i: next(a for lid, _, a in per[f]["log"] if lid == int(ids[i]))
    assert act(3, 2) == (3 if rejected else 1) and act(4, 2) == (3 if rejected else 2), "the reference does not judge the repeat as planned"
    assert act(4, 4) == 1 and act(5, 4) == 2
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per)


def _planner(rejected):
    c = planner_case(rejected)
    where = f"tail rule, predecessor {'rejected' if rejected else 'accepted'}"
    args, batches = (c["mu"], c["S"], c["ids"], c["frames"]), [(0, 5), (5, 3)]
    run = GRun(*args, batches=batches[:1])
    plan = gw.plan_list(run.ctx)
    assert plan == [3, 2, 1, 1] and plan[3] > 0, f"{where}: plan stats {plan}"   # frames 1..3 in the window, frame 4 left to the device
    prof = run.ctx.profile_get()
    assert prof["k_ekf_win_step"][0] == 1 and prof[WIN_FINISH][0] == 1 and prof[FRAME_FINISH][0] == 2
    run.step(*batches[1])
    assert gw.plan_list(run.ctx) == [6, 2, 2, 1], f"{where}: plan stats after the second batch {gw.plan_list(run.ctx)}"
    res = gw.check_against_reference(run, c["lit"], c["per"], where)
    gw.check_against_twin(res, GRun(*args, batches=batches, windows=False), where)


@pytest.mark.parametrize("rejected", [0, 1])
def test_planner_tail_rule(rejected):
    _planner(rejected)


@pytest.mark.gpu
@pytest.mark.parametrize("rejected", [0, 1])
def test_planner_tail_rule_on_gpu(rejected):
    _planner(rejected)


# ---- 8. one rig sequence --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rig_case():
    rng = np.random.RandomState(9)
    L = 12
    mu, S = random_state(rng, L, heading=-0.7)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    seen = [0, 2, 3, 5, 8, 9, 11]
    frames, marks = gw.make_frames(rng, mu, ids, [([], set()), (seen, set()), (seen, {4}), (seen, set())])
    gw.assert_repeats_decidable(frames)
    # camera c of a step gets the step's observations c, c + 2, ...: the merged list is camera 0's, then camera 1's
    merged = [f[0::2] + f[1::2] for f in frames]
    lit, per = reference(mu, S, ids, merged, marks=marks)
    return dict(mu=mu, S=S, ids=ids, frames=frames, merged=merged, lit=lit, per=per)


def _rig():
    c = rig_case()
    run = GRun(c["mu"], c["S"], c["ids"], c["frames"], rig=2, ML=13)
    res = gw.check_against_reference(run, c["lit"], c["per"], "rig steps")     # (slot records read at max_batch + step)
    assert res["plan"] == [3, 1, 1, 0]
    window_launches(res)
    assert res["health"]["rejected"].tolist() == [0, 0, 1, 0]
    assert (run.ctx.get_slot_health(0, run.slots)["attempted"] == 0).all(), "a rig step's record landed in a frame slot"
    single = GRun(c["mu"], c["S"], c["ids"], c["merged"], ML=13).results()
    assert single["plan"] == [3, 1, 1, 0]
    for x, y in zip(res["state"] + (res["ids"], res["stats"][:, 1:]), single["state"] + (single["ids"], single["stats"][:, 1:])):
        assert np.array_equal(x, y), "the rig's window differs from a single context's on the merged lists"
    assert res["health"].tobytes() == single["health"].tobytes()


def test_rig_steps_in_a_gated_consistent_window():
    _rig()


@pytest.mark.gpu
def test_rig_steps_in_a_gated_consistent_window_on_gpu():
    _rig()


# ---- 9. the switch and the fallbacks --------------------------------------------------------------------------------------------------------------

def test_arguments_and_persistence():
    from test_localize import POSE0, SIG0, emu_context, random_map
    ctx = emu_context(2, max_landmarks=4)
    assert ctx.get_gated_consistent_windows() is False, "off by default"
    for bad in (-1, 2, 7):
        assert ctx.lib.aslam_set_gated_consistent_windows(ctx.h, bad) == E_INVALID
        assert ctx.get_gated_consistent_windows() is False, "a refused call changes nothing"
    flag = ctypes.c_int(7)
    assert ctx.lib.aslam_set_gated_consistent_windows(None, 1) == E_INVALID
    assert ctx.lib.aslam_get_gated_consistent_windows(ctx.h, None) == E_INVALID
    assert ctx.lib.aslam_get_gated_consistent_windows(None, ctypes.byref(flag)) == E_INVALID and flag.value == 7
    ctx.set_gated_consistent_windows(True)
    assert ctx.get_gated_consistent_windows() is True, "settable without a gate"
    assert (ctx.get_consistent_windows(), ctx.get_consistent_innovations(), ctx.get_slam_gate_windows()) == (False, False, False), "a switch of its own"
    ids, xyth = random_map(np.random.RandomState(1), 4)
    ctx.localize_begin(ids, xyth, POSE0, SIG0)
    assert ctx.get_gated_consistent_windows() is True
    ctx.set_gated_consistent_windows(False)                        # settable while localizing
    ctx.set_gated_consistent_windows(True)
    ctx.localize_end()
    assert ctx.get_gated_consistent_windows() is True
    ctx.fleet_begin([gw.CAM] * 2, ids, xyth, [POSE0] * 2, [SIG0] * 2)
    assert ctx.get_gated_consistent_windows() is True
    ctx.fleet_end()
    ctx.fleet_slam_begin([gw.CAM] * 2)
    assert ctx.get_gated_consistent_windows() is True
    ctx.fleet_end()
    assert ctx.get_gated_consistent_windows() is True
    ctx.set_gated_consistent_windows(False)
    assert ctx.get_gated_consistent_windows() is False


def same_bits(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a["state"] + (a["ids"], a["stats"]), b["state"] + (b["ids"], b["stats"])))
            and a.get("health", np.zeros(0)).tobytes() == b.get("health", np.zeros(0)).tobytes()
            and a.get("track", np.zeros(0)).tobytes() == b.get("track", np.zeros(0)).tobytes())


def _switch_and_fallbacks(monkeypatch):
    c = width_case(4, "third")
    args = (c["mu"], c["S"], c["ids"], c["frames"])
    n = len(c["frames"])
    # the new switch off: the gated context keeps the per-frame path whatever the other switches say (tests/test_consistent_windows.py)
    g_off = GRun(*args, gcw=False, cwin=False).results()
    g_on = GRun(*args, gcw=False).results()
    assert g_on["plan"] == [0, n, 0, 0] and launches(g_on["prof"]) == launches(g_off["prof"]) and same_bits(g_on, g_off)
    assert not any(k.startswith("k_ekf_win") for k in launches(g_on["prof"]))
    # on, with one of the other conditions off: today's path, launch for launch and bit for bit
    # ... no gate: the ungated consistent window
    a, b = CRun(*args).results(), GRun(*args, gate=None).results()
    assert launches(a["prof"]) == launches(b["prof"]) and b["prof"]["k_ekf_win_step"][0] == 1 and b["prof"][WIN_FINISH][0] == 0 and same_bits(a, b)
    # ... the gate's window switch off, or the consistent window's: the per-frame path
    for kw in (dict(switch=False), dict(cwin=False)):
        r = GRun(*args, **kw).results()
        assert r["plan"] == [0, n, 0, 0] and launches(r["prof"]) == launches(g_off["prof"]) and same_bits(r, g_off), f"{kw}: ran {launches(r['prof'])}"
    # ... consistent innovations off: the gated frozen window, bit for bit
    a, b = gw.Run(*args).results(), GRun(*args, consistent=False).results()
    assert launches(a["prof"]) == launches(b["prof"]) and b["prof"][WIN_FINISH][0] == 1 and a["plan"] == b["plan"] == [n - 1, 1, 1, 0] and same_bits(a, b)
    # ... the piece schedule, or no windows at all: the per-frame path
    monkeypatch.setenv("ASLAM_WIN_PIECE", "8")
    r = GRun(*args).results()
    monkeypatch.delenv("ASLAM_WIN_PIECE")
    assert r["plan"] == [0, n, 0, 0] and ekf_kernels_run(r["prof"]) == CHAIN_KERNELS["fast"] | {FRAME_FINISH} and same_bits(r, g_off)
    r = GRun(*args, windows=False).results()
    assert ekf_kernels_run(r["prof"]) == CHAIN_KERNELS["fast"] | {FRAME_FINISH} and same_bits(r, g_off)
    # every condition on: the window, one form whatever the logger-parts and worker-publish knobs say
    on = GRun(*args).results()
    assert on["plan"] == [n - 1, 1, 1, 0]
    window_launches(on)
    for env in ({"ASLAM_WIN_LOGGER_PARTS": "0"}, {"ASLAM_WIN_LOGGER_PARTS": "3", "ASLAM_WIN_WORKER_PUBLISH": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = GRun(*args).results()
        for k in env:
            monkeypatch.delenv(k)
        assert r["plan"] == on["plan"] and launches(r["prof"]) == launches(on["prof"]) and same_bits(r, on), f"{env}"


def _setter_finalises_a_pending_batch():
    """a batch submitted with the switch on keeps its windows when the switch is cleared before anything waited for it"""
    c = width_case(4, "third")
    args = (c["mu"], c["S"], c["ids"], c["frames"])
    n = len(c["frames"])
    got = []
    for wait in (True, False):
        run = GRun(*args, batches=[])
        run.arm()
        run.ctx.run_staged(0, 4, with_ekf=2)                       # deferred: enqueued by the next call
        if wait:
            run.ctx.sync()
        run.ctx.set_gated_consistent_windows(False)
        run.ctx.run_staged(4, n - 4, with_ekf=2)                   # the per-frame path
        run.ctx.sync()
        res = run.results()
        assert res["plan"] == [3, 1 + n - 4, 1, 0] and res["prof"][WIN_FINISH][0] == 1 and res["prof"][FRAME_FINISH][0] == 1 + n - 4, f"plan {res['plan']}"
        got.append(res)
    assert same_bits(*got)
    for f in range(n):
        check_slot_health(got[0]["health"][f], c["per"][f]["health"], f"frame {f}")
    check_track(got[0]["track"], c["per"][-1]["track"], "switch cleared behind a pending batch")


def _other_modes_are_unaffected():
    """localization, fleet localization and fleet SLAM keep their launches and bits with every switch set against all but the new one"""
    from ekf_reference import observe, predicted_pose
    from slam_gate_reference import OUTLIER
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
        ctx.set_slam_gate_windows(True)
        ctx.set_consistent_innovations(True)
        ctx.set_consistent_windows(True)
        ctx.set_gated_consistent_windows(switch)
        if mode == "fleet":
            ctx.fleet_begin([gw.CAM] * 2, ids, xyth, [pose] * 2, [sig] * 2)
        elif mode == "fleet_slam":
            ctx.fleet_slam_begin([gw.CAM] * 2)
            for r in range(2):
                ctx.fleet_set_state(r, mu, S, ids)
        else:
            ctx.localize_begin(ids, xyth, pose, sig)
        ctx.stage_encoders([0.0, WL, 0.0], [0.0, WR, 0.0], [0.0, DT, 0.0])
        for s, f in enumerate(frames):
            ctx.inject_observations(s, [o[0] for o in f], [1] * len(f), np.array([o[1] for o in f]), np.array([o[2] for o in f]))
        ctx.profile_enable(True)
        ctx.profile_reset()
        if mode == "localize":
            ctx.run_staged(0, 3, with_ekf=2)
            out = ctx.get_state() + ctx.get_observations() + (ctx.get_slot_ekf_stats(0, 3),)
        else:
            ctx.fleet_run_staged(0, [1, 1, 0], with_ekf=2)
            ctx.sync()
            out = (ctx.fleet_get_poses() if mode == "fleet" else ctx.fleet_get_state(0) + ctx.fleet_get_state(1)) + (ctx.get_slot_ekf_stats(0, 3),)
            if mode == "fleet_slam":
                out += (ctx.get_slot_health(0, 3).view(np.uint8),)
        assert not any(k.startswith("k_ekf_win") for k in launches(ctx.profile_get())), f"{mode}: a window kernel ran"
        return out, launches(ctx.profile_get())

    for mode in ("localize", "fleet", "fleet_slam"):
        (a, ka), (b, kb) = run(False, mode), run(True, mode)
        assert ka == kb, f"{mode}: the switch changed the launches"
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), f"{mode}: the switch changed a result"


def test_switch_and_fallbacks(monkeypatch):
    _switch_and_fallbacks(monkeypatch)


def test_setter_finalises_a_pending_batch():
    _setter_finalises_a_pending_batch()


def test_other_modes_are_unaffected():
    _other_modes_are_unaffected()


@pytest.mark.gpu
def test_switch_modes_and_pending_batch_on_gpu(monkeypatch):
    _switch_and_fallbacks(monkeypatch)
    _setter_finalises_a_pending_batch()
    _other_modes_are_unaffected()


# ---- 10. rendered frames (GPU only) ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_rendered_ring_equals_the_per_frame_twin():
    """8 rendered frames of the small ring through detection and SLAM with the default gate and every switch on, against the per-frame
    gated consistent twin on the same raw observations"""
    from test_localize import gpu_context, render_frames, small_ring
    assert capi.lib_path().endswith("libaruco_slam_hip.so"), "the gpu cases must run the native gfx950 library"
    w = synth.RingWorld(small_ring())
    n = 8
    win = gpu_context(w, n, persistent_waves=4)
    os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        twin = gpu_context(w, n, persistent_waves=4)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)
    for ctx in (win, twin):
        ctx.set_slam_gate()
        ctx.set_slam_gate_windows(True)
        ctx.set_consistent_innovations(True)
        ctx.set_consistent_windows(True)
        ctx.set_gated_consistent_windows(True)
    frs, imgs = render_frames(win, w, 0, n)
    enc = [[getattr(f, k) for f in frs] for k in ("wl", "wr", "dt")]
    win.stage_frames(np.stack(imgs))
    win.stage_encoders(*enc)
    win.profile_enable(True)
    win.profile_reset()
    win.run_staged(0, n, with_ekf=True)
    win.sync()
    twin.stage_encoders(*enc)
    for s in range(n):
        twin.inject_observations(s, *win.get_slot_raw_observations(s))
    twin.run_staged(0, n, with_ekf=2)
    twin.sync()
    plan, prof = win.plan_stats(), win.profile_get()
    assert plan["windows"] >= 1 and prof["k_ekf_win_step"][0] == plan["windows"] == prof[WIN_FINISH][0], f"no gated consistent window on the ring: {plan}"
    assert np.array_equal(win.get_landmark_ids(), twin.get_landmark_ids()) and win.get_landmark_ids().size >= 2
    assert np.array_equal(win.get_slot_ekf_stats(0, n)[:, 1:], twin.get_slot_ekf_stats(0, n)[:, 1:])
    for x, y in zip(win.get_observations()[:3], twin.get_observations()[:3]):
        assert np.array_equal(x, y), "pops differ from the twin"
    hw, ht = win.get_slot_health(0, n), twin.get_slot_health(0, n)
    for k in gw.INT_FIELDS:
        assert np.array_equal(hw[k], ht[k]), f"{k} differs from the twin"
    for k in ("nis_sum", "d2_max"):
        assert np.allclose(hw[k], ht[k], rtol=1e-9, atol=0.0), f"{k} differs from the twin"
    assert win.get_track_health().tobytes() == twin.get_track_health().tobytes()
    (mu_w, S_w), (mu_t, S_t) = win.get_state(), twin.get_state()
    e_mu, e_S = float(np.abs(mu_w - mu_t).max() / np.abs(mu_t).max()), gw.rel_err(S_w, S_t)
    print(f"rendered ring, plan {plan}: against the twin mu {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert e_mu <= 1e-10 and e_S <= 1e-10
