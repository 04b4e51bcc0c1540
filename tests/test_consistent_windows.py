"""Consistent innovations inside EKF windows (aslam_set_consistent_windows): with consistent innovations on, the
one-launch window chain corrects its mean with e_i = ze_i - H_i (mu_{i-1} - mu_0), the log header carries e_i, and Sigma keeps the bits
of a frozen-mean window.  The gated consistent window is not built (§33, Dropped): a gated context keeps the per-frame path, which the
switch test below pins.

Reference: consistent_reference.consistent_step iterated over the frames in long double (ref_sequence below: pop order = ascending
landmark index, a sighting within 0.01 of the previous frame's sighting of the same landmark is dropped as "stationary"; every case
asserts that no repeat lies within 1e-6 of that threshold).  Inputs as in tests/test_slam_gate_windows.py (random_state /
observe of tests/ekf_reference.py, noise 0.03, the state seated) and, for the hand-over cases, the sequences of
tests/test_ekf_window_logger_mean.py (make_case: the first frames add the landmarks on the per-frame chain; the long-double sequence
then starts from the per-frame consistent twin's state behind the last frame that adds one).
Tolerances, the project's: mu against the long-double sequence rtol 1e-9 / atol 1e-11, Sigma 1e-9 relative; windowed against the
per-frame consistent twin (ASLAM_NO_WINDOWS) 1e-10 relative; everything discrete exact.  Every case not marked gpu runs on the
session's library (the emulation without a GPU)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import test_ekf_window_logger_mean as lm
import test_slam_gate_windows as gw
from aruco_slam_amd import capi, synth
from consistent_reference import consistent_step
from ekf_reference import CHAIN_KERNELS, LD, ekf_kernels_run, observe, predicted_pose, random_state, rel_err
from test_ekf_sizes import DT, ID_TABLE, WL, WR
from test_ekf_window import D, K

E_INVALID = -1
SOLVES = ("k_ekf_mid", "k_ekf_mid64", "k_ekf_small")


# ---- the reference sequence ---------------------------------------------------------------------------------------------------------

def ref_sequence(mu, S, ids, frames, motions, consistent=True, last=None):
    """consistent_step in long double over frames = [[(id, z, Rdiag)]] with motions = [(wl, wr, dt)]; ids: landmark index -> id;
    last: {index: z} of the frame before the first (its popped sightings).  Returns mu, Sigma (long double)"""
    index = {int(i): k for k, i in enumerate(ids)}
    mu, S = np.array(mu, LD), np.array(S, LD)
    last = dict(last or {})
    for obs, (wl, wr, dt) in zip(frames, motions):
        fused, nxt = [], {}
        for k, z, r in sorted(((index[int(i)], np.asarray(z, float), np.asarray(r, float)) for i, z, r in obs), key=lambda o: o[0]):
            d = float(np.linalg.norm(last[k] - z)) if k in last else np.inf
            assert np.isnan(d) or abs(d - 0.01) > 1e-6, f"a repeated sighting {d} from its predecessor: the 0.01 test hangs on rounding"
            if d < 0.01:
                nxt[k] = np.full(3, np.nan)                        # stationary: popped, not fused, last_observation_ stays unset
            else:
                fused.append((k, z, r))
                nxt[k] = z
        mu, S, _ = consistent_step(mu, S, wl, wr, dt, fused, consistent=consistent)
        last = nxt
    return mu, S


def check_ref(mu_g, S_g, mu_r, S_r, where):
    assert mu_g.shape == mu_r.shape and np.isfinite(mu_g).all() and np.isfinite(S_g).all(), f"{where}: state"
    e_mu, e_S = float(np.abs(mu_g - mu_r).max()), rel_err(S_g, S_r)
    print(f"{where}: against the long-double sequence |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert np.allclose(mu_g, np.asarray(mu_r, float), rtol=1e-9, atol=1e-11), f"{where}: mu differs by {e_mu}"
    assert e_S <= 1e-9, f"{where}: Sigma differs by {e_S} (relative)"


def check_twin(mu_w, S_w, mu_t, S_t, where):
    e_mu, e_S = float(np.abs(mu_w - mu_t).max() / np.abs(mu_t).max()), rel_err(S_w, S_t)
    print(f"{where}: against the per-frame consistent twin mu {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert e_mu <= 1e-10 and e_S <= 1e-10, f"{where}: differs from the twin ({e_mu}, {e_S})"


class CRun(gw.Run):
    """gw.Run (state seated, every frame injected, run in batches) without a gate unless one is asked for, the two consistent switches
    set before the first call"""

    def __init__(self, *a, consistent=True, cwin=True, **kw):
        self._sw, self._armed = (consistent, cwin), False
        kw.setdefault("gate", None)
        kw.setdefault("switch", False)
        super().__init__(*a, **kw)

    def arm(self):
        if not self._armed:
            self.ctx.set_consistent_innovations(self._sw[0])
            self.ctx.set_consistent_windows(self._sw[1])
            self._armed = True

    def step(self, first, count):
        self.arm()
        super().step(first, count)


def bits(res, run):
    """what does not depend on the innovation: Sigma, landmark ids, pop lists, slot statistics"""
    return dict(S=res["state"][1].tobytes(), ids=res["ids"].tobytes(), stats=res["stats"].tobytes(),
                pops={f: p.tobytes() for f, p in run.pops.items()})


def launches(prof):
    return {k: v[0] for k, v in prof.items() if k.startswith("k_ekf") and v[0] > 0}


# ---- 1. the three widths; 2. where the six-column gather can go wrong -----------------------------------------------------------------
# gw.SHAPES: T = 4 (L 4, 6 frames), T = 8 (L 25, 3 frames), T = 12 (L 50, 3 frames), every frame sees every landmark.  At T = 8 the
# landmark at position 20 has its columns 63, 64, 65 across the first chunk boundary of the logger's mean, at T = 12 the one at position
# 41 has 126, 127, 128 across the second, and every 64-column chunk holds landmarks: the case asserts on the reference alone that the
# running innovation moves those very landmarks.  The inputs are the first draw on which the reference's two means (running and frozen)
# lie more than 2e-3 apart: chosen on the reference, before any device run.

#
# Sigma.  Within a frame S_i, K_i and the Sigma update do not depend on the innovation, so Sigma keeps the bits of the frozen-mean
# window.  Over several frames it cannot: the next frame's predict and its H are formed at the mean the frame before left, which the
# running innovation moves (the long-double reference's two Sigmas differ by 3e-5 on these shapes; asserted below).  So the bit-equality
# of Sigma is asserted where it holds, at every width: one_frame = a window of one frame with all its corrections followed by an empty
# frame at rest (wl = wr = 0: its predict adds exact zeros to P), where Sigma, ids, pops and slot statistics are the frozen window's
# bits.  On the several-frame shapes everything that is not a function of the mean (ids, pops, slot statistics) is compared bit for bit.

@functools.lru_cache(maxsize=None)
def width_case(T, one_frame=False):
    sh = gw.SHAPES[T]
    L, Kf = sh["L"], 2 if one_frame else sh["frames"]
    motions = [(WL, WR, DT), (0.0, 0.0, DT)] if one_frame else [(WL, WR, DT)] * Kf
    plan = [([], set()), (list(range(L)), set()), ([], set())] if one_frame else [([], set())] + [(list(range(L)), set())] * Kf
    for seed in range(900 + T, 920 + T):                           # the first draw on which the reference alone separates the two means
        rng = np.random.RandomState(seed)
        mu, S = random_state(rng, L, heading=0.4)
        ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
        frames, _ = gw.make_frames(rng, mu, ids, plan, motions=[None] + motions)
        mu_r, S_r = ref_sequence(mu, S, ids, frames[1:], motions)
        mu_f, S_f = ref_sequence(mu, S, ids, frames[1:], motions, consistent=False)
        sep = np.abs(np.asarray(mu_r - mu_f, float))
        if sep.max() > 2e-3:
            break
    gw.assert_repeats_decidable(frames)
    assert sep.max() > 2e-3, f"T {T}: the reference alone separates the two means by {sep.max()} only"
    for pos in {8: (20,), 12: (20, 41)}.get(T, ()):
        assert sep[3 + 3 * pos:6 + 3 * pos].max() > 1e-5, f"T {T}: the landmark at position {pos} does not feel the running innovation"
    for ch in range(16 * T // 64):
        assert sep[64 * ch:min(64 * ch + 64, 3 + 3 * L)].max() > 1e-5, f"T {T}: chunk {ch} of the mean does not feel the running innovation"
    dS = float(np.abs(np.asarray(S_r - S_f, float)).max())
    assert (dS == 0.0) if one_frame else (dS > 1e-7), f"T {T}: the reference's two Sigmas differ by {dS}"
    return dict(mu=mu, S=S, ids=ids, frames=frames, mu_ref=mu_r, S_ref=S_r, motions=[None] + motions, K=Kf)


def _width(T, one_frame=False):
    sh, c = gw.SHAPES[T], width_case(T, one_frame)
    args, kw = (c["mu"], c["S"], c["ids"], c["frames"]), dict(cap=sh["cap"], ML=sh["ML"], motions=c["motions"])
    where = f"T {T}" + (" one frame" if one_frame else "")
    run = CRun(*args, **kw)
    res = run.results()
    check_ref(*res["state"], c["mu_ref"], c["S_ref"], where)
    twin = CRun(*args, windows=False, **kw).results()
    assert not any(k.startswith("k_ekf_win") for k in launches(twin["prof"])), "the twin ran a window kernel"
    check_twin(*res["state"], *twin["state"], where)
    assert np.array_equal(res["ids"], twin["ids"]) and np.array_equal(res["stats"], twin["stats"])
    # a frozen-mean windowed run of the same frames: the innovation changes nothing but the mean
    frozen_run = CRun(*args, consistent=False, cwin=False, **kw)
    frozen = frozen_run.results()
    b_on, b_off = bits(res, run), bits(frozen, frozen_run)
    for k in b_on:
        if k != "S" or one_frame:
            assert b_on[k] == b_off[k], f"{where}: {k} differs from the frozen-mean window"
    d = float(np.abs(res["state"][0] - frozen["state"][0]).max())
    print(f"{where}: |mu - mu_frozen| {d:.3g}")
    assert d > 1e-3, f"{where}: the switch changed nothing"
    # one window, the arming frame alone on the per-frame chain: the launches of the frozen run, kernel for kernel
    assert res["plan"] == [c["K"], 1, 1, 0] and run.ctx.plan_stats()["windows"] >= 1
    assert res["prof"]["k_ekf_win_step"][0] == 1
    assert launches(res["prof"]) == launches(frozen["prof"]), f"{where}: ran {launches(res['prof'])}"
    assert all(res["prof"][k][0] == frozen["prof"][k][0] for k in SOLVES)


@pytest.mark.parametrize("one_frame", [False, True], ids=["frames", "one_frame"])
@pytest.mark.parametrize("T", [4, 8, 12])
def test_three_widths(T, one_frame):
    _width(T, one_frame)


@pytest.mark.gpu
@pytest.mark.parametrize("one_frame", [False, True], ids=["frames", "one_frame"])
@pytest.mark.parametrize("T", [4, 8, 12])
def test_three_widths_on_gpu(T, one_frame):
    _width(T, one_frame)


# ---- 3. the mean's hand-overs; 4. mu_R and window to window -----------------------------------------------------------------------------
# The cases of tests/test_ekf_window_logger_mean.py: a window that begins with two empty frames, has one in the middle and ends with one;
# m = 1 frames; m = 4, 1, 3 in a row; an all-stationary frame; a different R per marker; m = 63 on the 192-wide image; rows past column
# 64 on the 128-wide image; a 64-frame window and the frames behind it (a run longer than one window); three windows handed over in a
# row; 30 landmarks with 4 of them in S (the other 26 means move only through psi: the header carries e).

def run_frames(frames, batch, consistent=True, cwin=True, windows=True, env=None, max_landmarks=40, max_updates=24):
    """make_case frames through a context in calls of `batch` frames: state, ids, pops and slot statistics behind every call"""
    env = dict(env or {}, **({} if windows else {"ASLAM_NO_WINDOWS": "1"}))
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        nfr = len(frames)
        ctx = capi.Context(max_rows=64, max_cols=64, max_batch=nfr, persistent_waves=4, max_landmarks=max_landmarks, r2c_t=(0.1, -0.05, 0.0),
                           max_updates_per_frame=max_updates)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx.set_camera(K, D)
    ctx.set_consistent_innovations(consistent)
    ctx.set_consistent_windows(cwin)
    t = [fr["t"] for fr in frames]
    ctx.stage_encoders([fr["wl"] for fr in frames], [fr["wr"] for fr in frames], [0.0] + [t[i] - t[i - 1] for i in range(1, nfr)])
    for f, fr in enumerate(frames):
        obs = fr["obs"]
        ctx.inject_observations(f, fr["ids"], [0 if o is None else 1 for o in obs],
                                np.array([np.zeros(3) if o is None else o["z"] for o in obs]).reshape(-1, 3),
                                np.array([np.ones(3) if o is None else np.diag(o["R"]) for o in obs]).reshape(-1, 3))
    ctx.profile_enable(True)
    ctx.profile_reset()
    out = []
    for f0 in range(0, nfr, batch):
        nb = min(batch, nfr - f0)
        ctx.run_staged(f0, nb, with_ekf=2)
        ctx.sync()                                                 # (raises if a workgroup of a window launch gave up waiting)
        mu, S = ctx.get_state()
        ob = ctx.get_observations()
        out.append(dict(last=f0 + nb - 1, mu=mu, S=S, ids=ctx.get_landmark_ids(), pops=np.stack(ob[:3], 1), stats=ctx.get_slot_ekf_stats(f0, nb)))
    return out, ctx.profile_get(), ctx.plan_stats()


def frame_obs(fr):
    return [(int(i), o["z"], np.diag(o["R"])) for i, o in zip(fr["ids"], fr["obs"]) if o is not None]


@functools.lru_cache(maxsize=None)
def handover_twin(name):
    """the per-frame consistent twin, one frame per call: its state behind every frame"""
    frames, _ = lm.reference(name)
    out, prof, _ = run_frames(frames, 1, windows=False, **lm.CASES[name][4])
    assert not any(k.startswith("k_ekf_win") for k in launches(prof)), "the twin ran a window kernel"
    return out


def _handover(name):
    _, batch, windows, hand_overs, kw = lm.CASES[name]
    frames, _ = lm.reference(name)
    n = len(frames)
    twin = handover_twin(name)
    win, prof, plan = run_frames(frames, batch, **kw)
    assert prof["k_ekf_win_step"][0] == windows and prof["k_ekf_win_next"][0] == hand_overs and plan["windows"] == windows, \
        f"{name}: {prof['k_ekf_win_step'][0]} windows, {prof['k_ekf_win_next'][0]} hand-overs; built for {windows}, {hand_overs}"
    for w in win:
        t = twin[w["last"]]
        check_twin(w["mu"], w["S"], t["mu"], t["S"], f"{name} frame {w['last']}")
        assert np.array_equal(w["ids"], t["ids"]) and np.array_equal(w["pops"], t["pops"]), f"{name} frame {w['last']}: ids / pops differ from the twin"
        assert np.array_equal(w["stats"][-1], t["stats"][-1]), f"{name} frame {w['last']}: slot statistics differ from the twin"
    # the long-double sequence from the twin's state behind the last frame that adds a landmark
    seen, n_add = set(), 0
    for f, fr in enumerate(frames):
        new = {int(i) for i in fr["ids"]} - seen
        if new:
            n_add, seen = f + 1, seen | new
    assert n_add < n and win[-1]["last"] == n - 1
    start = twin[n_add - 1]
    ids = win[-1]["ids"]
    assert np.array_equal(ids, start["ids"])
    index = {int(i): k for k, i in enumerate(ids)}
    tt = [fr["t"] for fr in frames]
    motions = [(fr["wl"], fr["wr"], tt[f] - tt[f - 1]) for f, fr in enumerate(frames)]
    last = {index[i]: z for i, z, _ in frame_obs(frames[n_add - 1])}
    mu_r, S_r = ref_sequence(start["mu"], start["S"], ids, [frame_obs(fr) for fr in frames[n_add:]], motions[n_add:], last=last)
    check_ref(win[-1]["mu"], win[-1]["S"], mu_r, S_r, name)
    return win, prof


@pytest.mark.parametrize("name", sorted(lm.CASES))
def test_mean_hand_overs(name):
    _handover(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(lm.CASES))
def test_mean_hand_overs_on_gpu(name):
    _handover(name)


def test_large_state_moves_the_means_outside_the_window():
    """30 landmarks, 4 in S: the 26 means outside move only through psi, which the replay forms from the header's innovation.  The
    frozen-mean window moves them elsewhere, so the agreement with the twin above is not vacuous"""
    name = "large_state"
    frames, _ = lm.reference(name)
    kw = lm.CASES[name][4]
    win, _, _ = run_frames(frames, lm.CASES[name][1], **kw)
    frozen, _, _ = run_frames(frames, lm.CASES[name][1], consistent=False, cwin=False, **kw)
    inside = {3 + 3 * k + q for k in (3, 11, 18, 27) for q in range(3)} | {0, 1, 2}
    outside = [c for c in range(win[-1]["mu"].size) if c not in inside]
    d = float(np.abs(win[-1]["mu"][outside] - frozen[-1]["mu"][outside]).max())
    print(f"large_state: the means outside S differ from the frozen window's by {d:.3g}")
    assert d > 1e-6, "the means outside S did not see the running innovation"


# ---- 6. the switch and the modes ------------------------------------------------------------------------------------------------------

def test_arguments_and_persistence():
    from test_localize import POSE0, SIG0, emu_context, random_map
    ctx = emu_context(2, max_landmarks=4)
    assert ctx.get_consistent_windows() is False, "off by default"
    for bad in (-1, 2, 7):
        assert ctx.lib.aslam_set_consistent_windows(ctx.h, bad) == E_INVALID
        assert ctx.get_consistent_windows() is False, "a refused call changes nothing"
    flag = ctypes.c_int(7)
    assert ctx.lib.aslam_set_consistent_windows(None, 1) == E_INVALID
    assert ctx.lib.aslam_get_consistent_windows(ctx.h, None) == E_INVALID
    assert ctx.lib.aslam_get_consistent_windows(None, ctypes.byref(flag)) == E_INVALID and flag.value == 7
    ctx.set_consistent_windows(True)
    assert ctx.get_consistent_windows() is True and ctx.get_consistent_innovations() is False, "a switch of its own"
    ids, xyth = random_map(np.random.RandomState(1), 4)
    ctx.localize_begin(ids, xyth, POSE0, SIG0)
    assert ctx.get_consistent_windows() is True
    ctx.set_consistent_windows(False)                              # settable while localizing
    ctx.set_consistent_windows(True)
    ctx.localize_end()
    assert ctx.get_consistent_windows() is True
    ctx.fleet_begin([gw.CAM] * 2, ids, xyth, [POSE0] * 2, [SIG0] * 2)
    assert ctx.get_consistent_windows() is True
    ctx.fleet_end()
    ctx.fleet_slam_begin([gw.CAM] * 2)
    assert ctx.get_consistent_windows() is True
    ctx.fleet_end()
    assert ctx.get_consistent_windows() is True
    ctx.set_consistent_windows(False)
    assert ctx.get_consistent_windows() is False


def _switch_and_fallbacks(monkeypatch):
    c = width_case(4)
    args = (c["mu"], c["S"], c["ids"], c["frames"])
    n = len(c["frames"])
    # consistent innovations on, the windows switch off: as before, no window
    off = CRun(*args, cwin=False).results()
    assert off["plan"] == [0, n, 0, 0] and not any(k.startswith("k_ekf_win") for k in launches(off["prof"]))
    check_ref(*off["state"], c["mu_ref"], c["S_ref"], "windows switch off")
    # the windows switch on, consistent innovations off: bit for bit a default context, the same kernels
    plain_run, on_run = CRun(*args, consistent=False, cwin=False), CRun(*args, consistent=False, cwin=True)
    plain, on = plain_run.results(), on_run.results()
    assert launches(plain["prof"]) == launches(on["prof"]) and on["prof"]["k_ekf_win_step"][0] == 1 and on["plan"] == plain["plan"]
    assert bits(plain, plain_run) == bits(on, on_run) and np.array_equal(plain["state"][0], on["state"][0])
    # the piece schedule, or the mean not on the logger wave: the per-frame path, the same results
    for env in ({"ASLAM_WIN_PIECE": "8"}, {"ASLAM_WIN_LOGGER_PARTS": "1"}, {"ASLAM_WIN_LOGGER_PARTS": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = CRun(*args).results()
        for k in env:
            monkeypatch.delenv(k)
        assert r["plan"] == [0, n, 0, 0] and ekf_kernels_run(r["prof"]) == CHAIN_KERNELS["fast"], f"{env}: ran {launches(r['prof'])}"
        assert np.array_equal(r["state"][0], off["state"][0]) and np.array_equal(r["state"][1], off["state"][1])
    # a SLAM gate: the gated consistent window is not built, so the gated context keeps the per-frame path whatever the switches say
    g_off = CRun(*args, gate=gw.INF, switch=True, cwin=False).results()
    g_on = CRun(*args, gate=gw.INF, switch=True, cwin=True).results()
    assert g_on["plan"] == [0, n, 0, 0] and launches(g_on["prof"]) == launches(g_off["prof"])
    assert np.array_equal(g_on["state"][0], g_off["state"][0]) and g_on["health"].tobytes() == g_off["health"].tobytes()
    check_ref(*g_on["state"], c["mu_ref"], c["S_ref"], "gated context")


def _setter_finalises_a_pending_batch():
    """a batch submitted with the switch on keeps its windows when the switch is cleared before anything waited for it"""
    c = width_case(4)
    args = (c["mu"], c["S"], c["ids"], c["frames"])
    n = len(c["frames"])
    got = []
    for wait in (True, False):
        run = CRun(*args, batches=[])
        run.arm()
        run.ctx.run_staged(0, 4, with_ekf=2)                       # deferred: enqueued by the next call
        if wait:
            run.ctx.sync()
        run.ctx.set_consistent_windows(False)
        run.ctx.run_staged(4, n - 4, with_ekf=2)                   # the per-frame path
        run.ctx.sync()
        res = run.results()
        assert res["plan"] == [3, 1 + n - 4, 1, 0] and res["prof"]["k_ekf_win_step"][0] == 1, f"plan {res['plan']}"
        got.append(res)
    a, b = got
    for x, y in zip(a["state"] + (a["stats"],), b["state"] + (b["stats"],)):
        assert np.array_equal(x, y)
    check_ref(*a["state"], c["mu_ref"], c["S_ref"], "switch cleared behind a pending batch")


def _other_modes_are_unaffected():
    """localization, fleet localization and fleet SLAM results keep their bits with both switches set against consistent innovations alone"""
    rng = np.random.RandomState(2)
    L = 6
    mu, S = random_state(rng, L, heading=0.3)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    xyth = mu[3:].reshape(-1, 3)
    pose, sig = mu[:3], np.diag([0.02, 0.03, 0.01])
    at = predicted_pose(mu, WL, WR, DT)
    frames = [[(int(ids[i]), z, r) for i, z, r in observe(rng, mu, range(L), post_predict=at)] for _ in range(3)]

    def run(switch, mode):
        ctx = capi.Context(max_rows=64, max_cols=64, max_batch=3, persistent_waves=4, max_landmarks=L, max_updates_per_frame=24)
        ctx.set_consistent_innovations(True)
        ctx.set_consistent_windows(switch)
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


# ---- 7. one rig sequence ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rig_case():
    rng = np.random.RandomState(19)
    L = 12
    mu, S = random_state(rng, L, heading=-0.7)
    ids = rng.permutation(ID_TABLE)[:L].astype(np.int32)
    seen = [0, 2, 3, 5, 8, 9, 11]
    frames, _ = gw.make_frames(rng, mu, ids, [([], set())] + [(seen, set())] * 3)
    gw.assert_repeats_decidable(frames)
    # camera c of a step gets the step's observations c, c + 2, ...: the merged list is camera 0's, then camera 1's
    merged = [f[0::2] + f[1::2] for f in frames]
    mu_r, S_r = ref_sequence(mu, S, ids, merged[1:], [(WL, WR, DT)] * 3)
    return dict(mu=mu, S=S, ids=ids, frames=frames, merged=merged, mu_ref=mu_r, S_ref=S_r)


def _rig():
    c = rig_case()
    run = CRun(c["mu"], c["S"], c["ids"], c["frames"], rig=2, ML=13)
    res = run.results()
    assert res["plan"] == [3, 1, 1, 0] and res["prof"]["k_ekf_win_step"][0] == 1, f"plan {res['plan']}"
    check_ref(*res["state"], c["mu_ref"], c["S_ref"], "rig steps")
    single = CRun(c["mu"], c["S"], c["ids"], c["merged"], ML=13).results()
    assert single["plan"] == [3, 1, 1, 0]
    for x, y in zip(res["state"] + (res["ids"], res["stats"][:, 1:]), single["state"] + (single["ids"], single["stats"][:, 1:])):
        assert np.array_equal(x, y), "the rig's window differs from a single context's on the merged lists"


def test_rig_steps_in_a_consistent_window():
    _rig()


@pytest.mark.gpu
def test_rig_steps_in_a_consistent_window_on_gpu():
    _rig()


# ---- 9. rendered frames (GPU only) ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_rendered_ring_equals_the_per_frame_twin():
    """8 rendered frames of the small ring through detection and SLAM with both switches on, against the per-frame consistent twin on
    the same raw observations"""
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
        ctx.set_consistent_innovations(True)
    win.set_consistent_windows(True)
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
    assert plan["windows"] >= 1 and prof["k_ekf_win_step"][0] == plan["windows"], f"no window on the ring: {plan}"
    assert np.array_equal(win.get_landmark_ids(), twin.get_landmark_ids()) and win.get_landmark_ids().size >= 2
    assert np.array_equal(win.get_slot_ekf_stats(0, n)[:, 1:], twin.get_slot_ekf_stats(0, n)[:, 1:])
    for x, y in zip(win.get_observations()[:3], twin.get_observations()[:3]):
        assert np.array_equal(x, y), "pops differ from the twin"
    (mu_w, S_w), (mu_t, S_t) = win.get_state(), twin.get_state()
    check_twin(mu_w, S_w, mu_t, S_t, f"rendered ring, plan {plan}")
