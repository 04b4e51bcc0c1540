"""Every device path that contains a predict, at filter parameters away from the defaults of aslam_init and at the motion edges
(parameter sets, motions and mutants: tests/params_reference.py).

The device holds three hand-written copies of the reference's addEncoder (aruco_slam.cpp:35-73):
  predict_block (ekf.hip)                  k_ekf_predict (aslam_add_encoder), k_ekf_plan<EkfSingle>, k_ekf_plan<EkfFleet>
  the prepare wave (ekf_window.hip)        k_ekf_win_step at every width, with the logger's mean and with its own (ASLAM_WIN_PIECE), gated
  loc_steps (ekf_localize.h)               k_loc_steps and k_fleet_steps, gated, on an uncertain map and both
and every other test of them runs at kl == kr = 0.05, b = 0.09, Q_k = 0.01, where kl for kr, kr in the noise's second column or b
for 2 b change no bit of a result.  Here every path runs under set A and set B (and the defaults, as the control) on motions that
reverse, spin, move one wheel only, go straight although wl != wr, stand still and turn by more than 2 pi, from headings next to
+pi and -pi (the predict wraps both ways).

Tolerances are the project's: Sigma 1e-9 relative, mu allclose(rtol 1e-9, atol 1e-11), everything discrete exact.  The reference is
the long-double form (ekf_reference.reference_step, params_reference.slam_frame, umap_reference.UncertainMapLocalizer); the numpy
literal transcription (oracle/ekf_literal.py) and the double references are compared too where the project has them.  Every case also
asserts, on the reference alone, that its double form agrees with the long-double form to 1e-12 (the case is well conditioned), and
every path that each mutant of params_reference.MUTANTS moves at least one of its cases by 1e-6 (test_sensitivity_floor).

Each test has a plain form, which runs on the session's library (the emulation build without a GPU), and a gpu twin that calls the
same check.  The profile names no variant of a kernel: k_ekf_predict has no span of its own (the check is that no other EKF kernel
ran and the state moved), the gated / uncertain-map steps run under k_loc_steps / k_fleet_steps (the check adds the context's mode)."""
import functools
import math

import numpy as np
import pytest

import params_reference as pr
import test_slam_gate_windows as gw
from aruco_slam_amd import capi
from ekf_reference import CHAIN_CAP, CHAIN_KERNELS, LD, ekf_kernels_run, observe, predicted_pose, random_state, reference_step, rel_err
from plan_reference import new_z
from slam_gate_reference import gated_reference_step
from test_ekf_sizes import _Injected
from test_ekf_window import make_case, run_device
from tests.gate_reference import DEFAULTS as GATE_DEFAULTS, GatedLocalizer, check_slot_health, check_track
from tests.test_innovation_gate import CAM, fleet_call, sight
from tests.test_localize import SIG0, FrozenMapLocalizer, inject, random_map
from tests.umap_reference import UncertainMapLocalizer

SETS = ("defaults", "A", "B")
R = lambda a, b: list(range(a, b))  # noqa: E731
WORST = {}                                          # path -> [worst |d mu|, worst relative Sigma error] of this session


def pose_kw(name):
    p = pr.SETS[name]
    return dict(kl=p["kl"], kr=p["kr"], b=p["b"])


def close(path, where, mu_g, S_g, mu_r, S_r):
    """the device's (mu, Sigma) against a reference's at the project's tolerances"""
    assert mu_g.shape == np.shape(mu_r), f"{where}: state size"
    e_mu, e_S = float(np.abs(mu_g - np.asarray(mu_r, LD)).max()), rel_err(S_g, S_r)
    w = WORST.setdefault(path, [0.0, 0.0])
    w[0], w[1] = max(w[0], e_mu), max(w[1], e_S)
    print(f"{path} {where}: |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")
    assert np.allclose(mu_g, np.asarray(mu_r, float), rtol=1e-9, atol=1e-11), f"{where}: mu differs by {e_mu}"
    assert e_S <= 1e-9, f"{where}: Sigma differs by {e_S} (relative)"


def context(name, ML=8, batch=4, cap=24, **kw):
    return capi.Context(max_rows=64, max_cols=64, max_batch=batch, persistent_waves=4, max_landmarks=ML, max_updates_per_frame=cap,
                        **pr.ctx_params(name), **kw)


def pops_of(ctx):
    gi, gx, ga, _, _ = ctx.get_observations()
    return np.stack([gi, gx, ga], 1).reshape(-1, 3)


def spd_blocks(rng, n, scale=0.05):
    A = rng.normal(0, scale, (n, 3, 3))
    return A @ A.transpose(0, 2, 1) + 1e-6 * np.eye(3)


# ---- 1. k_ekf_predict through aslam_add_encoder ----------------------------------------------------------------------------------
# random: random_state(L = 8); tiny: Sigma = 1e-6 I, so that Q is the result and not a perturbation; L400: N = 1203 > 3 + 4 * 256, the
# last columns go through the tail loop of predict_block, the others through its register-held columns

PREDICT_GROUPS = [(n, k) for n in ("A", "B") for k in ("random", "tiny", "L400")] + [("defaults", "random")]


@functools.lru_cache(maxsize=None)
def predict_cases(name, kind):
    """[(where, mu, Sigma, (wl, wr, dt))] and per case the long-double reference"""
    mo = pr.motions(name)
    chosen = {"random": list(mo) + ["dt0"], "tiny": ["forward", "right_only", "spin"], "L400": ["right_only"]}[kind]
    if name == "defaults":
        chosen = ["forward", "right_only", "dt0"]
    L = 400 if kind == "L400" else 8
    out = []
    for i, m in enumerate(chosen):
        for h, heading in enumerate(pr.HEADINGS[:1] if kind == "L400" else pr.HEADINGS):
            rng = np.random.RandomState(1000 * SETS.index(name) + 10 * i + h)
            mu, S = random_state(rng, L, heading=heading)
            if kind == "tiny":
                S = 1e-6 * np.eye(mu.size)
            motion = (2.0, 2.3, 0.0) if m == "dt0" else mo[m]
            mu_r, S_r = reference_step(mu, S, *motion, [], **pr.step_params(name))
            mu_d, S_d = reference_step(mu, S, *motion, [], dtype=np.float64, **pr.step_params(name))
            pr.agree(mu_d, S_d, mu_r, S_r, f"predict {name} {kind} {m} h{h}")
            if m == "large_turn":                     # the reference wraps once only: the heading stays far outside [-pi, pi)
                assert float(mu_r[2]) < -math.pi - 12 and (h or abs(float(mu_r[2]) + 19.58) < 0.01)
            out.append((f"{name} {kind} {m} h{h}", mu, S, motion, mu_r, S_r))
    return out


def check_predict(name, kind):
    cases = predict_cases(name, kind)
    L = (cases[0][1].size - 3) // 3
    ids = np.arange(L, dtype=np.int32)
    ctx = context(name, ML=L, batch=2)
    ctx.profile_enable(True)
    ctx.add_encoder(0.0, 0.0, 0.0)                    # arms
    moved = 0
    for where, mu, S, (wl, wr, dt), mu_r, S_r in cases:
        ctx.add_encoder(0.0, 0.0, 0.0)                # the clock back to 0 (a sample that moves nothing), so that the next dt is exact
        ctx.set_state(mu, S, ids)
        ctx.profile_reset()
        ctx.add_encoder(wl, wr, dt)
        ctx.sync()
        mu_g, S_g = ctx.get_state()
        assert ekf_kernels_run(ctx.profile_get()) == set(), "aslam_add_encoder is the predict-only launch"
        close("k_ekf_predict", where, mu_g, S_g, mu_r, S_r)
        if dt == 0.0 or (wl == 0.0 and wr == 0.0):    # nothing moves: the bytes stay
            assert mu_g.tobytes() == mu.tobytes() and S_g.tobytes() == S.tobytes(), f"{where}: a sample that moves nothing changed the state"
        else:
            moved += int(not np.array_equal(S_g, S))
    assert moved == sum(1 for c in cases if c[3][2] != 0.0 and (c[3][0] != 0.0 or c[3][1] != 0.0)), "a predict left Sigma as it was"
    ctx.close()


def predict_floor():
    per = {m: [] for m in pr.MUTANTS}
    wraps = set()
    for name, kind in PREDICT_GROUPS:
        for where, mu, S, motion, mu_r, S_r in predict_cases(name, kind):
            p = pr.SETS[name]
            assert pr.moved(*pr.step(mu, S, *motion, [], p), mu_r, S_r) <= 1e-16, f"{where}: predict_terms is not reference_step's predict"
            dth = float(pr.predict_terms(mu[2], *motion, p)[1])
            wraps.add("down" if mu[2] + dth >= math.pi else "up" if mu[2] + dth < -math.pi else "none")
            for m in pr.MUTANTS:
                per[m].append(pr.moved(*pr.step(mu, S, *motion, [], p, mutant=m), mu_r, S_r))
    assert wraps == {"down", "up", "none"}, wraps
    return per


@pytest.mark.parametrize("name,kind", PREDICT_GROUPS)
def test_predict_only(name, kind):
    check_predict(name, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", PREDICT_GROUPS)
def test_predict_only_on_gpu(name, kind):
    check_predict(name, kind)


# ---- 2. per-frame chains: k_ekf_plan<EkfSingle> ------------------------------------------------------------------------------------
# one arming sample, a frame of predict + 4 corrections (reference_step), then a frame that corrects 2 other landmarks and adds 2 new
# ones (the augment follows the predicted pose: LiteralSlam with the parameters, and params_reference.slam_frame in long double)

CHAIN_CASES = ([("fast", "A", m, i % 2) for i, m in enumerate(("forward", "reverse", "spin", "left_only", "right_only", "straight"))]
               + [("fast", "B", m, (i + 1) % 2) for i, m in enumerate(("forward", "reverse", "spin", "left_only", "right_only", "straight",
                                                                      "large_turn"))]
               + [("mid", "A", "right_only", 0), ("mid", "B", "spin", 1), ("general", "A", "spin", 1), ("general", "B", "right_only", 0),
                  ("fast", "defaults", "forward", 0)])
CHAIN_IDS = [f"{c}-{n}-{m}-h{h}" for c, n, m, h in CHAIN_CASES]


def two_slam_frames(rng, name, mname, h, L=8):
    """a dense state and two frames on it: [(wl, wr, dt, [(id, 1, z, Rdiag)] in detection order)], the long-double results after each
    frame and the literal transcription's after the second"""
    p, mo = pr.SETS[name], pr.motions(name)
    mu, S = random_state(rng, L, heading=pr.HEADINGS[h])
    ids = rng.permutation(1024)[:L + 2].astype(np.int32)
    perm = rng.permutation(L)
    seen, later = np.sort(perm[:4]), np.sort(perm[4:6])
    m1, m2 = mo[mname], mo["reverse" if mname != "reverse" else "forward"]
    obs1 = observe(rng, mu, seen, post_predict=predicted_pose(mu, *m1, **pose_kw(name)))
    mu1, S1 = reference_step(mu, S, *m1, obs1, **pr.step_params(name))
    pr.agree(*reference_step(mu, S, *m1, obs1, dtype=np.float64, **pr.step_params(name)), mu1, S1, "frame 1")
    mu1f = np.asarray(mu1, float)
    obs2 = observe(rng, mu1f, later, post_predict=predicted_pose(mu1f, *m2, **pose_kw(name)))
    new = [(int(ids[L + k]), 1, new_z(rng), rng.uniform(0.02, 0.2, 3)) for k in range(2)]
    listed1 = [(int(ids[i]), 1, z, r) for i, z, r in obs1]
    listed2 = [(int(ids[i]), 1, z, r) for i, z, r in obs2] + new
    listed1 = [listed1[i] for i in rng.permutation(len(listed1))]
    listed2 = [listed2[i] for i in rng.permutation(len(listed2))]
    lit = _Injected(**pr.ctx_params(name))
    lit.mu, lit.sigma, lit.id_map = mu.copy(), S.copy(), {int(i): k for k, i in enumerate(ids[:L])}
    lit.add_encoder(0.0, 0.0, 0.0)
    logs = []
    for motion, listed in ((m1, listed1), (m2, listed2)):
        lit.last_time = 0.0                           # (the sample's dt exactly)
        lit.add_encoder(*motion)
        lit._obs = [(o[0], o[2], o[3]) for o in listed]
        k = len(listed)
        lit.add_poses(list(range(k)), np.zeros((k, 8)), np.zeros((k, 3)), np.zeros((k, 3)))
        logs.append(np.array(lit.log, np.int32).reshape(-1, 3))
    by_id = {o[0]: o for o in listed2}
    new_popped = [(by_id[int(i)][2], by_id[int(i)][3]) for i, _, a in logs[1] if a == 0]

    def second(mutant=None, dtype=LD):
        a, b = pr.slam_frame(mu, S, *m1, [], obs1, p, mutant, dtype)
        return pr.slam_frame(a, b, *m2, new_popped, obs2, p, mutant, dtype)
    mu2, S2 = second()
    assert pr.moved(*pr.slam_frame(mu, S, *m1, [], obs1, p), mu1, S1) <= 1e-16
    pr.agree(*second(dtype=np.float64), mu2, S2, "frame 2")
    pr.agree(lit.mu, lit.sigma, mu2, S2, "frame 2, literal transcription")
    floor = {m: pr.moved(*second(mutant=m), mu2, S2) for m in pr.MUTANTS}
    return dict(mu=mu, S=S, ids=ids, L=L, frames=[m1 + (listed1,), m2 + (listed2,)], seen=seen, ref1=(mu1, S1), ref2=(mu2, S2),
                lit=(lit.mu.copy(), lit.sigma.copy()), logs=logs, floor=floor,
                ids_after=np.array([i for i, _ in sorted(lit.id_map.items(), key=lambda kv: kv[1])], np.int32))


@functools.lru_cache(maxsize=None)
def chain_case(chain, name, mname, h):
    return two_slam_frames(np.random.RandomState(7000 + CHAIN_CASES.index((chain, name, mname, h))), name, mname, h)


def check_chain(chain, name, mname, h):
    c = chain_case(chain, name, mname, h)
    L = c["L"]
    ctx = context(name, ML=L + 2, batch=3, cap=CHAIN_CAP[chain])
    ctx.set_state(c["mu"], c["S"], c["ids"][:L])
    f1, f2 = c["frames"]
    ctx.stage_encoders([0.0, f1[0], f2[0]], [0.0, f1[1], f2[1]], [0.0, f1[2], f2[2]])
    inject(ctx, 0, [])
    inject(ctx, 1, f1[3])
    inject(ctx, 2, f2[3])
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.run_staged(0, 2, with_ekf=2)
    ctx.sync()
    ran = ekf_kernels_run(ctx.profile_get())
    assert ran == CHAIN_KERNELS[chain], f"ran {sorted(ran)}"
    where = f"{chain} {name} {mname} h{h}"
    assert np.array_equal(pops_of(ctx), c["logs"][0]), f"{where}: pop order / branches differ"
    assert ctx.get_slot_ekf_stats(1, 1)[0].tolist() == [4, 0, 4, 0]
    close(f"k_ekf_plan<EkfSingle> {chain}", where + " frame 1", *ctx.get_state(), *c["ref1"])
    ctx.run_staged(2, 1, with_ekf=2)
    ctx.sync()
    assert np.array_equal(pops_of(ctx), c["logs"][1]), f"{where}: pop order / branches of the second frame differ"
    assert ctx.get_slot_ekf_stats(2, 1)[0].tolist() == [4, 2, 2, 0]
    mu_g, S_g = ctx.get_state()
    close(f"k_ekf_plan<EkfSingle> {chain}", where + " frame 2", mu_g, S_g, *c["ref2"])
    close(f"k_ekf_plan<EkfSingle> {chain}", where + " frame 2, literal", mu_g, S_g, *c["lit"])
    assert np.array_equal(ctx.get_landmark_ids(), c["ids_after"])
    ctx.close()


def chain_floor():
    per = {m: [] for m in pr.MUTANTS}
    for case in CHAIN_CASES:
        for m, d in chain_case(*case)["floor"].items():
            per[m].append(d)
    return per


@pytest.mark.parametrize("chain,name,mname,h", CHAIN_CASES, ids=CHAIN_IDS)
def test_per_frame_chain(chain, name, mname, h):
    check_chain(chain, name, mname, h)


@pytest.mark.gpu
@pytest.mark.parametrize("chain,name,mname,h", CHAIN_CASES, ids=CHAIN_IDS)
def test_per_frame_chain_on_gpu(chain, name, mname, h):
    check_chain(chain, name, mname, h)


# ---- 3. windows: the prepare wave ---------------------------------------------------------------------------------------------------
# make_case / run_device of tests/test_ekf_window.py with the parameters; the frames cycle through the set's motions, standstill
# included (the first sample arms).  Against the literal transcription after every call (run_device), against the long-double replay and the per-frame chain
# (ASLAM_NO_WINDOWS) at the end.

# name: (groups, landmarks, batch, windows, first motion of the cycle)
WINDOW_SHAPES = {
    "w64": ([(9, R(0, 8), False), (1, [], False)], 8, 10, 1, 0),                     # 27 columns; every motion of the cycle inside the window
    "w128": ([(5, R(0, 22), False)], 22, 5, 1, 2),                                   # 69 columns: the 128-wide image
    "two_empty_first": ([(4, R(0, 8), False), (2, [], False), (2, R(0, 8), False)], 8, 4, 2, 3),   # the second call: empty, empty, full, full
    "empty_middle": ([(5, R(0, 8), False), (1, [], False), (2, R(0, 8), False)], 8, 4, 2, 5),      # the second call: full, empty, full, full
}
WINDOW_CASES = [(s, n) for s in WINDOW_SHAPES for n in ("A", "B")] + [("w64", "defaults")]
PIECE_CASES = [("w64", "A"), ("w64", "B")]


@functools.lru_cache(maxsize=None)
def window_case(shape, name):
    groups, n_land, batch, windows, start = WINDOW_SHAPES[shape]
    nfr = sum(g[0] for g in groups)
    mot = pr.cycle(name, nfr, start=start, skip=("large_turn",))
    if name == "B" and shape == "w64":
        # the turn beyond 2 pi in the window's last frame, which sees nothing: corrections behind a predict of that noise, on sightings
        # that make_case draws without regard to the pose, leave the double reference 1e-10 from the long-double one
        mot[-1] = pr.LARGE_TURN
    frames, exp = make_case(300 + 10 * list(WINDOW_SHAPES).index(shape) + SETS.index(name), groups, n_land, params=pr.ctx_params(name),
                            motions=mot)
    p = pr.SETS[name]
    mu_r, S_r = pr.replay_make_case(frames, exp, p)
    where = f"window {shape} {name}"
    pr.agree(*pr.replay_make_case(frames, exp, p, dtype=np.float64), mu_r, S_r, where)
    pr.agree(exp[-1]["mu"], exp[-1]["sigma"], mu_r, S_r, where + ", literal transcription")
    floor = {m: pr.moved(*pr.replay_make_case(frames, exp, p, mutant=m), mu_r, S_r) for m in pr.MUTANTS}
    return dict(frames=frames, exp=exp, ref=(mu_r, S_r), floor=floor, n_corr=[int((e["log"][:, 2] == 1).sum()) for e in exp])


def check_window(shape, name, path="k_ekf_win_step"):
    _, n_land, batch, windows, _ = WINDOW_SHAPES[shape]
    c = window_case(shape, name)
    kw = dict(params=pr.ctx_params(name), max_landmarks=n_land + 2)
    (mu, S), prof, worst = run_device(c["frames"], c["exp"], batch=batch, **kw)
    assert prof["k_ekf_win_step"][0] >= windows, f"{prof['k_ekf_win_step'][0]} window launches, the case is built for {windows}"
    where = f"{shape} {name}"
    print(f"{path} {where}: worst Sigma error against the literal transcription {worst:.3g}")
    close(path, where, mu, S, *c["ref"])
    (mu2, S2), prof2, _ = run_device(c["frames"], c["exp"], batch=batch, windows=False, **kw)
    assert prof2["k_ekf_win_step"][0] == 0 and prof2["k_ekf_plan"][0] > 0
    close(path, where + ", per-frame chain", mu, S, mu2, S2)
    return prof


def window_floor():
    per = {m: [] for m in pr.MUTANTS}
    for case in WINDOW_CASES:
        for m, d in window_case(*case)["floor"].items():
            per[m].append(d)
    for m, d in gated_window_case("A")["floor"].items():
        per[m].append(d)
    return per


def test_window_shapes_are_what_they_are_built_for():
    for shape, name in WINDOW_CASES:
        c = window_case(shape, name)
        _, n_land, batch, _, _ = WINDOW_SHAPES[shape]
        assert 3 + 3 * n_land <= 64 or (shape == "w128" and 64 < 3 + 3 * n_land <= 128 and n_land > 20)
        calls = [c["n_corr"][f0:f0 + batch] for f0 in range(0, len(c["n_corr"]), batch)]
        if shape == "two_empty_first":
            assert calls[1][:2] == [0, 0] and min(calls[1][2:]) > 0
        if shape == "empty_middle":
            assert calls[1][1] == 0 and calls[1][0] > 0 and min(calls[1][2:]) > 0
        if shape in ("w64", "w128"):
            assert min(c["n_corr"][1:9 if shape == "w64" else None]) == n_land, "a gate dropped an observation"
        if (shape, name) == ("w64", "B"):
            assert c["n_corr"][-1] == 0 and float(c["ref"][0][2]) < -math.pi - 12, "the window's last predict leaves the heading wrapped once"


@pytest.mark.parametrize("shape,name", WINDOW_CASES)
def test_window(shape, name):
    check_window(shape, name)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,name", WINDOW_CASES)
def test_window_on_gpu(shape, name):
    check_window(shape, name)


@pytest.mark.parametrize("shape,name", PIECE_CASES)
def test_window_pieces_of_one_frame(shape, name, monkeypatch):
    """ASLAM_WIN_PIECE = 1: every frame a launch of its own, the prepare wave's own mean instead of the logger's"""
    monkeypatch.setenv("ASLAM_WIN_PIECE", "1")
    prof = check_window(shape, name, path="k_ekf_win_step, pieces of 1")
    assert prof["k_ekf_win_step"][0] > WINDOW_SHAPES[shape][3], "the window was not cut into pieces"


@pytest.mark.gpu
@pytest.mark.parametrize("shape,name", PIECE_CASES)
def test_window_pieces_of_one_frame_on_gpu(shape, name, monkeypatch):
    test_window_pieces_of_one_frame(shape, name, monkeypatch)


# the gated window of tests/test_slam_gate_windows.py: 8 landmarks, five window frames, four planted outliers at gate_d2 = 1
GATED_OUT = {(0, 3), (1, 0), (3, 7), (4, 4)}


@functools.lru_cache(maxsize=None)
def gated_window_case(name):
    L, K = 8, 5
    p, P = pr.SETS[name], pr.ctx_params(name)
    rng = np.random.RandomState(4400 + SETS.index(name))
    mu, S = random_state(rng, L, heading=pr.HEADINGS[SETS.index(name) % 2])
    ids = rng.permutation(gw.ID_TABLE)[:L].astype(np.int32)
    mot = [(0.0, 0.0, 0.0)] + pr.cycle(name, K, start=1)
    plan = [([], set())] + [(R(0, L), {a for k, a in GATED_OUT if k == f}) for f in range(K)]
    frames, marks = gw.make_frames(rng, mu, ids, plan, motions=mot, params=P)
    gw.assert_repeats_decidable(frames)
    lit, per = gw.reference(mu, S, ids, frames, marks=marks, motions=mot, params=P)
    index = {int(i): k for k, i in enumerate(ids)}

    def long_form(dtype):
        a, b = mu, S
        for f in range(1, K + 1):
            obs = sorted(((index[i], z, r) for i, z, r in frames[f]), key=lambda o: o[0])
            a, b, _ = gated_reference_step(a, b, *mot[f], obs, gw.GATE, ids=ids, dtype=dtype, **pr.step_params(name))
        return a, b
    mu_r, S_r = long_form(LD)
    where = f"gated window {name}"
    pr.agree(*long_form(np.float64), mu_r, S_r, where)
    pr.agree(lit.mu, lit.sigma, mu_r, S_r, where + ", gated transcription")
    floor = {}
    for m in pr.MUTANTS:
        mut = pr.MutantGatedLiteral(gate=dict(gate_d2=gw.GATE), mutant=m, **P)
        mut.seat(mu, S, ids)
        for f, obs in enumerate(frames):
            mut.last_time = 0.0
            mut.add_encoder(*mot[f])
            mut.add_frame(obs)
        floor[m] = pr.moved(mut.mu, mut.sigma, lit.mu, lit.sigma)
    return dict(mu=mu, S=S, ids=ids, frames=frames, mot=mot, lit=lit, per=per, ref=(mu_r, S_r), floor=floor)


def check_gated_window(name):
    c, P = gated_window_case(name), pr.ctx_params(name)
    where = f"gated window {name}"
    kw = dict(cap=24, ML=8, motions=c["mot"], params=P)
    run = gw.Run(c["mu"], c["S"], c["ids"], c["frames"], **kw)
    res = gw.check_against_reference(run, c["lit"], c["per"], where)       # 1e-9 / 1e-11, every discrete result exactly
    assert int(res["health"]["rejected"].sum()) == len(GATED_OUT)
    assert res["prof"]["k_ekf_win_step"][0] == 1 and res["prof"][gw.WIN_FINISH][0] == 1, f"ran {sorted(ekf_kernels_run(res['prof']))}"
    mu_g, S_g = res["state"]
    close("k_ekf_win_step, gated", where, mu_g, S_g, *c["ref"])
    twin = gw.Run(c["mu"], c["S"], c["ids"], c["frames"], windows=False, **kw).results()
    assert not any(k.startswith("k_ekf_win") and v[0] > 0 for k, v in twin["prof"].items()), "the twin ran a window kernel"
    assert np.array_equal(res["stats"], twin["stats"]) and np.array_equal(res["ids"], twin["ids"])
    for k in gw.INT_FIELDS:
        assert np.array_equal(res["health"][k], twin["health"][k]), f"{where}: {k} differs from the per-frame twin"
    assert res["track"].tobytes() == twin["track"].tobytes()
    close("k_ekf_win_step, gated", where + ", per-frame chain", mu_g, S_g, *twin["state"])


@pytest.mark.parametrize("name", SETS)
def test_gated_window(name):
    check_gated_window(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_gated_window_on_gpu(name):
    check_gated_window(name)


# ---- 4. localization: loc_steps --------------------------------------------------------------------------------------------------------
# an arming sample and three frames with the motions cycling, 4 of 8 landmarks sighted per frame; the gated variants plant one moved
# marker.  The long-double form of the fixed-map filters is UncertainMapLocalizer on a map of zero covariances.

LOC_VARIANTS = ("plain", "gated", "umap", "umap_gated")
LOC_CASES = [(v, n) for v in LOC_VARIANTS for n in ("A", "B")] + [("plain", "defaults"), ("umap", "defaults")]
GATE = dict(gate_d2=GATE_DEFAULTS["gate_d2"])


def loc_reference(cls, variant, name, ids, xyth, C, pose0, **kw):
    P = pr.ctx_params(name)
    gate = GATE if "gated" in variant else None
    if cls in (UncertainMapLocalizer, pr.MutantUncertain):
        return cls(ids, xyth, C if "umap" in variant else np.zeros((len(ids), 9)), pose0, SIG0, gate=gate, **kw, **P)
    if "gated" in variant:
        return cls(ids, xyth, pose0, SIG0, gate=gate, **kw, **P)
    return cls(ids, xyth, pose0, SIG0, **kw, **P)


def loc_sequence(rng, name, ids, xyth, pose0, start, gated, large_last=False):
    """[(wl, wr, dt, [(id, 1, z, Rdiag)])]: the arming sample and three frames seen from the pose the motion model leaves.
    large_last: the last frame is the turn beyond 2 pi and sees nothing (corrections in or behind a predict of its noise, 4.5 rad^2 on
    the heading, leave the double reference 2e-12 to 6e-12 from the long-double one: measured)"""
    mot = [(0.0, 0.0, 0.0)] + pr.cycle(name, 3, start=start, skip=("standstill", "large_turn"))
    if large_last:
        mot[-1] = pr.LARGE_TURN
    pose = np.asarray(pose0, float)
    bad = 2
    frames = []
    for f, m in enumerate(mot):
        if f:
            pose = predicted_pose(pose, *m, **pose_kw(name))
        sel = [] if m == pr.LARGE_TURN else rng.permutation(len(ids))[:4].tolist()
        frames.append(m + (sight(pose, ids, xyth, sel, rng, moved=(1,) if gated and f == bad else ()),))
    return frames


def run_reference(ref, frames, umap):
    """per frame what the reference leaves; full = the dense Sigma on an uncertain map, Sigma_xx on a fixed one"""
    out = []
    for fr in frames:
        ref.add_encoder(*fr[:3])
        ref.add_observations(fr[3])
        full = ref.full_sigma() if umap else ref.P
        out.append(dict(mu=np.array(ref.mu), P=np.array(ref.P), full=np.array(full), stats=list(ref.stats), log=ref.log_array(),
                        health=dict(ref.health) if getattr(ref, "health", None) else None, track=dict(getattr(ref, "track", {}))))
    return out


@functools.lru_cache(maxsize=None)
def loc_case(variant, name):
    k = LOC_CASES.index((variant, name))
    rng = np.random.RandomState(5100 + k)
    n = 8
    ids, xyth = random_map(rng, n)
    C = spd_blocks(rng, n)
    pose0 = np.array([0.1, -0.2, pr.HEADINGS[k % 2]])
    frames = loc_sequence(rng, name, ids, xyth, pose0, start=k, gated="gated" in variant, large_last=name == "B" and "gated" not in variant)
    ref = loc_reference(UncertainMapLocalizer, variant, name, ids, xyth, C, pose0)          # long double
    want = run_reference(ref, frames, "umap" in variant)
    ref.assert_margins()
    where = f"localize {variant} {name}"
    if "umap" in variant:
        dbl = run_reference(loc_reference(UncertainMapLocalizer, variant, name, ids, xyth, C, pose0, dtype=np.float64), frames, "umap" in variant)
    else:
        dbl = run_reference(loc_reference(GatedLocalizer if "gated" in variant else FrozenMapLocalizer, variant, name, ids, xyth, C, pose0), frames, "umap" in variant)
    pr.agree(dbl[-1]["mu"], dbl[-1]["full"], ref.x, ref.S if "umap" in variant else ref.S[:3, :3], where)
    assert all(np.array_equal(a["log"], b["log"]) and a["stats"] == b["stats"] for a, b in zip(dbl, want))
    if "gated" in variant:
        assert sum(int((w["log"][:, 2] == 3).sum()) for w in want) == 1, "the reference alone rejects the moved marker and nothing else"
    if "umap" in variant:
        assert np.abs(ref.cross).max() > 1e-6, "the cross block is not live"
    if frames[-1][:3] == pr.LARGE_TURN:
        assert want[-1]["mu"][2] < -math.pi - 12, "the single wrap leaves the heading far outside [-pi, pi)"
    floor = {}
    for m in pr.MUTANTS:
        cls = pr.MutantUncertain if "umap" in variant else pr.MutantGated if "gated" in variant else pr.MutantFrozen
        mut = run_reference(loc_reference(cls, variant, name, ids, xyth, C, pose0, mutant=m), frames, "umap" in variant)[-1]
        floor[m] = pr.moved(mut["mu"], mut["full"], want[-1]["mu"], want[-1]["full"])
    return dict(ids=ids, xyth=xyth, C=C, pose0=pose0, frames=frames, want=want, ref=ref, floor=floor)


def check_strip(path, where, pose, X, want):
    """pose and the strip [Sigma_xx | Sigma_xl] against the reference: 1e-9 on the pose (rtol 1e-9, atol 1e-11), 1e-9 of max |Sigma|"""
    full = want["full"]
    close(path, where, np.asarray(pose), np.asarray(X), want["mu"], full[:3, :X.shape[1]])
    if X.shape[1] > 3:
        e = float(np.abs(X[:, 3:] - full[:3, 3:]).max() / np.abs(full).max())
        assert e <= 1e-9, f"{where}: the cross block Sigma_xl differs by {e} of max |Sigma|"


def check_localize(variant, name):
    c = loc_case(variant, name)
    ids, xyth, frames = c["ids"], c["xyth"], c["frames"]
    ctx = context(name, ML=len(ids), batch=len(frames))
    if "gated" in variant:
        ctx.set_innovation_gate(**GATE)
    if "umap" in variant:
        ctx.localize_begin_uncertain(ids, xyth, c["C"], c["pose0"], SIG0)
    else:
        ctx.localize_begin(ids, xyth, c["pose0"], SIG0)
    assert ctx.is_localizing() and ctx.is_map_uncertain() == ("umap" in variant) and (ctx.get_innovation_gate() is not None) == ("gated" in variant)
    ctx.stage_encoders(*[[f[k] for f in frames] for k in range(3)])
    for s, fr in enumerate(frames):
        inject(ctx, s, fr[3])
    ctx.profile_enable(True)
    ctx.profile_reset()
    path = "k_loc_steps" + {"plain": "", "gated": "_gated", "umap": "_umap", "umap_gated": "_umap_gated"}[variant]
    for s, w in enumerate(c["want"]):
        ctx.run_staged(s, 1, with_ekf=2)
        ctx.sync()
        where = f"{variant} {name} frame {s}"
        mu, S = ctx.get_state()
        check_strip(path, where, mu[:3], S[:3, :] if "umap" in variant else S[:3, :3], w)
        assert np.array_equal(mu[3:], xyth.reshape(-1)), f"{where}: the map moved"
        if "umap" not in variant:
            assert not S[3:, :].any() and not S[:, 3:].any(), f"{where}: a landmark block is not zero"
        assert np.array_equal(pops_of(ctx), w["log"]), f"{where}: pops / actions differ"
        assert ctx.get_slot_ekf_stats(s, 1)[0].tolist() == w["stats"], where
        if "gated" in variant:
            check_slot_health(ctx.get_slot_health(s, 1)[0], w["health"], where)
            check_track(ctx.get_track_health(), w["track"], where)
    assert ctx.profile_get()["k_loc_steps"][0] == len(frames)
    ctx.close()


def loc_floor():
    per = {m: [] for m in pr.MUTANTS}
    for case in LOC_CASES:
        for m, d in loc_case(*case)["floor"].items():
            per[m].append(d)
    return per


@pytest.mark.parametrize("variant,name", LOC_CASES)
def test_localize(variant, name):
    check_localize(variant, name)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,name", LOC_CASES)
def test_localize_on_gpu(variant, name):
    check_localize(variant, name)


# ---- 5. fleet localization: two robots on different motions ----------------------------------------------------------------------------

FLEET_LOC_CASES = [(v, n) for v in ("plain", "umap") for n in ("A", "B")] + [("plain", "defaults")]


@functools.lru_cache(maxsize=None)
def fleet_loc_case(variant, name):
    k = FLEET_LOC_CASES.index((variant, name))
    rng = np.random.RandomState(6100 + k)
    n = 8
    ids, xyth = random_map(rng, n)
    C = spd_blocks(rng, n)
    poses0 = np.array([[0.1, -0.2, pr.HEADINGS[0]], [-0.4, 0.3, pr.HEADINGS[1]]])
    seqs = [loc_sequence(rng, name, ids, xyth, poses0[r], start=k + 4 * r, gated=False, large_last=name == "B" and r == 1) for r in range(2)]
    assert all(a[:3] != b[:3] for a, b in zip(seqs[0][1:], seqs[1][1:])), "the two robots are on the same motion"
    refs, want, floor = [], [], {m: 0.0 for m in pr.MUTANTS}
    for r in range(2):
        ref = loc_reference(UncertainMapLocalizer, variant, name, ids, xyth, C, poses0[r])
        want.append(run_reference(ref, seqs[r], variant == "umap"))
        refs.append(ref)
        where = f"fleet localize {variant} {name} robot {r}"
        if variant == "umap":
            dbl = run_reference(loc_reference(UncertainMapLocalizer, variant, name, ids, xyth, C, poses0[r], dtype=np.float64), seqs[r], variant == "umap")
        else:
            dbl = run_reference(loc_reference(FrozenMapLocalizer, variant, name, ids, xyth, C, poses0[r]), seqs[r], variant == "umap")
        pr.agree(dbl[-1]["mu"], dbl[-1]["full"], ref.x, ref.S if variant == "umap" else ref.S[:3, :3], where)
        for m in pr.MUTANTS:
            mut = run_reference(loc_reference(pr.MutantUncertain if variant == "umap" else pr.MutantFrozen, variant, name, ids, xyth, C,
                                              poses0[r], mutant=m), seqs[r], variant == "umap")[-1]
            floor[m] = max(floor[m], pr.moved(mut["mu"], mut["full"], want[r][-1]["mu"], want[r][-1]["full"]))
    return dict(ids=ids, xyth=xyth, C=C, poses0=poses0, seqs=seqs, want=want, floor=floor)


def check_fleet_localize(variant, name):
    c = fleet_loc_case(variant, name)
    ids, xyth, seqs = c["ids"], c["xyth"], c["seqs"]
    T = len(seqs[0])
    ctx = context(name, ML=len(ids), batch=2 * T)
    if variant == "umap":
        ctx.fleet_begin_uncertain([CAM] * 2, ids, xyth, c["C"], c["poses0"], [SIG0] * 2)
    else:
        ctx.fleet_begin([CAM] * 2, ids, xyth, c["poses0"], [SIG0] * 2)
    assert ctx.is_fleet() and ctx.is_map_uncertain() == (variant == "umap")
    order = [r for t in range(T) for r in (1, 0)]
    frames = [seqs[r][t] for t in range(T) for r in (1, 0)]
    ctx.profile_enable(True)
    ctx.profile_reset()
    fleet_call(ctx, order, frames)
    ctx.sync()
    assert ctx.profile_get()["k_fleet_steps"][0] >= 1 and ctx.profile_get()["k_loc_steps"][0] == 0
    stats = ctx.get_slot_ekf_stats(0, len(order))
    for s, r in enumerate(order):
        assert stats[s].tolist() == c["want"][r][s // 2]["stats"], f"slot {s} (robot {r})"
    poses, sigs = ctx.fleet_get_poses()
    path = "k_fleet_steps" + ("_umap" if variant == "umap" else "")
    for r in range(2):
        X = np.concatenate([sigs[r], ctx.fleet_get_cross(r)], 1) if variant == "umap" else sigs[r]
        check_strip(path, f"{variant} {name} robot {r}", poses[r], X, c["want"][r][-1])
    ctx.close()


def fleet_loc_floor():
    per = {m: [] for m in pr.MUTANTS}
    for case in FLEET_LOC_CASES:
        for m, d in fleet_loc_case(*case)["floor"].items():
            per[m].append(d)
    return per


@pytest.mark.parametrize("variant,name", FLEET_LOC_CASES)
def test_fleet_localize(variant, name):
    check_fleet_localize(variant, name)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,name", FLEET_LOC_CASES)
def test_fleet_localize_on_gpu(variant, name):
    check_fleet_localize(variant, name)


# ---- 6. fleet SLAM: k_ekf_plan<EkfFleet> --------------------------------------------------------------------------------------------------
# two robots, each on a dense state of its own, through the two frames of section 2 on different motions

FLEET_SLAM_CASES = [("A", ("right_only", "spin")), ("B", ("large_turn", "right_only")), ("defaults", ("forward", "right_only"))]


@functools.lru_cache(maxsize=None)
def fleet_slam_case(name, mnames):
    k = [c[0] for c in FLEET_SLAM_CASES].index(name)
    return [two_slam_frames(np.random.RandomState(8000 + 10 * k + r), name, mnames[r], r) for r in range(2)]


def check_fleet_slam(name, mnames):
    robots = fleet_slam_case(name, mnames)
    L = robots[0]["L"]
    ctx = context(name, ML=L + 2, batch=6)
    ctx.fleet_slam_begin([CAM] * 2)
    assert ctx.is_fleet_slam()
    for r, c in enumerate(robots):
        ctx.fleet_set_state(r, c["mu"], c["S"], c["ids"][:L])
    order = [1, 0] * 3
    frames = [(0.0, 0.0, 0.0, [])] * 2 + [robots[r]["frames"][t] for t in range(2) for r in (1, 0)]
    ctx.profile_enable(True)
    ctx.profile_reset()
    fleet_call(ctx, order, frames)
    ctx.sync()
    ran = ekf_kernels_run(ctx.profile_get())
    assert ran == CHAIN_KERNELS["fast"], f"ran {sorted(ran)}"
    stats = ctx.get_slot_ekf_stats(0, 6)
    assert stats.tolist() == [[0, 0, 0, 0]] * 2 + [[4, 0, 4, 0]] * 2 + [[4, 2, 2, 0]] * 2
    for r, c in enumerate(robots):
        mu_g, S_g = ctx.fleet_get_state(r)
        where = f"{name} robot {r} {mnames[r]}"
        close("k_ekf_plan<EkfFleet>", where, mu_g, S_g, *c["ref2"])
        close("k_ekf_plan<EkfFleet>", where + ", literal", mu_g, S_g, *c["lit"])
        assert np.array_equal(ctx.fleet_get_landmark_ids(r), c["ids_after"])
    ctx.close()


def fleet_slam_floor():
    per = {m: [] for m in pr.MUTANTS}
    for case in FLEET_SLAM_CASES:
        for c in fleet_slam_case(*case):
            for m, d in c["floor"].items():
                per[m].append(d)
    return per


@pytest.mark.parametrize("name,mnames", FLEET_SLAM_CASES)
def test_fleet_slam(name, mnames):
    check_fleet_slam(name, mnames)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mnames", FLEET_SLAM_CASES)
def test_fleet_slam_on_gpu(name, mnames):
    check_fleet_slam(name, mnames)


# ---- the case sets can tell every mutant apart (CPU only) ------------------------------------------------------------------------------

FLOORS = {"k_ekf_predict": predict_floor, "per-frame chains": chain_floor, "windows": window_floor, "localization": loc_floor,
          "fleet localization": fleet_loc_floor, "fleet SLAM": fleet_slam_floor}


@pytest.mark.parametrize("path", sorted(FLOORS))
def test_sensitivity_floor(path):
    """every mutant moves at least one case of the path by 1e-6, a thousand times the tolerance the device is held to"""
    per = FLOORS[path]()
    print(path, {m: f"{v:.2e}" for m, v in pr.check_floor(path, per).items()})
    if path == "k_ekf_predict":                       # left_only is blind to kr in the second noise column, right_only is not
        p = pr.SETS["A"]
        for where, mu, S, motion, mu_r, S_r in predict_cases("A", "random"):
            d = pr.moved(*pr.step(mu, S, *motion, [], p, mutant="kr_noise"), mu_r, S_r)
            assert "left_only" not in where or d == 0.0
            assert "right_only" not in where or d >= pr.FLOOR


def test_control_cases_are_blind_to_what_kl_equal_kr_hides():
    """the defaults cannot tell kl from kr: what the suite could not see before these cases"""
    for where, mu, S, motion, mu_r, S_r in predict_cases("defaults", "random"):
        for m in ("swap_k", "kr_noise", "Qk_default"):
            assert pr.moved(*pr.step(mu, S, *motion, [], pr.DEFAULTS, mutant=m), mu_r, S_r) == 0.0, (where, m)


def test_a_case_set_that_cannot_tell_a_mutant_apart_fails():
    per = {m: [1.0] for m in pr.MUTANTS}
    per["kr_noise"] = [0.0, 5e-7]
    with pytest.raises(AssertionError, match="kr_noise"):
        pr.check_floor("a blind path", per)
    with pytest.raises(AssertionError):
        pr.check_floor("a path without a mutant", {m: [1.0] for m in pr.MUTANTS[:-1]})


def test_straight_motions_are_exactly_straight():
    for name in ("A", "B"):
        wl, wr, dt = pr.straight(pr.SETS[name])
        assert wl != wr and float(pr.predict_terms(0.3, wl, wr, dt, pr.SETS[name], dtype=np.float64)[1]) == 0.0
