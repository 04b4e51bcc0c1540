"""The hand-over of an EKF window on states far larger than the window (ekf_window.hip: k_ekf_win_gather, k_ekf_win_thin,
k_ekf_update_mfma at depth SP, k_ekf_win_fix; between two windows k_ekf_win_next or its four-launch form), against the long-double
step of tests/ekf_reference.py applied frame by frame.

A window runs its frames on the image of its set S; the rest R of mu and Sigma follows once per window through the hand-over, work
proportional to N = 3 + 3 L with the 64 / 128 / 160 / 256 wide tiles, the `c < N` guards and the leading dimension's residues.  Every
case here seats a dense random state (random_state: the cross-covariances between S and R are not small, the heading lies just below
pi) with L far above |S|, arms the filter with an empty frame and lets K frames observe the frame's landmark set (shuffled detection
order, no "stationary" repeat: make_frames of test_slam_gate_windows.py).  Before anything numeric, exact: the last frame's pop list,
[m, 0, m, 0] for every frame, the number of windows planned, k_ekf_win_flush once per window, k_ekf_win_next as the mode has it.

The shapes (landmark i = state rows 3 + 3 i .. 5 + 3 i; landmarks 20, 41, 62 / 63 straddle, end at or start at rows 64 / 128 / 192):
  1. edges      one T = 4 window, N = 129 .. 258 around the tile edges, max_landmarks = L and one above it so that the leading
                dimension takes every residue 0 / 1 / 63 (mod 64): N = ld and N < ld
  2. widths     |S| = 20, 21, 41, 42, 63 (images of 64, 128, 192) on L = 106
  3. next       window -> window on a rest, the three entry kinds of k_ekf_win_next, in the modes default, ASLAM_WIN_NEXT_SPLIT and
                ASLAM_WIN_NO_EARLY; default and split are equal to the bit (the claim above k_ekf_win_next)
  4. tile160    max_landmarks 937 / 938 / 1065 / 1066 (k_ekf_update_mfma<5> for 938 .. 1065: update_tile4 looks at ld only) with
                N = 159, 162, 321, 324 around its 160 and 320 column edges
  5. headline   L = 200, 20 corrections a frame, 4 frames
  6. padding    a case of 1. with max_landmarks > L, followed in the same batch by a frame with a new marker id: the augment builds on
                what the hand-over left beyond N (LiteralSlam in double; the project's 1e-9 bar)
  7. gated      one gated window on a rest, one planted outlier (helpers and bars of test_slam_gate_windows.py)
  8. full size  GPU only: L = max_landmarks = 937 .. 1066, |S| = 40, against the step in double at the project's 1e-9 bar (long double
                takes minutes at N = 3000)
Every case of 1. to 7. runs on the session's library (the emulation without a GPU; each takes under three seconds there) and once more
marked gpu through the same function; 8. is gpu only.

What is compared in 1. to 5.: the error of each block relative to the largest magnitude of that block in the reference: mu over pose
and S, mu over R, Sigma[S,S], Sigma[S,R], Sigma[R,S] (both copies are written), Sigma[R,R]; S is the last window's set.  One
assertion is exact: Sigma[S,R] == Sigma[R,S]^T, k_ekf_win_fix stores one value to both places.

Measured worst cases over all cases of 1. to 5., emulation build / MI355X (the bounds in EMU_TOL / GPU_TOL are at most 10x these;
the margin covers other seeds and a compiler's re-association; three other sets of seeds stayed within 2x of them on the emulation):
  block  emulation  MI355X    EMU_TOL  GPU_TOL   worst case
  mu_S   1.09e-15   1.09e-15  1e-14    1e-14     widths, |S| = 42
  mu_R   6.60e-16   6.60e-16  6e-15    6e-15     next, cap64
  S_SS   2.42e-15   2.53e-15  2e-14    2e-14     widths, |S| = 41
  S_SR   1.49e-14   1.49e-14  1e-13    1e-13     next, cap64, ASLAM_WIN_NO_EARLY
  S_RS   1.49e-14   1.49e-14  1e-13    1e-13     next, cap64, ASLAM_WIN_NO_EARLY
  S_RR   4.13e-15   3.87e-15  4e-14    3e-14     widths, |S| = 63
6., 7. and 8. keep the project's bars, their references are in double; measured there, emulation / MI355X: 6. Sigma 1.0e-15 /
9.0e-16 relative, 7. Sigma 5.9e-16 / 6.9e-16 against the reference, 8. (MI355X only) Sigma 3.7e-15, its worst block S_RS 7.3e-15.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from aruco_slam_amd import capi
from ekf_reference import LD, random_state, reference_step, rel_err
from test_ekf_sizes import DT, LD_RESIDUES, WL, WR, _above, _Injected, landmark_ids, pick
from test_slam_gate_windows import Run, assert_repeats_decidable, check_against_reference, check_against_twin, make_frames, reference

BLOCKS = ("mu_S", "mu_R", "S_SS", "S_SR", "S_RS", "S_RR")
# bounds per library, each at most 10x the worst case measured on it (the module docstring), none looser than the project's 1e-9
EMU_TOL = dict(mu_S=1e-14, mu_R=6e-15, S_SS=2e-14, S_SR=1e-13, S_RS=1e-13, S_RR=4e-14)
GPU_TOL = dict(mu_S=1e-14, mu_R=6e-15, S_SS=2e-14, S_SR=1e-13, S_RS=1e-13, S_RR=3e-14)


@pytest.fixture(scope="module")
def tol(on_emulation):
    return EMU_TOL if on_emulation else GPU_TOL


# ---- the case builder and its reference -------------------------------------------------------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def build_case(seed, L, sets, tail=(), dtype=LD):
    """sets = ((frames, landmark indices), ...): a dense state of L landmarks, frame 0 arming the filter, then each set observed in
    `frames` frames; tail: known landmarks of one more frame, which also sees a marker id the map does not hold.  The reference
    (shared by every run of the case, read only): reference_step in `dtype` frame by frame over the frames of `sets`."""
    rng = np.random.RandomState(seed)
    mu, S = random_state(rng, L)
    ids, _ = landmark_ids(rng, L)
    seen = [sorted(s) for k, s in sets for _ in range(k)] + ([sorted(tail)] if tail else [])
    frames, _ = make_frames(rng, mu, ids, [([], set())] + [(s, set()) for s in seen])
    assert_repeats_decidable(frames)
    if tail:
        new_id = next(i for i in range(1024) if i not in set(ids.tolist()))
        z = np.array([rng.uniform(0.5, 2), rng.uniform(-1, 1), rng.uniform(-3, 3)])
        frames[-1].insert(int(rng.randint(len(tail) + 1)), (new_id, z, rng.uniform(0.02, 0.2, 3)))
    index = {}
    for k, i in enumerate(ids):
        index.setdefault(int(i), k)
    mu_r, S_r = np.array(mu, dtype), np.array(S, dtype)
    n_win = len(frames) - (1 if tail else 0)
    for obs in frames[1:n_win]:
        pops = sorted(((index[i], z, r) for i, z, r in obs), key=lambda o: o[0])
        mu_r, S_r = reference_step(mu_r, S_r, WL, WR, DT, pops, dtype=dtype)
    _frozen(mu, S, ids, mu_r, S_r)
    return dict(mu=mu, S=S, ids=ids, frames=frames, seen=seen, mu_r=mu_r, S_r=S_r)


@contextlib.contextmanager
def switches(names):
    """the environment switches a context reads when it is created"""
    for n in names:
        os.environ[n] = "1"
    try:
        yield
    finally:
        for n in names:
            os.environ.pop(n, None)


def run_batch(c, cap, ML, env=(), waves=4):
    """the case's frames in one batch on a fresh context (profile on); returns the context"""
    frames, n = c["frames"], len(c["frames"])
    with switches(env):
        ctx = capi.Context(max_rows=64, max_cols=64, max_batch=n, persistent_waves=waves, max_landmarks=ML, max_updates_per_frame=cap)
    ctx.set_state(c["mu"], c["S"], c["ids"])
    ctx.stage_encoders([0.0] + [WL] * (n - 1), [0.0] + [WR] * (n - 1), [0.0] + [DT] * (n - 1))
    for s, obs in enumerate(frames):
        ctx.inject_observations(s, [o[0] for o in obs], [1] * len(obs), np.array([o[1] for o in obs]).reshape(-1, 3),
                                np.array([o[2] for o in obs]).reshape(-1, 3))
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.run_staged(0, n, with_ekf=2)
    ctx.sync()
    return ctx


def run_case(c, cap, ML, windows, env=(), waves=4):
    """run_batch and the exact preconditions; returns (mu, Sigma, profile)"""
    ctx, n = run_batch(c, cap, ML, env, waves), len(c["frames"])
    n_win = len(c["seen"])
    assert ctx.get_slot_ekf_stats(0, n).tolist() == [[0, 0, 0, 0]] + [[len(s), 0, len(s), 0] for s in c["seen"]]
    gi, gx, ga, _, _ = ctx.get_observations()
    last = np.array(c["seen"][-1])
    assert np.array_equal(gx, last) and np.array_equal(gi, c["ids"][last]) and (ga == 1).all(), "pop order / branches differ"
    plan, prof = ctx.plan_stats(), ctx.profile_get()
    assert plan["windows"] == windows and plan["frames_in_windows"] == n_win and plan["frames_device_planned"] == 0, f"plan {plan}"
    assert prof["k_ekf_win_flush"][0] == windows, f"k_ekf_win_flush ran {prof['k_ekf_win_flush'][0]} times for {windows} windows"
    early = 0 if "ASLAM_WIN_NO_EARLY" in env else windows - 1
    assert prof["k_ekf_win_next"][0] == early, f"k_ekf_win_next ran {prof['k_ekf_win_next'][0]} times, {early} expected"
    mu_g, S_g = ctx.get_state()
    ctx.close()
    return mu_g, S_g, prof


def rows_of(landmarks):
    return np.concatenate([[0, 1, 2]] + [[3 + 3 * i, 4 + 3 * i, 5 + 3 * i] for i in landmarks]).astype(int)


def block_errors(mu_g, S_g, mu_r, S_r, landmarks):
    """the six block errors, each relative to the largest magnitude of its block in the reference; Sigma[S,R] against Sigma[R,S]^T"""
    assert mu_g.shape == mu_r.shape and S_g.shape == S_r.shape and np.isfinite(mu_g).all() and np.isfinite(S_g).all()
    s = rows_of(landmarks)
    r = np.setdiff1d(np.arange(mu_r.size), s)
    assert r.size > 0, "the case has no rest"
    sub = lambda A, a, b: A[np.ix_(a, b)]
    e = dict(mu_S=rel_err(mu_g[s], mu_r[s]), mu_R=rel_err(mu_g[r], mu_r[r]), S_SS=rel_err(sub(S_g, s, s), sub(S_r, s, s)),
             S_SR=rel_err(sub(S_g, s, r), sub(S_r, s, r)), S_RS=rel_err(sub(S_g, r, s), sub(S_r, r, s)),
             S_RR=rel_err(sub(S_g, r, r), sub(S_r, r, r)))
    return e, np.array_equal(sub(S_g, s, r), sub(S_g, r, s).T)


def check_blocks(name, got, c, tol):
    """prints every figure, then asserts the symmetry of the two copies and the bound of every block"""
    mu_g, S_g = got[0], got[1]
    e, mirrored = block_errors(mu_g, S_g, c["mu_r"], c["S_r"], c["seen"][-1])
    print(f"flush {name}: " + " ".join(f"{k} {e[k]:.3g}" for k in BLOCKS) + f" mirrored {mirrored}")
    assert mirrored, f"{name}: Sigma[S,R] is not Sigma[R,S]^T to the bit"
    bad = {k: e[k] for k in BLOCKS if not e[k] <= tol[k]}
    assert not bad, f"{name}: blocks past their bound: {bad} (bounds {tol})"


# ---- 1. one window, N at the tile edges -------------------------------------------------------------------------------------------

EDGE_L = (42, 52, 53, 63, 64, 84, 85)
EDGES = [(L, ML) for j, L in enumerate(EDGE_L) for ML in (L, _above(L, LD_RESIDUES[j % 3]))]
K_EDGE = 3


def edge_set(L):
    return tuple(sorted({i for i in (0, 20, 41, 42, 62, 63, L - 1) if i < L}))


def _edge(L, ML, tol):
    c = build_case(1000 + L, L, ((K_EDGE, edge_set(L)),))
    check_blocks(f"edges L {L} max_landmarks {ML} (N {3 + 3 * L}, ld {3 + 3 * ML})", run_case(c, 24, ML, 1), c, tol)


def test_edges_cover_every_leading_dimension_residue():
    assert {(3 + 3 * ml) % 64 for _, ml in EDGES} >= {0, 1, 63}
    assert any(ml == L for L, ml in EDGES) and any(ml > L for L, ml in EDGES)
    assert all(3 + 3 * len(edge_set(L)) <= 64 for L in EDGE_L)                    # T = 4


@pytest.mark.parametrize("L,ML", EDGES, ids=[f"L{L}-ml{ml}" for L, ml in EDGES])
def test_one_window_at_the_tile_edges(L, ML, tol):
    _edge(L, ML, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("L,ML", EDGES, ids=[f"L{L}-ml{ml}" for L, ml in EDGES])
def test_one_window_at_the_tile_edges_on_gpu(L, ML, tol):
    _edge(L, ML, tol)


# ---- 2. the three widths on a rest ------------------------------------------------------------------------------------------------

WIDTH_L = 106
WIDTH_SETS = (20, 21, 41, 42, 63)


def width_set(n):
    """landmarks 0 and 105 and n - 2 scattered between them"""
    return tuple(pick(np.random.RandomState(n), np.arange(WIDTH_L), n).tolist())


def _widths(n, tol):
    c = build_case(2000 + n, WIDTH_L, ((3, width_set(n)),))
    check_blocks(f"widths |S| {n}", run_case(c, 64, WIDTH_L, 1), c, tol)


def test_width_sets_select_the_three_images():
    tiles = [-(-(3 + 3 * len(width_set(n))) // 64) for n in WIDTH_SETS]
    assert tiles == [1, 2, 2, 3, 3] and all({0, WIDTH_L - 1} <= set(width_set(n)) and len(set(width_set(n))) == n for n in WIDTH_SETS)


@pytest.mark.parametrize("n", WIDTH_SETS)
def test_three_widths_on_a_rest(n, tol):
    _widths(n, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("n", WIDTH_SETS)
def test_three_widths_on_a_rest_on_gpu(n, tol):
    _widths(n, tol)


# ---- 3. window to window on a rest ------------------------------------------------------------------------------------------------

# the union of the two sets exceeds the set limit of the context (41 landmarks for cap <= 24, 63 above): two windows
NEXT = {
    "cap24": dict(cap=24, L=85, ML=106, sets=(tuple(range(0, 24)), tuple(range(20, 44)))),
    "cap64": dict(cap=64, L=106, ML=106, sets=(tuple(range(0, 50)), tuple(range(40, 90)))),
    # the second set holds landmarks 0 and L - 1, which the first lacked
    "ends": dict(cap=24, L=85, ML=106, sets=(tuple(range(1, 24)), (0,) + tuple(range(20, 42)) + (84,))),
}
MODES = {"default": (), "split": ("ASLAM_WIN_NEXT_SPLIT",), "no_early": ("ASLAM_WIN_NO_EARLY",)}


def _next(name, tol):
    p = NEXT[name]
    a, b = (set(s) for s in p["sets"])
    assert a & b and a - b and b - a and len(a | b) > (41 if p["cap"] <= 24 else 63)        # the three entry kinds; two windows
    c = build_case(3000 + len(name) + p["L"], p["L"], tuple((3, s) for s in p["sets"]))
    got = {}
    for mode, env in MODES.items():
        got[mode] = run_case(c, p["cap"], p["ML"], 2, env=env)
        check_blocks(f"next {name} {mode}", got[mode], c, tol)
    assert np.array_equal(got["default"][0], got["split"][0]) and np.array_equal(got["default"][1], got["split"][1]), \
        f"{name}: k_ekf_win_next and its four-launch form differ in a bit"


@pytest.mark.parametrize("name", sorted(NEXT))
def test_window_to_window_on_a_rest(name, tol):
    _next(name, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NEXT))
def test_window_to_window_on_a_rest_on_gpu(name, tol):
    _next(name, tol)


# ---- 4. the 160-wide update tile in its window role -------------------------------------------------------------------------------

TILE160 = [(L, ML) for ML in (937, 938, 1065, 1066) for L in (52, 53, 106, 107)]


def _tile160(L, ML, tol):
    c = build_case(4000 + L, L, ((3, (0, 20, 41, L - 1)),))
    check_blocks(f"tile160 L {L} max_landmarks {ML} (N {3 + 3 * L})", run_case(c, 24, ML, 1), c, tol)


@pytest.mark.parametrize("L,ML", TILE160, ids=[f"L{L}-ml{ml}" for L, ml in TILE160])
def test_wide_update_tile_in_its_window_role(L, ML, tol):
    _tile160(L, ML, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("L,ML", TILE160, ids=[f"L{L}-ml{ml}" for L, ml in TILE160])
def test_wide_update_tile_in_its_window_role_on_gpu(L, ML, tol):
    _tile160(L, ML, tol)


# ---- 5. the headline shape --------------------------------------------------------------------------------------------------------

def _headline(tol):
    seen = tuple(sorted(set(range(100, 116)) | {0, 20, 41, 199}))
    assert len(seen) == 20
    c = build_case(5000, 200, ((4, seen),))
    check_blocks("headline L 200", run_case(c, 24, 208, 1), c, tol)


def test_headline_shape(tol):
    _headline(tol)


@pytest.mark.gpu
def test_headline_shape_on_gpu(tol):
    _headline(tol)


# ---- 6. the padding after a window ------------------------------------------------------------------------------------------------

def _padding():
    """the augment of a new landmark right after a window reads Sigma and mu beyond N as the hand-over left them"""
    L, ML, tail = 85, _above(85, LD_RESIDUES[0]), (30, 84)
    c = build_case(6000, L, ((K_EDGE, edge_set(L)),), tail=tail)
    frames = c["frames"]
    lit = _Injected()
    lit.mu, lit.sigma = c["mu"].copy(), c["S"].copy()
    lit.id_map = {int(i): k for k, i in enumerate(c["ids"])}
    for f, obs in enumerate(frames):
        lit.last_time = 0.0                                        # (every sample's dt is DT exactly)
        lit.add_encoder(WL if f else 0.0, WR if f else 0.0, DT if f else 0.0)
        lit._obs = obs
        lit.add_poses(list(range(len(obs))), np.zeros((len(obs), 8)), np.zeros((len(obs), 3)), np.zeros((len(obs), 3)))
    lg = np.array(lit.log, np.int32).reshape(-1, 3)
    assert lg[:, 1].tolist() == [-1, 30, 84] and lg[:, 2].tolist() == [0, 1, 1]
    ctx, n = run_batch(c, 24, ML), len(frames)
    m = len(edge_set(L))
    assert ctx.get_slot_ekf_stats(0, n).tolist() == [[0, 0, 0, 0]] + [[m, 0, m, 0]] * K_EDGE + [[3, 1, 2, 0]]
    gi, gx, ga, _, _ = ctx.get_observations()
    assert np.array_equal(np.stack([gi, gx, ga], 1).reshape(-1, 3), lg), "pop order / branches differ"
    plan, prof = ctx.plan_stats(), ctx.profile_get()
    assert plan["windows"] == 1 and plan["frames_in_windows"] == K_EDGE and prof["k_ekf_win_flush"][0] == 1, f"plan {plan}"
    mu_g, S_g = ctx.get_state()
    assert mu_g.shape == lit.mu.shape == (3 + 3 * (L + 1),)
    e_mu, e_S = float(np.abs(mu_g - lit.mu).max()), rel_err(S_g, lit.sigma)
    e_new = rel_err(S_g[-3:, :], lit.sigma[-3:, :]), rel_err(S_g[:, -3:], lit.sigma[:, -3:])
    print(f"padding after a window: |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative, the new rows {e_new[0]:.3g}, columns {e_new[1]:.3g}")
    assert np.allclose(mu_g, lit.mu, rtol=1e-9, atol=1e-11), f"mu differs by {e_mu}"
    assert e_S <= 1e-9 and max(e_new) <= 1e-9, f"Sigma differs by {e_S} (relative), the new landmark's by {e_new}"


def test_augment_after_a_window_builds_on_clean_padding():
    _padding()


@pytest.mark.gpu
def test_augment_after_a_window_builds_on_clean_padding_on_gpu():
    _padding()


# ---- 7. one gated window on a rest ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gated_case():
    rng = np.random.RandomState(7000)
    L = 85
    mu, S = random_state(rng, L)
    ids, _ = landmark_ids(rng, L)
    seen = list(edge_set(L))
    plan = [([], set()), (seen, set()), (seen, {3}), (seen, set())]
    frames, marks = make_frames(rng, mu, ids, plan)
    assert_repeats_decidable(frames)
    lit, per = reference(mu, S, ids, frames, marks=marks)          # (asserts that the reference alone separates the outlier)
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per, seen=seen)


def _gated():
    c = gated_case()
    args = (c["mu"], c["S"], c["ids"], c["frames"])
    run = Run(*args, cap=24, ML=90)
    res = check_against_reference(run, c["lit"], c["per"], "gated window on a rest")
    assert res["plan"] == [3, 1, 1, 0] and res["prof"]["k_ekf_win_flush"][0] == 1 and res["prof"]["k_ekf_win_gate_finish"][0] == 1
    assert res["health"]["rejected"].tolist() == [0, 0, 1, 0]
    check_against_twin(res, Run(*args, cap=24, ML=90, windows=False), "gated window on a rest")
    mu_g, S_g = res["state"]
    s = rows_of(c["seen"])
    r = np.setdiff1d(np.arange(mu_g.size), s)
    assert np.array_equal(S_g[np.ix_(s, r)], S_g[np.ix_(r, s)].T), "Sigma[S,R] is not Sigma[R,S]^T to the bit"


def test_gated_window_on_a_rest():
    _gated()


@pytest.mark.gpu
def test_gated_window_on_a_rest_on_gpu():
    _gated()


# ---- 8. full size, GPU only -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("L", [937, 938, 1065, 1066])
def test_full_size_hand_over_on_gpu(L):
    """both tile widths of the update kernel at depth SP and the edges of their tiles: test_update_tile_widths_on_gpu's grid in
    the window role (double reference: long double takes minutes here)"""
    rng = np.random.RandomState(8000 + L)
    seen = tuple(pick(rng, landmark_ids(rng, L)[1], 40).tolist())
    c = build_case(8000 + L, L, ((3, seen),), dtype=np.float64)
    mu_g, S_g, _ = run_case(c, 64, L, 1, waves=64)
    e, mirrored = block_errors(mu_g, S_g, c["mu_r"], c["S_r"], seen)
    e_mu, e_S = float(np.abs(mu_g - c["mu_r"]).max()), rel_err(S_g, c["S_r"])
    print(f"full size L {L}: |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative; " + " ".join(f"{k} {e[k]:.3g}" for k in BLOCKS))
    assert mirrored, "Sigma[S,R] is not Sigma[R,S]^T to the bit"
    assert np.allclose(mu_g, c["mu_r"], rtol=1e-9, atol=1e-11), f"mu differs by {e_mu}"
    assert e_S <= 1e-9 and max(e.values()) <= 1e-9, f"Sigma differs by {e_S} (relative), blocks {e}"
