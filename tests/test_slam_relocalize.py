"""SLAM relocalization (aslam_slam_relocalize / aslam_fleet_slam_relocalize, k_slam_reloc_solve and k_slam_reloc_seat in
slam_relocalize.h): a lost SLAM filter's pose from one frame against its own map, with Sigma_xx' and the pose <->
landmark strip, against the long-double restatement tests/slam_relocalize_reference.py.

Bar: that of tests/test_relocalize.py.  1e-9 absolute on the pose (heading through the wrap), 1e-9 of max|Sigma_xx'| on Sigma_xx',
1e-9 of max|Sigma'| on the strip; status, counts, best and runner-up exact, after asserting with the reference that no pair of
hypotheses lies within MARGIN of a tolerance.  What must be exact is compared as bytes: the mirror of the strip, the symmetry of
Sigma_xx', everything a seat must not touch.  States come from aslam_set_state / aslam_fleet_set_state with a random symmetric
positive-definite Sigma whose landmarks share a common-mode term, so that landmark <-> landmark cross terms matter.
Every device case runs on the session's library (the emulation without a GPU) and again under -m gpu."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from tests import relocalize_reference as ref
from tests import slam_relocalize_reference as sref
from tests.test_fleet_slam import no_windows_context
from tests.test_localize import E_INVALID, E_STATE, POSE0, SIG0, inject, random_map, small_ring
from tests.test_relocalize import crowd, refused, sightings

TOL = 1e-9
MARGIN = 1e-6
CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
WORST = dict(pose=0.0, sigma=0.0, strip=0.0)     # largest differences against the reference seen in this session (printed per check)
WL, WR, DT = 3.0, 2.0, 0.05


def slam_context(ML, slots=1, windows=False):
    kw = dict(max_rows=64, max_cols=64, max_batch=slots, persistent_waves=4, max_landmarks=max(ML, 1))
    return capi.Context(**kw) if windows else no_windows_context(**kw)


def random_filter(rng, L, pose=(0.3, -0.2, 0.4), common=0.02, sigma=True):
    """mu, Sigma, ids, map of a SLAM filter with L landmarks: Sigma = A A^T + eps I plus a common-mode term per coordinate (every
    landmark shares a translation / rotation error), exactly symmetric"""
    N = 3 + 3 * L
    ids, xyth = random_map(rng, L)
    mu = np.concatenate([np.asarray(pose, float), xyth.reshape(-1)])
    if not sigma:
        return mu, np.zeros((N, N)), ids, xyth
    A = rng.normal(size=(N, N)) * (0.05 / math.sqrt(N))
    S = A @ A.T + 1e-4 * np.eye(N)
    for k in range(3):
        u = np.zeros(N)
        u[3 + k::3] = 1.0
        u[k] = 0.5
        S += common * np.outer(u, u)
    return mu, 0.5 * (S + S.T), ids, xyth


def check_record(got, want, where):
    for k in ("status", "n_candidates", "n_inliers", "runner_up", "best"):
        assert int(got[k]) == int(want[k]), f"{where}: {k} {int(got[k])}, reference {int(want[k])}"
    d = np.asarray(got["pose"]) - want["pose"]
    d[2] = ref.wrap(d[2])
    e_pose = float(np.abs(d).max())
    scale = float(np.abs(want["sigma"]).max())
    e_sig = float(np.abs(np.asarray(got["sigma"]) - want["sigma"]).max()) / scale if scale > 0 else float(np.abs(got["sigma"]).max())
    WORST["pose"], WORST["sigma"] = max(WORST["pose"], e_pose), max(WORST["sigma"], e_sig)
    print(f"{where}: |pose - reference| {e_pose:.3g}, |Sigma_xx' - reference| / max {e_sig:.3g}; worst so far {WORST}")
    assert e_pose <= TOL and e_sig <= TOL, f"{where}: pose differs by {e_pose}, Sigma_xx' by {e_sig}"


def check_seat(before, after, ids_after, ids, got, want, where, applied=True):
    """the state after the call: a solved apply wrote the record's pose and Sigma_xx', the strip and its exact mirror, and nothing else"""
    (mu0, S0), (mu1, S1) = before, after
    assert np.array_equal(ids_after, ids), f"{where}: the landmark ids changed"
    assert mu1.shape == mu0.shape and S1.shape == S0.shape
    if not applied or int(want["status"]) != 0:
        assert mu1.tobytes() == mu0.tobytes() and S1.tobytes() == S0.tobytes(), f"{where}: a call that seats nothing wrote the state"
        return
    assert np.array_equal(mu1[:3], got["pose"]) and np.array_equal(S1[:3, :3], got["sigma"]), f"{where}: the seat is not the record"
    assert np.array_equal(S1[:3, :3], S1[:3, :3].T), f"{where}: Sigma_xx' is not exactly symmetric"
    assert S1[:3, 3:].tobytes() == np.ascontiguousarray(S1[3:, :3].T).tobytes(), f"{where}: rows 0..2 are not the transpose of columns 0..2"
    assert mu1[3:].tobytes() == mu0[3:].tobytes(), f"{where}: a landmark mean moved"
    assert np.ascontiguousarray(S1[3:, 3:]).tobytes() == np.ascontiguousarray(S0[3:, 3:]).tobytes(), f"{where}: Sigma_ll changed"
    if mu0.size > 3:
        scale = float(np.abs(want["Sigma_new"]).max())
        e_strip = float(np.abs(S1[3:, :3] - want["strip"]).max()) / scale
        WORST["strip"] = max(WORST["strip"], e_strip)
        print(f"{where}: |strip - reference| / max|Sigma'| {e_strip:.3g}; worst so far {WORST}")
        assert e_strip <= TOL, f"{where}: the strip differs by {e_strip}"


def solve_and_seat(mu, S, ids, obs, where, ML=None, apply=True, **params):
    """set the state, inject, relocalize, compare record and state with the reference; -> (ctx, record, reference)"""
    full = {**ref.DEFAULTS, **params}
    assert ref.margin(ids, mu[3:].reshape(-1, 3), obs, **full) >= MARGIN, f"{where}: a pair of hypotheses sits on a threshold"
    want = sref.relocalize(mu, S, ids, obs, **full)
    ctx = slam_context(ML or len(ids))
    ctx.set_state(mu, S, ids)
    inject(ctx, 0, obs)
    before = ctx.get_state()
    assert before[0].tobytes() == mu.tobytes() and np.array_equal(before[1], S)
    got = ctx.slam_relocalize(0, apply=apply, **params)
    check_record(got, want, where)
    check_seat(before, ctx.get_state(), ctx.get_landmark_ids(), ids, got, want, where, applied=apply)
    return ctx, got, want


# ---- record and seat against the reference ------------------------------------------------------------------------------------------

def _single_supporter():
    """one supporter at min_inliers 1: pose = its hypothesis, Sigma_xx' = J R J^T + G P G^T, strip = Sigma_ll columns G^T"""
    rng = np.random.RandomState(1)
    mu, S, ids, xyth = random_filter(rng, 7)
    obs = sightings((1.1, -0.6, 2.0), ids, xyth, [4], rng, noise=0.01)
    ctx, got, want = solve_and_seat(mu, S, ids, obs, "one supporter", min_inliers=1)
    assert got["status"] == 0 and got["n_inliers"] == 1 and got["best"] == 0
    z, r = obs[0][2], obs[0][3]
    th = ref.wrap(xyth[4, 2] - z[2])
    c, s = math.cos(th), math.sin(th)
    hyp = np.array([xyth[4, 0] - (c * z[0] - s * z[1]), xyth[4, 1] - (s * z[0] + c * z[1]), th])
    J = np.array([[-c, s, -(s * z[0] + c * z[1])], [-s, -c, c * z[0] - s * z[1]], [0.0, 0.0, -1.0]])
    G = np.array([[1.0, 0.0, s * z[0] + c * z[1]], [0.0, 1.0, -(c * z[0] - s * z[1])], [0.0, 0.0, 1.0]])
    li = 3 + 3 * 4
    Sxx = J @ np.diag(r) @ J.T + G @ S[li:li + 3, li:li + 3] @ G.T
    mu1, S1 = ctx.get_state()
    assert np.abs(got["pose"] - hyp).max() <= TOL
    assert np.abs(got["sigma"] - Sxx).max() <= TOL * np.abs(Sxx).max()
    assert np.abs(S1[3:, :3] - S[3:, li:li + 3] @ G.T).max() <= TOL * np.abs(S).max()
    _, got2, _ = solve_and_seat(mu, S, ids, obs, "one supporter, min_inliers 2", min_inliers=2)
    assert got2["status"] == 2 and not np.any(got2["pose"]) and not np.any(got2["sigma"])


def _inliers_and_outliers():
    """8 noisy inliers and 5 wrong-id outliers"""
    rng = np.random.RandomState(2)
    mu, S, ids, xyth = random_filter(rng, 24)
    pose = (1.2, 0.4, -2.2)
    inl = sightings(pose, ids, xyth, list(range(8)), rng, noise=0.01)
    outl = sightings(pose, ids, xyth, [12, 13, 14, 15, 16], rng, noise=0.01, label=[17, 18, 19, 20, 21])
    where_out = [0, 3, 8, 9, 12]                                              # an outlier heads the list
    obs, rest, bad = [], iter(inl), iter(outl)
    for p in range(13):
        obs.append(next(bad) if p in where_out else next(rest))
    _, got, want = solve_and_seat(mu, S, ids, obs, "8 inliers, 5 outliers")
    assert want["inliers"] == [p for p in range(13) if p not in where_out]
    assert got["status"] == 0 and got["n_inliers"] == 8 and got["best"] == 1 and got["n_candidates"] == 13
    assert math.hypot(got["pose"][0] - pose[0], got["pose"][1] - pose[1]) < 0.05


def _one_id_twice():
    rng = np.random.RandomState(3)
    mu, S, ids, xyth = random_filter(rng, 10)
    obs = sightings((0.2, 0.9, -0.7), ids, xyth, [0, 1, 2, 1, 3], rng, noise=0.01)
    _, got, want = solve_and_seat(mu, S, ids, obs, "id twice, both inliers")
    assert got["status"] == 0 and got["n_inliers"] == 5 and want["inliers"] == [0, 1, 2, 3, 4]


def _headings_across_the_wrap():
    rng = np.random.RandomState(13)
    mu, S, ids, xyth = random_filter(rng, 12)
    lo = sightings((0.6, -1.1, math.pi - 1e-4), ids, xyth, [0, 1, 2, 3], rng)
    hi = sightings((0.6, -1.1, -math.pi + 1e-4), ids, xyth, [4, 5, 6, 7], rng)
    obs = [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3]]
    hyps = np.array([c[1][2] for c in ref.candidates(ids, xyth, obs)])
    assert (hyps > 3.0).sum() == 4 and (hyps < -3.0).sum() == 4
    _, got, _ = solve_and_seat(mu, S, ids, obs, "both sides of the wrap")
    assert got["status"] == 0 and got["n_inliers"] == 8
    assert abs(ref.wrap(got["pose"][2] - math.pi)) <= 2e-4, "the headings were averaged through 0"
    assert -math.pi <= got["pose"][2] < math.pi


def _supporters(n):
    """n supporters (ids repeat: a map of 40 landmarks), so that the supporters fill one wave, cross into the second, fill both"""
    rng = np.random.RandomState(100 + n)
    mu, S, ids, xyth = random_filter(rng, 40)
    obs = crowd(rng, ids, xyth, n, (-0.6, 0.3, 2.9), p_inlier=1.0)
    _, got, want = solve_and_seat(mu, S, ids, obs, f"{n} supporters")
    assert got["status"] == 0 and got["n_inliers"] == n and want["inliers"] == list(range(n))


SUPPORTERS = [63, 64, 65, 128]

# ---- the seat kernel's size edges -----------------------------------------------------------------------------------------------

# (L, max_landmarks): N = 3 + 3 L against tiles of 256 state indices; N = 255 ends inside tile 0, 258 and 261 reach into tile 1,
# L = max_landmarks makes N the leading dimension, 171 -> N = 516 reaches into a third tile
SIZES = [(1, 16), (84, 100), (85, 100), (86, 100), (85, 85), (171, 171)]


def _size_edge(L, ML):
    rng = np.random.RandomState(1000 + 7 * L + ML)
    mu, S, ids, xyth = random_filter(rng, L)
    sel = sorted({0, L - 1, L // 2, L // 3})                                 # the first and the last landmark index among them
    obs = sightings((0.4, 0.5, -1.3), ids, xyth, sel, rng, noise=0.01)
    _, got, _ = solve_and_seat(mu, S, ids, obs, f"L {L} of {ML}", ML=ML, min_inliers=1)
    assert got["status"] == 0 and got["n_inliers"] == len(sel)


def _empty_map():
    """L = 0: status 1, nothing written"""
    ctx = slam_context(16)
    mu, S = np.array([0.1, 0.2, 0.3]), np.diag([0.01, 0.02, 0.03])
    ctx.set_state(mu, S, np.zeros(0, np.int32))
    inject(ctx, 0, [(5, 1, np.array([1.0, 0.2, 0.3]), np.full(3, 0.02))])
    got = ctx.slam_relocalize(0, apply=True, min_inliers=1)
    assert got["status"] == 1 and got["best"] == -1 and got["n_candidates"] == 0 and not np.any(got["pose"]) and not np.any(got["sigma"])
    mu1, S1 = ctx.get_state()
    assert np.array_equal(mu1, mu) and np.array_equal(S1, S)


def _zero_map_covariance():
    """Sigma_ll = 0: status, counts and best are aslam_relocalize's on a localizing context with the same map and list"""
    rng = np.random.RandomState(5)
    mu, S, ids, xyth = random_filter(rng, 20, sigma=False)
    pose = (0.9, -1.4, 0.8)
    obs = sightings(pose, ids, xyth, list(range(9)), rng, noise=0.01) + sightings(pose, ids, xyth, [10, 11], rng, label=[12, 13])
    _, got, _ = solve_and_seat(mu, S, ids, obs, "Sigma_ll = 0")
    loc = slam_context(20)
    loc.localize_begin(ids, xyth, POSE0, SIG0)
    inject(loc, 0, obs)
    old = loc.relocalize(0, apply=False)
    for k in ("status", "n_candidates", "n_inliers", "runner_up", "best"):
        assert int(got[k]) == int(old[k]), k
    d = got["pose"] - old["pose"]
    d[2] = ref.wrap(d[2])
    assert np.abs(d).max() <= TOL and np.abs(got["sigma"] - old["sigma"]).max() <= TOL * np.abs(old["sigma"]).max()


# ---- what a call that seats nothing leaves behind -------------------------------------------------------------------------------

def _no_seat_keeps_state_and_list():
    """apply = 0 and an unsolved apply = 1 leave aslam_get_state bit-identical and the last-observed list intact: the same sighting
    again is still "stationary"; after a solved apply = 1 the list is empty and the same sighting is fused"""
    rng = np.random.RandomState(6)
    mu, S, ids, xyth = random_filter(rng, 12)
    obs = sightings(mu[:3], ids, xyth, [0, 1, 2, 3, 4], rng, noise=0.01)
    for seated in (False, True):
        ctx = slam_context(12, slots=4)
        ctx.set_state(mu, S, ids)
        inject(ctx, 0, [])
        for s in (1, 2, 3):
            inject(ctx, s, obs)
        ctx.stage_encoders([0.0] * 4, [0.0] * 4, [0.0] * 4)
        ctx.run_staged(0, 2, with_ekf=2)                                       # armed; one frame of five corrections: a list
        ctx.sync()
        assert ctx.get_slot_ekf_stats(1, 1).tolist() == [[5, 0, 5, 0]]
        mu0, S0 = ctx.get_state()
        assert ctx.slam_relocalize(2, apply=False)["status"] == 0
        assert ctx.slam_relocalize(2, apply=True, min_inliers=6)["status"] == 2
        mu1, S1 = ctx.get_state()
        assert mu0.tobytes() == mu1.tobytes() and S0.tobytes() == S1.tobytes(), "a call that seats nothing wrote the state"
        if seated:
            assert ctx.slam_relocalize(2, apply=True)["status"] == 0
        ctx.run_staged(2, 1, with_ekf=2)
        ctx.sync()
        assert ctx.get_slot_ekf_stats(2, 1).tolist() == ([[5, 0, 5, 0]] if seated else [[5, 0, 0, 5]])


# ---- consistency ------------------------------------------------------------------------------------------------------------------

def ekf_update(mu, S, i, z, r):
    """one EKF correction of landmark index i (the reference's measurement model), numpy: what follows a seat"""
    x, y, th = mu[:3]
    lx, ly, lt = mu[3 + 3 * i: 6 + 3 * i]
    c, s = math.cos(th), math.sin(th)
    dx, dy = lx - x, ly - y
    H = np.zeros((3, mu.size))
    H[:, :3] = [[-c, -s, -dx * s + dy * c], [s, -c, -dx * c - dy * s], [0.0, 0.0, -1.0]]
    H[:, 3 + 3 * i: 6 + 3 * i] = [[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]
    Si = H @ S @ H.T + np.diag(r)
    K = S @ H.T @ np.linalg.inv(Si)
    out = S - K @ Si @ K.T
    return 0.5 * (out + out.T)


def _consistency():
    """the seated Sigma' is positive semi-definite: lambda_min >= -1e-12 max|Sigma'|, reference and device"""
    rng = np.random.RandomState(7)
    mu, S, ids, xyth = random_filter(rng, 30, common=0.05)
    pose = (-0.7, 0.8, 1.9)
    sel = list(range(10))
    obs = sightings(pose, ids, xyth, sel, rng, noise=0.01)
    want = sref.relocalize(mu, S, ids, obs)
    lam_ref = float(np.linalg.eigvalsh(want["Sigma_new"]).min())
    assert lam_ref >= -1e-12 * np.abs(want["Sigma_new"]).max(), f"the reference alone is not consistent here: {lam_ref}"
    ctx, got, _ = solve_and_seat(mu, S, ids, obs, "consistency")
    mu1, S1 = ctx.get_state()
    lam_dev = float(np.linalg.eigvalsh(S1).min())
    assert lam_dev >= -1e-12 * np.abs(S1).max(), f"lambda_min {lam_dev}"
    # for comparison: one further correction of a supporter landmark after this seat, and after a seat with Sigma_xl = 0
    naive = S1.copy()
    naive[3:, :3] = 0.0
    naive[:3, 3:] = 0.0
    z, r = obs[0][2], obs[0][3]
    after, after_naive = ekf_update(mu1, S1, sel[0], z, r), ekf_update(mu1, naive, sel[0], z, r)
    print(f"lambda_min: reference Sigma' {lam_ref:.3e}, device Sigma' {lam_dev:.3e}; after one more correction of a supporter landmark "
          f"{np.linalg.eigvalsh(after).min():.3e}, trace Sigma_xx {np.trace(after[:3, :3]):.3e}; with a Sigma_xl = 0 seat "
          f"{np.linalg.eigvalsh(after_naive).min():.3e}, trace Sigma_xx {np.trace(after_naive[:3, :3]):.3e}")


# ---- seated means seated ------------------------------------------------------------------------------------------------------------

def state_close(a, b, where):
    (mu_a, S_a), (mu_b, S_b) = a, b
    assert mu_a.shape == mu_b.shape, where
    d = mu_a - mu_b
    d[2] = ref.wrap(d[2])
    e_mu, e_S = float(np.abs(d).max()), float(np.abs(S_a - S_b).max() / np.abs(S_b).max())
    print(f"{where}: |mu - twin| {e_mu:.3g}, |Sigma - twin| / max|Sigma| {e_S:.3g}")
    assert e_mu <= TOL and e_S <= TOL, f"{where}: mu differs by {e_mu}, Sigma by {e_S}"


@functools.lru_cache(maxsize=None)
def tracking_case():
    """a filter, the list it is relocalized on, and frames that follow: frame 0 updates supporter landmarks and augments a new id,
    the later ones update known landmarks only (window material), all seen from a pose that moves as the encoders say"""
    rng = np.random.RandomState(9)
    mu, S, ids, xyth = random_filter(rng, 14)
    pose = np.array([0.8, -0.5, 1.2])
    reloc = sightings(pose, ids, xyth, [0, 1, 2, 3, 4, 5], rng, noise=0.01)
    new_id, new_lm = 777, np.array([1.5, 0.5, -2.0])
    before = [sightings(mu[:3] + [0.01 * k, 0.0, 0.0], ids, xyth, [6, 7], rng, noise=0.01) for k in (1, 2)]
    frames = []
    for k in range(4):
        pose = pose + np.array([0.02, 0.015, 0.03])                            # roughly what (WL, WR, DT) drives
        obs = sightings(pose, ids, xyth, [1, 2, 3] if k else [0, 1], rng, noise=0.01)
        if k == 0:
            obs += sightings(pose, [new_id], [new_lm], [0], rng, noise=0.01)
        frames.append(obs)
    return mu, S, ids, reloc, before, frames


def _seated_per_frame():
    """after apply = 1 two further frames (a predict, updates of supporter landmarks, an augment) match a twin context that was given
    aslam_set_state(reference mu', Sigma'): per-frame path"""
    mu, S, ids, reloc, _, frames = tracking_case()
    want = sref.relocalize(mu, S, ids, reloc)
    assert want["status"] == 0
    res = []
    for twin in (False, True):
        ctx = slam_context(20, slots=4)
        ctx.set_state(mu, S, ids)
        ctx.stage_encoders([0.0, 0.0, WL, WL], [0.0, 0.0, WR, WR], [0.0, 0.0, DT, DT])
        inject(ctx, 0, [])
        inject(ctx, 1, reloc)
        inject(ctx, 2, frames[0])
        inject(ctx, 3, frames[1])
        ctx.run_staged(0, 1, with_ekf=2)                                       # armed: the frames that follow predict
        if twin:
            ctx.set_state(want["mu_new"], want["Sigma_new"], ids)
        else:
            check_record(ctx.slam_relocalize(1, apply=True), want, "seated, per-frame path")
        ctx.run_staged(2, 2, with_ekf=2)
        ctx.sync()
        res.append((ctx.get_state(), ctx.get_landmark_ids(), ctx.get_slot_ekf_stats(2, 2)))
    assert np.array_equal(res[0][1], res[1][1]) and res[0][1][-1] == 777 and np.array_equal(res[0][2], res[1][2])
    assert res[0][2].tolist() == [[3, 1, 2, 0], [3, 0, 3, 0]], res[0][2].tolist()
    state_close(res[0][0], res[1][0], "two frames after the seat, per-frame path")


def _seated_with_windows():
    """the same with windows on: the batch before the call is still pending when the call comes, and the batch after it runs through
    a window; the twin is seated with aslam_set_state(reference mu', Sigma') computed from its own state after the first batch"""
    mu, S, ids, reloc, before, frames = tracking_case()
    res = []
    for twin in (False, True):
        ctx = slam_context(20, slots=8, windows=True)
        ctx.set_state(mu, S, ids)
        ctx.stage_encoders([0.0] + [WL] * 6 + [0.0], [0.0] + [WR] * 6 + [0.0], [0.0] + [DT] * 6 + [0.0])
        for s, obs in enumerate([[]] + before + frames + [reloc]):             # slot 7: the list relocalized on
            inject(ctx, s, obs)
        ctx.run_staged(0, 3, with_ekf=2)                                       # left pending: planned and enqueued by the next call
        if twin:
            mu_b, S_b = ctx.get_state()
            want = sref.relocalize(mu_b, S_b, ids, reloc)
            assert want["status"] == 0 and ref.margin(ids, mu_b[3:].reshape(-1, 3), reloc) >= MARGIN
            ctx.set_state(want["mu_new"], want["Sigma_new"], ids)
        else:
            got = ctx.slam_relocalize(7, apply=True)
        plan0 = ctx.plan_stats()
        ctx.run_staged(3, 4, with_ekf=2)
        ctx.sync()
        plan1 = ctx.plan_stats()
        assert plan1["windows"] > plan0["windows"] and plan1["frames_in_windows"] - plan0["frames_in_windows"] >= 2, \
            f"the batch after the seat ran through no window: {plan0} -> {plan1}"
        res.append((ctx.get_state(), ctx.get_landmark_ids(), ctx.get_slot_ekf_stats(3, 4)))
        if twin:
            check_record(got, want, "seated, windows on")
    assert np.array_equal(res[0][1], res[1][1]) and res[0][1][-1] == 777 and np.array_equal(res[0][2], res[1][2])
    state_close(res[0][0], res[1][0], "four frames after the seat, windows on")


# ---- fleet SLAM ---------------------------------------------------------------------------------------------------------------------

def fleet_context(R, ML, slots=None):
    ctx = slam_context(ML, slots=slots or R)
    ctx.fleet_slam_begin([CAM] * R)
    return ctx


def _fleet_equals_solo_calls():
    """three robots with different L in one call equal three solo aslam_slam_relocalize calls on single contexts holding the same
    state, bit for bit; a permuted robot order gives the same bits; the unsolved robot keeps its state bits"""
    rng = np.random.RandomState(10)
    Ls, ML = [9, 30, 17], 32
    filt = [random_filter(rng, L, pose=(0.1 * r, -0.2, 0.3 + r)) for r, L in enumerate(Ls)]
    lists = [sightings((1.0, 0.4, -0.9), filt[0][2], filt[0][3], [0, 1, 2, 8], rng, noise=0.01),
             sightings((0.2, 0.1, 0.5), filt[1][2], filt[1][3], [29], rng, noise=0.01),       # one candidate: unsolved at min_inliers 2
             crowd(rng, filt[2][2], filt[2][3], 70, (-1.1, 0.9, 3.0))]
    solo = []
    for (mu, S, ids, _), obs in zip(filt, lists):
        ctx = slam_context(ML)
        ctx.set_state(mu, S, ids)
        inject(ctx, 0, obs)
        rec = ctx.slam_relocalize(0, apply=True)
        check_record(rec, sref.relocalize(mu, S, ids, obs), f"solo L {len(ids)}")
        solo.append((rec, ctx.get_state()))
    assert [int(s[0]["status"]) for s in solo] == [0, 2, 0]
    for order in ([0, 1, 2], [2, 0, 1]):                                       # slot 1 + i belongs to robot order[i]
        fleet = fleet_context(3, ML, slots=5)
        for r, (mu, S, ids, _) in enumerate(filt):
            fleet.fleet_set_state(r, mu, S, ids)
        for i, r in enumerate(order):
            inject(fleet, 1 + i, lists[r])
        got = fleet.fleet_slam_relocalize(1, order, apply=True)
        for i, r in enumerate(order):
            assert got[i].tobytes() == solo[r][0].tobytes(), f"order {order}: robot {r}'s record differs from the solo call"
            mu_f, S_f = fleet.fleet_get_state(r)
            assert mu_f.tobytes() == solo[r][1][0].tobytes() and S_f.tobytes() == solo[r][1][1].tobytes(), f"order {order}: robot {r}'s state"
            assert np.array_equal(fleet.fleet_get_landmark_ids(r), filt[r][2])
        mu_f, S_f = fleet.fleet_get_state(1)
        assert mu_f.tobytes() == filt[1][0].tobytes() and np.array_equal(S_f, filt[1][1]), "the unsolved robot was written"


@functools.lru_cache(maxsize=None)
def big_fleet_case():
    rng = np.random.RandomState(11)
    R, L = 64, 12
    filt = [random_filter(rng, L, pose=rng.uniform(-1, 1, 3)) for _ in range(R)]
    sizes = [int(rng.randint(1, 21)) for _ in range(R)]
    sizes[0], sizes[63] = 20, 1
    truth = np.stack([rng.uniform(-2, 2, R), rng.uniform(-2, 2, R), rng.uniform(-math.pi, math.pi, R)], 1)
    lists = [crowd(rng, filt[r][2], filt[r][3], sizes[r], truth[r]) for r in range(R)]
    want = [sref.relocalize(filt[r][0], filt[r][1], filt[r][2], lists[r]) for r in range(R)]
    assert min(ref.margin(filt[r][2], filt[r][3], lists[r]) for r in range(R)) >= MARGIN
    assert {int(w["status"]) for w in want} == {0, 2}, "the case should hold solved and unsolved slots"
    return filt, lists, want


def _64_robots():
    filt, lists, want = big_fleet_case()
    R = 64
    fleet = fleet_context(R, 16)
    robots = [(r * 29 + 5) % R for r in range(R)]                              # slot i belongs to robot robots[i] (a permutation)
    for i, r in enumerate(robots):
        fleet.fleet_set_state(r, filt[r][0], filt[r][1], filt[r][2])
        inject(fleet, i, lists[r])
    got = fleet.fleet_slam_relocalize(0, robots, apply=True)
    for i, r in enumerate(robots):
        check_record(got[i], want[r], f"robot {r} ({len(lists[r])} observations)")
        check_seat((filt[r][0], filt[r][1]), fleet.fleet_get_state(r), fleet.fleet_get_landmark_ids(r), filt[r][2], got[i], want[r], f"robot {r}")


# ---- the SLAM gate's track record -------------------------------------------------------------------------------------------------

def _gate_record_cleared_by_a_solved_seat():
    rng = np.random.RandomState(12)
    mu, S, ids, xyth = random_filter(rng, 10)
    obs = sightings(mu[:3], ids, xyth, [0, 1, 2, 3], rng, noise=0.01)
    zero = np.zeros(1, capi.TRACK_HEALTH_DTYPE).tobytes()
    ctx = slam_context(10, slots=3)
    ctx.set_slam_gate()
    ctx.set_state(mu, S, ids)
    ctx.stage_encoders([0.0] * 3, [0.0] * 3, [0.0] * 3)
    inject(ctx, 0, [])
    inject(ctx, 1, obs)
    inject(ctx, 2, obs)
    ctx.run_staged(0, 2, with_ekf=2)
    tr = ctx.get_track_health()
    assert tr["frames"] > 0 and tr.tobytes() != zero
    assert ctx.slam_relocalize(2, apply=True, min_inliers=5)["status"] == 2
    assert ctx.get_track_health().tobytes() == tr.tobytes(), "an unsolved call cleared the track record"
    assert ctx.slam_relocalize(2, apply=False)["status"] == 0
    assert ctx.get_track_health().tobytes() == tr.tobytes(), "apply = 0 cleared the track record"
    assert ctx.slam_relocalize(2, apply=True)["status"] == 0
    assert ctx.get_track_health().tobytes() == zero, "a solved seat left the track record"
    # the fleet: the solved robot's record only
    fleet = fleet_context(2, 10, slots=2)
    fleet.set_slam_gate()
    for r in range(2):
        fleet.fleet_set_state(r, mu, S, ids)
    fleet.stage_encoders([0.0] * 2, [0.0] * 2, [0.0] * 2)
    for _ in range(2):                                                         # a round that arms, a round that fuses
        for r in range(2):
            inject(fleet, r, obs)
        fleet.fleet_run_staged(0, [0, 1], with_ekf=2)
    h = fleet.fleet_get_health()
    assert all(h[r].tobytes() != zero for r in range(2))
    inject(fleet, 1, obs[:1])
    assert fleet.fleet_slam_relocalize(0, [0, 1], apply=True)["status"].tolist() == [0, 2]
    h1 = fleet.fleet_get_health()
    assert h1[0].tobytes() == zero and h1[1].tobytes() == h[1].tobytes()


# ---- arguments and modes ------------------------------------------------------------------------------------------------------------

def _arguments_and_modes():
    rng = np.random.RandomState(14)
    mu, S, ids, xyth = random_filter(rng, 9)
    obs = sightings((0.1, 0.2, 0.3), ids, xyth, [0, 1, 2], rng)
    ctx = slam_context(16, slots=4)
    ctx.set_state(mu, S, ids)
    inject(ctx, 0, obs)
    want = sref.relocalize(mu, S, ids, obs)
    check_record(ctx.slam_relocalize(0, apply=False), want, "NULL params: the defaults")
    check_record(ctx.slam_relocalize(0, apply=False, tol_xy=0.25, tol_th=0.2, min_inliers=2), want, "defaults spelled out")
    for bad in [dict(tol_xy=0.0), dict(tol_xy=-0.1), dict(tol_xy=math.nan), dict(tol_xy=math.inf), dict(tol_th=0.0), dict(tol_th=-0.1),
                dict(tol_th=math.nan), dict(tol_th=math.inf), dict(tol_th=math.pi), dict(tol_th=4.0), dict(min_inliers=0),
                dict(min_inliers=-1), dict(min_inliers=129)]:
        refused(E_INVALID, ctx.slam_relocalize, 0, False, **bad)
    assert ctx.slam_relocalize(0, apply=False, tol_th=3.14, min_inliers=128)["status"] == 2
    refused(E_INVALID, ctx.slam_relocalize, -1, False)
    refused(E_INVALID, ctx.slam_relocalize, 4, False)
    assert ctx.lib.aslam_slam_relocalize(ctx.h, 0, None, 0, None) == E_INVALID  # no result pointer
    # SLAM: the fleet call and both localization calls refuse
    refused(E_STATE, ctx.fleet_slam_relocalize, 0, [0])
    refused(E_STATE, ctx.relocalize, 0)
    refused(E_STATE, ctx.fleet_relocalize, 0, [0])
    # localizing
    ctx.localize_begin(ids, xyth, POSE0, SIG0)
    refused(E_STATE, ctx.slam_relocalize, 0)
    refused(E_STATE, ctx.fleet_slam_relocalize, 0, [0])
    ctx.localize_end()
    # fleet localization
    ctx.fleet_begin([CAM] * 2, ids, xyth, [POSE0] * 2, [SIG0] * 2)
    refused(E_STATE, ctx.slam_relocalize, 0)
    refused(E_STATE, ctx.fleet_slam_relocalize, 0, [0])
    ctx.fleet_end()
    # fleet SLAM: the fleet call only
    ctx.fleet_slam_begin([CAM] * 3)
    refused(E_STATE, ctx.slam_relocalize, 0)
    refused(E_STATE, ctx.relocalize, 0)
    refused(E_STATE, ctx.fleet_relocalize, 0, [0])
    ctx.fleet_set_state(2, mu, S, ids)
    inject(ctx, 0, obs)
    first = ctx.fleet_slam_relocalize(0, [2], apply=False)
    check_record(first[0], want, "robot 2 of a SLAM fleet")
    assert ctx.fleet_slam_relocalize(0, [0], apply=False)["status"].tolist() == [1]          # robot 0's map is empty
    refused(E_INVALID, ctx.fleet_slam_relocalize, 0, [3], False)               # a robot outside the fleet
    refused(E_INVALID, ctx.fleet_slam_relocalize, 0, [-1], False)
    refused(E_INVALID, ctx.fleet_slam_relocalize, 0, [1, 1], False)            # a robot named twice
    refused(E_INVALID, ctx.fleet_slam_relocalize, -1, [0], False)              # slot ranges
    refused(E_INVALID, ctx.fleet_slam_relocalize, 3, [0, 1], False)
    refused(E_INVALID, ctx.fleet_slam_relocalize, 0, [], False)
    refused(E_INVALID, ctx.fleet_slam_relocalize, 0, [0], False, tol_xy=0.0)
    refused(E_INVALID, ctx.fleet_slam_relocalize, 0, [0], False, min_inliers=129)
    rs = np.zeros(1, np.int32)
    assert ctx.lib.aslam_fleet_slam_relocalize(ctx.h, 0, 1, rs.ctypes.data_as(C.POINTER(C.c_int)), None, 0, None) == E_INVALID
    out = np.zeros(1, capi.RELOC_DTYPE)
    assert ctx.lib.aslam_fleet_slam_relocalize(ctx.h, 0, 1, None, None, 0, out.ctypes.data_as(C.c_void_p)) == E_INVALID
    # the scratch buffers are freed by aslam_fleet_end: a call in a new fleet allocates again and gives the same bits
    ctx.fleet_end()
    ctx.fleet_slam_begin([CAM] * 3)
    ctx.fleet_set_state(2, mu, S, ids)
    inject(ctx, 0, obs)
    assert ctx.fleet_slam_relocalize(0, [2], apply=False).tobytes() == first.tobytes()
    ctx.fleet_end()
    assert ctx.slam_relocalize(0, apply=False)["status"] in (0, 1, 2)           # and the single call after a fleet ended
    ctx.close()


# ---- the cases on the session's library, and again on the MI355X ------------------------------------------------------------------

def test_single_supporter():
    _single_supporter()


def test_inliers_and_outliers():
    _inliers_and_outliers()


def test_one_id_twice():
    _one_id_twice()


def test_headings_across_the_wrap():
    _headings_across_the_wrap()


@pytest.mark.parametrize("n", SUPPORTERS)
def test_supporters_in_both_waves(n):
    _supporters(n)


@pytest.mark.parametrize("L,ML", SIZES)
def test_seat_size_edges(L, ML):
    _size_edge(L, ML)


def test_empty_map():
    _empty_map()


def test_zero_map_covariance_equals_relocalize():
    _zero_map_covariance()


def test_no_seat_keeps_state_and_list():
    _no_seat_keeps_state_and_list()


def test_consistency():
    _consistency()


def test_seated_per_frame():
    _seated_per_frame()


def test_seated_with_windows():
    _seated_with_windows()


def test_fleet_equals_solo_calls():
    _fleet_equals_solo_calls()


def test_64_robots_in_one_call():
    _64_robots()


def test_gate_record_cleared_by_a_solved_seat():
    _gate_record_cleared_by_a_solved_seat()


def test_arguments_and_modes():
    _arguments_and_modes()


@pytest.mark.gpu
def test_record_and_seat_on_gpu():
    _single_supporter()
    _inliers_and_outliers()
    _one_id_twice()
    _headings_across_the_wrap()
    _empty_map()
    _zero_map_covariance()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SUPPORTERS)
def test_supporters_in_both_waves_on_gpu(n):
    _supporters(n)


@pytest.mark.gpu
@pytest.mark.parametrize("L,ML", SIZES)
def test_seat_size_edges_on_gpu(L, ML):
    _size_edge(L, ML)


@pytest.mark.gpu
def test_no_seat_and_consistency_on_gpu():
    _no_seat_keeps_state_and_list()
    _consistency()


@pytest.mark.gpu
def test_seated_per_frame_on_gpu():
    _seated_per_frame()


@pytest.mark.gpu
def test_seated_with_windows_on_gpu():
    _seated_with_windows()


@pytest.mark.gpu
def test_fleet_on_gpu():
    _fleet_equals_solo_calls()
    _64_robots()


@pytest.mark.gpu
def test_gate_arguments_and_modes_on_gpu():
    _gate_record_cleared_by_a_solved_seat()
    _arguments_and_modes()


# ---- on the MI355X: rendered frames of the 240 x 320 ring ------------------------------------------------------------------------

def relative_pose(p, origin):
    """pose p in the frame whose origin is the pose `origin`: the frame a SLAM filter started at `origin` works in"""
    c, s = math.cos(origin[2]), math.sin(origin[2])
    dx, dy = p[0] - origin[0], p[1] - origin[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, ref.wrap(ref.wrap(p[2] - origin[2]))])


class RingSlam:
    """a SLAM context that has built its map over one lap of the rendered 240 x 320 ring under the default SLAM gate"""

    def __init__(self):
        self.w = w = synth.RingWorld(small_ring())
        self.cfg = cfg = w.cfg
        self.lap, B = w.lap_length(), 8
        self.ctx = ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=B, max_landmarks=w.L + 8)
        synth.apply_detector(cfg, ctx=ctx)
        ctx.set_camera(w.K, np.zeros(5))
        ctx.set_slam_gate()
        self.origin = w.frame(0).true_pose
        for t0 in range(0, self.lap, B):
            self.run(t0, min(B, self.lap - t0))
        ctx.sync()
        self.ids = ctx.get_landmark_ids()
        mu, _ = ctx.get_state()
        assert len(self.ids) >= w.L // 2 and not ctx.get_track_health()["lost"], "the lap did not build a map"
        d = self.truth(w.frame(self.lap - 1)) - mu[:3]
        print(f"after one lap: {len(self.ids)} landmarks, pose {math.hypot(d[0], d[1]):.4f} m {abs(ref.wrap(d[2])):.4f} rad from the truth")

    def run(self, t0, n, with_ekf=1):
        w, cfg, ctx = self.w, self.cfg, self.ctx
        frs = [w.frame(t0 + k) for k in range(n)]
        imgs = [ctx.synth_render(k, cfg.rows, cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=t0 + k) for k, fr in enumerate(frs)]
        ctx.stage_frames(np.stack(imgs))
        ctx.stage_encoders([fr.wl for fr in frs], [fr.wr for fr in frs], [fr.dt for fr in frs])
        ctx.run_staged(0, n, with_ekf=with_ekf)
        return frs

    def truth(self, fr):
        return relative_pose(fr.true_pose, self.origin)

    def displace(self):
        """the same map, the pose moved by 1 m and 0.5 rad.  The issue leaves the direction open.  The markers in view are 1.6 to 2 m
        ahead.  In the filter's own frame a heading error delta moves the predicted markers sideways by about -delta times their
        distance, and a position error of 1 m in direction a moves them sideways by sin(heading - a).  The truth heads along 0 at
        the end of the lap and turns left by 3 degrees a frame.  With delta = -0.5 and a = -37 degrees, d = (0.8, -0.6), the filter's
        heading minus a grows from 8 degrees on: both shifts are to the left and add for the next 30 frames, the largest innovations
        1 m and 0.5 rad can make, which is the case in which a gate has to report `lost`.  With (0.8, 0.6) and +0.5 rad the heading
        error shifts to the right and the position error, from the third frame on, to the left."""
        mu, S = self.ctx.get_state()
        mu[:3] += [0.8, -0.6, -0.5]                                            # |(0.8, -0.6)| = 1 m
        self.ctx.set_state(mu, S, self.ids)

    def relocalize_and_track(self, t, where):
        """one detection-only tick at frame t, aslam_slam_relocalize(apply = 1), 10 tracking frames; the issue's assertions"""
        ctx, ids = self.ctx, self.ids
        fr = self.run(t, 1, with_ekf=0)[0]
        got = ctx.slam_relocalize(0, apply=True)                               # straight behind the detection: no sync in between
        ctx.sync()
        i, v, z, rd = ctx.get_slot_raw_observations(0)
        obs = [(int(i[k]), int(v[k]), z[k], rd[k]) for k in range(len(i))]
        mu_l, S_l = ctx.get_state()
        # the reference on the state the seat left: it reads mu_l and Sigma_ll only, which the seat does not write
        assert ref.margin(ids, mu_l[3:].reshape(-1, 3), obs) >= MARGIN
        want = sref.relocalize(mu_l, S_l, ids, obs)
        check_record(got, want, where)
        assert got["status"] == 0, f"{where}: status {int(got['status'])} with {int(got['n_candidates'])} candidates, {int(got['n_inliers'])} inliers"
        assert np.array_equal(mu_l[:3], got["pose"]) and np.array_equal(S_l[:3, :3], got["sigma"])
        truth = self.truth(fr)
        d_xy, d_th = math.hypot(*(got["pose"][:2] - truth[:2])), abs(ref.wrap(got["pose"][2] - truth[2]))
        print(f"{where}:\n| inliers | runner-up | candidates | to truth (m) | to truth (rad) |\n|---|---|---|---|---|\n"
              f"| {int(got['n_inliers'])} | {int(got['runner_up'])} | {int(got['n_candidates'])} | {d_xy:.4f} | {d_th:.4f} |")
        assert d_xy < 0.5 and d_th < 0.25, f"{where}: {d_xy} m, {d_th} rad from the truth"     # half the injected offset
        assert not ctx.get_track_health()["lost"] and ctx.get_track_health()["frames"] == 0
        fused = 0
        for k in range(10):
            fr = self.run(t + 1 + k, 1)[0]
            ctx.sync()
            fused += int(ctx.get_slot_ekf_stats(0, 1)[0, 2])
        tr = ctx.get_track_health()
        mu_e, _ = ctx.get_state()
        truth = self.truth(fr)
        print(f"{where}, after 10 tracking frames: {fused} corrections accepted, {int(tr['rejected_total'])} rejected, lost {int(tr['lost'])}, pose "
              f"{math.hypot(*(mu_e[:2] - truth[:2])):.4f} m {abs(ref.wrap(mu_e[2] - truth[2])):.4f} rad from the truth")
        assert fused > 0 and not tr["lost"]


@pytest.mark.gpu
def test_gpu_lost_slam_filter_recovers_on_rendered_frames():
    """The issue's rendered case: a SLAM filter builds its map over one lap of the ring under the default SLAM gate, is displaced by
    1 m and 0.5 rad (aslam_set_state with the same map), runs until `lost` is reported, is relocalized on one detection-only tick and
    tracks for 10 frames.  The wait for `lost` is bounded by one lap: by then every marker of the ring has been sighted again from
    the displaced pose.

    The direction of the displacement matters (RingSlam.displace).  CalculateCovariance's R is wide at 240 x 320 (r_x 0.01 to 1.05,
    r_theta a tenth of it), so the default gate (gate_d2 16.266, min_accept_percent 50) passes about half of a displaced filter's
    corrections, and the accepted ones drag pose and map.  With (+0.8, +0.6, +0.5), where the position error partly cancels the
    heading error in the innovations, the gate never reports `lost`: 120 frames, 293 corrections accepted, 60 rejected, bad_streak
    never above 1 (MI355X).  With the errors adding, (+0.8, -0.6, -0.5) and every direction within 45 degrees of it, `lost` comes
    after 24 frames.  DESIGN.md §19 had already found R to overstate the scatter of these sightings; nothing here tunes it."""
    ring = RingSlam()
    ring.displace()
    ctx, t = ring.ctx, ring.lap
    while not ctx.get_track_health()["lost"]:
        assert t < 2 * ring.lap, f"the displaced filter was not reported lost within one lap: {ctx.get_track_health()}"
        ring.run(t, 1)
        ctx.sync()
        t += 1
    print(f"lost after {t - ring.lap} frames: {ctx.get_track_health()}")
    ring.relocalize_and_track(t, "rendered ring, lost")


@pytest.mark.gpu
def test_gpu_displaced_slam_filter_recovers_on_rendered_frames():
    """the same scene and assertions for a filter that its caller knows to be displaced (carried away, loaded at an unknown pose):
    one lap, the pose moved by 1 m and 0.5 rad, one detection-only tick, aslam_slam_relocalize(apply = 1), 10 tracking frames"""
    ring = RingSlam()
    ring.displace()
    ring.relocalize_and_track(ring.lap + 1, "rendered ring, displaced")
