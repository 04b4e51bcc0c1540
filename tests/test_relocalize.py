"""Relocalization (aslam_relocalize / aslam_fleet_relocalize, k_relocalize in relocalize.h): a pose and its covariance
from one frame's observations against the frozen map, against the numpy restatement tests/relocalize_reference.py.

Bar: the project's bar for f64 state against a literal reference (tests/test_merge_maps.py): 1e-9 absolute on poses (the heading
difference taken through the angle wrap: -pi and pi - 1e-16 are one heading), 1e-9 relative to max|Sigma| on covariances; status,
counts, best and runner-up exact.  Sines and cosines may differ in the last bit between numpy and the device, so every case that
compares a discrete result first asserts, with the reference itself, that no pair of hypotheses lies within 1e-6 of tol_xy^2 or
tol_th (MARGIN).

What "seated" means is checked against aslam_fleet_set_pose itself: a robot seated by aslam_fleet_relocalize must from then on give
the bits of a twin fleet whose robot was seated with aslam_fleet_set_pose(the result).  Its next frame arms it, which in this
library means that frame's encoder sample is not applied; the frame's observations are fused as after aslam_fleet_set_pose."""
import ctypes as C
import math

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from tests import relocalize_reference as ref
from tests.test_localize import (E_INVALID, E_STATE, FrozenMapLocalizer, POSE0, SIG0, emu_context, inject, observe, random_map,
                                 small_ring)

TOL = 1e-9
MARGIN = 1e-6
CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
WORST = dict(pose=0.0, sigma=0.0)           # largest differences against the reference seen in this session (printed per test)


def sightings(pose, ids, xyth, sel, rng, noise=0.0, label=None):
    """observations (id, valid, z, Rdiag) of landmarks sel (positions into the map) from `pose`; label: the ids they are reported
    under instead (a wrong-id outlier is an observation of one landmark reported under another's id)"""
    out = []
    for k, li in enumerate(sel):
        lid = int(ids[li] if label is None else ids[label[k]])
        out.append((lid, 1, observe(pose, xyth[li], rng, noise), rng.uniform(0.01, 0.05, 3)))
    return out


def check(got, want, where):
    for k in ("status", "n_candidates", "n_inliers", "runner_up", "best"):
        assert int(got[k]) == int(want[k]), f"{where}: {k} {int(got[k])}, reference {int(want[k])}"
    d = np.asarray(got["pose"]) - want["pose"]
    d[2] = ref.wrap(d[2])
    e_pose = float(np.abs(d).max())
    scale = float(np.abs(want["sigma"]).max())
    e_sig = float(np.abs(np.asarray(got["sigma"]) - want["sigma"]).max()) / scale if scale > 0 else float(np.abs(got["sigma"]).max())
    WORST["pose"], WORST["sigma"] = max(WORST["pose"], e_pose), max(WORST["sigma"], e_sig)
    print(f"{where}: |pose - reference| {e_pose:.3g}, |Sigma - reference| / max|Sigma| {e_sig:.3g}; worst so far {WORST}")
    assert e_pose <= TOL and e_sig <= TOL, f"{where}: pose differs by {e_pose}, Sigma by {e_sig}"


def localizer(ids, xyth, slots=1, **kw):
    ctx = emu_context(slots, max_landmarks=max(len(ids), 16), **kw)
    ctx.localize_begin(ids, xyth, POSE0, SIG0)
    return ctx


def solve(ctx, ids, xyth, obs, where, slot=0, **params):
    """inject, relocalize without seating, assert the margin and compare with the reference"""
    assert ref.margin(ids, xyth, obs, **{**ref.DEFAULTS, **params}) >= MARGIN, f"{where}: a pair of hypotheses sits on a threshold"
    inject(ctx, slot, obs)
    got = ctx.relocalize(slot, apply=False, **params)
    want = ref.relocalize(ids, xyth, obs, **{**ref.DEFAULTS, **params})
    check(got, want, where)
    return got, want


def refused(code, fn, *a, **kw):
    with pytest.raises(capi.AslamError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (fn, e.value)


# ---- single slot against the reference ----------------------------------------------------------------------------------------

def test_no_candidate():
    rng = np.random.RandomState(1)
    ids, xyth = random_map(rng, 9)
    ctx = localizer(ids, xyth)
    good = sightings((0.5, -0.4, 0.3), ids, xyth, [0, 1, 2, 3, 4, 5], rng)
    z, r = good[0][2], good[0][3]
    junk = [(900, 1, z, r),                                                   # an id outside the map
            (good[1][0], 0, good[1][2], r),                                   # gated
            (good[2][0], 1, np.array([np.nan, z[1], z[2]]), r),               # NaN observation
            (good[3][0], 1, np.array([z[0], z[1], np.inf]), r),
            (good[4][0], 1, z, np.array([r[0], 0.0, r[2]])),                  # r <= 0
            (good[5][0], 1, z, np.array([r[0], r[1], -0.01])),
            (good[5][0], 1, z, np.array([np.nan, r[1], r[2]]))]
    for name, obs in [("empty slot", []), ("only unusable observations", junk)]:
        got, _ = solve(ctx, ids, xyth, obs, name)
        assert got["status"] == 1 and got["best"] == -1 and got["n_candidates"] == 0
        assert not np.any(got["pose"]) and not np.any(got["sigma"])
    got, _ = solve(ctx, ids, xyth, junk + good[:1], "one usable observation behind the unusable ones", min_inliers=1)
    assert got["status"] == 0 and got["best"] == len(junk) and got["n_candidates"] == 1


def test_single_candidate():
    rng = np.random.RandomState(2)
    ids, xyth = random_map(rng, 9)
    ctx = localizer(ids, xyth)
    pose = (0.7, -0.3, 1.1)
    obs = sightings(pose, ids, xyth, [4], rng, noise=0.01)
    got, _ = solve(ctx, ids, xyth, obs, "min_inliers 1", min_inliers=1)
    assert got["status"] == 0 and got["n_inliers"] == 1 and got["runner_up"] == 0 and got["best"] == 0
    z, r = obs[0][2], obs[0][3]
    th = ref.wrap(xyth[4, 2] - z[2])
    c, s = math.cos(th), math.sin(th)
    hyp = np.array([xyth[4, 0] - (c * z[0] - s * z[1]), xyth[4, 1] - (s * z[0] + c * z[1]), th])
    J = np.array([[-c, s, -(s * z[0] + c * z[1])], [-s, -c, c * z[0] - s * z[1]], [0.0, 0.0, -1.0]])
    Cov = J @ np.diag(r) @ J.T
    assert np.abs(got["pose"] - hyp).max() <= TOL
    assert np.abs(got["sigma"] - Cov).max() <= TOL * np.abs(Cov).max()
    got, _ = solve(ctx, ids, xyth, obs, "min_inliers 2", min_inliers=2)
    assert got["status"] == 2 and got["n_inliers"] == 1 and got["best"] == 0
    assert not np.any(got["pose"]) and not np.any(got["sigma"])


@pytest.mark.parametrize("theta", [0.02, math.pi - 1e-3, -math.pi + 1e-3, math.nextafter(math.pi, 0.0), -math.pi],
                         ids=["near 0", "below pi", "above -pi", "the last heading below pi", "exactly -pi"])
def test_exact_observations_recover_the_pose(theta):
    rng = np.random.RandomState(3)
    ids, xyth = random_map(rng, 12)
    ctx = localizer(ids, xyth)
    pose = np.array([-0.8, 1.3, theta])
    obs = sightings(pose, ids, xyth, list(range(8)), rng)
    got, _ = solve(ctx, ids, xyth, obs, f"theta {theta}")
    assert got["status"] == 0 and got["n_inliers"] == 8 and got["n_candidates"] == 8 and got["runner_up"] == 0 and got["best"] == 0
    d = got["pose"] - pose
    d[2] = ref.wrap(d[2])
    assert np.abs(d).max() <= TOL, f"truth missed by {np.abs(d).max()}"
    assert -math.pi <= got["pose"][2] < math.pi


def test_headings_fuse_across_the_wrap():
    """hypotheses on both sides of the wrap: four sightings from heading pi - 1e-4, four from -pi + 1e-4, at one position"""
    rng = np.random.RandomState(13)
    ids, xyth = random_map(rng, 12)
    ctx = localizer(ids, xyth)
    lo = sightings((0.6, -1.1, math.pi - 1e-4), ids, xyth, [0, 1, 2, 3], rng)
    hi = sightings((0.6, -1.1, -math.pi + 1e-4), ids, xyth, [4, 5, 6, 7], rng)
    obs = [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3]]
    hyps = np.array([c[1][2] for c in ref.candidates(ids, xyth, obs)])
    assert (hyps > 3.0).sum() == 4 and (hyps < -3.0).sum() == 4
    got, _ = solve(ctx, ids, xyth, obs, "both sides of the wrap")
    assert got["status"] == 0 and got["n_inliers"] == 8 and got["runner_up"] == 0
    assert abs(ref.wrap(got["pose"][2] - math.pi)) <= 1e-4, "the headings were averaged through 0"
    assert math.hypot(got["pose"][0] - 0.6, got["pose"][1] + 1.1) <= 1e-3


def test_noisy_inliers_and_gross_outliers():
    rng = np.random.RandomState(4)
    ids, xyth = random_map(rng, 24)
    ctx = localizer(ids, xyth)
    pose = (1.2, 0.4, -2.2)
    inl = sightings(pose, ids, xyth, list(range(12)), rng, noise=0.01)
    outl = sightings(pose, ids, xyth, [12, 13, 14, 15, 16], rng, noise=0.01, label=[17, 18, 19, 20, 21])
    obs = [None] * 17
    where_out = [0, 3, 8, 9, 16]                                              # an outlier heads the list
    for p, o in zip(where_out, outl):
        obs[p] = o
    rest = iter(inl)
    obs = [o if o is not None else next(rest) for o in obs]
    got, want = solve(ctx, ids, xyth, obs, "12 inliers, 5 outliers")
    assert want["inliers"] == [p for p in range(17) if p not in where_out]
    assert got["status"] == 0 and got["n_inliers"] == 12 and got["best"] == 1 and got["n_candidates"] == 17
    assert 1 <= got["runner_up"] < 12
    assert math.hypot(got["pose"][0] - pose[0], got["pose"][1] - pose[1]) < 0.05


def test_equal_clusters_lowest_position_wins():
    rng = np.random.RandomState(5)
    ids, xyth = random_map(rng, 16)
    ctx = localizer(ids, xyth)
    A, B = np.array([0.5, 0.5, 0.4]), np.array([-1.5, 0.8, 2.0])
    a = sightings(A, ids, xyth, [0, 1, 2, 3], rng)
    b = sightings(B, ids, xyth, [4, 5, 6, 7], rng)
    obs = [a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3]]
    got, _ = solve(ctx, ids, xyth, obs, "A first")
    assert got["status"] == 0 and got["best"] == 0 and got["n_inliers"] == 4 and got["runner_up"] == 4
    assert np.abs(got["pose"] - A).max() <= TOL
    obs[0], obs[1] = obs[1], obs[0]
    got, _ = solve(ctx, ids, xyth, obs, "B first")
    assert got["status"] == 0 and got["best"] == 0 and got["n_inliers"] == 4 and got["runner_up"] == 4
    assert np.abs(got["pose"] - B).max() <= TOL


def test_one_id_twice():
    rng = np.random.RandomState(6)
    ids, xyth = random_map(rng, 10)
    ctx = localizer(ids, xyth)
    pose = (0.2, 0.9, -0.7)
    obs = sightings(pose, ids, xyth, [0, 1, 2, 1, 3], rng, noise=0.01)
    got, want = solve(ctx, ids, xyth, obs, "id twice, both inliers")
    assert got["status"] == 0 and got["n_candidates"] == 5 and got["n_inliers"] == 5 and want["inliers"] == [0, 1, 2, 3, 4]
    obs[3] = (obs[3][0], 1, obs[3][2] + np.array([0.9, -0.7, 0.5]), obs[3][3])      # the second sighting of the id is off
    got, want = solve(ctx, ids, xyth, obs, "id twice, one an outlier")
    assert got["status"] == 0 and got["n_candidates"] == 5 and got["n_inliers"] == 4 and want["inliers"] == [0, 1, 2, 4]


def crowd(rng, ids, xyth, n, pose, p_inlier=0.6, noise=0.005):
    """n candidates from a map of fewer landmarks (ids repeat): inliers seen from `pose` (the last of the list always one), wrong-id
    outliers in between"""
    obs = []
    L = len(ids)
    for k in range(n):
        li = int(rng.randint(L))
        if rng.uniform() < p_inlier or k == n - 1:
            obs += sightings(pose, ids, xyth, [li], rng, noise=noise)
        else:
            obs += sightings(pose, ids, xyth, [li], rng, noise=noise, label=[(li + 1 + int(rng.randint(L - 1))) % L])
    return obs


@pytest.mark.parametrize("n", [63, 64, 65, 128])
def test_wave_boundary_and_full_list(n):
    rng = np.random.RandomState(100 + n)
    ids, xyth = random_map(rng, 40)
    ctx = localizer(ids, xyth)
    pose = (-0.6, 0.3, 2.9)
    obs = crowd(rng, ids, xyth, n, pose)
    got, want = solve(ctx, ids, xyth, obs, f"{n} candidates")
    assert got["status"] == 0 and got["n_candidates"] == n and got["n_inliers"] >= n // 3
    if n > 64:
        assert min(want["inliers"]) < 64 <= max(want["inliers"]), "supporters in both waves"


# ---- argument errors and mode rules ---------------------------------------------------------------------------------------------

def test_argument_and_mode_rules():
    rng = np.random.RandomState(7)
    ids, xyth = random_map(rng, 9)
    ctx = emu_context(4, max_landmarks=16)
    obs = sightings((0.1, 0.2, 0.3), ids, xyth, [0, 1, 2], rng)
    inject(ctx, 0, obs)
    # SLAM mode: neither call
    refused(E_STATE, ctx.relocalize, 0)
    refused(E_STATE, ctx.fleet_relocalize, 0, [0])
    # localizing: the single call only
    ctx.localize_begin(ids, xyth, POSE0, SIG0)
    refused(E_STATE, ctx.fleet_relocalize, 0, [0])
    assert ctx.relocalize(0, apply=False)["status"] == 0                       # NULL params: the defaults
    want = ref.relocalize(ids, xyth, obs)
    check(ctx.relocalize(0, apply=False, tol_xy=0.25, tol_th=0.2, min_inliers=2), want, "defaults spelled out")
    for bad in [dict(tol_xy=0.0), dict(tol_xy=-0.1), dict(tol_xy=math.nan), dict(tol_xy=math.inf), dict(tol_th=0.0), dict(tol_th=-0.1),
                dict(tol_th=math.nan), dict(tol_th=math.inf), dict(tol_th=math.pi), dict(tol_th=4.0), dict(min_inliers=0),
                dict(min_inliers=-1), dict(min_inliers=129)]:
        refused(E_INVALID, ctx.relocalize, 0, False, **bad)
    assert ctx.relocalize(0, apply=False, tol_th=3.14, min_inliers=128)["status"] == 2
    refused(E_INVALID, ctx.relocalize, -1, False)
    refused(E_INVALID, ctx.relocalize, 4, False)
    assert ctx.lib.aslam_relocalize(ctx.h, 0, None, 0, None) == E_INVALID      # no result pointer
    ctx.localize_end()
    refused(E_STATE, ctx.relocalize, 0)
    # fleet SLAM: no shared map
    ctx.fleet_slam_begin([CAM, CAM])
    refused(E_STATE, ctx.fleet_relocalize, 0, [0])
    refused(E_STATE, ctx.relocalize, 0)
    # fleet localization: the fleet call only
    ctx.fleet_begin([CAM, CAM, CAM], ids, xyth, [POSE0] * 3, [SIG0] * 3)
    refused(E_STATE, ctx.relocalize, 0)
    inject(ctx, 0, obs)
    assert ctx.fleet_relocalize(0, [2], apply=False)["status"].tolist() == [0]
    refused(E_INVALID, ctx.fleet_relocalize, 0, [3], False)                    # a robot outside the fleet
    refused(E_INVALID, ctx.fleet_relocalize, 0, [-1], False)
    refused(E_INVALID, ctx.fleet_relocalize, 0, [1, 1], False)                 # a robot named twice
    refused(E_INVALID, ctx.fleet_relocalize, -1, [0], False)                   # slot ranges
    refused(E_INVALID, ctx.fleet_relocalize, 3, [0, 1], False)
    refused(E_INVALID, ctx.fleet_relocalize, 0, [], False)
    refused(E_INVALID, ctx.fleet_relocalize, 0, [0], False, tol_xy=0.0)
    refused(E_INVALID, ctx.fleet_relocalize, 0, [0], False, min_inliers=129)
    rs = np.zeros(1, np.int32)
    assert ctx.lib.aslam_fleet_relocalize(ctx.h, 0, 1, rs.ctypes.data_as(C.POINTER(C.c_int)), None, 0, None) == E_INVALID
    out = np.zeros(1, capi.RELOC_DTYPE)
    assert ctx.lib.aslam_fleet_relocalize(ctx.h, 0, 1, None, None, 0, out.ctypes.data_as(C.c_void_p)) == E_INVALID
    p = capi.RelocalizeParams()
    ctx.lib.aslam_default_relocalize_params(C.byref(p))
    assert (p.tol_xy, p.tol_th, p.min_inliers) == (0.25, 0.2, 2)


# ---- seating ---------------------------------------------------------------------------------------------------------------------

def test_single_apply():
    rng = np.random.RandomState(8)
    ids, xyth = random_map(rng, 12)
    ctx = localizer(ids, xyth, slots=3)
    true = np.array([1.4, -0.9, 2.5])                                          # far from POSE0: the filter alone would not get here
    frames = [sightings(true, ids, xyth, [0, 1, 2, 3, 4], rng, noise=0.01)] * 3   # the same list: "stationary" unless the list was emptied
    for s, obs in enumerate(frames):
        inject(ctx, s, obs)
    ctx.stage_encoders([3.0] * 3, [2.0] * 3, [0.05] * 3)
    ctx.run_staged(0, 1, with_ekf=2)                                           # one step: armed, a last-observed list
    ctx.sync()
    mu0, S0 = ctx.get_state()
    res = ctx.relocalize(1, apply=False)
    mu1, S1 = ctx.get_state()
    assert res["status"] == 0 and np.array_equal(mu0, mu1) and np.array_equal(S0, S1), "apply = 0 wrote the state"
    # an unsolved slot with apply = 1 writes nothing either
    assert ctx.relocalize(1, apply=True, min_inliers=6)["status"] == 2
    mu1, S1 = ctx.get_state()
    assert np.array_equal(mu0, mu1) and np.array_equal(S0, S1), "an unsolved apply wrote the state"
    res2 = ctx.relocalize(1, apply=True)
    assert res2.tobytes() == res.tobytes(), "apply changed the result"
    mu, S = ctx.get_state()
    assert np.array_equal(mu[:3], res["pose"]) and np.array_equal(S[:3, :3], res["sigma"])
    assert np.array_equal(mu[3:], xyth.reshape(-1)) and not np.any(S[3:, :]) and not np.any(S[:, 3:]), "the map moved"
    assert ctx.is_localizing()
    # the next step: the arming is untouched (this encoder sample is applied), the last-observed list is empty
    ctx.run_staged(1, 1, with_ekf=2)
    ctx.sync()
    want = FrozenMapLocalizer(ids, xyth, res["pose"], res["sigma"])
    want.is_init = True
    want.add_encoder(3.0, 2.0, 0.05)
    want.add_observations(frames[1])
    mu, S = ctx.get_state()
    assert np.abs(mu[:3] - want.mu).max() <= TOL and np.abs(S[:3, :3] - want.P).max() <= TOL * np.abs(want.P).max()
    assert ctx.get_slot_ekf_stats(1, 1).tolist() == [[5, 0, 5, 0]]
    assert math.hypot(mu[0] - true[0], mu[1] - true[1]) < 0.05


def fleet_of(ids, xyth, R, poses0, slots=None):
    ctx = emu_context(slots or R, max_landmarks=max(len(ids), 16))
    ctx.fleet_begin([CAM] * R, ids, xyth, poses0, [SIG0] * R)
    return ctx


def test_fleet_apply_seats_like_set_pose():
    rng = np.random.RandomState(9)
    ids, xyth = random_map(rng, 14)
    R = 3
    poses0 = np.array([POSE0, POSE0 + 0.1, POSE0 - 0.1])
    truth = [np.array([1.4, -0.9, 2.5]), np.array([-1.0, 1.0, -3.0]), np.array([0.3, 0.2, 0.1])]
    # tick 0 arms everyone; tick 1 is the frame relocalized on: robot 1 sees a single marker (unsolved at min_inliers 2), robot 2
    # nothing usable; ticks 2 and 3 repeat tick 1's observations of robots 0 and 1 exactly ("stationary" unless the list was emptied)
    tick0 = [sightings(truth[r], ids, xyth, [0, 1, 2], rng, noise=0.01) for r in range(R)]
    tick1 = [sightings(truth[0], ids, xyth, [3, 4, 5, 6], rng, noise=0.01), sightings(truth[1], ids, xyth, [7], rng, noise=0.01),
             [(901, 1, np.zeros(3), np.full(3, 0.02))]]
    ticks = [tick0, tick1, tick1, tick1]
    enc = ([3.0] * R, [2.0] * R, [0.05] * R)

    def step(ctx, obs_of):
        for r in range(R):
            inject(ctx, r, obs_of[r])
        ctx.stage_encoders(*enc)
        ctx.fleet_run_staged(0, list(range(R)), with_ekf=2)
        ctx.sync()
        return ctx.get_slot_ekf_stats(0, R)

    a, b = fleet_of(ids, xyth, R, poses0), fleet_of(ids, xyth, R, poses0)
    for ctx in (a, b):
        step(ctx, ticks[0])
        step(ctx, ticks[1])
        for r in range(R):
            inject(ctx, r, ticks[1][r])
    before = a.fleet_get_poses()
    res = a.fleet_relocalize(0, [0, 1, 2], apply=False)
    after = a.fleet_get_poses()
    assert all(np.array_equal(x, y) for x, y in zip(before, after)), "apply = 0 wrote a pose"
    assert res["status"].tolist() == [0, 2, 1]
    for r in range(R):
        check(res[r], ref.relocalize(ids, xyth, ticks[1][r]), f"robot {r}")
    res1 = a.fleet_relocalize(0, [0, 1, 2], apply=True)
    assert res1.tobytes() == res.tobytes()
    poses, sigs = a.fleet_get_poses()
    assert np.array_equal(poses[0], res["pose"][0]) and np.array_equal(sigs[0], res["sigma"][0]), "the getters do not return the result"
    for r in (1, 2):
        assert np.array_equal(poses[r], before[0][r]) and np.array_equal(sigs[r], before[1][r]), f"unsolved robot {r} was written"
    b.fleet_set_pose(0, res["pose"][0], res["sigma"][0])                       # the twin: seated by hand
    # the next frame repeats the last one: for the seated robot it arms only (no predict) and, its list emptied, fuses all four
    # observations; robots 1 and 2 stay armed (they predict) and robot 1's repeated observation is "stationary"
    for t in (2, 3):
        sa, sb = step(a, ticks[t]), step(b, ticks[t])
        assert np.array_equal(sa, sb), f"tick {t}: stats differ from the twin seated with aslam_fleet_set_pose"
        pa, pb = a.fleet_get_poses(), b.fleet_get_poses()
        assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]), f"tick {t}: poses differ from the twin"
        if t == 2:
            assert sa.tolist() == [[4, 0, 4, 0], [1, 0, 0, 1], [1, 0, 0, 0]]
            want = FrozenMapLocalizer(ids, xyth, res["pose"][0], res["sigma"][0])      # disarmed: the sample only arms it
            want.add_encoder(3.0, 2.0, 0.05)
            want.add_observations(ticks[2][0])
            assert np.abs(pa[0][0] - want.mu).max() <= TOL and np.abs(pa[1][0] - want.P).max() <= TOL * np.abs(want.P).max()
            assert np.abs(pa[0][2] - before[0][2]).max() > 1e-4, "the unsolved robot 2 lost its armed flag: no predict"
        else:
            assert sa.tolist() == [[4, 0, 0, 4], [1, 0, 1, 0], [1, 0, 0, 0]]     # a no-op leaves NaN behind: robot 1 fuses again
            want.add_encoder(3.0, 2.0, 0.05)                                   # armed now: the step after that predicts
            want.add_observations(ticks[3][0])
            assert np.abs(pa[0][0] - want.mu).max() <= TOL


def test_fleet_equals_single_and_repeats():
    rng = np.random.RandomState(10)
    ids, xyth = random_map(rng, 30)
    R = 3
    lists = [crowd(rng, ids, xyth, 7, (0.4, 0.1, -1.0)), crowd(rng, ids, xyth, 70, (-1.1, 0.9, 3.0)), crowd(rng, ids, xyth, 128, (2.0, -2.0, 0.6))]
    fleet = fleet_of(ids, xyth, R, [POSE0] * R, slots=5)
    for r in range(R):
        inject(fleet, 1 + r, lists[r])
    order = [2, 0, 1]                                                          # slot 1 + i belongs to robot order[i]
    got = fleet.fleet_relocalize(1, order, apply=False)
    again = fleet.fleet_relocalize(1, order, apply=False)
    assert got.tobytes() == again.tobytes(), "a second identical call gave other bits"
    single = localizer(ids, xyth)
    for i in range(R):
        inject(single, 0, lists[i])
        one = single.relocalize(0, apply=False)
        assert one.tobytes() == got[i].tobytes(), f"slot {1 + i}: the fleet's record differs from aslam_relocalize on the same list"
        assert ref.margin(ids, xyth, lists[i]) >= MARGIN
        check(got[i], ref.relocalize(ids, xyth, lists[i]), f"slot {1 + i}")
    assert got["status"].tolist() == [0, 0, 0]


@pytest.fixture(scope="module")
def big_fleet_case():
    rng = np.random.RandomState(11)
    ids, xyth = random_map(rng, 40)
    R = 256
    sizes = [int(rng.randint(1, 21)) if r % 16 else int(rng.randint(21, 129)) for r in range(R)]
    sizes[0], sizes[255], sizes[128] = 128, 1, 127
    truth = np.stack([rng.uniform(-2, 2, R), rng.uniform(-2, 2, R), rng.uniform(-math.pi, math.pi, R)], 1)
    lists = [crowd(rng, ids, xyth, sizes[r], truth[r]) for r in range(R)]
    want = [ref.relocalize(ids, xyth, obs) for obs in lists]
    assert min(ref.margin(ids, xyth, obs) for obs in lists) >= MARGIN
    return ids, xyth, lists, want


def test_256_robots_in_one_call(big_fleet_case):
    ids, xyth, lists, want = big_fleet_case
    R = 256
    fleet = fleet_of(ids, xyth, R, [POSE0] * R)
    for r in range(R):
        inject(fleet, r, lists[r])
    robots = [(r * 77 + 5) % R for r in range(R)]                              # slot r belongs to robot robots[r] (a permutation)
    got = fleet.fleet_relocalize(0, robots, apply=True)
    assert {int(w["status"]) for w in want} == {0, 2}, "the case should hold solved and unsolved slots"
    for r in range(R):
        check(got[r], want[r], f"slot {r} ({len(lists[r])} observations)")
    poses, sigs = fleet.fleet_get_poses()
    for r in range(R):
        if got["status"][r] == 0:
            assert np.array_equal(poses[robots[r]], got["pose"][r]) and np.array_equal(sigs[robots[r]], got["sigma"][r])
        else:
            assert np.array_equal(poses[robots[r]], POSE0) and np.array_equal(sigs[robots[r]], SIG0)


def test_buffer_survives_fleet_end():
    """the result buffer of the first call is freed by aslam_fleet_end: a call in a new fleet allocates again and gives the same bits"""
    rng = np.random.RandomState(12)
    ids, xyth = random_map(rng, 9)
    obs = sightings((0.3, -0.6, 1.9), ids, xyth, [0, 1, 2, 3], rng, noise=0.01)
    ctx = fleet_of(ids, xyth, 2, [POSE0] * 2)
    inject(ctx, 1, obs)
    first = ctx.fleet_relocalize(0, [1, 0], apply=False)
    ctx.fleet_end()
    ctx.fleet_begin([CAM] * 2, ids, xyth, [POSE0] * 2, [SIG0] * 2)
    second = ctx.fleet_relocalize(0, [1, 0], apply=False)
    assert first.tobytes() == second.tobytes() and first["status"].tolist() == [1, 0]
    ctx.fleet_end()
    ctx.localize_begin(ids, xyth, POSE0, SIG0)                                 # and the single call after a fleet ended
    assert ctx.relocalize(1, apply=False).tobytes() == first[1].tobytes()
    ctx.close()


# ---- on the MI355X: rendered frames of the 240 x 320 ring ------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_lost_fleet_recovers_on_rendered_frames():
    """4 robots started 1 m and 0.5 rad off the truth: one detection tick, aslam_fleet_relocalize(apply = 1), then 10 ticks of tracking"""
    w = synth.RingWorld(small_ring())
    cfg = w.cfg
    R = 4
    cams = [(w.K, np.zeros(5), (0.0, 0.0, 0.0))] * R
    phases = [5, 35, 65, 95]
    off = np.array([0.8, 0.6, 0.5])                                            # |(0.8, 0.6)| = 1 m
    truth0 = np.array([w.pose[p] for p in phases])
    ctx = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=R, max_landmarks=w.L + 8)
    synth.apply_detector(cfg, ctx=ctx)
    ctx.fleet_begin(cams, w.ids, w.world, truth0 + off, [np.diag([1e-4, 1e-4, 1e-5])] * R)

    def tick(t, with_ekf):
        frs = [w.rig_frame(phases[r] + t, [cams[r][2]])[0] for r in range(R)]
        imgs = [ctx.synth_render(r, cfg.rows, cfg.cols, cams[r][0], fr.ids, fr.poses, noise_amp=2, seed=1000 * r + t) for r, fr in enumerate(frs)]
        ctx.stage_frames(np.stack(imgs))
        ctx.stage_encoders([fr.wl for fr in frs], [fr.wr for fr in frs], [fr.dt for fr in frs])
        ctx.fleet_run_staged(0, list(range(R)), with_ekf=with_ekf)
        return frs

    frs = tick(1, 0)
    got = ctx.fleet_relocalize(0, list(range(R)), apply=True)                  # straight behind the detection: no sync in between
    ctx.sync()
    solved = []
    for r in range(R):
        i, v, z, rd = ctx.get_slot_raw_observations(r)
        obs = [(int(i[k]), int(v[k]), z[k], rd[k]) for k in range(len(i))]
        known = sum(1 for o in obs if o[1] and o[0] in set(w.ids.tolist()))
        hyp = np.array([c[1] for c in ref.candidates(w.ids, w.world, obs)])
        assert ref.margin(w.ids, w.world, obs) >= MARGIN
        want = ref.relocalize(w.ids, w.world, obs)
        check(got[r], want, f"robot {r}")
        if known >= 2:
            assert got["status"][r] == 0, f"robot {r} sees {known} map markers and did not solve"
        if got["status"][r] == 0:
            solved.append(r)
            tp = np.array(frs[r].true_pose)
            d_xy, d_th = math.hypot(*(got["pose"][r][:2] - tp[:2])), abs(ref.wrap(got["pose"][r][2] - tp[2]))
            inl = hyp[[k for k, c in enumerate(ref.candidates(w.ids, w.world, obs)) if c[0] in want["inliers"]]]
            spread_xy = max(math.hypot(*(a[:2] - b[:2])) for a in inl for b in inl)
            spread_th = max(abs(ref.wrap(a[2] - b[2])) for a in inl for b in inl)
            print(f"robot {r}: {known} map markers, {int(got['n_inliers'][r])} inliers, runner-up {int(got['runner_up'][r])}, to truth {d_xy:.4f} m "
                  f"{d_th:.4f} rad, spread of the inlier hypotheses {spread_xy:.4f} m {spread_th:.4f} rad")
            assert d_xy < 0.5 and d_th < 0.25, f"robot {r}: {d_xy} m, {d_th} rad from the truth"
    assert solved, "no robot saw two map markers: the scene does not exercise the feature"
    fused = np.zeros(R, int)
    for t in range(2, 12):
        frs = tick(t, 1)
        ctx.sync()
        fused += ctx.get_slot_ekf_stats(0, R)[:, 2]
    assert all(fused[r] > 0 for r in solved), fused
    poses, _ = ctx.fleet_get_poses()
    for r in solved:
        tp = frs[r].true_pose
        d_xy, d_th = math.hypot(poses[r][0] - tp[0], poses[r][1] - tp[1]), abs(ref.wrap(poses[r][2] - tp[2]))
        print(f"robot {r} after 10 ticks: {int(fused[r])} corrections, {d_xy:.4f} m {d_th:.4f} rad from the truth")
