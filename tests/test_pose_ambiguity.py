"""The pose ambiguity check (k_pose_alt, pose.hip) on injected quads, against the long-double restatement in
tests/ambiguity_reference.py.

aslam_debug_inject_candidates writes a slot's candidate list and aslam_debug_run_pose launches the pose stage; with
aslam_set_pose_ambiguity set, k_pose_alt follows k_pose.  The tests check:
  - the alt pose against the reference's converged second minimum (or the primary, where the descent returns to it): rotation
    distance and relative distance of t.  The bound comes from the reference alone: the worst distance, over the geometry cases,
    between the reference's own stopped iterate and its converged minimum - what the stopping rule permits - times 10;
  - the alt observation and dtheta against the reference formulas fed the kernel's own alt pose, at test_pose_kernel.py's obs_ref
    bound, and rms / rms_alt against sqrt(pose_reference.cost / 4) at that file's cost bound, with that file's measure (the
    difference over max(|reference|, 1): a residual of a noise-free case is the float rounding of its corners, a few 1e-5 px out of
    coordinates near 1e3 px, so its relative accuracy in double is limited by that cancellation, not by the kernel);
  - the flags against the rule applied to the record's own doubles, exactly; the slot sums; valid = 0 exactly where flag 2 is set;
    x, y, theta, R and the marker list bit for bit;
  - the group width (0 .. 128 markers, the marker cap), a record's independence of its neighbours, every camera source and mode,
    the refusals, and with the switch off bit-identical outputs.

Measured worst cases, emulation build / MI355X:
  reference's stopped iterate to its minimum (rotation, t relative):  4.8e-7, 3.3e-8   -> bound 4.8e-6, 3.3e-7
  alt pose to the reference's minimum (rotation, t relative):         4.8e-7, 3.3e-8 / 4.8e-7, 3.3e-8
  alt observation, dtheta vs reference:                               1.1e-15 / 1.1e-15   (bound 5e-15)
  rms, rms_alt vs reference:                                          1.2e-13 / 1.2e-13   (bound 1e-10 / 5e-9)
Runs on whichever library the session loads: the emulation here, the gfx950 build on the MI355X (the rendered scene needs the GPU)."""
import math

import numpy as np
import pytest

import ambiguity_reference as ar
import pose_reference as pr
import test_pose_kernel as tpk
from aruco_slam_amd import capi

E_INVALID, E_STATE, E_CAPACITY = -1, -5, -4
L = tpk.L
K900 = tpk.K900
DEFAULTS = dict(ratio=1.5, floor_px=0.5, min_dtheta=0.05, reject=1)

# (distance, yaw tilt about the camera's y axis, t_x); t = (t_x, 0.05, d)
PRESENT = [(1.5, 0.6, 0.2), (2.5, 0.3, 0.2), (2.5, 0.6, -0.8), (2.9, 0.3, 0.2), (2.0, 0.8, 0.2)]
ABSENT = [(0.8, 0.1, 0.2), (0.8, 0.3, 0.2), (0.8, 0.6, 0.2), (0.8, 0.8, 0.2), (1.5, 0.1, 0.2), (1.5, 0.2, 0.2), (1.5, 0.3, 0.2)]
GEOMETRY = PRESENT + ABSENT
NOISE = (0.0, 0.3, 0.7)
MOUNTS = [(0.1, -0.05, 0.4), (-0.2, 0.05, math.pi), (0.0, 0.15, -math.pi / 2), (0.05, -0.15, 2.5)]

WORST = {}


def note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module")
def tol(on_emulation):
    return tpk.EMU_TOL if on_emulation else tpk.GPU_TOL


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst cases: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def context(batch, landmarks=16, **over):
    return capi.Context(max_rows=64, max_cols=64, max_batch=batch, persistent_waves=4, max_landmarks=landmarks, **over)


def geometry_corners(d, tilt, tx, K, D, noise, rng):
    R = pr.rot_y(tilt) @ pr.facing()
    t = np.array([tx, 0.05, d], np.longdouble)
    c = np.asarray(pr.project(R, t, K, D, L), np.float64)
    return (c + noise * rng.normal(size=c.shape)).astype(np.float32)


def inject(ctx, slot, quads, ids=None, rots=None):
    n = len(quads)
    ids = np.arange(n) if ids is None else np.asarray(ids)
    rots = np.zeros(n, int) if rots is None else np.asarray(rots)
    cand = np.array([tpk.injected(np.asarray(q, np.float32).reshape(4, 2), r) for q, r in zip(quads, rots)], np.float32).reshape(-1, 8)
    ctx.inject_candidates(slot, ids, rots, cand if n else np.zeros((0, 8)))


def snapshot(ctx, slot):
    return ctx.get_slot_detections(slot) + ctx.get_slot_raw_observations(slot)


def same_bits(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_records(ctx, slot, cam, prm, before, tol):
    """everything a record promises short of the minimum itself: `before` = snapshot of the slot after the same pose stage with the
    switch off.  Returns (records, sum, raw observations)"""
    K, D, mount = cam
    rec, s = ctx.get_slot_pose_ambiguity(slot)
    ids, corners, rv, tv = ctx.get_slot_detections(slot)
    oids, valid, xyth, Rd = ctx.get_slot_raw_observations(slot)
    b_ids, b_corners, b_rv, b_tv, b_oids, b_valid, b_xyth, b_Rd = before
    assert same_bits((ids, corners, rv, tv), (b_ids, b_corners, b_rv, b_tv)), f"slot {slot}: the marker list changed"
    assert same_bits((oids, xyth, Rd), (b_oids, b_xyth, b_Rd)), f"slot {slot}: x, y, theta or R of an observation changed"
    n = len(ids)
    assert len(rec) == n and s["checked"] == n
    if n == 0:
        assert (s["ambiguous"], s["rejected"]) == (0, 0)
        return rec, s, (oids, valid, xyth, Rd)
    fin = (rec["flags"] & 4) == 0
    assert fin.all(), f"slot {slot}: non-finite second solve"
    assert ((rec["iters"] >= 1) & (rec["iters"] <= 20)).all()
    # the alt observation and dtheta against the reference formulas fed the kernel's own alt pose
    z = pr.observation(rec["rvec_alt"], rec["tvec_alt"], mount)
    e = max(tpk.rel(rec["xyth_alt"][:, :2], z[:, :2]), float(tpk.angle_diff(rec["xyth_alt"][:, 2], z[:, 2]).max()))
    e = max(e, float(np.max(np.abs(rec["dtheta"] - np.asarray(ar.dtheta(z[:, 2], xyth[:, 2]), np.float64)))))
    note("alt observation vs reference", e)
    assert e <= tol["obs_ref"], f"slot {slot}: alt observation differs from the reference by {e:.3g}"
    assert ((rec["xyth_alt"][:, 2] >= -math.pi) & (rec["xyth_alt"][:, 2] < math.pi)).all() and (rec["dtheta"] <= math.pi).all()
    r1 = np.sqrt(pr.cost(rv, tv, corners, K, D, L) / 4)
    r2 = np.sqrt(pr.cost(rec["rvec_alt"], rec["tvec_alt"], corners, K, D, L) / 4)
    e = max(tpk.rel(rec["rms"], r1), tpk.rel(rec["rms_alt"], r2))
    note("rms vs reference", e)
    assert e <= tol["cost"], f"slot {slot}: rms / rms_alt differ from the reference by {e:.3g}"
    # the rule on the record's own doubles, the sums, valid
    want = ar.flags(rec["rms"], rec["rms_alt"], rec["dtheta"], b_valid, fin, **prm)
    assert np.array_equal(rec["flags"], want), f"slot {slot}: flags {rec['flags'].tolist()}, the rule gives {want.tolist()}"
    assert (s["checked"], s["ambiguous"], s["rejected"]) == ar.slot_sum(want)
    assert np.array_equal(valid, np.where((want & 2) != 0, 0, b_valid)), f"slot {slot}: valid differs from the flags"
    return rec, s, (oids, valid, xyth, Rd)


def run_checked(ctx, cams, slots, prm, tol, robots=None):
    """the slots' pose stage with the switch off, then with prm; cams[i]: (K, D, mount) of slot i"""
    ctx.set_pose_ambiguity(None)
    ctx.run_pose(0, len(slots), robots)
    before = [snapshot(ctx, s) for s in range(len(slots))]
    ctx.set_pose_ambiguity(**prm)
    ctx.run_pose(0, len(slots), robots)
    return [check_records(ctx, s, cams[s], prm, before[s], tol) for s in range(len(slots))], before


# ---- 1 - 3: geometry cases, the alt pose against the reference's minimum ------------------------------------------------------------

@pytest.fixture(scope="module")
def geometry():
    """the four distortion cameras of test_pose_kernel.py as a rig with non-zero mounts: slot i is camera i and holds every geometry
    case at every noise level (fixed seed), corner rotation k % 4"""
    cams = [(K900, D, MOUNTS[i]) for i, D in enumerate(tpk.CAMERAS.values())]
    rng = np.random.RandomState(5)
    slots = []
    for K, D, _ in cams:
        quads, meta = [], []
        for noise in NOISE:
            for g in GEOMETRY:
                quads.append(geometry_corners(*g, K, D, noise, rng))
                meta.append((g, noise))
        slots.append((quads, meta))
    return cams, slots


def test_alt_pose_reaches_the_second_minimum(geometry, tol):
    """every geometry case x noise x camera: the alt pose against the reference's converged minimum, at 10x the worst distance of the
    reference's own stopped iterate from that minimum (measured: rotation 4.8e-7, t 3.3e-8; bound 4.8e-6, 3.3e-7).  The reference
    alone separates the cases: noise-free, a case of PRESENT has a second minimum tens of degrees off at 0.8 .. 6.3 px rms, a case of
    ABSENT returns to the primary pose.  Defaults: nothing noise-free is flagged (rms ~ 0), reject = 1"""
    cams, slots = geometry
    ctx = context(len(slots))
    ctx.set_camera_rig(cams)
    for s, (quads, _) in enumerate(slots):
        inject(ctx, s, quads, rots=np.arange(len(quads)) % 4)
    got, _ = run_checked(ctx, cams, slots, DEFAULTS, tol)
    stop_rot = stop_t = dev_rot = dev_t = 0.0
    for s, ((quads, meta), (rec, _, (_, _, xyth, _))) in enumerate(zip(slots, got)):
        K, D, mount = cams[s]
        ids, corners, rv, tv = ctx.get_slot_detections(s)
        assert len(ids) == len(quads)
        (r, t, c, it), (rm, tm, step) = ar.second_pose(rv, tv, corners, K, D, L)
        assert (step < 1e-15).all(), "the reference did not converge"
        nt = np.linalg.norm(np.asarray(tm, np.float64), axis=1)
        stop_rot = max(stop_rot, float(pr.rotation_distance(r, rm).max()))
        stop_t = max(stop_t, float(np.max(np.max(np.abs(np.asarray(t - tm, np.float64)), axis=1) / nt)))
        dev_rot = max(dev_rot, float(pr.rotation_distance(rec["rvec_alt"], rm).max()))
        dev_t = max(dev_t, float(np.max(np.max(np.abs(rec["tvec_alt"] - np.asarray(tm, np.float64)), axis=1) / nt)))
        # the reference alone separates the noise-free cases
        dth = np.asarray(ar.dtheta(pr.observation(rm, tm, mount)[:, 2], pr.observation(rv, tv, mount)[:, 2]), np.float64)
        rms_min = np.sqrt(np.asarray(pr.cost(rm, tm, corners, K, D, L), np.float64) / 4)
        for k, (g, noise) in enumerate(meta):
            if noise == 0.0 and g in PRESENT:
                assert dth[k] > 0.3 and 0.5 < rms_min[k] < 8.0, (g, dth[k], rms_min[k])
            if noise == 0.0 and g in ABSENT:
                assert dth[k] < 1e-6 and rms_min[k] < 1e-3, (g, dth[k], rms_min[k])
            if noise == 0.0:
                assert rec["flags"][k] == 0, (g, rec[k])             # the defaults: max(1.5 rms, 0.5) is far below a second minimum's rms
    note("reference stop to minimum (rotation)", stop_rot); note("reference stop to minimum (t)", stop_t)
    note("alt pose to minimum (rotation)", dev_rot); note("alt pose to minimum (t)", dev_t)
    assert dev_rot <= 10 * stop_rot and dev_t <= 10 * stop_t, f"alt pose {dev_rot:.3g} / {dev_t:.3g} from the minimum, the reference's own iterate {stop_rot:.3g} / {stop_t:.3g}"


# ---- 4: the rule, parameter sweep ---------------------------------------------------------------------------------------------------

SWEEP = [dict(ratio=1.0), dict(ratio=1e6), dict(floor_px=0.0), dict(floor_px=10.0), dict(min_dtheta=0.0), dict(min_dtheta=3.0),
         dict(reject=0), dict(ratio=1e6, reject=0), dict(floor_px=10.0, min_dtheta=0.0)]


def test_flag_rule_over_parameters(geometry, tol):
    """each threshold moved across the cases: ratio 1 / 1e6, floor_px 0 / 10, min_dtheta 0 / 3, reject 0.  Flags, sums and valid follow
    the rule on the record's doubles exactly; a list with range-gated sightings (valid = 0 before the check) is among them"""
    cams, slots = geometry
    cams, slots = cams[:2], slots[:2]
    ctx = context(2, useful_distance_threshold=2.7)                # the 2.9 m cases are invalid before the check: flagged, never rejected
    ctx.set_camera_rig(cams)
    for s, (quads, _) in enumerate(slots):
        inject(ctx, s, quads, rots=np.arange(len(quads)) % 4)
    seen = {}
    for over in SWEEP:
        prm = dict(DEFAULTS, **over)
        got, before = run_checked(ctx, cams, slots, prm, tol)
        assert ctx.get_pose_ambiguity() == prm
        fl = np.concatenate([g[0]["flags"] for g in got])
        seen[tuple(sorted(over.items()))] = fl
        gated = np.concatenate([b[5] for b in before]) == 0
        assert gated.any() and not (fl[gated] & 2).any()
    key = lambda **o: seen[tuple(sorted(o.items()))]
    assert (key(ratio=1e6) & 1).sum() > (key(ratio=1.0) & 1).sum()
    assert (key(floor_px=10.0) & 1).sum() > (key(floor_px=0.0) & 1).sum()
    assert (key(min_dtheta=0.0) & 1).sum() > (key(min_dtheta=3.0) & 1).sum() and not key(min_dtheta=3.0).any()
    assert (key(ratio=1e6) & 2).any() and (key(ratio=1e6, reject=0) & 1).any() and not (key(ratio=1e6, reject=0) & 2).any()
    assert np.array_equal(key(ratio=1e6) & 1, key(ratio=1e6, reject=0) & 1)
    assert (key(floor_px=10.0, min_dtheta=0.0) & 1).sum() > (key(floor_px=10.0) & 1).sum()


# ---- 5: sizes -----------------------------------------------------------------------------------------------------------------------

AMBIGUOUS = dict(ratio=1.0, floor_px=10.0, min_dtheta=0.05, reject=1)      # flags whatever has a second minimum within 10 px rms


def test_marker_counts_around_the_group_width(tol):
    """0, 1, 15, 16, 17, 31, 32, 33, 64, 65 and 128 markers in the slots of one call (32 markers per pass of the workgroup, 8 per
    wave), and a marker's record alone against the same marker at position 127: bit-identical"""
    counts = [0, 1, 15, 16, 17, 31, 32, 33, 64, 65, 128]
    rng = np.random.RandomState(21)
    quads = [q[2] for q in tpk.distinct_quads(128, rng)]
    cam = (K900, tpk.D_DEFAULT, (0.0, 0.0, 0.0))
    ctx = context(len(counts))
    ctx.set_camera(K900, tpk.D_DEFAULT)
    for s, n in enumerate(counts):
        inject(ctx, s, quads[127:] if n == 1 else quads[:n], ids=[127] if n == 1 else None)
    got, _ = run_checked(ctx, [cam] * len(counts), counts, AMBIGUOUS, tol)
    assert [int(g[1]["checked"]) for g in got] == counts
    full = got[counts.index(128)][0]
    assert 0 < (full["flags"] & 1).sum() < 128                   # both kinds among them
    assert got[counts.index(1)][0][0].tobytes() == full[127].tobytes(), "a marker's record depends on its neighbours"
    for s, n in enumerate(counts):                               # ... and on nothing else: a prefix of the list gives the same records
        assert got[s][0].tobytes() == full[:n].tobytes() or n == 1


def test_marker_cap():
    """300 identified candidates: the first 128 are checked, the overflow is reported as without the switch"""
    rng = np.random.RandomState(300)
    positions = sorted(rng.choice(2048, 300, replace=False).tolist())
    sl = tpk.list_case(positions, 2048, 2)
    ctx = context(1, landmarks=8)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    ctx.set_pose_ambiguity(**AMBIGUOUS)
    ctx.inject_candidates(0, sl.ids, sl.rots, np.array(sl.corners, np.float32).reshape(-1, 8))
    ctx.run_pose(0, 1)
    rec, s = ctx.get_slot_pose_ambiguity(0)
    ids, _, _, _ = ctx.get_slot_detections(0)
    assert len(rec) == 128 and s["checked"] == 128 and ids.tolist() == list(range(128))
    assert s["ambiguous"] == ((rec["flags"] & 1) != 0).sum() and s["rejected"] == ((rec["flags"] & 2) != 0).sum()
    with pytest.raises(capi.AslamError) as e:
        ctx.sync()
    assert e.value.code == E_CAPACITY


# ---- 6: modes -----------------------------------------------------------------------------------------------------------------------

def mode_quads(K, D, rng):
    """ids 0 .. 5: three markers with a second minimum (flagged under AMBIGUOUS) between three without"""
    cases = [(0.8, 0.3, 0.1), (2.5, 0.3, 0.2), (1.2, 0.1, -0.3), (2.0, 0.8, 0.5), (0.9, 0.5, -0.2), (2.5, 0.6, -0.8)]
    return [geometry_corners(*g, K, D, 0.0, rng) for g in cases], [1, 3, 5]


WL, WR, DT = 2.0, 2.3, 1 / 30.0


def slam_run(prm, tol):
    rng = np.random.RandomState(6)
    quads, flagged = mode_quads(K900, tpk.D_DEFAULT, rng)
    ctx = context(2)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    if prm is not None:
        ctx.set_pose_ambiguity(**prm)
    ctx.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
    inject(ctx, 0, [])
    inject(ctx, 1, quads)
    ctx.run_pose(0, 2)
    ctx.run_staged(0, 2, with_ekf=2)
    ctx.sync()
    return ctx, flagged


def test_slam_rejected_new_id_is_not_appended(tol):
    """SLAM on injected candidates then EKF steps: with reject = 1 the flagged new ids never become landmarks; with reject = 0 they
    do and the records flag them"""
    on, flagged = slam_run(AMBIGUOUS, tol)
    off, _ = slam_run(dict(AMBIGUOUS, reject=0), tol)
    rec_on, s_on = on.get_slot_pose_ambiguity(1)
    rec_off, s_off = off.get_slot_pose_ambiguity(1)
    assert np.nonzero(rec_on["flags"] & 1)[0].tolist() == flagged and (rec_on["flags"][flagged] == 3).all()
    assert np.nonzero(rec_off["flags"] & 1)[0].tolist() == flagged and (rec_off["flags"][flagged] == 1).all()
    assert (s_on["rejected"], s_off["rejected"]) == (3, 0)
    assert sorted(on.get_landmark_ids().tolist()) == [0, 2, 4] and sorted(off.get_landmark_ids().tolist()) == [0, 1, 2, 3, 4, 5]
    st_on, st_off = on.get_slot_ekf_stats(1, 1)[0], off.get_slot_ekf_stats(1, 1)[0]
    assert st_on[0] == st_off[0] == 6 and (st_on[1], st_off[1]) == (3, 6)
    assert on.get_slot_raw_observations(1)[1].tolist() == [1, 0, 1, 0, 1, 0]


def test_switch_off_is_bit_identical(tol):
    """a context that never heard of the switch, one that had it set and cleared again: every output the same bits"""
    a, _ = slam_run(None, tol)
    b, _ = slam_run(None, tol)
    b.set_pose_ambiguity(**AMBIGUOUS)
    b.set_pose_ambiguity(None)
    assert b.get_pose_ambiguity() is None
    inject(b, 1, mode_quads(K900, tpk.D_DEFAULT, np.random.RandomState(6))[0])
    inject(a, 1, mode_quads(K900, tpk.D_DEFAULT, np.random.RandomState(6))[0])
    for c in (a, b):
        c.run_pose(0, 2)
        c.run_staged(0, 2, with_ekf=2)
        c.sync()
    assert same_bits(snapshot(a, 1), snapshot(b, 1))
    assert same_bits(a.get_state(), b.get_state()) and np.array_equal(a.get_landmark_ids(), b.get_landmark_ids())
    assert "k_pose_alt" in a.profile_get() and a.profile_get()["k_pose_alt"][0] == 0


def test_localization_rejected_sighting_is_not_fused(tol):
    """localization against a map of the six ids: the flagged sightings are not fused with reject = 1"""
    def run(prm):
        rng = np.random.RandomState(6)
        quads, flagged = mode_quads(K900, tpk.D_DEFAULT, rng)
        ctx = context(2)
        ctx.set_camera(K900, tpk.D_DEFAULT)
        ctx.set_pose_ambiguity(**prm)
        ctx.localize_begin(np.arange(6), [[2.0, 0.3 * k - 0.8, 3.0] for k in range(6)], [0.0, 0.0, 0.0], np.eye(3) * 1e-2)
        ctx.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
        inject(ctx, 0, [])
        inject(ctx, 1, quads)
        ctx.run_pose(0, 2)
        ctx.run_staged(0, 2, with_ekf=2)
        ctx.sync()
        return ctx
    on, off = run(AMBIGUOUS), run(dict(AMBIGUOUS, reject=0))
    assert on.get_slot_raw_observations(1)[1].tolist() == [1, 0, 1, 0, 1, 0] and off.get_slot_raw_observations(1)[1].all()
    st_on, st_off = on.get_slot_ekf_stats(1, 1)[0], off.get_slot_ekf_stats(1, 1)[0]
    assert st_on[2] == 3 and st_off[2] == 6, (st_on, st_off)
    assert not np.array_equal(on.get_state()[0][:3], off.get_state()[0][:3])


def test_rig_rejection_survives_the_merge(tol):
    """two cameras with different mounts: the records follow each camera's mount, and the merged step list appends only what passed"""
    cams = [(K900, tpk.D_DEFAULT, (0.1, 0.0, 0.0)), (np.array([[620.0, 0, 630], [0, 626.2, 350], [0, 0, 1]]), tpk.D_STRONG, (-0.2, 0.05, math.pi))]
    rng = np.random.RandomState(7)
    lists = [mode_quads(K, D, rng)[0] for K, D, _ in cams]
    out = {}
    for reject in (1, 0):
        prm = dict(AMBIGUOUS, reject=reject)
        ctx = context(4)
        ctx.set_camera_rig(cams)
        for s in range(4):
            inject(ctx, s, lists[s % 2] if s >= 2 else [], ids=np.arange(6) + 10 * (s % 2) if s >= 2 else None)
        ctx.stage_encoders([0.0, 0.0, WL, WL], [0.0, 0.0, WR, WR], [0.0, 0.0, DT, DT])
        got, _ = run_checked(ctx, [cams[s % 2] for s in range(4)], range(4), prm, tol)
        ctx.run_staged_rig(0, 2, with_ekf=2)
        ctx.sync()
        out[reject] = (sorted(ctx.get_landmark_ids().tolist()), [g[0]["flags"].tolist() for g in got[2:]])
    flagged = lambda fl: [i for i, f in enumerate(fl) if f & 1]
    f0, f1 = flagged(out[1][1][0]), flagged(out[1][1][1])
    assert f0 and f1 and all(f == 3 for k in (0, 1) for i, f in enumerate(out[1][1][k]) if i in (f0, f1)[k])
    assert out[1][0] == sorted([i for i in range(6) if i not in f0] + [10 + i for i in range(6) if i not in f1])
    assert out[0][0] == sorted(list(range(6)) + list(range(10, 16)))


@pytest.mark.parametrize("kind", ["slam", "localize"])
def test_fleet_cameras_come_from_the_table(kind, tol):
    """both fleet kinds: slot i is robot robots[i]'s, its camera and mount read from the fleet's table"""
    n = 3
    cams = tpk.rig_cameras(n)
    ctx = context(4)
    if kind == "slam":
        ctx.fleet_slam_begin(cams)
    else:
        ctx.fleet_begin(cams, [500], [[5.0, 0.0, 0.0]], np.zeros((n, 3)), np.tile(np.eye(3) * 1e-2, (n, 1, 1)))
    robots = [2, 0, 1, 2]
    rng = np.random.RandomState(9)
    for s, r in enumerate(robots):
        inject(ctx, s, mode_quads(cams[r][0], cams[r][1], rng)[0])
    got, _ = run_checked(ctx, [cams[r] for r in robots], robots, AMBIGUOUS, tol, robots=robots)
    assert all((g[0]["flags"] & 2).any() for g in got)


# ---- 7: errors ----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    ctx = context(2)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    with pytest.raises(capi.AslamError) as e:
        ctx.get_slot_pose_ambiguity(0)
    assert e.value.code == E_STATE
    ctx.set_pose_ambiguity(ratio=2.0, floor_px=0.25, min_dtheta=0.1, reject=0)
    want = dict(ratio=2.0, floor_px=0.25, min_dtheta=0.1, reject=0)
    for bad in (dict(ratio=0.99), dict(ratio=math.inf), dict(ratio=math.nan), dict(floor_px=-1e-9), dict(floor_px=math.inf),
                dict(floor_px=math.nan), dict(min_dtheta=-1e-9), dict(min_dtheta=math.pi), dict(min_dtheta=math.nan), dict(reject=2),
                dict(reject=-1)):
        with pytest.raises(capi.AslamError) as e:
            ctx.set_pose_ambiguity(**bad)
        assert e.value.code == E_INVALID, bad
        assert ctx.get_pose_ambiguity() == want                   # a refused call changes nothing
    for slot in (-1, 2):
        with pytest.raises(capi.AslamError) as e:
            ctx.get_slot_pose_ambiguity(slot)
        assert e.value.code == E_INVALID
    n = capi.C.c_int()
    assert ctx.lib.aslam_get_slot_pose_ambiguity(ctx.h, 0, -1, capi.C.byref(n), None, None) == E_INVALID
    assert ctx.lib.aslam_get_slot_pose_ambiguity(ctx.h, 0, 4, capi.C.byref(n), None, None) == E_INVALID
    assert ctx.lib.aslam_get_slot_pose_ambiguity(ctx.h, 0, 0, None, None, None) == E_INVALID
    assert ctx.lib.aslam_set_pose_ambiguity(None, None) == E_INVALID
    rec, s = ctx.get_slot_pose_ambiguity(1)                       # never checked: empty
    assert len(rec) == 0 and s["checked"] == 0
    ctx.set_pose_ambiguity(None)
    assert ctx.get_pose_ambiguity() is None
    with pytest.raises(capi.AslamError) as e:
        ctx.get_slot_pose_ambiguity(0)
    assert e.value.code == E_STATE
    ctx.set_pose_ambiguity()
    assert ctx.get_pose_ambiguity() == DEFAULTS


# ---- 8: one rendered scene ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rendered_far_tilted_marker():
    """640 x 480: an arming frame, then frames with a near frontal marker (id 3, 0.9 m) and a far tilted one (id 7, 2.5 m, 0.3 rad).  The
    reference puts the far marker's second minimum at 1.06 px rms on exact corners; floor_px = 3 is above it, so the far marker is
    ambiguous by construction: with reject = 1 its id never enters the map, with reject = 0 it does and the record flags it"""
    rows, cols, n = 480, 640, 4
    K = np.array([[900.0, 0, 320], [0, 900, 240], [0, 0, 1]])
    near = np.concatenate([np.asarray(pr.rot_y(0.05) @ pr.facing(), np.float64).reshape(9), [-0.151, 0.02, 0.9]])
    far = np.concatenate([np.asarray(pr.rot_y(0.3) @ pr.facing(), np.float64).reshape(9), [0.2, 0.05, 2.5]])
    maps = {}
    for reject in (1, 0):
        ctx = capi.Context(max_rows=rows, max_cols=cols, max_batch=n, max_landmarks=16)
        ctx.set_camera(K, np.zeros(5))
        ctx.set_pose_ambiguity(ratio=1.0, floor_px=3.0, min_dtheta=0.05, reject=reject)
        for i in range(n):
            ctx.synth_render(i, rows, cols, K, [] if i == 0 else [3, 7], np.zeros((0, 12)) if i == 0 else np.array([near, far]), noise_amp=2,
                             seed=i, download=False)
        ctx.stage_encoders([0.0] * n, [0.0] * n, [0.0] + [1 / 30.0] * (n - 1))
        ctx.run_staged(0, n, with_ekf=True)
        ctx.sync()
        for i in range(1, n):
            ids = ctx.get_slot_detections(i)[0].tolist()
            assert sorted(ids) == [3, 7], f"frame {i}: detected {ids}"
            rec, s = ctx.get_slot_pose_ambiguity(i)
            by_id = dict(zip(ids, rec))
            assert by_id[7]["flags"] == (3 if reject else 1) and by_id[3]["flags"] == 0, (i, rec)
            assert by_id[7]["dtheta"] > 0.05 and by_id[7]["rms_alt"] <= 3.0 and by_id[3]["dtheta"] < 0.05
            assert (s["checked"], s["ambiguous"], s["rejected"]) == (2, 1, reject)
        maps[reject] = sorted(ctx.get_landmark_ids().tolist())
    assert maps[1] == [3] and maps[0] == [3, 7]
