"""The observation covariance (k_pose_cov, pose.hip) on injected quads, against the long-double restatement in
tests/obs_covariance_reference.py.

aslam_debug_inject_candidates writes a slot's candidate list and aslam_debug_run_pose launches the pose stage; with
aslam_set_observation_covariance set, k_pose_cov follows k_pose.  The tests check:
  - cov against the reference fed the kernel's own stored pose: the largest absolute difference over the 9 entries, divided by the
    largest absolute entry of the reference's, at most 64 kappa_2(N_ref) 2^-53 per marker - the forward error of a backward-stable
    6 x 6 solve on inputs a few ulps off, derived, not measured; sigma2 and e2 against pose_reference.cost at test_pose_kernel.py's
    cost bound; cov symmetric to the bit;
  - the rule on the record's own doubles: R within 2 ulp of scale cov[ii] + floor, flags, slot sums and valid exactly, r_ref and
    everything else of the slot bit-identical to the switch-off pose stage;
  - the statistical consistency the feature is for: d^2 of the observation error against the noise-free truth under cov has the mean
    of chi^2_3 within 5 standard errors, and under the reference's diagonal R a mean below 0.1;
  - the group width (0 .. 128 markers), a record's independence of its neighbours, every camera source and mode, both switches
    together, the new R in the filter (bit-identical to a switch-off context fed the same raw observations), the refusals, and with
    the switch off bit-identical outputs.

Measured worst cases, emulation build / MI355X (the same figures on both: no contraction, one fixed order):
  kappa_2(N) over every case of this file:                            436 .. 5.93e4
  cov vs reference (relative to the reference's largest entry):       1.27e-13 / 1.27e-13
  ... as a fraction of the bound 64 kappa_2(N) 2^-53:                 0.0175 / 0.0175
  e2, sigma2 vs reference:                                            2.0e-13 / 2.0e-13   (bound 1e-10 / 5e-9)
  mean d^2 per table geometry (reference = kernel to 3 decimals):     2.697, 3.330, 3.214, 2.900, 2.831; pooled 2.994
  ... with the reference's diagonal R:                                0.0140, 0.0053, 0.0025, 0.0033, 0.0021
Runs on whichever library the session loads: the emulation here, the gfx950 build on the MI355X (the rendered scene needs the GPU)."""
import math

import numpy as np
import pytest

import ambiguity_reference as ar
import obs_covariance_reference as ocr
import pose_reference as pr
import test_pose_ambiguity as tpa
import test_pose_kernel as tpk
from aruco_slam_amd import capi, synth
from test_fleet_slam import no_windows_context

E_INVALID, E_STATE = -1, -5
L = tpk.L
K900 = tpk.K900
DEFAULTS = dict(ocr.DEFAULTS)
MOUNTS = tpa.MOUNTS
GEOMETRY = tpa.GEOMETRY + [(2.9, 0.0, 0.0), (0.5, 0.0, 0.0), (2.9, 1.3, 0.9)]
NOISE = (0.0, 0.3, 0.7)
# the geometries of the consistency table: distance, tilt, t_x
TABLE = [(0.8, 0.3, 0.2), (1.5, 0.6, 0.2), (2.0, 0.8, 0.2), (1.5, 0.3, -0.4), (2.5, 0.6, -0.8)]
STAT_MOUNT = (0.1, -0.05, 0.4)
WL, WR, DT = 2.0, 2.3, 1 / 30.0

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


context = tpa.context
inject = tpa.inject
snapshot = tpa.snapshot
same_bits = tpa.same_bits
geometry_corners = tpa.geometry_corners


def check_rule(ctx, slot, prm, before, threshold=3.0):
    """everything a record promises short of the covariance itself: `before` = snapshot of the slot after the same pose stage with the
    switch off.  Returns (records, sum, raw observations)"""
    rec, s = ctx.get_slot_obs_covariance(slot)
    ids, corners, rv, tv = ctx.get_slot_detections(slot)
    oids, valid, xyth, Rd = ctx.get_slot_raw_observations(slot)
    b_ids, b_corners, b_rv, b_tv, b_oids, b_valid, b_xyth, b_Rd = before
    assert same_bits((ids, corners, rv, tv), (b_ids, b_corners, b_rv, b_tv)), f"slot {slot}: the marker list changed"
    assert same_bits((oids, xyth), (b_oids, b_xyth)), f"slot {slot}: id, x, y or theta of an observation changed"
    n = len(ids)
    assert len(rec) == n and s["checked"] == n
    if n == 0:
        assert (s["degenerate"], s["gated"]) == (0, 0)
        return rec, s, (oids, valid, xyth, Rd)
    assert rec["r_ref"].tobytes() == b_Rd.tobytes(), f"slot {slot}: r_ref is not the switch-off R"
    assert rec["cov"].tobytes() == np.ascontiguousarray(rec["cov"].transpose(0, 2, 1)).tobytes(), f"slot {slot}: cov is not symmetric to the bit"
    flag1 = (rec["flags"] & 1) != 0
    assert not rec["cov"][flag1].any() and Rd[flag1].tobytes() == b_Rd[flag1].tobytes()
    assert np.array_equal(flag1, ocr.degenerate(rec["cov"]) | flag1)     # a finite record has a positive diagonal
    assert not ocr.degenerate(rec["cov"][~flag1]).any()
    r, want = ocr.rule(rec["cov"], flag1, tv, threshold, **prm)
    ok = ~flag1
    assert (np.abs(Rd[ok] - r[ok]) <= 2 * np.spacing(r[ok])).all(), f"slot {slot}: R is not scale cov[ii] + floor"
    # flag 2 on the R that was written (within 2 ulp of the rule's: a norm inside that margin of gate_norm would be a badly made case)
    with np.errstate(all="ignore"):
        norm = np.sqrt(Rd[:, 0] * Rd[:, 0] + Rd[:, 1] * Rd[:, 1] + Rd[:, 2] * Rd[:, 2])
    want = np.where(ok, (want & ~2) | np.where(norm > np.float64(prm["gate_norm"]), 2, 0), want)
    assert np.array_equal(rec["flags"], want), f"slot {slot}: flags {rec['flags'].tolist()}, the rule gives {want.tolist()}"
    assert (s["checked"], s["degenerate"], s["gated"]) == ocr.slot_sum(want)
    assert np.array_equal(valid, ((rec["flags"] & 7) == 0).astype(np.int32)), f"slot {slot}: valid differs from the flags"
    return rec, s, (oids, valid, xyth, Rd)


def run_checked(ctx, slots, prm, robots=None, threshold=3.0, refine=False):
    """the slots' pose stage with the switch off, then with prm"""
    ctx.set_observation_covariance(None)
    ctx.run_pose(0, len(slots), robots, refine=refine)
    before = [snapshot(ctx, s) for s in range(len(slots))]
    ctx.set_observation_covariance(**prm)
    assert ctx.get_observation_covariance() == prm
    ctx.run_pose(0, len(slots), robots, refine=refine)
    return [check_rule(ctx, s, prm, before[s], threshold) for s in range(len(slots))], before


def check_covariance(ctx, slot, cam, prm, rec, tol):
    """the records of a slot against the reference fed the kernel's own stored pose.  Returns the reference's flag 1"""
    K, D, mount = cam
    _, corners, rv, tv = ctx.get_slot_detections(slot)
    cov, sigma2, e2, N = ocr.covariance(rv, tv, corners, K, D, L, mount, **prm)
    deg = ocr.degenerate(cov)
    assert np.array_equal((rec["flags"] & 1) != 0, deg), f"slot {slot}: flag 1 {(rec['flags'] & 1).tolist()}, the reference {deg.tolist()}"
    ok = ~deg
    if ok.any():
        kap = ocr.kappa2(N[ok])
        ref = np.asarray(cov[ok], np.longdouble)
        err = np.asarray(np.max(np.abs(rec["cov"][ok].astype(np.longdouble) - ref), axis=(1, 2)) / np.max(np.abs(ref), axis=(1, 2)), np.float64)
        bound = 64 * kap * 2.0 ** -53
        note("cov vs reference (relative)", err.max()); note("cov vs reference / bound", (err / bound).max()); note("kappa_2(N)", kap.max())
        WORST["kappa_2(N) min"] = min(WORST.get("kappa_2(N) min", np.inf), float(kap.min()))
        assert (err <= bound).all(), f"slot {slot}: cov off by {err.max():.3g}, {(err / bound).max():.3g} of the bound"
        e = max(tpk.rel(rec["e2"][ok], e2[ok]), tpk.rel(rec["sigma2"][ok], sigma2[ok]))
        note("e2, sigma2 vs reference", e)
        assert e <= tol["cost"], f"slot {slot}: e2 / sigma2 differ from the reference by {e:.3g}"
    return deg


# ---- 1: the covariance against the reference ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def geometry():
    """slot i: camera i of the four distortion cameras, every geometry case at every noise level (fixed seed), corner rotation k % 4"""
    rng = np.random.RandomState(5)
    slots = []
    for D in tpk.CAMERAS.values():
        slots.append([geometry_corners(*g, K900, D, noise, rng) for noise in NOISE for g in GEOMETRY])
    return slots


@pytest.mark.parametrize("mount", range(len(MOUNTS)))
def test_covariance_against_the_reference(geometry, mount, tol):
    """15 geometries x 3 noise levels x 4 distortion cameras x 4 mounts (psi = pi and -pi / 2 among them) under the defaults
    (use_residual = 1).  Bound per marker: 64 kappa_2(N_ref) 2^-53.  Measured: kappa_2(N) between 436 and 5.93e4; worst cov error
    1.27e-13 relative, 0.0175 of the bound, on the emulation and on the MI355X alike."""
    cams = [(K900, D, MOUNTS[mount]) for D in tpk.CAMERAS.values()]
    ctx = context(len(cams))
    ctx.set_camera_rig(cams)
    for s, quads in enumerate(geometry):
        inject(ctx, s, quads, rots=np.arange(len(quads)) % 4)
    got, _ = run_checked(ctx, geometry, DEFAULTS)
    for s, (rec, _, _) in enumerate(got):
        assert len(rec) == len(GEOMETRY) * len(NOISE)
        deg = check_covariance(ctx, s, cams[s], DEFAULTS, rec, tol)
        assert not deg.any()
        gated4 = (rec["flags"] & 4) != 0
        assert gated4.sum() == len(NOISE), "the oblique 2.9 m case lies past the range gate, the others inside"


# ---- 2: the rule ----------------------------------------------------------------------------------------------------------------------

def test_range_gate_around_three_metres():
    """markers at |t| = 2.8 .. 3.2 m: flag 4 against pose_reference.range_gate, away from its margin"""
    rng = np.random.RandomState(3)
    dist = [2.8, 2.9, 2.97, 3.03, 3.1, 3.2]
    quads = [geometry_corners(math.sqrt(d * d - 0.2 ** 2 - 0.05 ** 2), 0.4, 0.2, K900, tpk.D_DEFAULT, 0.0, rng) for d in dist]
    ctx = context(1)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    inject(ctx, 0, quads)
    (rec, s, _), = run_checked(ctx, [quads], DEFAULTS)[0]
    passes, margin = pr.range_gate(ctx.get_slot_detections(0)[3])
    assert (margin > 1e-3).all()
    assert ((rec["flags"] & 4) == 0).tolist() == passes.tolist() == [True] * 3 + [False] * 3
    assert not (rec["flags"] & 3).any() and s["gated"] == 0


def test_gate_norm_between_two_markers():
    """gate_norm placed at the geometric mean of a near and a far marker's |R| (a clear margin: the two differ by a large factor),
    then +inf"""
    rng = np.random.RandomState(4)
    quads = [geometry_corners(0.8, 0.3, 0.2, K900, tpk.D_DEFAULT, 0.3, rng), geometry_corners(2.9, 0.0, 0.0, K900, tpk.D_DEFAULT, 0.3, rng)]
    ctx = context(1)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    inject(ctx, 0, quads)
    (_, _, (_, valid, _, Rd)), = run_checked(ctx, [quads], dict(DEFAULTS, gate_norm=math.inf))[0]
    norm = np.sqrt((Rd * Rd).sum(axis=1))
    assert valid.tolist() == [1, 1] and norm[1] > 4 * norm[0]
    prm = dict(DEFAULTS, gate_norm=float(math.sqrt(norm[0] * norm[1])))
    (rec, s, (_, valid, _, _)), = run_checked(ctx, [quads], prm)[0]
    assert rec["flags"].tolist() == [0, 2] and valid.tolist() == [1, 0] and s["gated"] == 1


def test_scale_and_floors():
    """scale and the floors enter R and nothing else: cov, sigma2 and e2 of the record do not move"""
    rng = np.random.RandomState(8)
    quads = [geometry_corners(*g, K900, tpk.D_STRONG, 0.3, rng) for g in TABLE]
    ctx = context(1)
    ctx.set_camera(K900, tpk.D_STRONG)
    inject(ctx, 0, quads)
    (base, _, _), = run_checked(ctx, [quads], DEFAULTS)[0]
    for over in (dict(scale=7.5), dict(floor_xy=0.0, floor_th=0.0), dict(floor_xy=1e-3, floor_th=0.25), dict(use_residual=0, sigma_px=0.3)):
        (rec, _, _), = run_checked(ctx, [quads], dict(DEFAULTS, **over))[0]
        if "use_residual" not in over:
            assert rec.tobytes() == base.tobytes()
        else:
            assert (rec["sigma2"] == 0.3 * 0.3).all() and rec["e2"].tobytes() == base["e2"].tobytes()


def test_sighting_the_reference_gate_dropped_comes_back(tol):
    """test_pose_kernel.py's covariance-gate case: corner noise sized so that the reference's |diag R| lands at 0.5x, 0.99x, 1.01x and 2x
    its gate.  k_pose drops the last two; their first-order covariance is small and they come back valid"""
    rng = np.random.RandomState(4)
    R = pr.rot_x(0.25) @ pr.facing()
    t = np.array([0.1, 0.05, 1.5], np.longdouble)
    c0 = tpk.corners_of(R, t, K900, tpk.D_DEFAULT)
    pattern = rng.normal(size=(4, 2))
    quads = []
    for target in (0.5, 0.99, 1.01, 2.0):
        lo, hi = 0.0, 200.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if tpk.gate_value((c0 + mid * pattern).astype(np.float32), K900, tpk.D_DEFAULT) < target else (lo, mid)
        quads.append((c0 + hi * pattern).astype(np.float32))
    ctx = context(1)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    inject(ctx, 0, quads)
    got, before = run_checked(ctx, [quads], DEFAULTS)
    rec, _, (_, valid, _, _) = got[0]
    assert before[0][5].tolist() == [1, 1, 0, 0] and valid.tolist() == [1, 1, 1, 1] and not rec["flags"].any()
    check_covariance(ctx, 0, (K900, tpk.D_DEFAULT, (0.0, 0.0, 0.0)), DEFAULTS, rec, tol)
    assert (np.diff(rec["sigma2"]) > 0).all()                      # use_residual: the worse the fit, the larger the pixel variance


def test_degenerate_quads(tol):
    """four coincident corners and four collinear ones between two ordinary markers: flag 1 exactly where the reference, fed the pose
    k_pose stored, has no finite positive covariance; the neighbours are untouched by it"""
    rng = np.random.RandomState(9)
    good = [geometry_corners(1.5, 0.3, 0.2, K900, tpk.D_DEFAULT, 0.3, rng) for _ in range(2)]
    point = np.full((4, 2), 300.0, np.float32)
    line = np.array([[100, 100], [140, 140], [180, 180], [220, 220]], np.float32)
    quads = [good[0], point, line, good[1]]
    ctx = context(2)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    inject(ctx, 0, quads)
    inject(ctx, 1, good)
    got, _ = run_checked(ctx, [quads, good], DEFAULTS)
    rec, s, (_, valid, _, _) = got[0]
    cam = (K900, tpk.D_DEFAULT, (0.0, 0.0, 0.0))
    _, corners, rv, tv = ctx.get_slot_detections(0)
    with np.errstate(all="ignore"):
        cov, _, _, N = ocr.covariance(rv, tv, corners, *cam[:2], L, cam[2], **DEFAULTS)
        kap = ocr.kappa2(N)
    deg = ocr.degenerate(cov)
    print("degenerate quads: reference flag 1", deg.tolist(), "kernel flags", rec["flags"].tolist(), "kappa_2(N)", [f"{k:.3g}" for k in kap],
          "poses", rv[1:3].tolist(), tv[1:3].tolist())
    assert ((rec["flags"] & 1) != 0).tolist() == deg.tolist() and not deg[[0, 3]].any()
    assert s["degenerate"] == deg.sum() and not valid[deg].any()
    assert rec[[0, 3]].tobytes() == got[1][0].tobytes()


# ---- 3: statistical consistency -------------------------------------------------------------------------------------------------------

def test_statistical_consistency():
    """The five geometries of DESIGN.md §31's table, strong distortion, mount (0.1, -0.05, 0.4); 128 draws of N(0, 0.3^2) corner noise
    each, sigma_px = 0.3 without the residual term.  d^2 = e^T cov^-1 e of the observation error against the noise-free truth is
    chi^2_3 (mean 3, variance 6) if cov is the error's covariance: pooled mean in 3 +- 5 sqrt(6 / 640) = [2.52, 3.48], each geometry's
    in 3 +- 5 sqrt(6 / 128) = [1.92, 4.08].  The same two conditions are asserted first on the reference alone (Gauss-Newton to the
    minimum, reference covariance), so that a failure there is the test's.  With the reference's diagonal R the pooled mean is
    below 0.1.  Measured, the reference, the emulation and the MI355X alike: 2.697, 3.330, 3.214, 2.900, 2.831, pooled 2.994; with the
    reference's R 0.0140, 0.0053, 0.0025, 0.0033, 0.0021."""
    K, D, mount = K900, tpk.D_STRONG, STAT_MOUNT
    prm = dict(DEFAULTS, sigma_px=0.3, use_residual=0, scale=1.0)
    rng = np.random.default_rng(7)
    slots, truth, poses = [], [], []
    for d, tilt, tx in TABLE:
        R = pr.rot_y(tilt) @ pr.facing()
        t = np.array([tx, 0.05, d], np.longdouble)
        exact = np.asarray(pr.project(R, t, K, D, L), np.float64)
        slots.append((exact[None] + 0.3 * rng.normal(size=(128, 4, 2))).astype(np.float32))
        truth.append(np.asarray(ocr.observation_at(R, t, mount), np.float64))
        poses.append((R, t))

    def conditions(means, who):
        pooled = float(np.mean(means))
        print(f"{who}: mean d^2 per geometry {[round(float(m), 3) for m in means]}, pooled {pooled:.3f}")
        assert 2.52 <= pooled <= 3.48, f"{who}: pooled mean d^2 {pooled:.3f}"
        assert all(1.92 <= m <= 4.08 for m in means), f"{who}: a geometry's mean d^2 outside [1.92, 4.08]: {means}"

    # the reference alone
    ref_means = []
    for (R, t), c, z in zip(poses, slots, truth):
        r0 = np.repeat(ar.rodrigues_inv(R[None]), 128, axis=0)
        rv, tv, step = ar.converge(r0, np.repeat(t[None], 128, axis=0), c, K, D, L)
        assert (step < 1e-15).all()
        cov = ocr.covariance(rv, tv, c, K, D, L, mount, **prm)[0]
        ref_means.append(float(np.mean(ocr.mahalanobis(pr.observation(rv, tv, mount), np.repeat(z[None], 128, axis=0), cov))))
    conditions(ref_means, "reference")

    ctx = context(len(TABLE))
    ctx.set_camera_rig([(K, D, mount)])
    for s, c in enumerate(slots):
        inject(ctx, s, c)
    got, _ = run_checked(ctx, slots, prm)
    means, means_ref_R = [], []
    for (rec, s, (_, valid, xyth, _)), z in zip(got, truth):
        assert len(rec) == 128 and not rec["flags"].any() and valid.all()
        zz = np.repeat(z[None], 128, axis=0)
        means.append(float(np.mean(ocr.mahalanobis(xyth, zz, rec["cov"]))))
        means_ref_R.append(float(np.mean(ocr.mahalanobis(xyth, zz, rec["r_ref"]))))
    conditions(means, "k_pose_cov")
    print(f"with the reference's diagonal R: mean d^2 per geometry {[round(m, 4) for m in means_ref_R]}")
    assert np.mean(means_ref_R) < 0.1


# ---- 4: sizes -------------------------------------------------------------------------------------------------------------------------

def test_marker_counts_around_the_group_width(tol):
    """0, 1, 31, 32, 33 and 128 markers in the slots of one call (32 markers per pass of the workgroup), and a marker's record alone
    against the same marker at position 127: bit-identical"""
    counts = [0, 1, 31, 32, 33, 128]
    rng = np.random.RandomState(21)
    quads = [q[2] for q in tpk.distinct_quads(128, rng)]
    cam = (K900, tpk.D_DEFAULT, (0.0, 0.0, 0.0))
    ctx = context(len(counts))
    ctx.set_camera(K900, tpk.D_DEFAULT)
    for s, n in enumerate(counts):
        inject(ctx, s, quads[127:] if n == 1 else quads[:n], ids=[127] if n == 1 else None)
    got, _ = run_checked(ctx, counts, DEFAULTS)
    assert [int(g[1]["checked"]) for g in got] == counts
    full = got[counts.index(128)][0]
    check_covariance(ctx, counts.index(128), cam, DEFAULTS, full, tol)
    assert got[counts.index(1)][0][0].tobytes() == full[127].tobytes(), "a marker's record depends on its neighbours"
    assert got[counts.index(1)][2][3].tobytes() == got[counts.index(128)][2][3][127:].tobytes()
    for s, n in enumerate(counts):
        assert got[s][0].tobytes() == full[:n].tobytes() or n == 1


# ---- 5: camera sources and modes --------------------------------------------------------------------------------------------------------

def mode_quads(K, D, rng):
    return tpa.mode_quads(K, D, rng)[0]


def test_single_camera_both_hooks(tol):
    """the single camera through aslam_debug_run_pose and aslam_debug_run_pose_refined (flat frames: the refinement leaves every
    corner where it is, so both give the same records).  The refined hook wants every corner inside the 64 x 64 frame: a camera of
    that size"""
    rng = np.random.RandomState(6)
    K = np.array([[60.0, 0, 32], [0, 60, 32], [0, 0, 1]])
    quads = [geometry_corners(d, tilt, tx, K, tpk.D_DEFAULT, 0.05, rng) for d, tilt, tx in ((0.8, 0.3, 0.1), (1.5, 0.6, -0.3), (2.5, 0.3, 0.5))]
    assert all((q > 1).all() and (q < 62).all() for q in quads)
    cam = (K, tpk.D_DEFAULT, (0.0, 0.0, 0.0))
    ctx = context(1)
    ctx.set_camera(K, tpk.D_DEFAULT)
    ctx.set_detector_params(doCornerRefinement=1)
    ctx.stage_frames(np.full((1, 64, 64), 128, np.uint8), 0)
    inject(ctx, 0, quads)
    (plain, _, _), = run_checked(ctx, [quads], DEFAULTS)[0]
    (refined, _, _), = run_checked(ctx, [quads], DEFAULTS, refine=True)[0]
    check_covariance(ctx, 0, cam, DEFAULTS, refined, tol)
    assert plain.tobytes() == refined.tobytes()


def test_rig_of_four_with_mounts(tol):
    cams = tpk.rig_cameras(4)
    rng = np.random.RandomState(7)
    lists = [mode_quads(K, D, rng) for K, D, _ in cams]
    ctx = context(8, landmarks=32)
    ctx.set_camera_rig(cams)
    for s in range(8):
        inject(ctx, s, lists[s % 4], ids=np.arange(6) + 10 * (s % 4))
    got, _ = run_checked(ctx, list(range(8)), DEFAULTS)
    for s in range(8):
        check_covariance(ctx, s, cams[s % 4], DEFAULTS, got[s][0], tol)
    assert got[1][0].tobytes() == got[5][0].tobytes()
    # the merged step lists carry the new R
    ctx.stage_encoders([0.0] * 4 + [WL] * 4, [0.0] * 4 + [WR] * 4, [0.0] * 4 + [DT] * 4)
    ctx.run_staged_rig(0, 2, with_ekf=2)
    ctx.sync()
    assert sorted(ctx.get_landmark_ids().tolist()) == sorted(10 * c + i for c in range(4) for i in range(6))


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
        inject(ctx, s, mode_quads(cams[r][0], cams[r][1], rng))
    got, _ = run_checked(ctx, robots, DEFAULTS, robots=robots)
    for s, r in enumerate(robots):
        check_covariance(ctx, s, cams[r], DEFAULTS, got[s][0], tol)


def test_both_switches_together(tol):
    """k_pose -> k_pose_cov -> k_pose_alt.  Marker 0: far, tilted, noisy - the reference's gate drops it, so the ambiguity check alone
    flags it without rejecting (valid was 0 already); k_pose_cov revalidates it and k_pose_alt then judges and rejects it.  Marker 1: the
    same geometry noise-free, rejected by k_pose_alt either way - it stays rejected although k_pose_cov passed it.  Marker 2: near, passes
    both"""
    rng = np.random.RandomState(11)
    pattern = rng.normal(size=(4, 2))
    far = geometry_corners(2.5, 0.3, 0.2, K900, tpk.D_DEFAULT, 0.0, rng)
    quads = [(far + 1.2 * pattern).astype(np.float32), far, geometry_corners(0.8, 0.3, 0.2, K900, tpk.D_DEFAULT, 0.0, rng)]
    ctx = context(1)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    inject(ctx, 0, quads)
    ctx.set_pose_ambiguity(**tpa.AMBIGUOUS)
    ctx.run_pose(0, 1)
    alone = ctx.get_slot_pose_ambiguity(0)[0]["flags"].tolist()
    valid_alone = ctx.get_slot_raw_observations(0)[1].tolist()
    ctx.set_observation_covariance(**DEFAULTS)
    ctx.run_pose(0, 1)
    both = ctx.get_slot_pose_ambiguity(0)[0]["flags"].tolist()
    cov_rec, cov_sum = ctx.get_slot_obs_covariance(0)
    valid_both = ctx.get_slot_raw_observations(0)[1].tolist()
    ctx.set_pose_ambiguity(None)
    ctx.run_pose(0, 1)
    assert ctx.get_slot_raw_observations(0)[1].tolist() == [1, 1, 1]      # k_pose_cov alone passes all three
    assert ctx.get_slot_obs_covariance(0)[0].tobytes() == cov_rec.tobytes()
    assert alone == [1, 3, 0] and valid_alone == [0, 0, 1]
    assert both == [3, 3, 0] and valid_both == [0, 0, 1]
    assert not cov_rec["flags"].any() and (cov_sum["degenerate"], cov_sum["gated"]) == (0, 0)


# ---- 6: the new R reaches the filter and nothing else changes ---------------------------------------------------------------------------

def filter_lists(n_slots, rng):
    """slot 0 empty (it arms the filter), then the six mode markers with fresh corner noise per slot"""
    out = [[]]
    for _ in range(n_slots - 1):
        out.append([(np.asarray(q, np.float64) + 0.2 * rng.normal(size=(4, 2))).astype(np.float32)
                    for q in mode_quads(K900, tpk.D_DEFAULT, np.random.RandomState(6))])
    return out


def make_context(windows, n):
    kw = dict(max_rows=64, max_cols=64, max_batch=n, persistent_waves=4, max_landmarks=16)
    return capi.Context(**kw) if windows else no_windows_context(**kw)


def ab_filter(windows, localize, n=8):
    lists = filter_lists(n, np.random.RandomState(12))
    enc = ([0.0] + [WL] * (n - 1), [0.0] + [WR] * (n - 1), [0.0] + [DT] * (n - 1))
    out = []
    raw = None
    for on in (True, False):
        ctx = make_context(windows, n)
        ctx.set_camera(K900, tpk.D_DEFAULT)
        if localize:
            ctx.localize_begin(np.arange(6), [[2.0, 0.3 * k - 0.8, 3.0] for k in range(6)], [0.0, 0.0, 0.0], np.eye(3) * 1e-2)
        ctx.stage_encoders(*enc)
        if on:
            ctx.set_observation_covariance(**DEFAULTS)
            for s, q in enumerate(lists):
                inject(ctx, s, q)
            ctx.run_pose(0, n)
            raw = [ctx.get_slot_raw_observations(s) for s in range(n)]
            assert all((ctx.get_slot_obs_covariance(s)[0]["flags"] == 0).all() for s in range(n))
        else:
            for s, (ids, valid, xyth, Rd) in enumerate(raw):
                ctx.inject_observations(s, ids, valid, xyth, Rd)
        ctx.run_staged(0, n, with_ekf=2)
        ctx.sync()
        out.append((ctx.get_state(), ctx.get_landmark_ids(), ctx.plan_stats()))
    (sa, ia, pa), (sb, ib, pb) = out
    assert sa[0].size > 3 or localize
    if not localize:
        assert (pa["windows"] > 0) == (pb["windows"] > 0) == windows, f"the EKF windows were not as asked: {pa}, {pb}"
    assert same_bits(sa, sb) and np.array_equal(ia, ib), "the switch changed something besides the raw observations"
    # and the new R is what the filter consumed: with the reference's R the state differs
    ctx = make_context(windows, n)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    if localize:
        ctx.localize_begin(np.arange(6), [[2.0, 0.3 * k - 0.8, 3.0] for k in range(6)], [0.0, 0.0, 0.0], np.eye(3) * 1e-2)
    ctx.stage_encoders(*enc)
    for s, q in enumerate(lists):
        inject(ctx, s, q)
    ctx.run_pose(0, n)
    ctx.run_staged(0, n, with_ekf=2)
    ctx.sync()
    assert not same_bits(ctx.get_state(), sa)


@pytest.mark.parametrize("windows", [True, False])
def test_new_r_reaches_the_slam_filter(windows):
    """context A: switch on, pose stage on injected candidates for 8 slots, EKF steps; context B: switch off, A's raw observations
    injected, the same EKF steps.  mu, Sigma and the landmark ids bit for bit, with EKF windows on and off"""
    ab_filter(windows, False)


def test_new_r_reaches_the_localization_filter():
    ab_filter(True, True)


# ---- 7: refusals and persistence ----------------------------------------------------------------------------------------------------------

def test_refusals():
    ctx = context(2)
    ctx.set_camera(K900, tpk.D_DEFAULT)
    on, p = capi.C.c_int(7), capi.ObsCovarianceParams()
    assert ctx.lib.aslam_get_observation_covariance(ctx.h, capi.C.byref(on), capi.C.byref(p)) == 0 and on.value == 0
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS           # the defaults while the switch is off
    assert ctx.get_observation_covariance() is None
    with pytest.raises(capi.AslamError) as e:
        ctx.get_slot_obs_covariance(0)
    assert e.value.code == E_STATE
    want = dict(sigma_px=0.25, scale=2.0, floor_xy=0.0, floor_th=1e-4, gate_norm=math.inf, use_residual=0)
    ctx.set_observation_covariance(**want)
    assert ctx.get_observation_covariance() == want
    bad_values = dict(sigma_px=(0.0, -1.0, math.inf, math.nan), scale=(0.0, -1.0, math.inf, math.nan),
                      floor_xy=(-1e-12, math.inf, math.nan), floor_th=(-1e-12, math.inf, math.nan), gate_norm=(0.0, -1.0, -math.inf, math.nan),
                      use_residual=(2, -1))
    for k, vals in bad_values.items():
        for v in vals:
            with pytest.raises(capi.AslamError) as e:
                ctx.set_observation_covariance(**{k: v})
            assert e.value.code == E_INVALID, (k, v)
            assert ctx.get_observation_covariance() == want           # a refused call changes nothing
    for slot in (-1, 2):
        with pytest.raises(capi.AslamError) as e:
            ctx.get_slot_obs_covariance(slot)
        assert e.value.code == E_INVALID
    n = capi.C.c_int()
    assert ctx.lib.aslam_get_slot_obs_covariance(ctx.h, 0, -1, capi.C.byref(n), None, None) == E_INVALID
    assert ctx.lib.aslam_get_slot_obs_covariance(ctx.h, 0, 4, capi.C.byref(n), None, None) == E_INVALID
    assert ctx.lib.aslam_get_slot_obs_covariance(ctx.h, 0, 0, None, None, None) == E_INVALID
    assert ctx.lib.aslam_set_observation_covariance(None, None) == E_INVALID
    assert ctx.lib.aslam_get_observation_covariance(None, capi.C.byref(on), None) == E_INVALID
    assert ctx.lib.aslam_get_slot_obs_covariance(None, 0, 0, capi.C.byref(n), None, None) == E_INVALID
    rec, s = ctx.get_slot_obs_covariance(1)                         # never processed: empty
    assert len(rec) == 0 and s["checked"] == 0
    ctx.set_observation_covariance(None)
    assert ctx.get_observation_covariance() is None
    with pytest.raises(capi.AslamError) as e:
        ctx.get_slot_obs_covariance(0)
    assert e.value.code == E_STATE
    ctx.set_observation_covariance()
    assert ctx.get_observation_covariance() == DEFAULTS


def test_switch_off_is_bit_identical(tol):
    """a context that never heard of the switch, one that had it set, used and cleared again: every output the same bits, and no
    k_pose_cov launch in the first"""
    def run(ctx):
        inject(ctx, 0, [])
        inject(ctx, 1, mode_quads(K900, tpk.D_DEFAULT, np.random.RandomState(6)))
        ctx.run_pose(0, 2)
        ctx.run_staged(0, 2, with_ekf=2)
        ctx.sync()

    ctxs = []
    for _ in range(2):
        ctx = context(2)
        ctx.set_camera(K900, tpk.D_DEFAULT)
        ctx.stage_encoders([0.0, WL], [0.0, WR], [0.0, DT])
        ctxs.append(ctx)
    a, b = ctxs
    run(a)
    b.set_observation_covariance(**DEFAULTS)
    inject(b, 0, [])
    inject(b, 1, mode_quads(K900, tpk.D_DEFAULT, np.random.RandomState(6)))
    b.run_pose(0, 2)
    assert not same_bits(snapshot(a, 1), snapshot(b, 1))
    b.set_observation_covariance(None)
    assert b.get_observation_covariance() is None
    run(b)
    assert same_bits(snapshot(a, 1), snapshot(b, 1))
    assert same_bits(a.get_state(), b.get_state()) and np.array_equal(a.get_landmark_ids(), b.get_landmark_ids())
    assert "k_pose_cov" in a.profile_get() and a.profile_get()["k_pose_cov"][0] == 0


# ---- 8: one rendered scene ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rendered_ring_feeds_the_filter_the_new_r():
    """320 x 240, 6 markers in view, 8 frames of the synthetic ring: the switch-on SLAM state equals a switch-off context fed the
    switch-on context's raw observations, bit for bit, and no marker is degenerate"""
    cfg = synth.SceneConfig(rows=240, cols=320, f=225.0, grid=(3, 2), n_panels=4, kind="ring")
    w = synth.RingWorld(cfg)
    n = 8
    frames = [w.frame(i) for i in range(n)]
    a = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=n, max_landmarks=32)
    a.set_camera(w.K, np.zeros(5))
    a.set_observation_covariance(**DEFAULTS)
    for i, f in enumerate(frames):
        a.synth_render(i, cfg.rows, cfg.cols, w.K, f.ids, f.poses, noise_amp=2, seed=i, download=False)
    enc = ([f.wl for f in frames], [f.wr for f in frames], [f.dt for f in frames])
    a.stage_encoders(*enc)
    a.run_staged(0, n, with_ekf=True)
    a.sync()
    seen = 0
    b = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=n, max_landmarks=32)
    b.set_camera(w.K, np.zeros(5))
    b.stage_encoders(*enc)
    for i in range(n):
        rec, s = a.get_slot_obs_covariance(i)
        ids, valid, xyth, Rd = a.get_slot_raw_observations(i)
        assert len(rec) == len(ids) and s["degenerate"] == 0 and not (rec["flags"] & 1).any()
        assert not np.array_equal(Rd, rec["r_ref"]) or len(ids) == 0
        seen += len(ids)
        b.inject_observations(i, ids, valid, xyth, Rd)
    assert seen >= 4 * (n - 1), f"only {seen} markers detected over {n} frames"
    b.run_staged(0, n, with_ekf=2)
    b.sync()
    assert a.get_state()[0].size > 3
    assert same_bits(a.get_state(), b.get_state()) and np.array_equal(a.get_landmark_ids(), b.get_landmark_ids())
