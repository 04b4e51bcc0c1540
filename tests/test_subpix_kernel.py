"""Corner refinement (corner_sub_pix_one in pose.hip, run by k_pose when doCornerRefinement is set) on injected quads, against the
oracle bit for bit and against the long-double restatement in tests/subpix_reference.py.

aslam_debug_inject_candidates writes a slot's candidates and aslam_debug_run_pose_refined launches what a detection call launches
after identification, with the detection call's own RefineCfg, over the frames staged in the slots.  The frames are closed-form
blurred corners, saddles, edges and squares (subpix_reference.py), at most 64 x 80 pixels.

One step against long double (cornerRefinementMaxIterations = 1; windows 1, 2, 3, 5, 7; 400 cases per window: 50 frames, L-corners
and saddles in turn, 8 starts each within 1 px of the apex (0.5 px for window 1), every other start on integer coordinates, where the
horizontal fraction is 0 and the 0.0001 clamp acts).  A case is compared when the reference step stays 0.25 px inside the window and
1 px inside the image and det >= 0.02 a c (away from the det, leave-the-image and reset decisions); the others still go through the
bit-exact comparison with the oracle.  Excluded per window: 0 %, 0 %, 0 %, 0 %, 0 % (the cap is 5 %).  The deviation is counted in
float32 spacings at the coordinate; in pixels it is about 2e-6 everywhere (the float32 patch samples), so the small coordinates of
window 1 (apexes from 6 px) count most spacings.  Worst deviation from the long-double step, windows 1 / 2 / 3 / 5 / 7:
  oracle (orc.corner_sub_pix, max_iter = 1):  1.82 / 1.06 / 0.70 / 0.68 / 0.68 spacings (2.7e-6 / 2.2e-6 / 2.0e-6 / 2.0e-6 / 2.0e-6 px)
  emulation build:                            1.82 / 1.06 / 0.70 / 0.68 / 0.68 spacings (equal to the oracle bit for bit)
  MI355X:                                     1.82 / 1.06 / 0.70 / 0.68 / 0.68 spacings (equal to the oracle bit for bit)
The bound is 4 x the oracle's worst of the window and never less than one spacing: 7.3 / 4.3 / 2.8 / 2.8 / 2.8 spacings
(ONE_STEP_BOUND).

Whole trajectories, borders, degenerate windows, lists, frames and cameras are compared with orc.corner_sub_pix on the same frame and
start, bit for bit; the reference driver (subpix_reference.iterate) says which stopping rule and which sampling path each case
reaches, and the tests assert that the intended ones are reached.
On the MI355X the module takes 3.1 s: the two multi-slot tests (a fresh process each) 0.7 s each, every other test below 0.3 s.
Runs on whichever library the session loads: the emulation here, the gfx950 build on the MI355X."""
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import subpix_reference as sr
import test_pose_kernel as tpk
from aruco_slam_amd import capi, synth
from oracle import pyoracle as orc

E_INVALID, E_STATE = -1, -5
L = tpk.L
# orc.corner_sub_pix(max_iter = 1) against the long-double step per window, in float32 spacings, measured (the module docstring); the
# kernel is allowed 4 x that and never less than one spacing
ONE_STEP_ORACLE_WORST = {1: 1.83, 2: 1.07, 3: 0.71, 5: 0.69, 7: 0.69}
ONE_STEP_BOUND = {w: max(1.0, 4 * v) for w, v in ONE_STEP_ORACLE_WORST.items()}
WORST = {}


def note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nsubpix worst cases: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


@pytest.fixture(autouse=True)
def oracle_defaults():
    yield
    orc.set_detector_params()


def camera_for(rows, cols):
    return np.array([[100.0, 0, cols / 2], [0, 100.0, rows / 2], [0, 0, 1]])


def context(rows, cols, batch=1, camera=True):
    ctx = capi.Context(max_rows=rows, max_cols=cols, max_batch=batch, persistent_waves=4, max_landmarks=16)
    if camera:
        ctx.set_camera(camera_for(rows, cols), np.zeros(5))
    return ctx


def refine_on(ctx, win, iters, acc):
    ctx.set_detector_params(doCornerRefinement=1, cornerRefinementWinSize=win, cornerRefinementMaxIterations=iters, cornerRefinementMinAccuracy=acc)


def refine_points(ctx, slot, pts, robots=None):
    """cornerSubPix through k_pose on a list of points of the frame staged in `slot`: four to a marker, in candidate order (the last
    marker padded with its first point), every marker with its own id"""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    m = (n + 3) // 4
    assert 1 <= m <= 128
    padded = np.concatenate([pts, np.repeat(pts[:1], 4 * m - n, axis=0)])
    ctx.inject_candidates(slot, np.arange(m), np.zeros(m), padded.reshape(m, 8))
    ctx.run_pose(slot, 1, robots, refine=True)
    ids, corners, _, _ = ctx.get_slot_detections(slot)
    assert ids.tolist() == list(range(m))
    assert np.isfinite(corners).all()
    return corners.reshape(-1, 2)[:n]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_against_oracle(ctx, img, pts, win, iters, acc, slot=0, stage=True):
    """stage img, refine pts with (win, iters, acc) through the hook: equal to orc.corner_sub_pix bit for bit; returns the result"""
    if stage:
        ctx.stage_frames(img, slot)
    refine_on(ctx, win, iters, acc)
    got = refine_points(ctx, slot, pts)
    want = orc.corner_sub_pix(img, pts, win, iters, acc)
    bad = np.nonzero(~(got.view(np.uint32) == want.view(np.uint32)).all(axis=1))[0]
    assert len(bad) == 0, f"win {win} iters {iters} acc {acc}: point {pts[bad[0]]} -> {got[bad[0]]}, oracle {want[bad[0]]} ({len(bad)} differ)"
    return got


# ---- one step against long double --------------------------------------------------------------------------------------------------

ONE_ROWS, ONE_COLS, ONE_CASES, PER_FRAME = 64, 64, 400, 8
WINDOWS = (1, 2, 3, 5, 7)
_ONE = {}


def one_step_cases(win):
    """ONE_CASES // PER_FRAME frames (L-corners and saddles in turn, random apex and angle), PER_FRAME starts each within 1 px (half
    a pixel for window 1) of the apex, alternately rounded to integers; per case the reference step or None when it is excluded"""
    if win in _ONE:
        return _ONE[win]
    rng = np.random.RandomState(100 + win)
    frames, starts, ref = [], [], []
    reach = 0.5 if win == 1 else 1.0
    for f in range(ONE_CASES // PER_FRAME):
        x0, y0 = rng.uniform(6, ONE_COLS - 6), rng.uniform(6, ONE_ROWS - 6)
        ang = rng.uniform(0, 2 * math.pi)
        img = (sr.corner_l if f % 2 == 0 else sr.corner_x)(ONE_ROWS, ONE_COLS, x0, y0, ang, sigma=rng.uniform(0.7, 1.3))
        p = np.array([x0, y0]) + rng.uniform(-reach, reach, (PER_FRAME, 2))
        p[::2] = np.rint(p[::2])
        p = p.astype(np.float32)
        r = []
        for x, y in p:
            nx, ny, det, ac, _ = sr.step(img, x, y, win)
            ok = (nx is not None and det >= 0.02 * ac and max(abs(nx - x), abs(ny - y)) <= win - 0.25
                  and 1 <= nx <= ONE_COLS - 2 and 1 <= ny <= ONE_ROWS - 2)
            r.append((nx, ny) if ok else None)
        frames.append(img); starts.append(p); ref.append(r)
    _ONE[win] = (frames, starts, ref)
    return _ONE[win]


def one_step_deviation(win, refine):
    """worst |refine(frame, starts) - reference step| over the compared cases of this window, in float32 spacings and in pixels, and
    the share of excluded cases"""
    frames, starts, ref = one_step_cases(win)
    worst, worst_px, excluded, clamp = 0.0, 0.0, 0, 0
    for img, p, r in zip(frames, starts, ref):
        got = refine(img, p)
        for g, q, s in zip(got, r, p):
            if q is None:
                excluded += 1
                continue
            clamp += int(s[0] == np.floor(s[0]))
            for k in range(2):
                d = abs(sr.LD(g[k]) - q[k])
                worst_px = max(worst_px, float(d))
                worst = max(worst, float(d / sr.LD(np.spacing(np.float32(q[k])))))
    assert clamp >= ONE_CASES // 4, "too few compared cases start on an integer column"
    return worst, worst_px, excluded / ONE_CASES


@pytest.mark.parametrize("win", WINDOWS)
def test_one_step_oracle_against_long_double(win):
    """orc.corner_sub_pix(max_iter = 1) against the long-double step: the first check of the oracle's arithmetic that does not share
    its expressions.  Also the measurement behind ONE_STEP_BOUND, and the cap on excluded cases"""
    worst, px, excluded = one_step_deviation(win, lambda img, p: orc.corner_sub_pix(img, p, win, 1, 0.1))
    print(f"\nwin {win}: oracle vs long double {worst:.3g} spacings ({px:.3g} px), excluded {100 * excluded:.1f} %")
    note("oracle one step (spacings)", worst)
    assert excluded <= 0.05
    assert worst <= ONE_STEP_ORACLE_WORST[win], "the recorded oracle deviation (and the bound derived from it) is out of date"


@pytest.mark.parametrize("win", WINDOWS)
def test_one_step_against_long_double(win):
    """the kernel's single iteration within ONE_STEP_BOUND spacings of the long-double step, for every window size (a mask read with
    another window's pitch, a wrong patch origin or a dropped clamp moves the point by far more); every case, excluded or not, equal to
    the oracle bit for bit"""
    ctx = context(ONE_ROWS, ONE_COLS)

    def refine(img, p):
        return check_against_oracle(ctx, img, p, win, 1, 0.1)

    worst, px, excluded = one_step_deviation(win, refine)
    print(f"\nwin {win}: kernel vs long double {worst:.3g} spacings ({px:.3g} px), excluded {100 * excluded:.1f} %")
    note("kernel one step (spacings)", worst)
    assert excluded <= 0.05
    assert worst <= ONE_STEP_BOUND[win], f"win {win}: {worst:.3g} float spacings ({px:.3g} px) from the long-double step"


# ---- whole trajectories ------------------------------------------------------------------------------------------------------------

TRAJ_WIN = 3
# a strong edge crossed by a weak one: from these starts the iteration settles into a two-cycle along the strong edge, some 3 px long,
# and is still hopping at iteration 100
CYCLE_IMAGE = dict(x0=30.29, y0=33.11, angle=0.892, sigma=2.42, weak=13.7)
CYCLE_STARTS = [(30.01, 33.05), (29.42, 33.70), (29.28, 34.78), (28.84, 34.15)]


def trajectory_frames():
    rng = np.random.RandomState(5)
    out = []
    for f, make in enumerate((sr.corner_l, sr.corner_x, sr.corner_l)):
        x0, y0 = rng.uniform(16, 48, 2)
        img = make(64, 64, x0, y0, rng.uniform(0, 2 * math.pi), sigma=1.0 + 0.5 * f)
        out.append((img, (np.array([x0, y0]) + rng.uniform(-2, 2, (12, 2))).astype(np.float32)))
    out.append((sr.weak_cross(64, 64, **CYCLE_IMAGE), np.array(CYCLE_STARTS, np.float32)))
    return out


def test_trajectories_match_oracle():
    """iteration counts 1, 2, 3, 30, 99, 100 and 1000 (clamped to 100) x accuracies 10 (one iteration), 0.1 and 1e-6, bit for bit.
    The reference driver shows that the cases hold points stopped by the cap and by the accuracy, a point where 2 and 3 iterations
    differ, and a point where 100 and 1000 agree and 99 does not (an unclamped count, an unsquared accuracy or a count off by one
    changes one of them)"""
    ctx = context(64, 64)
    frames = trajectory_frames()
    seen = dict(cap=0, eps=0, eps_mid=0)
    for img, pts in frames:
        ctx.stage_frames(img, 0)
        got = {}
        for iters in (1, 2, 3, 30, 99, 100, 1000):
            for acc in (10.0, 0.1, 1e-6):
                got[iters, acc] = check_against_oracle(ctx, img, pts, TRAJ_WIN, iters, acc, stage=False)
        assert same_bits(got[30, 10.0], got[1, 10.0])                 # accuracy 10: one iteration whatever the count
        assert same_bits(got[1000, 1e-6], got[100, 1e-6])
        for i, (x, y) in enumerate(pts):
            d = sr.iterate(img, x, y, TRAJ_WIN, 30, 0.1)
            if d["err_margin"] > 0.05 and not d["reset"]:
                seen[d["end"]] = seen.get(d["end"], 0) + 1
                # the same point with the accuracy unsquared (0.1 instead of 0.01 as the bound on err) stops earlier and elsewhere
                u = sr.iterate(img, x, y, TRAJ_WIN, 30, math.sqrt(0.1))
                if d["end"] == "eps" and u["iters"] < d["iters"] and (u["x"], u["y"]) != (d["x"], d["y"]):
                    seen["eps_mid"] += 1
            d2, d3 = sr.iterate(img, x, y, TRAJ_WIN, 2, 1e-6), sr.iterate(img, x, y, TRAJ_WIN, 3, 1e-6)
            if d2["end"] == "cap" and d3["iters"] == 3 and not d3["reset"] and max(abs(d2["x"] - d3["x"]), abs(d2["y"] - d3["y"])) > 1e-3:
                seen["2 != 3"] = seen.get("2 != 3", 0) + 1
                assert not same_bits(got[2, 1e-6][i], got[3, 1e-6][i])
    assert seen["eps"] >= 5 and seen["eps_mid"] >= 1 and seen.get("2 != 3", 0) >= 5, seen
    # the two-cycle: stopped by the cap at 100, a different point after 99
    img, pts = frames[-1]
    hopping = 0
    for i, (x, y) in enumerate(pts):
        d99, d100 = sr.iterate(img, x, y, TRAJ_WIN, 99, 1e-6), sr.iterate(img, x, y, TRAJ_WIN, 1000, 1e-6)
        if d100["end"] == "cap" and d100["iters"] == 100 and max(abs(d99["x"] - d100["x"]), abs(d99["y"] - d100["y"])) > 0.5:
            hopping += 1
            assert not same_bits(got[99, 1e-6][i], got[100, 1e-6][i])
            if not d100["reset"]:
                assert abs(got[100, 1e-6][i][0] - d100["x"]) < 1e-2 and abs(got[100, 1e-6][i][1] - d100["y"]) < 1e-2
    assert hopping >= 2
    seen["cap"] += hopping
    assert seen["cap"] >= 2, seen


# ---- borders -----------------------------------------------------------------------------------------------------------------------

B_ROWS, B_COLS, B_WIN = 48, 80, 2                                 # patch width 7: ipx = floor(x - 3)
BORDER_APEXES = dict(left=(2.6, 20.4), right=(77.3, 25.7), top=(40.2, 2.3), bottom=(33.3, 45.6), top_left=(2.4, 2.7), top_right=(77.5, 2.2),
                     bottom_left=(2.3, 45.4), bottom_right=(77.6, 45.7))


@pytest.fixture(scope="module")
def border_ctx():
    return context(B_ROWS, B_COLS)


@pytest.mark.parametrize("where", list(BORDER_APEXES))
def test_borders(where, border_ctx):
    """saddles within win + 2 of each side and each corner of a 48 x 80 frame, starts around them: the clipped sampling path with the
    replication on that side (rows and cols swapped in the clamp reads other pixels on this frame)"""
    x0, y0 = BORDER_APEXES[where]
    assert min(x0, B_COLS - 1 - x0, y0, B_ROWS - 1 - y0) <= B_WIN + 2
    img = sr.corner_x(B_ROWS, B_COLS, x0, y0, 0.3, sigma=1.0)
    g = np.array([-1.5, -0.75, 0.0, 0.6, 1.4])
    pts = np.array([[x0 + dx, y0 + dy] for dx in g for dy in g])
    pts = np.clip(pts, 0, [B_COLS - 0.01, B_ROWS - 0.01]).astype(np.float32)
    got = check_against_oracle(border_ctx, img, pts, B_WIN, 30, 0.01)
    paths = [sr.iterate(img, x, y, B_WIN, 30, 0.01) for x, y in pts]
    assert sum(1 for d in paths if not any(d["inside"])) >= 10       # clipped from the first step to the last
    moved = sum(1 for p, q in zip(pts, got) if not same_bits(p, q))
    assert moved >= 10


def test_interior_clipped_switch(border_ctx):
    """starts that put ipx + pw at cols - 1 and at cols, ipx at 0 and at -1, the same in y (one iteration, so that the first patch is
    the one compared), and one trajectory that begins on the interior path and ends on the clipped one"""
    pw = 2 * B_WIN + 3
    off = (pw - 1) / 2
    # x: ipx + pw = cols - 1 for x in [cols - 1 - pw + off, +1), = cols one pixel on
    xr, yb = B_COLS - 1 - pw + off, B_ROWS - 1 - pw + off
    for apex, starts, want in (
            ((77.3, 25.7), [(xr, 25.0), (xr + 0.5, 25.5), (xr + 0.999, 25.2), (xr + 1.0, 25.0), (xr + 1.5, 25.4)], [True, True, True, False, False]),
            ((2.6, 20.4), [(off, 20.0), (off + 0.5, 20.5), (off - 0.001, 20.2), (off - 1.0, 20.0), (off - 0.5, 20.6)], [True, True, False, False, False]),
            ((33.3, 45.6), [(33.0, yb), (33.5, yb + 0.5), (33.2, yb + 0.999), (33.0, yb + 1.0), (33.4, yb + 1.5)], [True, True, True, False, False]),
            ((40.2, 2.3), [(40.0, off), (40.5, off + 0.5), (40.2, off - 0.001), (40.0, off - 1.0), (40.6, off - 0.5)], [True, True, False, False, False])):
        img = sr.corner_x(B_ROWS, B_COLS, apex[0], apex[1], 0.3, sigma=1.0)
        pts = np.array(starts, np.float32)
        assert [sr.patch(img, x, y, B_WIN)[1] for x, y in pts] == want
        got = check_against_oracle(border_ctx, img, pts, B_WIN, 1, 0.01)
        assert sum(1 for p, q in zip(pts, got) if not same_bits(p, q)) >= 4
    # interior first, clipped at the end: a saddle right of the switch, a start left of it
    img = sr.corner_x(B_ROWS, B_COLS, 76.7, 25.7, 0.3, sigma=1.0)
    pts = np.array([(75.6, 25.2), (75.2, 26.3), (75.9, 25.9)], np.float32)
    crossing = 0
    for x, y in pts:
        d = sr.iterate(img, x, y, B_WIN, 30, 1e-3)
        crossing += int(d["inside"][0] and not d["inside"][-1] and not d["reset"] and len(d["inside"]) >= 2)
    assert crossing >= 2
    check_against_oracle(border_ctx, img, pts, B_WIN, 30, 1e-3)


# ---- degenerate windows ------------------------------------------------------------------------------------------------------------

def test_flat_frame_and_exact_edge_leave_the_point_alone():
    """det == 0 exactly (a flat frame; an unblurred vertical edge, whose gy is 0 everywhere): the point comes back unchanged to the bit"""
    ctx = context(64, 64)
    pts = np.array([(20.0, 30.0), (31.4, 32.7), (33.25, 10.5), (2.2, 2.9), (62.1, 61.3), (0.0, 0.0), (63.9, 63.9), (32.0, 31.5)], np.float32)
    step_edge = np.ascontiguousarray(np.broadcast_to(np.where(np.arange(64) < 32, 40, 210).astype(np.uint8), (64, 64)))
    for img in (sr.flat(64, 64), sr.flat(64, 64, 0), sr.flat(64, 64, 255), step_edge):
        for x, y in pts:
            d = sr.iterate(img, x, y, 3, 30, 0.1)
            assert d["end"] == "det" and d["iters"] == 0
        got = check_against_oracle(ctx, img, pts, 3, 30, 0.1)
        assert same_bits(got, pts)


def test_straight_edge_and_leaving_the_image():
    """a blurred straight edge (rank-one gradients up to the uint8 rounding: the step is large and erratic) and starts whose first
    step leaves the image: equal to the oracle, finite, and the starts that leave come back unchanged"""
    ctx = context(64, 64)
    rng = np.random.RandomState(9)
    img = sr.edge(64, 64, 50.3, 30.2, 0.4, sigma=1.5)
    pts = np.array([(50.3, 30.2)]) + np.stack([rng.uniform(-3, 3, 60) * -math.sin(0.4), rng.uniform(-3, 3, 60) * math.cos(0.4)], -1) * 6 + rng.uniform(-1, 1, (60, 2))
    pts = np.clip(pts, 0, 63.9).astype(np.float32)
    ends = [sr.iterate(img, x, y, 2, 1, 0.1) for x, y in pts]
    leaving = [i for i, d in enumerate(ends) if d["end"] == "left"]
    assert len(leaving) >= 3, "no start of this set leaves the image in its first step"
    got = check_against_oracle(ctx, img, pts, 2, 1, 0.1)
    for i in leaving:
        assert ends[i]["reset"] and same_bits(got[i], pts[i])
    check_against_oracle(ctx, img, pts, 2, 30, 0.01, stage=False)


def test_reset_rule_at_its_threshold():
    """the final point exactly win from the start (kept: the rule is 'more than win'), a little nearer and a little farther.  A saddle's
    fixed point F is found first; starts at F.x - win, a few float spacings to either side, and one pixel row off, converge to it"""
    win = 3
    ctx = context(64, 64)
    img = sr.corner_x(64, 64, 40.37, 30.61, 0.25, sigma=1.2)
    F = orc.corner_sub_pix(img, [(40.0, 30.5)], win, 100, 1e-6)[0]
    d = sr.iterate(img, 40.0, 30.5, win, 100, 1e-6)
    assert d["end"] == "eps" and abs(d["x"] - F[0]) < 1e-4 and abs(d["y"] - F[1]) < 1e-4
    u = float(np.spacing(np.float32(F[0] - win)))
    pts = np.array([(F[0] - win + k * u, F[1] + dy) for dy in (0.0, 0.31, -0.42, 0.77) for k in (-40, -2, -1, 0, 1, 2, 40)], np.float32)
    ctx.stage_frames(img, 0)
    got = check_against_oracle(ctx, img, pts, win, 100, 1e-6)
    shift = np.abs(got[:, 0].astype(np.float64) - pts[:, 0])
    kept = np.array([not same_bits(g, p) for g, p in zip(got, pts)])
    at = kept & (shift == win)
    assert at.sum() >= 1, "no start ends exactly win from where it began"
    assert (kept & (shift < win)).sum() >= 1 and (~kept).sum() >= 1
    for (x, y), k in zip(pts, kept):
        r = sr.iterate(img, x, y, win, 100, 1e-6)
        if abs(float(r["shift"]) - win) > 1e-4:                       # the driver agrees wherever its own rounding cannot decide
            assert r["reset"] == (not k)


# ---- lanes and lists ---------------------------------------------------------------------------------------------------------------

L_ROWS, L_COLS, PITCH = 64, 80, 3
BLOCK_COLS = (L_COLS // PITCH) // 2                              # markers are 2 x 2 blocks of tiles


def block_quad(centres, m, jitter):
    br, bc = divmod(m, BLOCK_COLS)
    t = [(2 * br, 2 * bc), (2 * br, 2 * bc + 1), (2 * br + 1, 2 * bc + 1), (2 * br + 1, 2 * bc)]
    return np.array([centres[r, c] for r, c in t]) + jitter


def around_quad(centres, m, jitter):
    br, bc = divmod(m, BLOCK_COLS)
    t = [(2 * br - 1, 2 * bc - 1), (2 * br - 1, 2 * bc + 2), (2 * br + 2, 2 * bc + 2), (2 * br + 2, 2 * bc - 1)]
    return np.array([centres[r, c] for r, c in t]) + jitter


def run_list(ctx, img, sl, win=1, iters=1, acc=0.1):
    """inject a tpk.Slot's candidates, run the refining hook: ids and order as the oracle's filter leaves them, corner j of marker k the
    oracle's refinement of rotated corner j of its candidate, bit for bit"""
    ctx.stage_frames(img, 0)
    refine_on(ctx, win, iters, acc)
    ctx.inject_candidates(0, sl.ids, sl.rots, np.array(sl.corners, np.float32).reshape(-1, 8))
    ctx.run_pose(0, 1, refine=True)
    exp = sl.expected()
    ids, corners, _, _ = ctx.get_slot_detections(0)
    assert ids.tolist() == [sl.ids[i] for i in exp]
    rotated = np.array([np.roll(sl.corners[i], sl.rots[i], axis=0) for i in exp], np.float32)
    want = orc.corner_sub_pix(img, rotated.reshape(-1, 2), win, iters, acc).reshape(-1, 4, 2)
    assert np.isfinite(corners).all()
    assert len(np.unique(want.reshape(-1, 2), axis=0)) == 4 * len(exp), "two lanes share a result: the case cannot tell them apart"
    still = (want.view(np.uint32) == rotated.view(np.uint32)).all(axis=2).mean()
    assert still <= 0.2, f"the refinement leaves {100 * still:.0f} % of the corners where they were"
    bad = np.nonzero(~(corners.view(np.uint32) == want.view(np.uint32)).all(axis=(1, 2)))[0]
    assert len(bad) == 0, f"markers {bad.tolist()} of {len(exp)} differ from the oracle's refinement"
    return exp


@pytest.fixture(scope="module")
def tiles():
    return sr.tiled_saddles(L_ROWS, L_COLS, PITCH, np.random.RandomState(2))


def test_lanes_128_markers(tiles):
    """128 markers = 512 corners, each on its own saddle: four passes of the 128-lane loop, rotations 0..3, rejected candidates between"""
    img, centres = tiles
    rng = np.random.RandomState(3)
    sl = tpk.Slot(None)
    for m in range(128):
        if m % 3 == 1:
            sl.add(-1, rng.uniform(1, 60, (4, 2)))
        sl.add(900 - m, block_quad(centres, m, (0.3, -0.2)), rot=m % 4)
    assert len(run_list(context(L_ROWS, L_COLS), img, sl)) == 128


def test_lanes_33_markers_filtered(tiles):
    """33 kept markers (132 corners: a second pass of 4 lanes) out of 36 identified: three same-id quads nested in a later, larger one
    are removed, so that the output order is not the candidate order from the sixth marker on; rejected candidates between"""
    img, centres = tiles
    rng = np.random.RandomState(4)
    sl = tpk.Slot(None)
    nested = {5: 15, 17: 17, 29: 31}                             # list position -> block (off the frame's edge) of a removed inner quad
    for k in range(33):
        m = nested.get(k, 40 + k)
        sl.add(100 + m, block_quad(centres, m, (0.3, -0.2)), rot=k % 4)
        if k % 4 == 2:
            sl.add(-1, rng.uniform(1, 60, (4, 2)))
    for m in nested.values():
        sl.add(100 + m, around_quad(centres, m, (-0.25, 0.35)), rot=m % 4)
    exp = run_list(context(L_ROWS, L_COLS), img, sl)
    assert len(exp) == 33
    removed = [i for i, mid in enumerate(sl.ids) if mid >= 0 and i not in exp]
    assert len(removed) == 3 and min(removed) < 8                 # the compaction skips an entry ahead of 28 kept markers


# ---- frames ------------------------------------------------------------------------------------------------------------------------

def frames_case(kind):
    """one call over slots 3..7 of an 8-slot context, a different frame in each: gray slots as staged, bgr8 slots (distinct channels)
    as the detection pass before converted them"""
    rng = np.random.RandomState(12)
    ctx = context(B_ROWS, B_COLS, batch=8)
    grays, pts = [], []
    for s in range(5):
        img, centres = sr.tiled_saddles(B_ROWS, B_COLS, 8, np.random.RandomState(50 + s), sigma=1.0)
        grays.append(img)
        pts.append((centres.reshape(-1, 2)[rng.choice(60, 24, replace=False)] + rng.uniform(-1, 1, (24, 2))).astype(np.float32))
    if kind == "bgr8":
        frames = np.stack([np.stack([g, np.roll(g, 16, axis=1), 255 - g], -1) for g in grays])
        ctx.stage_frames(frames, 3)
        ctx.run_staged(3, 5, with_ekf=False)
        ctx.sync()
        grays = [orc.bgr2gray(f) for f in frames]
        assert not any(np.array_equal(g, f[..., 0]) for g, f in zip(grays, frames))
    else:
        ctx.stage_frames(np.stack(grays), 3)
    refine_on(ctx, 2, 30, 0.01)
    for s in range(5):
        ctx.inject_candidates(3 + s, np.arange(6), np.arange(6) % 4, pts[s].reshape(6, 8))
    ctx.run_pose(3, 5, refine=True)
    for s in range(5):
        ids, corners, _, _ = ctx.get_slot_detections(3 + s)
        assert ids.tolist() == list(range(6))
        rotated = np.array([np.roll(q, r, axis=0) for q, r in zip(pts[s].reshape(6, 4, 2), np.arange(6) % 4)], np.float32)
        want = orc.corner_sub_pix(grays[s], rotated.reshape(-1, 2), 2, 30, 0.01).reshape(6, 4, 2)
        assert same_bits(corners, want), f"{kind} slot {3 + s}: refined corners differ from the oracle's on this slot's frame"
        others = [orc.corner_sub_pix(grays[o], rotated.reshape(-1, 2), 2, 30, 0.01).reshape(6, 4, 2) for o in range(5) if o != s]
        assert not any(same_bits(want, o) for o in others)
    return True


@pytest.mark.parametrize("chunk", ["2", "8"])
def test_frames_of_a_multi_slot_call(chunk):
    """slots 3..7 in sub-batches of 2 (k_pose launches at slots 3, 5 and 7) and in one launch (a chunk larger than the call).  The
    chunk size is read once per process, so a fresh process runs the case"""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        import test_subpix_kernel as m
        assert m.frames_case("gray") and m.frames_case("bgr8")
        print("frames ok")
    """) % os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ASLAM_DETECT_CHUNK=chunk, PYTHONPATH=os.pathsep.join(sys.path))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "frames ok" in r.stdout, r.stdout + r.stderr


# ---- cameras -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tol(on_emulation):
    return tpk.EMU_TOL if on_emulation else tpk.GPU_TOL


def camera_cases():
    Ks = [np.array([[100.0, 0, 40], [0, 100, 24], [0, 0, 1]]), np.array([[92.0, 0, 38.5], [0, 93.0, 25], [0, 0, 1]]),
          np.array([[110.0, 0, 41], [0, 109.0, 23], [0, 0, 1]])]
    Ds = [np.zeros(5), np.array([0.0416, -0.0477, -0.00326, -0.00399, 0.0111]), np.array([-0.05, 0.01, 1e-3, -5e-4])]
    mounts = [(0.1, 0.0, 0.0), (-0.2, 0.05, math.pi), (0.0, 0.15, -math.pi / 2)]
    return list(zip(Ks, Ds, mounts))


def camera_frames():
    """three frames of two dark squares each; per frame the candidate list (ids, rotations, corners a little off the true ones)"""
    rng = np.random.RandomState(21)
    out = []
    for s in range(3):
        img, c1 = sr.square(B_ROWS, B_COLS, 10.3 + s, 9.6 + 2 * s, 17.0, 0.15 * (s + 1))
        img, c2 = sr.square(B_ROWS, B_COLS, 50.7 - s, 14.2 + s, 15.0, -0.2 * (s + 1), base=img)
        sl = tpk.Slot(None)
        sl.add(3 + s, c1 + rng.uniform(-0.8, 0.8, (4, 2)), rot=s % 4)
        sl.add(-1, rng.uniform(1, 40, (4, 2)))
        sl.add(9, c2 + rng.uniform(-0.8, 0.8, (4, 2)), rot=(s + 2) % 4)
        out.append((img, sl))
    return out


def test_cameras(tol):
    """the same lists through the single camera, a 3-camera rig (slot i is camera i % 3), a localization fleet and a SLAM fleet: the
    refined corners are the same in all four and are the stored marker corners; pose and observation are the oracle's on the refined
    corners with the slot's camera, and not those of the unrefined corners"""
    cams = camera_cases()
    frames = camera_frames()
    win, iters, acc = 3, 30, 0.01

    def single():
        ctx = context(B_ROWS, B_COLS, batch=3, camera=False)
        ctx.set_camera(cams[0][0], cams[0][1])
        return ctx, None, [cams[0][:2] + ((0.0, 0.0, 0.0),)] * 3

    def rig():
        ctx = context(B_ROWS, B_COLS, batch=3, camera=False)
        ctx.set_camera_rig(cams)
        return ctx, None, cams

    def fleet():
        ctx = context(B_ROWS, B_COLS, batch=3, camera=False)
        ctx.fleet_begin(cams, [500], [[5.0, 0.0, 0.0]], np.zeros((3, 3)), np.tile(np.eye(3) * 1e-2, (3, 1, 1)))
        return ctx, [2, 0, 1], [cams[2], cams[0], cams[1]]

    def fleet_slam():
        ctx = context(B_ROWS, B_COLS, batch=3, camera=False)
        ctx.fleet_slam_begin(cams)
        return ctx, [1, 2, 0], [cams[1], cams[2], cams[0]]

    refined = {}
    for name, make in (("single", single), ("rig", rig), ("fleet", fleet), ("fleet slam", fleet_slam)):
        ctx, robots, cam_of_slot = make()
        ctx.stage_frames(np.stack([f for f, _ in frames]), 0)
        refine_on(ctx, win, iters, acc)
        for s, (_, sl) in enumerate(frames):
            ctx.inject_candidates(s, sl.ids, sl.rots, np.array(sl.corners, np.float32).reshape(-1, 8))
        ctx.run_pose(0, 3, robots, refine=True)
        for s, (img, sl) in enumerate(frames):
            K, D, mount = cam_of_slot[s]
            exp = sl.expected()
            ids, corners, rv, tv = ctx.get_slot_detections(s)
            assert ids.tolist() == [sl.ids[i] for i in exp] and len(ids) == 2
            rotated = np.array([np.roll(sl.corners[i], sl.rots[i], axis=0) for i in exp], np.float32)
            want = orc.corner_sub_pix(img, rotated.reshape(-1, 2), win, iters, acc).reshape(-1, 4, 2)
            assert same_bits(corners, want), f"{name} slot {s}: stored corners are not the oracle's refined ones"
            assert np.abs(want - rotated).max() > 0.2
            refined.setdefault(s, corners)
            assert same_bits(corners, refined[s]), f"{name} slot {s}: refined corners differ from the single camera's"
            oids, valid, xyth, Rd = ctx.get_slot_raw_observations(s)
            assert np.array_equal(oids, ids)
            for j in range(len(ids)):
                rvo, tvo, _ = orc.solve_pnp(corners[j], L, K, D)
                e = max(float(tpk.pr.rotation_distance(rv[j:j + 1], rvo[None]).max()), float(np.max(np.abs(tv[j] - tvo)) / np.linalg.norm(tvo)))
                note("pose vs oracle", e)
                assert e <= tol["pose"], f"{name} slot {s} marker {j}: pose differs from the oracle's on the refined corners by {e:.3g}"
                rvu, tvu, _ = orc.solve_pnp(rotated[j], L, K, D)
                assert np.max(np.abs(tv[j] - tvu)) / np.linalg.norm(tvu) > 1e-4, "the pose is that of the unrefined corners"
                ok, z, r = tpk.observe_oracle(K, D, rv[j], tv[j], corners[j], mount)
                assert bool(valid[j]) == ok
                if ok:
                    e = max(tpk.rel(xyth[j, :2], z[:2]), float(tpk.angle_diff(xyth[j, 2], z[2])), tpk.rel(Rd[j], r))
                    note("observation vs oracle", e)
                    assert e <= tol["obs"], f"{name} slot {s} marker {j}: observation differs from the oracle by {e:.3g}"
            assert valid.any()


# ---- the product path --------------------------------------------------------------------------------------------------------------

REFINE_KW = dict(doCornerRefinement=1, cornerRefinementWinSize=5, cornerRefinementMaxIterations=30, cornerRefinementMinAccuracy=0.1)


def test_hook_equals_a_detection_pass():
    """three rendered 240 x 320 frames at slots 1..3 of one run_staged call: the detections of a pass without refinement, injected
    (rotation 0) and run through the hook, equal a full pass with refinement bit for bit - and the full pass equals the oracle's, so
    the product's own slot offset is covered as well"""
    rows, cols = 240, 320
    ctx = capi.Context(max_rows=rows, max_cols=cols, max_batch=4, persistent_waves=4, max_landmarks=16)
    imgs = []
    for s in range(3):
        ids, poses, K = synth.simple_scene(rows, cols, 300.0, 3, seed=1 + s, tz=(0.9, 1.4))
        ctx.set_camera(K, np.zeros(5))
        imgs.append(ctx.synth_render(1 + s, rows, cols, K, ids, poses, noise_amp=2, seed=5 + s))
    assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[1], imgs[2])
    ctx.run_staged(1, 3, with_ekf=False); ctx.sync()
    plain = [ctx.get_slot_detections(1 + s) for s in range(3)]
    assert all(len(p[0]) == 3 for p in plain)
    ctx.set_detector_params(**REFINE_KW)
    orc.set_detector_params(**REFINE_KW)
    ctx.run_staged(1, 3, with_ekf=False); ctx.sync()
    full = [ctx.get_slot_detections(1 + s) for s in range(3)]
    for s in range(3):
        oi, oc = orc.detect(imgs[s])
        assert np.array_equal(oi, full[s][0]) and same_bits(oc, full[s][1]), f"slot {1 + s}: the refining pass differs from the oracle"
        assert not same_bits(full[s][1], plain[s][1])
        ctx.inject_candidates(1 + s, plain[s][0], np.zeros(len(plain[s][0])), plain[s][1])
    ctx.run_pose(1, 3, refine=True)
    for s in range(3):
        ids, corners, rv, tv = ctx.get_slot_detections(1 + s)
        assert np.array_equal(ids, full[s][0]) and same_bits(corners, full[s][1]), f"slot {1 + s}: hook and detection pass differ"
        assert np.array_equal(rv, full[s][2]) and np.array_equal(tv, full[s][3])


def test_rig_step_with_refinement_matches_oracle():
    """one 2-camera run_staged_rig step with refinement on: each image's detections equal the oracle's"""
    rows, cols = 240, 320
    ctx = capi.Context(max_rows=rows, max_cols=cols, max_batch=2, persistent_waves=4, max_landmarks=16)
    imgs, Ks = [], []
    for s in range(2):
        ids, poses, K = synth.simple_scene(rows, cols, 300.0 - 20 * s, 3, seed=4 + s, tz=(0.9, 1.4))
        imgs.append(ctx.synth_render(s, rows, cols, K, ids, poses, noise_amp=2, seed=9 + s))
        Ks.append(K)
    ctx.set_camera_rig([(Ks[0], np.zeros(5), (0.1, 0.0, 0.0)), (Ks[1], np.zeros(5), (-0.1, 0.0, math.pi))])
    ctx.set_detector_params(**REFINE_KW)
    orc.set_detector_params(**REFINE_KW)
    ctx.stage_encoders([0.0, 0.0], [0.0, 0.0], [0.1, 0.1])
    ctx.run_staged_rig(0, 1, with_ekf=False); ctx.sync()
    for s in range(2):
        oi, oc = orc.detect(imgs[s])
        ids, corners, rv, tv = ctx.get_slot_detections(s)
        assert len(oi) == 3 and np.array_equal(oi, ids) and same_bits(oc, corners), f"camera {s}: detections differ from the oracle"
        assert np.abs(corners - np.round(corners)).max() > 1e-3
        for j in range(len(ids)):
            rvo, tvo, _ = orc.solve_pnp(corners[j], L, Ks[s], np.zeros(5))
            assert np.allclose(tvo, tv[j], rtol=1e-6, atol=1e-8)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def code_of(fn, *a, **k):
    with pytest.raises(capi.AslamError) as e:
        fn(*a, **k)
    return e.value.code


def test_hook_refusals():
    ctx = context(48, 80, batch=3)
    quad = np.array([[10, 10], [30, 10], [30, 30], [10, 30]], np.float32)
    ctx.stage_frames(sr.flat(48, 80), 0)
    ctx.inject_candidates(0, [1], [0], quad)
    assert code_of(ctx.run_pose, 0, 1, refine=True) == E_STATE            # refinement not enabled
    refine_on(ctx, 3, 30, 0.1)
    ctx.run_pose(0, 1, refine=True)
    ctx.inject_candidates(1, [1], [0], quad)
    assert code_of(ctx.run_pose, 0, 2, refine=True) == E_STATE            # slot 1 holds no frame
    assert code_of(ctx.run_pose, 1, 1, refine=True) == E_STATE
    ctx.run_pose(0, 2)                                                      # the plain hook needs none
    ctx.stage_frames(sr.flat(40, 64), 1)                                    # the current shape changes: slot 0 is stale
    assert code_of(ctx.run_pose, 0, 1, refine=True) == E_STATE
    ctx.run_pose(1, 1, refine=True)
    ctx.stage_frames(sr.flat(48, 80), 0)
    for bad in ((80.0, 10.0), (-0.5, 10.0), (10.0, 48.0), (10.0, -1e-3), (79.99, 48.0)):
        q = quad.copy(); q[2] = bad
        ctx.inject_candidates(0, [-1, 4], [0, 0], np.stack([quad, q]))
        assert code_of(ctx.run_pose, 0, 1, refine=True) == E_INVALID, bad
        ctx.inject_candidates(0, [4, -1], [0, 0], np.stack([quad, q]))     # a rejected candidate may lie anywhere
        ctx.run_pose(0, 1, refine=True)
    q = quad.copy(); q[1] = (79.99, 47.99); q[3] = (0.0, 0.0)
    ctx.inject_candidates(0, [4], [0], q)
    ctx.run_pose(0, 1, refine=True)                                         # the last pixel is inside
    assert code_of(ctx.run_pose, 0, 1, [0], refine=True) == E_INVALID      # robot_of_slot without a fleet
    assert code_of(ctx.run_pose, 2, 2, refine=True) == E_INVALID           # beyond the context's slots
    cams = camera_cases()
    fl = context(48, 80, batch=3, camera=False)
    fl.fleet_slam_begin(cams)
    fl.stage_frames(sr.flat(48, 80), 0)
    refine_on(fl, 3, 30, 0.1)
    fl.inject_candidates(0, [1], [0], quad)
    assert code_of(fl.run_pose, 0, 1, refine=True) == E_INVALID            # a fleet needs the robot of every slot
    assert code_of(fl.run_pose, 0, 1, [3], refine=True) == E_INVALID
    fl.run_pose(0, 1, [2], refine=True)
    nocam = context(48, 80, camera=False)
    nocam.stage_frames(sr.flat(48, 80), 0)
    refine_on(nocam, 3, 30, 0.1)
    nocam.inject_candidates(0, [1], [0], quad)
    assert code_of(nocam.run_pose, 0, 1, refine=True) == E_STATE
