"""k_quads and k_assemble (detect.hip) on injected contours and quads, against the oracle and against the exact restatement in
tests/quads_reference.py.

aslam_debug_inject_contours writes a slot's kept-contour list, aslam_debug_inject_quads its quad list; aslam_debug_run_quads
launches the production kernels of the quad stage (stages & 1) and of candidate assembly (stages & 2) on them, as a detection
call does.  Every case is checked twice, by exact equality of integers:
  (a) against the oracle's entry on the same lists (orc.quads), all cases;
  (b) against the reference, every contour / slot the reference decides without an ambiguous comparison (quads_reference.py).
Families that place a boundary on purpose use dyadic rates (no ambiguity possible: asserted); the families with the default
rates allow 1 % ambiguous contours and pairs (asserted).  Each test counts what it reached and asserts a minimum per named
case; the tally is printed at the end of the module.  Runs on whichever library the session loads: the emulation here, the
gfx950 build on the MI355X."""
import collections
from fractions import Fraction

import numpy as np
import pytest

import quads_reference as qr
from aruco_slam_amd import capi
from oracle import pyoracle as orc

K = np.array([[100.0, 0, 40], [0, 100, 40], [0, 0, 1]])
REACHED = collections.Counter()
LDS_PTS = 1536              # kQuadLdsPts
CAND_MAX, PAIR_MAX = 2048, 4096


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nquads cases reached: " + ", ".join(f"{k} {v}" for k, v in sorted(REACHED.items())))


@pytest.fixture(autouse=True)
def oracle_defaults():
    yield
    orc.set_detector_params()


def name(k):
    return k.replace("__", ", ").replace("_", " ")


def need(tally, **mins):
    REACHED.update(tally)
    short = {k: (tally[name(k)], v) for k, v in mins.items() if tally[name(k)] < v}
    assert not short, f"cases not reached (got, wanted): {short}"


class Rig:
    """a context with blank frames of one shape staged in every slot, and one set of rates on library, oracle and reference"""

    def __init__(self, rows, cols, batch, waves=4, **init):
        self.rows, self.cols, self.batch = rows, cols, batch
        self.ctx = capi.Context(max_rows=rows, max_cols=cols, max_batch=batch, persistent_waves=waves, max_landmarks=16, **init)
        self.ctx.set_camera(K, np.zeros(5))
        blank = np.zeros((1, rows, cols), np.uint8)
        for s in range(batch):
            self.ctx.stage_frames(blank, s)
        self.rates()

    def rates(self, approx=0.05, corner=0.05, border=3, marker=0.05):
        kw = dict(polygonalApproxAccuracyRate=approx, minCornerDistanceRate=corner, minDistanceToBorder=border, minMarkerDistanceRate=marker)
        self.ctx.set_detector_params(**kw)
        orc.set_detector_params(**kw)
        self.P = qr.Params(approx, corner, border, marker)
        self.dyadic = all(float(v) * 2 ** 20 == int(float(v) * 2 ** 20) for v in (approx, corner, marker))
        return self


def as_int(c):
    c = np.asarray(c)
    assert np.array_equal(c, np.round(c))
    return c.astype(np.int64)


_REF = {}


def ref_quad(rig, c):
    """the reference's verdict on one contour under the rig's current rates (kept: the pre-pass and the check share it)"""
    key = (rig.rows, rig.cols, rig.P.approx, rig.P.corner, rig.P.border, tuple(c))
    if key not in _REF:
        _REF[key] = qr.quad_of_contour(c, rig.rows, rig.cols, rig.P)
    return _REF[key]


def ambiguity_of_reference(rig, slots, tally):
    """the reference alone, before any kernel runs: at most 1 % of the contours and 1 % of the pairs of these inputs are ambiguous"""
    n_amb = n_all = p_amb = p_all = 0
    for contours, scales, keys in slots:
        res = [ref_quad(rig, c) for c in contours]
        n_all += len(res); n_amb += sum(r.ambiguous for r in res)
        order = sorted((i for i in range(len(res)) if res[i].corners is not None), key=lambda i: (scales[i], -keys[i]))
        re = [qr.reorder_corners(res[i].corners) for i in order]
        _, _, amb, decided = qr.filter_too_close(re, [len(contours[i]) for i in order], rig.P.marker)
        p_amb += amb; p_all += decided
    assert n_amb * 100 <= n_all and p_amb * 100 <= max(p_all, 1), f"seeds: {n_amb} of {n_all} contours, {p_amb} of {p_all} pairs ambiguous"
    tally["reference alone first"] += 1


def check_quads(rig, slots, tally, stages=1, ref=True, traces=None):
    """slots[s] = (contours, scales, keys).  Runs k_quads (and k_assemble with stages = 3) and checks every slot.
    Returns the reference's per-contour results of each slot."""
    ctx = rig.ctx
    for s, (contours, scales, keys) in enumerate(slots):
        ctx.inject_contours(s, contours, scales, keys)
    ctx.run_quads(0, len(slots), stages)
    out = []
    n_amb = n_all = 0
    for s, (contours, scales, keys) in enumerate(slots):
        kc, kn, _ = ctx.debug_candidates(s, 0)
        oc, on, osc, okey = orc.quads(rig.rows, rig.cols, scales, keys, contours=contours, stage=0)
        assert len(kn) == len(on), f"slot {s}: {len(kn)} quads, the oracle {len(on)}"
        assert np.array_equal(kc, oc) and np.array_equal(kn, on), f"slot {s}: quads differ from the oracle"
        tally["quads"] += len(kn)
        for c in contours:
            tally["lds path" if len(c) <= LDS_PTS else "global path"] += 1
        if stages & 2:
            kf, kfn, _ = ctx.debug_candidates(s, 2)
            of, ofn, _, _ = orc.quads(rig.rows, rig.cols, scales, keys, contours=contours, stage=2)
            assert np.array_equal(kf, of) and np.array_equal(kfn, ofn), f"slot {s}: final candidates differ from the oracle"
            tally["finals"] += len(kfn)
        if not ref:
            out.append(None)
            continue
        # the kernel's list is in candidate order and equals the oracle's, which names each quad's (scale, key)
        got = {(int(a), int(b)): (as_int(c).tolist(), int(n)) for a, b, c, n in zip(osc, okey, kc, kn)}
        res = []
        for i, c in enumerate(contours):
            if traces is not None:
                qr.approx_closed(c, rig.P.approx, traces.setdefault((s, i), {}))
            r2 = ref_quad(rig, c)
            res.append(r2)
            n_all += 1
            if r2.ambiguous:
                n_amb += 1
                continue
            k = (int(scales[i]), int(keys[i]))
            if r2.corners is None:
                assert k not in got, f"slot {s} contour {i}: the kernel made a quad, the reference rejects it ({r2.why})"
            else:
                assert k in got, f"slot {s} contour {i}: lost (the reference makes it a quad)"
                assert got[k] == ([list(p) for p in r2.corners], len(c)), f"slot {s} contour {i}: corners differ from the reference"
            tally["why " + r2.why] += 1
            tally["dp %d" % min(r2.dp_vertices, 12)] += 1
            if 5 <= r2.dp_vertices <= 8 and r2.vertices == 4:
                tally["dp %d to 4" % r2.dp_vertices] += 1
        if stages & 2 and ref:
            check_assembly_ref(rig, s, as_int(kc), kn, kf, kfn, tally)
        out.append(res)
    tally["ambiguous contours"] += n_amb
    tally["contours"] += n_all
    if rig.dyadic:
        assert n_amb == 0, "an ambiguous decision with dyadic rates"
    else:
        assert n_amb * 100 <= n_all, f"{n_amb} of {n_all} contours ambiguous"
    return out


def check_assembly_ref(rig, s, corners, sizes, kf, kfn, tally):
    """corners / sizes in candidate order (already verified); kf, kfn: what k_assemble kept"""
    re = [qr.reorder_corners([tuple(p) for p in q]) for q in corners.tolist()]
    kept, near, amb, decided = qr.filter_too_close(re, sizes, rig.P.marker)
    tally["pairs"] += decided
    tally["near pairs"] += len(near)
    tally["ambiguous pairs"] += amb
    if rig.dyadic:
        assert amb == 0, "an ambiguous pair with a dyadic rate"
    else:
        assert amb * 100 <= max(decided, 1), f"{amb} of {decided} pairs ambiguous"
    if amb:
        return near
    assert len(kfn) == len(kept), f"slot {s}: {len(kfn)} candidates kept, the reference keeps {len(kept)}"
    assert as_int(kf).tolist() == [[list(p) for p in re[i]] for i in kept], f"slot {s}: kept candidates differ from the reference"
    assert kfn.tolist() == [int(sizes[i]) for i in kept]
    return near


def check_assemble(rig, slots, tally):
    """slots[s] = (corners C x 4 x 2, sizes, scales, keys) in any order.  Runs k_assemble alone; returns the near pairs per slot."""
    ctx = rig.ctx
    for s, (corners, sizes, scales, keys) in enumerate(slots):
        ctx.inject_quads(s, corners, sizes, scales, keys)
    ctx.run_quads(0, len(slots), 2)
    out = []
    for s, (corners, sizes, scales, keys) in enumerate(slots):
        corners = np.asarray(corners, np.int64).reshape(-1, 4, 2); sizes = np.asarray(sizes, np.int64)
        kf, kfn, _ = ctx.debug_candidates(s, 2)
        of, ofn, _, _ = orc.quads(rig.rows, rig.cols, scales, keys, quads_in=(corners, sizes), stage=2)
        assert len(kfn) == len(ofn), f"slot {s}: {len(kfn)} kept, the oracle {len(ofn)}"
        assert np.array_equal(kf, of) and np.array_equal(kfn, ofn), f"slot {s}: kept candidates differ from the oracle"
        order = sorted(range(len(sizes)), key=lambda i: (int(scales[i]), -int(keys[i])))
        tally["candidates"] += len(sizes)
        tally["kept"] += len(kfn)
        out.append(check_assembly_ref(rig, s, corners[order], sizes[order], kf, kfn, tally))
    return out


# ---- shapes ---------------------------------------------------------------------------------------------------------------------

def line(a, b):
    """8-connected points from a (included) to b (excluded)"""
    n = max(abs(b[0] - a[0]), abs(b[1] - a[1]))
    return [(a[0] + (2 * i * (b[0] - a[0]) + n) // (2 * n), a[1] + (2 * i * (b[1] - a[1]) + n) // (2 * n)) for i in range(n)]


def outline(poly):
    return [p for k in range(len(poly)) for p in line(poly[k], poly[(k + 1) % len(poly)])]


def rot(pts, s):
    s %= len(pts)
    return pts[s:] + pts[:s]


def shift(pts, dx, dy):
    return [(x + dx, y + dy) for x, y in pts]


def sized_quad(N):
    """corners of a convex quadrilateral whose outline has exactly N points (N >= 4)"""
    c = N % 2
    b = max(1, N // 4)
    a = (N + c - 2 * b) // 2
    return [(0, 0), (a, 0), (a, b), (c, b)]


def rotated(poly, deg, cx=0, cy=0):
    t = np.deg2rad(deg)
    return [(int(round(cx + x * np.cos(t) - y * np.sin(t))), int(round(cy + x * np.sin(t) + y * np.cos(t)))) for x, y in poly]


@pytest.fixture(scope="module")
def big():
    """2100 x 2100: more than 2^22 pixels, room for outlines of a few thousand points"""
    return Rig(2100, 2100, 2)


@pytest.fixture(scope="module")
def small():
    """205 x 151 (odd-sized), a batch of slots"""
    return Rig(151, 205, 8)


# ---- k_quads --------------------------------------------------------------------------------------------------------------------

SIZES = (4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1535, 1536, 1537, 1600, 4096)


def test_sizes(big):
    """outlines of every point count around the unroll rounds and the LDS limit, each from four start points, and the largest
    contour the lists hold (65534 points: an outline whose points repeat, since no outline of a legal frame is that long)"""
    big.rates(approx=1 / 64, corner=1 / 64, border=3)
    t = collections.Counter()
    contours = []
    for N in SIZES:
        q = sized_quad(N)
        pts = shift(outline(q), 20, 20)
        assert len(pts) == N
        a = q[1][0]                                        # the second corner sits at index a
        for start in (a, a + 1, a // 2, a - 1):
            contours.append(rot(pts, start))
    base = shift(outline([(0, 0), (2000, 0), (2000, 2000), (0, 2000)]), 40, 40)
    rep = [p for i, p in enumerate(base) for _ in range(9 if i < 65534 - 8 * len(base) else 8)]
    assert len(rep) == 65534
    for start in (0, 5, 30001):
        contours.append(rot(rep, start))
    res = check_quads(big, [(contours, [0] * len(contours), list(range(len(contours))))], t)[0]
    assert all(r.why == "quad" for r in res[4:]), "every outline of 5 points and more is meant to pass"
    t["largest contour"] = sum(len(c) == 65534 for c in contours)
    need(t, lds_path=4 * 13, global_path=4 * 3 + 3, quads=len(contours) - 4, largest_contour=3)


def tie_rect(W, H, g, reverse):
    """a W x H rectangle started at the middle of its bottom side whose top side is resampled to g steps: its two top corners tie
    as the farthest point of the first search, g positions apart"""
    top = [(W - (i * W) // g, 0) for i in range(g)]                     # (W, 0) .. towards (0, 0), g points
    pts = line((W // 2, H), (W, H)) + line((W, H), (W, 0)) + top + line((0, 0), (0, H)) + line((0, H), (W // 2, H))
    return pts[:1] + pts[:0:-1] if reverse else pts


def tie_trapezoid(W, H, g, reverse, start):
    """a trapezoid on a long base whose top side (parallel to the base, g steps) ties point for point in the slice search"""
    inset = W // 4
    top = [(W - inset - (i * (W - 2 * inset)) // g, 0) for i in range(g)]
    pts = line((0, H), (W, H)) + line((W, H), (W - inset, 0)) + top + line((inset, 0), (0, H))
    if reverse:
        pts = pts[:1] + pts[:0:-1]
    return rot(pts, start)


def test_ties(big):
    """several points at exactly the same maximal distance: the earliest wins, as in the sequential scan"""
    big.rates(approx=1 / 64, corner=1 / 64, border=0)
    t = collections.Counter()
    contours = []
    gaps = (1, 2, 63, 64, 65, 255, 256, 257)
    for g in gaps:
        for rev in (False, True):
            for W, H in ((400, 300), (600, 200)):
                contours.append(shift(tie_rect(W, H, g, rev), 30, 30))
            for start in (0, 1, 37):
                contours.append(shift(tie_trapezoid(800, 120, g, rev, start), 30, 30))
    for s in (40, 41, 128, 256):                                        # squares, diamonds and octagons from a corner and mid-side
        for st in (0, s // 2, s):
            contours.append(rot(shift(outline([(0, 0), (s, 0), (s, s), (0, s)]), 50, 50), st))
            contours.append(rot(shift(outline([(s, 0), (2 * s, s), (s, 2 * s), (0, s)]), 50, 50), st))
            contours.append(rot(shift(outline([(s, 0), (2 * s, 0), (3 * s, s), (3 * s, 2 * s), (2 * s, 3 * s), (s, 3 * s), (0, 2 * s), (0, s)]), 50, 50), st))
    traces = {}
    check_quads(big, [(contours, [0] * len(contours), list(range(len(contours))))], t, traces=traces)
    for tr in traces.values():
        for kind in ("initial", "slice"):
            for g in tr.get(kind, ()):
                if g in gaps:
                    t["tie %s +%d" % (kind, g)] += 1
    need(t, **{"tie_%s_+%d" % (kind, g): 2 for kind in ("initial", "slice") for g in gaps}, why_quad=40)


def test_degenerate(small):
    small.rates(approx=1 / 32, corner=1 / 32, border=0)
    t = collections.Counter()
    spur = line((20, 20), (60, 45))
    contours = [[(30, 30)] * n for n in (1, 2, 3, 4, 64, 65, 300)]                                # all points equal
    contours += [spur + [(60, 45)] + spur[:0:-1], line((10, 10), (90, 10)) + line((90, 10), (10, 10))]      # out and back
    contours += [[(10, 10), (50, 40)], [(10, 10), (50, 40)] * 40, [(10, 10)] * 30 + [(50, 40)] * 30]   # two distinct points
    contours += [[(10, 10)], [(10, 10), (12, 10)], [(10, 10), (40, 10), (20, 30)]]                    # 1, 2, 3 points
    contours += [rot(c, len(c) // 3) for c in contours[7:9]]
    res = check_quads(small, [(contours, [0] * len(contours), list(range(len(contours))))], t)[0]
    assert all(r.corners is None for r in res)
    need(t, dp_1=7, dp_2=4, contours=len(contours))


def bent_quad(W, H, d, apexes, bumps, deg):
    """a tall W x H quad with slight apexes (d pixels) on its short sides and slight bumps on its long sides: Douglas-Peucker keeps
    them (they end its first chords), the clean-up pass takes them out again"""
    poly = [(0, -d if apexes > 0 else 0), (W // 2, 0)]
    poly += [(W // 2 + d, H // 2)] if bumps > 0 else []
    poly += [(W // 2, H)]
    poly += [(0, H + d)] if apexes > 1 else []
    poly += [(-(W // 2), H)]
    poly += [(-(W // 2) - d, H // 2)] if bumps > 1 else []
    poly += [(-(W // 2), 0)]
    if apexes == 0:
        poly = poly[1:]
    return rotated(poly, deg, 1000, 800)


def test_vertex_counts(big):
    """polygons that leave Douglas-Peucker with 3..9 and more vertices; 5..8 that the clean-up brings to exactly 4; arbitrary lists"""
    big.rates(approx=1 / 64, corner=1 / 128, border=3)
    t = collections.Counter()
    contours = []
    for k in (3, 4, 5, 6, 7, 8, 9, 12, 16, 24):
        for r in (150, 333):
            for ph in (0.0, 0.4):
                poly = [(int(round(600 + r * np.cos(2 * np.pi * i / k + ph))), int(round(600 + r * np.sin(2 * np.pi * i / k + ph)))) for i in range(k)]
                contours.append(outline(poly))
    for deg in (20, 33, 47, 61, 110, 200):
        for d in (2, 3, 4):
            for apexes, bumps in ((1, 0), (2, 0), (2, 1), (2, 2), (1, 1), (1, 2)):
                c = outline(bent_quad(50, 420, d, apexes, bumps, deg))
                contours += [c, rot(c, len(c) // 2), c[:1] + c[:0:-1]]
    n_bent = len(contours)
    for deg in (0, 90):                                                  # the same along the axes: the clean-up spares a vertex between
        for d in (2, 3):                                                 # axis-parallel neighbours (dx == 0 or dy == 0) and stays no quad
            for apexes, bumps in ((1, 0), (2, 0), (2, 1), (2, 2)):
                c = outline(bent_quad(50, 420, d, apexes, bumps, deg))
                contours += [c, c[:1] + c[:0:-1]]
    axis = range(n_bent, len(contours))
    rng = np.random.default_rng(11)
    for i in range(60):                                                  # random walks, stars, combs
        n = int(rng.integers(5, 400))
        if i % 3 == 0:
            c = np.cumsum(rng.integers(-1, 2, (n, 2)), axis=0) + 700
        elif i % 3 == 1:
            th = np.sort(rng.uniform(0, 2 * np.pi, n)); r = np.where(np.arange(n) % 2, 300, 40 + 200 * rng.random())
            c = np.round(np.c_[700 + r * np.cos(th), 700 + r * np.sin(th)]).astype(int)
        else:
            c = np.c_[600 + np.arange(n) * 2, 600 + np.where(np.arange(n) % 4 < 2, 0, 150)]
            c = np.concatenate([c, c[::-1] + [0, 200]])
        contours.append([tuple(int(v) for v in p) for p in c])
    for i in range(150):                                                 # sparse lists: a few points in convex position, padded by repeats
        k = int(rng.integers(4, 8))
        th = np.sort(rng.uniform(0, 2 * np.pi, k)); r = rng.uniform(30, 400, k) if i % 2 else np.full(k, 200.0)
        c = [(int(round(900 + a * np.cos(b))), int(round(900 + a * np.sin(b)))) for a, b in zip(r, th)]
        contours.append([p for p in c for _ in range(1 + i % 3)])
    scales = [i % 3 for i in range(len(contours))]
    res = check_quads(big, [(contours, scales, list(range(len(contours))))], t)[0]
    t["axis parallel vertex spared"] = sum(res[i].dp_vertices > 4 and res[i].vertices > 4 for i in axis)
    need(t, axis_parallel_vertex_spared=8)
    need(t, dp_3=1, dp_4=4, dp_5=4, dp_6=4, dp_7=4, dp_8=4, dp_9=1, dp_12=4, dp_5_to_4=1, dp_6_to_4=1, dp_7_to_4=1, dp_8_to_4=1,
         why_quad=40, why_vertices=60)


def test_deviation_on_the_limit(small):
    """a slice whose farthest point lies exactly eps from its chord is not split (<=): a thin parallelogram on a 3-4-5 chord of
    length 50 with both other corners at cross product 200 = eps * 50 (n = 64, rate 1 / 16) is no quad; one step further out it is"""
    small.rates(approx=1 / 16, corner=1 / 64, border=3)
    t = collections.Counter()
    contours, want = [], []
    cross = []
    for b in ((10, 20), (10, 21), (9, 20), (11, 20)):
        q = [(0, 0), b, (30, 40), (30 - b[0], 40 - b[1])]
        for r in range(4):
            for lst in (rot(q, r), rot(q[::-1], r)):
                contours.append(padded(shift(lst, 40, 30), 64)); cross.append(abs(b[1] * 30 - b[0] * 40))
    assert cross.count(200) == 8 and min(cross) < 200 < max(cross)      # eps * |chord| = 4 * 50
    res = check_quads(small, [(contours, [0] * len(contours), list(range(len(contours))))], t)[0]
    for r, x in zip(res, cross):
        assert (r.why == "quad") == (x > 200)
        t["deviation on the limit, not split"] += x == 200 and r.dp_vertices == 2
        t["deviation above the limit, split"] += x > 200 and r.dp_vertices == 4
        t["deviation below the limit"] += x < 200 and r.dp_vertices == 2
    need(t, deviation_on_the_limit__not_split=8, deviation_above_the_limit__split=16, deviation_below_the_limit=8)


def padded(q, n):
    """the four points of q as a closed list of n points (the first one repeated)"""
    return [q[0]] * (n - 3) + list(q[1:])


def test_quad_tests(small):
    """convexity, corner distance and border distance, each on its limit: the lists are the four corners themselves"""
    t = collections.Counter()
    rows, cols = small.rows, small.cols
    # convexity: a reflex corner at each position, bow-ties, three corners in a line (the middle one survives Douglas-Peucker
    # only where the list doubles back, as a border does along a one-pixel spur)
    small.rates(approx=1 / 64, corner=1 / 64, border=3)
    convex = [(40, 40), (100, 44), (96, 100), (36, 90)]
    shapes = [convex, convex[::-1]]
    for i in range(4):
        q = list(convex); q[i] = (68, 70); shapes.append(q); shapes.append(q[::-1])
    shapes += [[(40, 40), (100, 100), (100, 40), (40, 100)], [(40, 40), (100, 100), (40, 100), (100, 40)]]
    for r in range(4):
        shapes.append(rot([(40, 40), (120, 40), (80, 40), (80, 90)], r))
        shapes.append(rot([(40, 40), (40, 120), (40, 80), (90, 80)], r))
    contours = [rot(list(s), r) for s in shapes for r in range(4)]
    # the approximation starts its vertex list where its own search ends, so rotating a list does not rotate the quad: lists found
    # by search whose quad has its first straight (or opposite) turn at each step of the convexity scan
    contours += [[(40, 72), (88, 56), (72, 88), (88, 96)], [(96, 72), (64, 88), (96, 72), (80, 96)],
                 [(64, 80), (72, 80), (48, 64), (96, 96)], [(80, 48), (80, 96), (80, 88), (104, 80)],
                 [(56, 96), (96, 104), (56, 56), (104, 88)], [(96, 96), (104, 96), (88, 80), (72, 40)],
                 [(56, 56), (40, 88), (88, 48), (48, 56)], [(96, 72), (104, 72), (96, 48), (64, 96)]]
    res = check_quads(small, [(contours, [0] * len(contours), list(range(len(contours))))], t)[0]
    t["not convex"] = sum(r.why == "convex" for r in res)
    t["convex"] = sum(r.why == "quad" for r in res)
    for c, r in zip(contours, res):
        if r.why == "convex":
            step, kind = qr.first_bad_turn(qr.approx_closed(c, small.P.approx)[0])
            t["%s turn at step %d" % (kind, step)] += 1
            t["orientation reaches 3 at step %d" % step] += 1
    # (a straight turn at step 3 with three equal turns before it: no list of 5 million searched gives one; it is counted if it comes)
    need(t, not_convex=40, convex=8, zero_turn_at_step_0=2, zero_turn_at_step_1=2, zero_turn_at_step_2=2,
         opposite_turn_at_step_1=2, opposite_turn_at_step_2=2, opposite_turn_at_step_3=2, orientation_reaches_3_at_step_0=2,
         orientation_reaches_3_at_step_1=2, orientation_reaches_3_at_step_2=2, orientation_reaches_3_at_step_3=2)
    # corner distance: (n rate)^2 = 9 with n = 48, rate 1 / 16; the shortest side squared 8, 9, 10
    small.rates(approx=1 / 256, corner=1 / 16, border=3)
    contours, want = [], []
    for side, ok in (((2, 2), False), ((3, 0), True), ((3, 1), True)):
        q = [(50, 50), (50 + side[0], 50 + side[1]), (70, 80), (40, 75)]
        for r in range(4):
            contours.append(padded(rot(q, r), 48)); want.append(ok)
            contours.append(padded(rot(q[::-1], r), 48)); want.append(ok)
    res = check_quads(small, [(contours, [0] * len(contours), list(range(len(contours))))], t)[0]
    assert [r.why for r in res] == ["quad" if w else "corner distance" for w in want]
    t["corner distance below"] = want.count(False); t["corner distance on or above"] = want.count(True)
    # border distance: one coordinate of one corner at minDistanceToBorder - 1, on it, + 1, from each edge
    for b in (0, 3, 7):
        small.rates(approx=1 / 64, corner=1 / 64, border=b)
        contours, want = [], []
        for corner in range(4):                                         # position in the list of the corner that goes to the edge
            for edge in range(4):                                       # left, top, right, bottom: the diamond's corner on that side
                for off in (-1, 0, 1):
                    q = [[40, 75], [100, 30], [160, 75], [100, 120]]
                    q[edge][edge % 2] = (b + off) if edge < 2 else ((cols if edge == 2 else rows) - 1 - b - off)
                    contours.append([tuple(p) for p in rot(q, edge - corner)]); want.append(off >= 0)
        res = check_quads(small, [(contours, [0] * len(contours), list(range(len(contours))))], t)[0]
        got = [r.why for r in res]
        assert got == ["quad" if w else "border" for w in want]
        t["border inside b%d" % b] = sum(g == "quad" for g in got); t["border outside b%d" % b] = sum(g == "border" for g in got)
    need(t, corner_distance_below=8, corner_distance_on_or_above=16, border_inside_b0=32, border_outside_b0=16,
         border_inside_b3=32, border_outside_b3=16, border_inside_b7=32, border_outside_b7=16)


def scene(rng, rows, cols, n_markers, lo=18, hi=60):
    """outlines of random projective squares, each with nested inner outlines at three scales (a marker's border pair)"""
    contours, scales = [], []
    for _ in range(n_markers):
        s = rng.uniform(lo, hi)
        cx, cy = rng.uniform(hi + 6, cols - hi - 6), rng.uniform(hi + 6, rows - hi - 6)
        th = rng.uniform(0, 2 * np.pi)
        q = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float) * (1 + rng.uniform(-0.25, 0.25, (4, 2)))
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        for scale in range(3):
            for shrink in (1.0, 1.0 - 2.0 / s, 0.72):
                poly = [(int(round(cx + v[0])), int(round(cy + v[1]))) for v in (q * s * shrink + rng.uniform(-0.6, 0.6, (4, 2)) * (scale > 0)) @ R.T]
                if len(set(poly)) == 4:
                    contours.append(outline(poly)); scales.append(scale)
    return contours, scales


def test_work_distribution(small):
    """both sides of the grab switch (32 contours with 4 waves), a remainder of a grab, empty slots in a batch, one frame alone"""
    small.rates()
    t = collections.Counter()
    rng = np.random.default_rng(3)
    pool, _ = scene(rng, small.rows, small.cols, 8)
    assert len(pool) >= 60
    ambiguity_of_reference(small, [(pool, [i % 3 for i in range(len(pool))], list(range(len(pool))))], t)
    for n in (31, 32, 33, 35):
        c = pool[:n]
        check_quads(small, [(c, [i % 3 for i in range(n)], list(range(n)))], t, stages=3)
        t["one slot of %d" % n] += 1
    slots = [([], [], [])] + [(pool[:1], [0], [5])] + [(pool[:50], [i % 3 for i in range(50)], list(range(50)))] + [([], [], [])] + \
            [(pool[10:60], [i % 3 for i in range(50)], list(range(100, 150)))]
    check_quads(small, slots, t, stages=3)
    check_quads(small, slots[1:2] * 8, t, stages=3)
    need(t, one_slot_of_31=1, one_slot_of_32=1, one_slot_of_33=1, one_slot_of_35=1, quads=200)


def test_more_slots_than_a_chunk():
    """a call of more slots than detect_chunk(): ASLAM_DETECT_CHUNK is read once per process, so a fresh process runs the case"""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent("""
        import collections, numpy as np, sys
        sys.path.insert(0, %r)
        import test_quads_kernel as m
        rig = m.Rig(151, 205, 7).rates()
        pool, _ = m.scene(np.random.default_rng(4), 151, 205, 4)
        t = collections.Counter()
        slots = [(pool[i:i + 12], [j %% 3 for j in range(len(pool[i:i + 12]))], list(range(len(pool[i:i + 12])))) for i in range(7)]
        m.check_quads(rig, slots, t, stages=3)
        assert t["quads"] >= 40, t
        print("chunked ok", t["quads"])
    """) % os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ASLAM_DETECT_CHUNK="3", PYTHONPATH=os.pathsep.join(sys.path))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "chunked ok" in r.stdout, r.stdout + r.stderr
    REACHED["slots beyond a chunk"] += 1


def grid_quads(n, rows, cols, side=6, pitch=12):
    """n passing outlines on a grid"""
    per_row = (cols - 20) // pitch
    assert n <= per_row * ((rows - 20) // pitch)
    return [shift(outline([(0, 0), (side, 0), (side, side), (0, side)]), 10 + pitch * (i % per_row), 10 + pitch * (i // per_row)) for i in range(n)]


def test_quad_capacity():
    """exactly 2048 passing quads in a slot: all returned; 2049: the call reports the overflow"""
    rig = Rig(640, 800, 1).rates(approx=1 / 32, corner=1 / 64, border=3, marker=1 / 1024)
    t = collections.Counter()
    c = grid_quads(CAND_MAX + 1, rig.rows, rig.cols)
    check_quads(rig, [(c[:CAND_MAX], [0] * CAND_MAX, list(range(CAND_MAX)))], t, stages=3, ref=False)
    assert t["quads"] == CAND_MAX and t["finals"] == CAND_MAX
    rig.ctx.inject_contours(0, c, [0] * len(c), list(range(len(c))))
    with pytest.raises(capi.AslamError) as e:
        rig.ctx.run_quads(0, 1, 1)
    assert e.value.code == -4
    REACHED["quad list full"] += 1
    REACHED["quad list overflow reported"] += 1


# ---- k_assemble -----------------------------------------------------------------------------------------------------------------

def square(x, y, s=20):
    return [(x, y), (x + s, y), (x + s, y + s), (x, y + s)]


def test_order(big):
    """scale ascending, key descending inside a scale, for keys on both sides of 2^22 (a frame of more than 2^22 pixels), among
    them a scale-1 key and a scale-0 key 2^22 apart"""
    big.rates(marker=1 / 1024)
    t = collections.Counter()
    top = big.rows * big.cols
    assert top > 2 ** 22
    keys = [0, 1, 2 ** 22 - 1, 2 ** 22, 2 ** 22 + 1, top]
    quads, sizes, scales, ks = [], [], [], []
    for sc in range(3):
        for k in keys:
            quads.append(square(30 + 40 * len(quads), 50 + 100 * sc)); sizes.append(80 + len(quads)); scales.append(sc); ks.append(k)
    quads.append(square(100, 900)); sizes.append(333); scales.append(1); ks.append(2 ** 22 + 7)      # the colliding pair
    quads.append(square(200, 900)); sizes.append(334); scales.append(0); ks.append(7)
    perm = np.random.default_rng(0).permutation(len(quads))
    sel = lambda v: [v[i] for i in perm]
    check_assemble(big, [(sel(quads), sel(sizes), sel(scales), sel(ks))], t)
    # the same keys through k_quads (contours), whose ordkey the debug read-out sorts by
    contours = [outline(q) for q in quads]
    check_quads(big.rates(approx=1 / 32, corner=1 / 64, marker=1 / 1024), [(sel(contours), sel(scales), sel(ks))], t, stages=3)
    need(t, kept=len(quads), quads=len(quads))
    REACHED["keys beyond 2^22"] += 1


def test_largest_key():
    """the largest key a 4095 x 4095 frame gives (one slot, blank frame, nothing but the injected quads)"""
    rig = Rig(4095, 4095, 1).rates(marker=1 / 1024)
    t = collections.Counter()
    top = 4095 * 4095
    keys = [0, 2 ** 22, 2 ** 23, 2 ** 23 + 2 ** 22, top - 1, top]
    quads = [square(30 + 40 * i, 50) for i in range(3 * len(keys))]
    sizes = [80 + i for i in range(len(quads))]
    scales = [i // len(keys) for i in range(len(quads))]
    ks = keys * 3
    perm = np.random.default_rng(1).permutation(len(quads)).tolist()
    sel = lambda v: [v[i] for i in perm]
    check_assemble(rig, [(sel(quads), sel(sizes), sel(scales), sel(ks))], t)
    need(t, kept=len(quads))


def test_corner_order(small):
    small.rates(marker=1 / 1024)
    t = collections.Counter()
    quads = [square(20, 20), square(60, 20)[::-1], [(100, 20), (120, 40), (140, 60), (100, 60)], [(150, 20), (170, 40), (190, 60), (190, 20)],
             [(20, 80), (40, 80), (60, 80), (80, 80)]]
    crosses = [(q[1][0] - q[0][0]) * (q[2][1] - q[0][1]) - (q[1][1] - q[0][1]) * (q[2][0] - q[0][0]) for q in quads]
    assert any(c < 0 for c in crosses) and crosses.count(0) >= 3 and any(c > 0 for c in crosses)
    check_assemble(small, [(quads, [100] * len(quads), [0] * len(quads), list(range(len(quads))))], t)
    need(t, kept=len(quads))


def test_near_pairs(small):
    """one pair per slot, on the limit of minMarkerDistanceRate (dyadic) and a quarter to each side, under each corner rotation, with
    equal and unequal point counts in both orders; pairs around the slack of the centroid pre-test"""
    small.rates(marker=1 / 8)
    t = collections.Counter()
    slots, want = [], []
    base = square(60, 50, 30)
    for fc in range(4):
        for n_i, n_j in ((64, 64), (64, 80), (80, 64)):                  # threshold (64 / 8)^2 = 64 = a mean of the four squared distances
            for total, near in ((4 * 64 - 1, True), (4 * 64, False), (4 * 64 + 1, False)):
                # corner offsets whose squared lengths sum to `total`
                offs = {255: [(8, 0), (7, 4), (7, 4), (6, 5)], 256: [(8, 0)] * 4, 257: [(8, 0), (8, 0), (8, 0), (8, 1)]}[total]
                assert sum(x * x + y * y for x, y in offs) == total
                other = [(p[0] + o[0], p[1] + o[1]) for p, o in zip(base, offs)]
                slots.append(([base, rot(other, fc)], [n_i, n_j], [0, 0], [9, 5])); want.append(near)
    # around the slack of the centroid pre-test (it lets a pair through while centroid distance^2 < threshold + 1): translations,
    # and translations with one corner a pixel further, whose centroid moves by a quarter pixel
    first_pre = len(slots)
    for d in (-2, -1, 0, 1, 2):
        for dx, dy in ((8, 0), (0, 8), (7, 4), (6, 5), (8, 1), (5, 6)):
            for bump in ((0, 0), (1, 0), (0, 1)):
                other = shift(base, dx, dy + d)
                other[2] = (other[2][0] + bump[0], other[2][1] + bump[1])
                slots.append(([base, other], [64, 64], [0, 0], [9, 5])); want.append(None)
    got = []
    for i in range(0, len(slots), small.batch):
        got += check_assemble(small, slots[i:i + small.batch], t)
    for g, w in zip(got, want):
        if w is not None:
            assert (len(g) == 1) == w
    t["pair below the limit"] = sum(w is True for w in want); t["pair on or above the limit"] = sum(w is False for w in want)
    for (q, _, _, _), g in zip(slots[first_pre:], got[first_pre:]):
        cd2 = sum(Fraction(sum(p[k] for p in q[0]) - sum(p[k] for p in q[1]), 4) ** 2 for k in (0, 1))
        if cd2 < 64:
            t["pretest passes" + (", near" if g else ", not near")] += 1
        elif cd2 < 65:
            assert not g                                                 # the mean squared corner distance is at least cd2
            t["pretest passes in its slack, not near"] += 1
        elif cd2 <= 66:
            t["pretest rejects within one of its limit"] += 1
    need(t, pair_below_the_limit=12, pair_on_or_above_the_limit=24, near_pairs=14, pretest_passes__near=4,
         pretest_passes_in_its_slack__not_near=4, pretest_rejects_within_one_of_its_limit=4)


def test_sequential_marking(small):
    """chains and stars whose outcome depends on the visiting order and on earlier removals; random clustered sets"""
    small.rates(marker=1 / 8)
    t = collections.Counter()
    slots = []
    for sizes in ([80, 72, 64, 72, 80, 64], [64, 72, 80, 88, 96, 104], [104, 96, 88, 80, 72, 64], [64] * 6, [80, 64, 80, 64, 80, 64]):
        for perm_seed in range(3):
            ks = np.random.default_rng(perm_seed).permutation(6).tolist()
            slots.append(([square(20 + 5 * i, 20, 30) for i in range(6)], sizes, [0] * 6, ks))                    # a chain A~B~C~...
            slots.append(([square(60, 60, 30)] + [square(60 + dx, 60 + dy, 30) for dx, dy in ((5, 0), (-5, 0), (0, 5), (0, -5), (4, 4))],
                          sizes, [0] * 6, ks))                                                                   # a star
    rng = np.random.default_rng(21)
    for C in (2, 3, 7, 40, 150, 300):
        centres = rng.integers(20, 120, (max(C // 6, 1), 2))
        q = [square(*(centres[i % len(centres)] + rng.integers(-4, 5, 2)).tolist(), 24) for i in range(C)]
        slots.append((q, rng.choice([64, 72, 80], C).tolist(), rng.integers(0, 3, C).tolist(), rng.permutation(C).tolist()))
    for i in range(0, len(slots), small.batch):
        check_assemble(small, slots[i:i + small.batch], t)
    need(t, near_pairs=500, kept=60)


def enumeration_pairs(C):
    """the pairs at the seams of k_assemble's enumeration (candidate a against the next (C - 1) / 2 in cyclic order, and for even C
    the first half against the one opposite), by kind"""
    half = (C - 1) // 2
    kinds = {"wrap": [(0, C - 1)] if C >= 2 else [],
             "opposite": [(a, a + C // 2) for a in sorted({0, 1, C // 2 - 1}) if C % 2 == 0 and C >= 4 and 0 <= a < C // 2],
             "farthest": [(a, a + half) for a in sorted({0, 2, C - 1 - half}) if half >= 1 and 0 <= a and a + half < C],
             "farthest wrapped": [(a + half - C, a) for a in sorted({C - 1, C - half}) if half >= 1 and 0 <= a + half - C < a < C],
             "adjacent": [(a, a + 1) for a in sorted({0, C // 2, C - 2}) if 0 <= a and a + 1 < C]}
    return {k: sorted(set(v)) for k, v in kinds.items()}


def test_pair_enumeration(small):
    """every C around the even / odd split of the cyclic enumeration, one near pair at each of its seams, all other candidates far from
    everything: a pair the kernel misses leaves one candidate too many, and the kept list is compared with oracle and reference"""
    small.rates(marker=1 / 8)
    t = collections.Counter()
    for C in (0, 1, 2, 3, 4, 5, 64, 65, 1023, 1024, 2047, 2048):
        # fillers: one square at C distinct places with 8 points each: threshold (8 / 8)^2 = 1, and two different translations of one
        # square are a mean squared distance of at least 1 apart: never near
        fill = [square(5 + 2 * (i % 64), 5 + 2 * (i // 64), 10) for i in range(C)]
        kinds = enumeration_pairs(C)
        todo = sorted({p for v in kinds.values() for p in v})
        if C >= 2:
            assert (0, C - 1) in todo
        if C >= 4 and C % 2 == 0:
            assert any(b - a == C // 2 for a, b in todo)
        if C >= 3:
            assert any(b - a == (C - 1) // 2 for a, b in todo)
        slots, planted = [], []
        while todo or not slots:                                         # pairs with disjoint indices share a slot
            used, here = set(), []
            for p in list(todo):
                if not used & set(p):
                    used |= set(p); here.append(p); todo.remove(p)
            quads, sizes = list(fill), [8] * C
            for k, (a, b) in enumerate(here):                            # 64 points each, one pixel apart, away from the fillers and each other
                quads[a] = square(300 + 40 * k, 300, 20); quads[b] = shift(quads[a], 1, 0)
                sizes[a] = sizes[b] = 64
            slots.append((quads, sizes, [0] * C, list(range(C - 1, -1, -1))))
            planted.append(here)
        for i in range(0, len(slots), small.batch):
            for here, near in zip(planted[i:i + small.batch], check_assemble(small, slots[i:i + small.batch], t)):
                assert sorted(near) == sorted(here), "the reference's near pairs are the planted ones and no others"
                for kind, v in kinds.items():
                    t["pair " + kind] += sum(p in near for p in v if p in here)
        t["C %d" % C] += 1
    need(t, C_0=1, C_1=1, C_2=1, C_3=1, C_4=1, C_5=1, C_64=1, C_65=1, C_1023=1, C_1024=1, C_2047=1, C_2048=1,
         pair_wrap=10, pair_opposite=2 + 3 * 3, pair_farthest=9, pair_farthest_wrapped=8, pair_adjacent=10)


def test_pair_capacity(small):
    """91 identical candidates are 4095 near pairs, with one more pair 4096: handled; 4097: reported"""
    small.rates(marker=1 / 8)
    t = collections.Counter()

    def group(n, extra, lone=0):
        q = [square(60, 60, 30)] * n + [square(150, 20, 30)] * 2 * extra + [square(150, 100, 30)] * 2 * (extra > 1) + [square(20, 100, 30)] * lone
        return q, [64] * len(q), [0] * len(q), list(range(len(q)))
    # (a pair the enumeration visits twice would be counted twice: 4096 pairs without an overflow report says none is, for odd and even C)
    for lone in (0, 1):
        near = check_assemble(small, [group(91, 0, lone)], t)[0]
        assert len(near) == PAIR_MAX - 1
        near = check_assemble(small, [group(91, 1, lone)], t)[0]
        assert len(near) == PAIR_MAX
        REACHED["pair list full, %s C" % ("even" if lone else "odd")] += 1
    q, n, s, k = group(91, 2)
    small.ctx.inject_quads(0, q, n, s, k)
    with pytest.raises(capi.AslamError) as e:
        small.ctx.run_quads(0, 1, 2)
    assert e.value.code == -4
    REACHED["pair list full"] += 1
    REACHED["pair list overflow reported"] += 1


# ---- both kernels ---------------------------------------------------------------------------------------------------------------

def test_scenes(small):
    """random projective squares with nested outlines at three scales, default rates, a batch of slots"""
    small.rates()
    t = collections.Counter()
    slots = []
    for s in range(small.batch):
        c, sc = scene(np.random.default_rng(100 + s), small.rows, small.cols, 24)
        slots.append((c, sc, np.random.default_rng(s).permutation(len(c)).tolist()))
    ambiguity_of_reference(small, slots, t)
    check_quads(small, slots, t, stages=3)
    need(t, contours=8 * 200, quads=1000, near_pairs=300, reference_alone_first=1)


@pytest.mark.gpu
def test_scenes_full_grid():
    """the default number of wavefronts, 64 slots of 2000 contours and more: grabs of 4, candidates appended by many wavefronts at once"""
    rig = Rig(480, 640, 64, waves=0).rates()
    t = collections.Counter()
    slots = []
    for s in range(rig.batch):
        rng = np.random.default_rng(500 + s)
        c, sc = scene(rng, rig.rows, rig.cols, 90, lo=10, hi=40)        # 9 outlines per marker: near pairs stay below kPairMax
        for i in range(2000 - len(c) + 40):                              # and polygons that are no quads, to 2000 contours and more
            k = (3, 8, 12)[i % 3]
            r, cx, cy, ph = rng.uniform(8, 14), rng.uniform(20, rig.cols - 20), rng.uniform(20, rig.rows - 20), rng.uniform(0, 6.28)
            c.append(outline([(int(round(cx + r * np.cos(2 * np.pi * j / k + ph))), int(round(cy + r * np.sin(2 * np.pi * j / k + ph)))) for j in range(k)]))
            sc.append(i % 3)
        assert len(c) >= 2000
        slots.append((c, sc, np.random.default_rng(s).permutation(len(c)).tolist()))
    check_quads(rig, slots, t, stages=3, ref=False)
    c, sc, k = slots[0]
    check_quads(rig, [(c, sc, k)], t, stages=3)                          # one slot against the reference as well
    need(t, quads=65 * 600, contours=2000)


# ---- the hooks refuse what the device relies on -----------------------------------------------------------------------------------

def test_hook_refusals():
    ctx = capi.Context(max_rows=64, max_cols=80, max_batch=2, persistent_waves=4, max_landmarks=16, cap_contours_per_frame=8, cap_points_per_frame=100)
    sq = square(10, 10, 5)

    def refused(code, fn, *a):
        with pytest.raises(capi.AslamError) as e:
            fn(*a)
        assert e.value.code == code, e.value

    refused(-5, ctx.inject_contours, 0, [sq], [0], [1])                   # no frame staged
    refused(-5, ctx.inject_quads, 0, [sq], [10], [0], [1])
    refused(-5, ctx.run_quads, 0, 1, 1)
    ctx.stage_frames(np.zeros((1, 64, 80), np.uint8), 0)
    refused(-5, ctx.run_quads, 0, 2, 1)                                   # slot 1 holds no frame
    refused(-5, ctx.inject_contours, 1, [sq], [0], [1])
    refused(-1, ctx.inject_contours, 2, [sq], [0], [1])                   # slot range
    refused(-1, ctx.run_quads, 0, 0, 1)
    for stages in (0, 4, -1):
        refused(-1, ctx.run_quads, 0, 1, stages)
    ok = lambda: ctx.inject_contours(0, [sq, sq], [0, 1], [1, 1])
    ok()
    refused(-1, ctx.inject_contours, 0, [sq] * 9, [0] * 9, list(range(9)))                 # cap_contours
    refused(-1, ctx.inject_contours, 0, [sq * 13, sq * 13], [0, 0], [1, 2])                # cap_points (104 > 100)
    ctx.inject_contours(0, [sq * 25], [0], [1])                                            # exactly cap_points
    refused(-1, ctx.inject_contours, 0, [sq, sq], [0, 0], [1, 1])                          # (scale, key) twice
    refused(-1, ctx.inject_contours, 0, [sq], [3], [1])                                    # scale
    refused(-1, ctx.inject_contours, 0, [sq], [-1], [1])
    refused(-1, ctx.inject_contours, 0, [sq], [0], [-1])                                   # key
    refused(-1, ctx.inject_contours, 0, [sq], [0], [64 * 80 + 1])
    ctx.inject_contours(0, [sq], [0], [64 * 80])
    for bad in ((16384, 0), (0, 16384), (-16385, 0), (0, -16385)):
        refused(-1, ctx.inject_contours, 0, [[bad] + sq], [0], [1])
        refused(-1, ctx.inject_quads, 0, [[bad] + sq[1:]], [10], [0], [1])
    ctx.inject_contours(0, [[(16383, -16384)] + sq], [0], [1])
    ctx.set_detector_params(adaptiveThreshWinSizeMin=3, adaptiveThreshWinSizeMax=3)         # one window in force
    refused(-1, ctx.inject_contours, 0, [sq], [1], [1])
    refused(-1, ctx.inject_quads, 0, [sq], [10], [1], [1])
    ctx.set_detector_params()
    # a size of 0 or beyond 65534 cannot be stated through the Python wrapper's point lists for contours: go through the C entry
    import ctypes as C
    z = np.zeros(4, np.int32); one = np.ones(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for size in (0, 65535, -3):
        sz = np.array([size], np.int32)
        assert ctx.lib.aslam_debug_inject_contours(ctx.h, 0, 1, p(z), p(one), p(sz), p(np.zeros(2 * 70000, np.int32))) == -1
        refused(-1, ctx.inject_quads, 0, [sq], [size], [0], [1])
    refused(-1, ctx.inject_quads, 0, [sq] * 2049, [10] * 2049, [0] * 2049, list(range(2049)))
    refused(-1, ctx.inject_quads, 0, [sq, sq], [10, 10], [2, 2], [4, 4])
    refused(-1, ctx.inject_quads, 0, [sq], [10], [0], [64 * 80 + 1])
    assert ctx.lib.aslam_debug_inject_contours(ctx.h, 0, -1, None, None, None, None) == -1
    assert ctx.lib.aslam_debug_inject_contours(ctx.h, 0, 1, None, None, None, None) == -1
    assert ctx.lib.aslam_debug_inject_quads(ctx.h, 0, 1, None, None, None, None) == -1
    ctx.inject_contours(0, [], [], [])
    ctx.inject_quads(0, np.zeros((0, 4, 2)), [], [], [])
    ctx.run_quads(0, 1, 3)
    assert len(ctx.debug_candidates(0, 2)[1]) == 0
    REACHED["refusals"] += 1
