"""Exact restatement of the quad and candidate-assembly stages of cv::aruco::detectMarkers (OpenCV 3.2), for
tests/test_quads_kernel.py.

Written from the OpenCV sources as specification - imgproc/approx.cpp::approxPolyDP_ (closed integer curves),
imgproc/convhull.cpp::isContourConvex_, aruco.cpp::_findMarkerContours, _reorderCandidatesCorners, _filterTooCloseCandidates and the
joining order of _detectInitialCandidates - and on purpose not shaped like oracle/detect.cpp or detect.hip: the Douglas-Peucker
phase is a recursion that returns vertex indices (no slice stack), the clean-up pass reads through a closure over a Python list,
convexity is "all four turns strictly the same way", and the filter compares integer sums.

Arithmetic: every squared distance, cross product and inner product is a Python integer.  Every comparison that involves a rate
is made between exact rationals (fractions.Fraction, the rate taken at its exact double value).  OpenCV makes those comparisons
in double, and that evaluation is the specification; so each such comparison also evaluates the rate side in double, the way
OpenCV writes it, and reports the decision as *ambiguous* when that double is not the exact value and the two sides lie within a
relative 2^-40 of each other.  With dyadic rates every product is exact in double and nothing is ever ambiguous.

_filterTooCloseCandidates sums float products of Point2f differences.  For integer corners those are exact while a squared
corner distance stays below 2^24 (differences below 4096); beyond that a pair is far from any threshold a legal contour can have
((65534 * rate)^2 needs rate > 1/16 to reach 2^24), and the tests keep corners within a few thousand pixels.
"""
import sys
from fractions import Fraction

import numpy as np

AMBIG_REL = Fraction(1, 2 ** 40)


class Rated:
    """comparisons against a rate-derived bound, exact, with the ambiguity rule of the module docstring"""

    def __init__(self):
        self.ambiguous = False

    def _note(self, lhs, exact, dbl):
        if Fraction(dbl) != exact or Fraction(float(lhs)) != lhs:
            if abs(lhs - exact) <= AMBIG_REL * max(abs(lhs), abs(exact)):
                self.ambiguous = True

    def le(self, lhs, exact, dbl):
        self._note(lhs, exact, dbl)
        return lhs <= exact

    def lt(self, lhs, exact, dbl):
        self._note(lhs, exact, dbl)
        return lhs < exact


def _d2(a, b):
    return (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2


def approx_closed(pts, rate, trace=None):
    """approxPolyDP(curve, n * rate, closed = true) of a closed list of integer points.
    Returns (vertices, vertices before the clean-up pass, ambiguous).  trace: a dict that receives, under "initial" and "slice",
    the index distances from the winning position of a farthest-point search to every later position that ties with it."""
    pts = [(int(x), int(y)) for x, y in pts]
    n = len(pts)
    cmp = Rated()
    if n == 0:
        return [], 0, False
    eps2 = (n * Fraction(rate)) ** 2            # exact
    eps_d = float(n) * rate                     # "double(n) * rate", then "eps *= eps"
    eps2_d = eps_d * eps_d

    # 1. three rounds of "the farthest point from where I stand", earliest on ties; a round that sees no other point stays
    here = 0
    hop = 0
    flat = False
    for _ in range(3):
        here = (here + hop) % n
        best = 0
        for j in range(1, n):
            d = _d2(pts[(here + j) % n], pts[here])
            if d > best:
                best, hop = d, j
        if trace is not None and best > 0:
            trace.setdefault("initial", set()).update(j - hop for j in range(hop + 1, n) if _d2(pts[(here + j) % n], pts[here]) == best)
        flat = cmp.le(best, eps2, eps2_d)

    # 2./3. Douglas-Peucker between the last stand point and its farthest point, both ways round
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))

    def split(a, b):
        """vertex indices of the open arc a -> b (cyclic), a included, b excluded"""
        if (a + 1) % n == b:
            return [a]
        ax, ay = pts[a]
        dx, dy = pts[b][0] - ax, pts[b][1] - ay
        best, far, ties = 0, None, []
        i = (a + 1) % n
        while i != b:
            d = abs((pts[i][1] - ay) * dx - (pts[i][0] - ax) * dy)
            if d > best:
                best, far, ties = d, i, []
            elif d == best and best > 0:
                ties.append((i - far) % n)
            i = (i + 1) % n
        if trace is not None:
            trace.setdefault("slice", set()).update(ties)
        seg2 = dx * dx + dy * dy
        if cmp.le(best * best, eps2 * seg2, eps2_d * float(seg2)):
            return [a]
        return split(a, far) + split(far, b)

    if flat:
        idx = [here]
    else:
        # a full round of reads ends where it began: the arcs are stand point -> farthest point -> stand point
        far = (here + hop) % n
        idx = split(here, far) + split(far, here)
    dst = [pts[i] for i in idx]
    before = m = len(dst)

    # 4. clean-up, in place as the specification does it (late reads can see slots the pass has already rewritten): walking once
    # round from the last vertex, drop a vertex on the (almost) straight, non-axis-parallel line between its neighbours; a removal
    # takes the next vertex along with it as the new anchor
    rd = [m - 1]

    def read():
        v = dst[rd[0]]
        rd[0] = (rd[0] + 1) % m
        return v

    anchor = read()
    wr = 0
    mid = read()
    left = m
    i = 0
    while i < m and left > 2:
        nxt = read()
        dx, dy = nxt[0] - anchor[0], nxt[1] - anchor[1]
        d = abs((mid[0] - anchor[0]) * dy - (mid[1] - anchor[1]) * dx)
        sip = (mid[0] - anchor[0]) * (nxt[0] - mid[0]) + (mid[1] - anchor[1]) * (nxt[1] - mid[1])
        seg2 = dx * dx + dy * dy
        if cmp.le(d * d, eps2 * seg2 / 2, 0.5 * eps2_d * float(seg2)) and dx != 0 and dy != 0 and sip >= 0:
            left -= 1
            dst[wr] = anchor = nxt
            wr = (wr + 1) % m
            mid = read()
            i += 2
            continue
        dst[wr] = anchor = mid
        wr = (wr + 1) % m
        mid = nxt
        i += 1
    verts = dst[:left]
    return verts, before, cmp.ambiguous


def is_convex4(q):
    """isContourConvex of 4 integer points: every turn strictly the same way"""
    signs = set()
    for i in range(4):
        a, b, c = q[i - 2], q[i - 1], q[i]
        t = (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0])
        signs.add((t > 0) - (t < 0))
    return signs == {1} or signs == {-1}


def first_bad_turn(q):
    """of a quad that is not convex: (step, kind) of the first turn, in isContourConvex's order, that is straight ("zero") or
    goes the other way than a turn before it ("opposite")"""
    seen = 0
    for i in range(4):
        a, b, c = q[i - 2], q[i - 1], q[i]
        t = (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0])
        if t == 0:
            return i, "zero"
        if seen and (t > 0) != (seen > 0):
            return i, "opposite"
        seen = t
    return None


class Params:
    def __init__(self, approx=0.05, corner=0.05, border=3, marker=0.05):
        self.approx, self.corner, self.border, self.marker = float(approx), float(corner), int(border), float(marker)


class QuadResult:
    __slots__ = ("corners", "ambiguous", "dp_vertices", "vertices", "why")


def quad_of_contour(pts, rows, cols, P):
    """the loop body of _findMarkerContours after the perimeter limits"""
    r = QuadResult()
    verts, r.dp_vertices, r.ambiguous = approx_closed(pts, P.approx)
    r.vertices = len(verts)
    r.corners = None
    if len(verts) != 4:
        r.why = "vertices"
        return r
    if not is_convex4(verts):
        r.why = "convex"
        return r
    n = len(pts)
    cmp = Rated()
    side = min([max(cols, rows) ** 2] + [_d2(verts[j], verts[(j + 1) % 4]) for j in range(4)])
    lim_d = float(n) * P.corner
    short = cmp.lt(side, (n * Fraction(P.corner)) ** 2, lim_d * lim_d)
    r.ambiguous = r.ambiguous or cmp.ambiguous
    if short:
        r.why = "corner distance"
        return r
    b = P.border
    if any(x < b or y < b or x > cols - 1 - b or y > rows - 1 - b for x, y in verts):
        r.why = "border"
        return r
    r.why = "quad"
    r.corners = verts
    return r


def initial_candidates(contours, scales, keys, rows, cols, P):
    """_detectInitialCandidates on given contours: scale ascending, inside a scale findContours' order (reverse discovery = key
    descending).  Returns (list of (corners, n, scale, key), per-contour QuadResult in input order)."""
    res = [quad_of_contour(c, rows, cols, P) for c in contours]
    order = sorted(range(len(contours)), key=lambda i: (scales[i], -keys[i]))
    return [(res[i].corners, len(contours[i]), scales[i], keys[i]) for i in order if res[i].corners is not None], res


def reorder_corners(q):
    """_reorderCandidatesCorners of one quad"""
    (x0, y0), (x1, y1), (x2, y2), _ = q
    cross = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    return [q[0], q[3], q[2], q[1]] if cross < 0 else list(q)


def filter_too_close(corners, sizes, rate):
    """_filterTooCloseCandidates.  corners: C x 4 x 2 integers (reordered), sizes: C contour point counts.
    Returns (kept indices, near pairs in visiting order, number of ambiguous pair decisions, pairs decided)."""
    c = np.asarray(corners, np.int64).reshape(-1, 4, 2)
    n = [int(v) for v in sizes]
    C = len(n)
    fr = Fraction(float(rate))
    near, ambiguous, decided = [], 0, 0
    nn = np.asarray(n, np.float64)
    for i in range(C - 1):
        # integer sums of the four squared corner distances under each cyclic shift: exact in int64
        rest = c[i + 1:]
        s4 = np.stack([((c[i][(np.arange(4) + fc) % 4][None] - rest) ** 2).sum(axis=(1, 2)) for fc in range(4)], axis=1)
        # clearly far pairs are settled in bulk: the sums are exact integers below 2^53, and the bound below exceeds the exact
        # threshold 4 (min n rate)^2 by a relative 1e-6, a million times any rounding in it
        lim = 4.0 * (np.minimum(nn[i], nn[i + 1:]) * float(rate)) ** 2
        maybe = np.nonzero(s4.min(axis=1) <= lim * (1 + 1e-6) + 1.0)[0]
        decided += C - 1 - i
        for o in maybe:
            j = i + 1 + int(o)
            m = min(n[i], n[j])
            lim_d = float(m) * float(rate)
            exact = (m * fr) ** 2
            cmp = Rated()
            hit = False
            for fc in range(4):
                if cmp.lt(Fraction(int(s4[o, fc]), 4), exact, lim_d * lim_d):
                    hit = True
                    break
            ambiguous += cmp.ambiguous
            if hit:
                near.append((i, j))
    gone = [False] * C
    for i, j in near:
        if gone[i] or gone[j]:
            continue
        gone[j if n[i] > n[j] else i] = True
    return [i for i in range(C) if not gone[i]], near, ambiguous, decided
