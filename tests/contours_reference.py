"""Exact restatement of the front of the detector, for tests/test_contours_kernel.py: bgr8 -> gray, adaptiveThreshold(MEAN_C,
BINARY_INV), findContours(RETR_LIST, CHAIN_APPROX_NONE) as OpenCV 3.2 computes them, and the border nodes of common.h.

Written from the published algorithm (Suzuki & Abe 1985 as OpenCV's contour scanner runs it: a raster scan over an integer image
padded with one background pixel all round, border marks 2 / -2, the outer / hole start rules, point-by-point following) and from
common.h's definitions of nodes and segments; not from oracle/detect.cpp.  Python integers and numpy integer arrays only, except the
second way of rounding the box mean, which is OpenCV's own double arithmetic and must agree with the integer one on every pixel.

Directions d = 0..7: E NE N NW W SW S SE (counter-clockwise on the screen, y down)."""
import collections

import numpy as np

DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)
NONE = 0xFFFFFFFF
CUT, OUTER, HOLE = 0, 1, 2

Border = collections.namedtuple("Border", "hole key start pts dirs")   # pts: (x, y) per point; dirs: the back direction at each point


def bgr2gray(bgr):
    b = bgr.astype(np.int64)
    return ((b[..., 0] * 1868 + b[..., 1] * 9617 + b[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def box_sum(gray, k):
    """sum over the k x k window around every pixel, border replicated: from an integer summed-area table"""
    r = k // 2
    p = np.pad(gray.astype(np.int64), r, mode="edge")
    I = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    I[1:, 1:] = p.cumsum(0).cumsum(1)
    rows, cols = gray.shape
    return I[k:k + rows, k:k + cols] - I[:rows, k:k + cols] - I[k:k + rows, :cols] + I[:rows, :cols]


def threshold(gray, k, C):
    """foreground mask (bool).  The mean is rounded two ways - floor((2 S + k^2) / (2 k^2)) and cvRound(S * (1.0 / k^2)) in double -
    which must agree on every pixel (k^2 is odd: no tie)"""
    assert k % 2 == 1 and k >= 3
    S = box_sum(gray, k)
    k2 = k * k
    mean = (2 * S + k2) // (2 * k2)
    mean_cv = np.rint(S.astype(np.float64) * (1.0 / k2)).astype(np.int64)
    assert np.array_equal(mean, mean_cv), f"window {k}: the two roundings of the mean differ"
    idelta = int(C // 1)                                           # cvFloor
    return gray.astype(np.int64) - mean <= -idelta


def windows_of(win_min=3, win_max=23, step=10):
    n = (win_max - win_min) // step + 1
    return [w + 1 if w % 2 == 0 else w for w in (win_min + i * step for i in range(n))]


def perim_limits(rows, cols, min_rate=0.03, max_rate=4.0):
    return int(min_rate * max(rows, cols)), int(max_rate * max(rows, cols))


def masks(fg):
    """bit d of a pixel's mask: its neighbour in direction d is foreground (beyond the frame: background)"""
    rows, cols = fg.shape
    p = np.pad(fg.astype(np.uint8), 1)
    m = np.zeros((rows, cols), np.int64)
    for d in range(8):
        m |= p[1 + DY[d]:1 + DY[d] + rows, 1 + DX[d]:1 + DX[d] + cols].astype(np.int64) << d
    return m


# ---- border following --------------------------------------------------------------------------------
def _follow(img, x, y, hole):
    s_end = s = 0 if hole else 4
    while True:
        s = (s - 1) & 7
        if img[y + DY[s]][x + DX[s]] != 0:
            break
        if s == s_end:
            break
    if s == s_end:                                                  # a single pixel
        img[y][x] = -2
        return [(x, y)], [s]
    x1, y1 = x + DX[s], y + DY[s]
    cx, cy = x, y
    pts, dirs = [], []
    while True:
        s_end = s
        dirs.append(s)
        while True:
            s += 1
            nx, ny = cx + DX[s & 7], cy + DY[s & 7]
            if img[ny][nx] != 0:
                break
        s &= 7
        if s != 0 and s - 1 < s_end:                                # the east neighbour was examined and is background
            img[cy][cx] = -2
        elif img[cy][cx] == 1:
            img[cy][cx] = 2
        pts.append((cx, cy))
        if (nx, ny) == (x, y) and (cx, cy) == (x1, y1):
            break
        cx, cy = nx, ny
        s = (s + 4) & 7
    return pts, dirs


def find_borders(fg):
    """all borders in scan order: Border(hole, key = raster position of the scan when it found the border, start pixel, points, back
    directions)"""
    rows, cols = fg.shape
    img = np.pad(fg.astype(np.int64), 1).tolist()
    out = []
    for y in range(1, rows + 1):
        row = img[y]
        prev = 0
        for x in range(1, cols + 2):
            p = row[x]
            if p != prev:
                hole = 0 if (prev == 0 and p == 1) else 1 if (p == 0 and prev >= 1) else None
                if hole is not None:
                    pts, dirs = _follow(img, x - hole, y, hole)
                    out.append(Border(hole, (y - 1) * cols + (x - 1), (x - hole - 1, y - 1), [(a - 1, b - 1) for a, b in pts], dirs))
                    p = row[x]
            prev = p
    return out


def shoelace(pts):
    n = len(pts)
    return sum(pts[i][0] * pts[(i + 1) % n][1] - pts[(i + 1) % n][0] * pts[i][1] for i in range(n))


# ---- independent invariants ----------------------------------------------------------------------------
def _components(mask, conn8):
    """sizes and touches-the-frame flags of the connected components of a bool array (plain flood fill)"""
    rows, cols = mask.shape
    seen = (~mask).tolist()
    nb = [(1, 0), (-1, 0), (0, 1), (0, -1)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if conn8 else [])
    out = []
    for y0 in range(rows):
        r0 = seen[y0]
        for x0 in range(cols):
            if r0[x0]:
                continue
            r0[x0] = True
            stack = [(x0, y0)]
            size, edge = 0, False
            while stack:
                x, y = stack.pop()
                size += 1
                edge = edge or x == 0 or y == 0 or x == cols - 1 or y == rows - 1
                for dx, dy in nb:
                    u, v = x + dx, y + dy
                    if 0 <= u < cols and 0 <= v < rows and not seen[v][u]:
                        seen[v][u] = True
                        stack.append((u, v))
            out.append((size, edge))
    return out


def check_invariants(fg, borders):
    """the reference against facts that need no border following"""
    fgc = _components(fg, True)
    bgc = _components(~fg, False)
    outer = [b for b in borders if not b.hole]
    holes = [b for b in borders if b.hole]
    assert sum(len(b.pts) > 1 for b in outer) == sum(s > 1 for s, _ in fgc), "outer borders != 8-connected components of more than one pixel"
    assert sum(len(b.pts) == 1 for b in outer) == sum(s == 1 for s, _ in fgc), "one-point borders != single pixels"
    assert len(holes) == sum(not e for _, e in bgc), "hole borders != 4-connected background components off the frame"
    keys = [b.key for b in borders]
    assert keys == sorted(keys) and len(set(keys)) == len(keys), "keys are not strictly increasing in scan order"
    for b in borders:
        n = len(b.pts)
        assert all(fg[y, x] for x, y in b.pts), "a border point is background"
        assert b.pts[0] == b.start
        for i in range(n):
            (x, y), (u, v) = b.pts[i], b.pts[(i + 1) % n]
            assert n == 1 or (max(abs(x - u), abs(y - v)) == 1), "consecutive points are not 8-neighbours (or the cycle does not close)"
        a = shoelace(b.pts)
        assert (a > 0) if b.hole else (a <= 0), "orientation: outer borders run counter-clockwise on screen, holes the other way"


# ---- border nodes (common.h) ---------------------------------------------------------------------------
def first_outer(m):
    return next(s for s in (0, 7, 6, 5) if (m >> s) & 1)


def first_hole(m):
    return next(s for s in (7, 6, 5, 4, 3, 2, 1) if (m >> s) & 1)


def step(m, s):
    """one border-following step from back direction s on a pixel with mask m: (dx, dy, new back direction)"""
    for k in range(1, 9):
        d = (s + k) & 7
        if (m >> d) & 1:
            return DX[d], DY[d], (d + 4) & 7
    raise AssertionError("isolated pixel")


def pack(x, y, s, scale, typ):
    return x | (y << 12) | (s << 24) | (scale << 27) | (typ << 29)


def nodes_of(fg, m, pitch):
    """{(x, y, s): type} - the start candidates of either type and the cut states on lattice pixels"""
    out = {}
    ys, xs = np.nonzero(fg)
    ml = m.tolist()
    for x, y in zip(xs.tolist(), ys.tolist()):
        mm = ml[y][x]
        if mm != 0 and (mm & 0x1E) == 0:
            out[(x, y, first_outer(mm))] = OUTER
        elif (mm & 3) == 2:
            out[(x, y, first_hole(mm))] = HOLE
        if x % pitch == 0 or y % pitch == 0:
            for s in range(8):
                if (mm >> s) & 1 and not (mm >> ((s + 1) & 7)) & 1:
                    out.setdefault((x, y, s), CUT)
    return out


def segments_of(m, nodes, max_perim):
    """{state: (next state or None when the walk exceeds max_perim, steps, shoelace partial sum)}"""
    ml = m.tolist()
    out = {}
    for (x0, y0, s0) in nodes:
        x, y, s, n, a = x0, y0, s0, 0, 0
        while True:
            dx, dy, s2 = step(ml[y][x], s)
            a += x * dy - dx * y
            x, y, s = x + dx, y + dy, s2
            n += 1
            if n > max_perim:                                       # no kept border is that long: cut, whatever stands here
                out[(x0, y0, s0)] = (None, n, a)
                break
            if (x, y, s) in nodes:
                out[(x0, y0, s0)] = ((x, y, s), n, a)
                break
    return out


def count_nodes(gray, windows, C, pitch):
    """the number of nodes of a frame, all scales together (no border following: for sizing images)"""
    n = 0
    for k in windows:
        fg = threshold(gray, k, C)
        n += len(nodes_of(fg, masks(fg), pitch))
    return n


class Scale:
    pass


class Frame:
    """everything the reference says about one gray frame; checked against the invariants on construction"""

    def __init__(self, gray, windows=(3, 13, 23), C=7.0, min_perim=None, max_perim=None):
        gray = np.ascontiguousarray(gray, np.uint8)
        self.gray, self.windows = gray, tuple(windows)
        self.rows, self.cols = gray.shape
        lo, hi = perim_limits(self.rows, self.cols)
        self.min_perim = lo if min_perim is None else min_perim
        self.max_perim = hi if max_perim is None else max_perim
        self.scales = []
        for k in self.windows:
            sc = Scale()
            sc.fg = threshold(gray, k, C)
            sc.m = masks(sc.fg)
            sc.borders = find_borders(sc.fg)
            check_invariants(sc.fg, sc.borders)
            # what the detector keeps; a single pixel has no border state (and its one point can never make a quad)
            sc.kept = [b for b in sc.borders if self.min_perim <= len(b.pts) <= self.max_perim and len(b.pts) > 1]
            sc.kept.sort(key=lambda b: -b.key)                     # OpenCV's output order: reverse discovery
            self.scales.append(sc)
        self._nodes = {}

    def nodes(self, pitch):
        """per scale: ({state: type}, {state: (next, steps, area)})"""
        if pitch not in self._nodes:
            res = []
            for sc in self.scales:
                nd = nodes_of(sc.fg, sc.m, pitch)
                res.append((nd, segments_of(sc.m, nd, self.max_perim)))
            self._nodes[pitch] = res
        return self._nodes[pitch]

    def counts(self, pitch=None):
        d = dict(contours=sum(len(sc.kept) for sc in self.scales), points=sum(len(b.pts) for sc in self.scales for b in sc.kept))
        if pitch:
            d["nodes"] = sum(len(nd) for nd, _ in self.nodes(pitch))
        return d

    def tile_nodes(self, pitch, tw=64, th=32):
        """nodes per 64 x 32 tile of the threshold kernel, all scales together"""
        c = collections.Counter()
        for nd, _ in self.nodes(pitch):
            for (x, y, _s) in nd:
                c[(x // tw, y // th)] += 1
        return c
