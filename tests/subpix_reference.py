"""cv::cornerSubPix restated from its definition in numpy.longdouble, and analytic test images for it.

One iteration moves a point c to the least-squares intersection of the gradient-orthogonal lines of a (2 win + 1)^2 window around it:
with g = (gx, gy) the central-difference gradient of the bilinearly interpolated image at window offset p = (px, py) and m the
window weight, solve  sum(m g g^T) (q - c) = sum(m g g^T p)  for q.  The interpolated patch has (w + 2)^2 samples, w = 2 win + 1, and
its first sample lies at c - (w + 1) / 2.  Every sample here is a direct four-tap bilinear evaluation on border-replicated pixels:
there is no running term carried along a row and no separate formula for patches inside the image.  One thing is kept from the
implementation because it changes the result and not just its rounding: a patch that lies inside the image (0 <= ipx,
ipx + w + 2 < cols, the same in y) takes its horizontal fraction as at least 0.0001f.  The window weights are float32 values,
exp(-y^2) exp(-x^2) with x, y = offset / win, built as aslam_set_detector_params documents; the sums, the determinant and the
new point are long double.

iterate() applies the step with cornerSubPix's stopping rules (points are float32 between steps) and reports which rule ended the
point; the images (corner_l, corner_x, edge, flat, square) are closed-form Gaussian-blurred shapes sampled to uint8."""
import math

import numpy as np

LD = np.longdouble
A_MIN = LD(np.float32(0.0001))
DET_MIN = LD(np.finfo(np.float64).eps) ** 2
_erf = np.vectorize(math.erf, otypes=[np.float64])


def window_weights(win):
    """the (2 win + 1)^2 float32 weights: (float)(expf(-y y) * expf(-x x)), x and y = (float)offset / win"""
    w = 2 * win + 1
    v = np.zeros(w, np.float32)
    for i in range(w):
        t = np.float32(i - win) / np.float32(win)
        v[i] = np.float32(math.exp(float(-t * t)))
    return (v[:, None] * v[None, :]).astype(np.float32)


def patch(img, cx, cy, win):
    """the (w + 2)^2 interpolated samples around (cx, cy) and whether the patch took the inside-the-image form"""
    rows, cols = img.shape
    n = 2 * win + 3
    ox, oy = LD(cx) - LD(n - 1) / 2, LD(cy) - LD(n - 1) / 2
    ix, iy = int(np.floor(ox)), int(np.floor(oy))
    a, b = ox - ix, oy - iy
    inside = 0 <= ix and ix + n < cols and 0 <= iy and iy + n < rows
    if inside:
        a = max(a, A_MIN)
    x0 = np.clip(ix + np.arange(n), 0, cols - 1); x1 = np.clip(ix + 1 + np.arange(n), 0, cols - 1)
    y0 = np.clip(iy + np.arange(n), 0, rows - 1); y1 = np.clip(iy + 1 + np.arange(n), 0, rows - 1)
    I = img.astype(LD)
    top = I[np.ix_(y0, x0)] * (1 - a) + I[np.ix_(y0, x1)] * a
    bot = I[np.ix_(y1, x0)] * (1 - a) + I[np.ix_(y1, x1)] * a
    return top * (1 - b) + bot * b, inside


def step(img, cx, cy, win):
    """one iteration from (cx, cy): (new x, new y, det, a * c, inside); new x = new y = None when |det| <= DBL_EPSILON^2"""
    P, inside = patch(img, cx, cy, win)
    w = 2 * win + 1
    gx = P[1:w + 1, 2:w + 2] - P[1:w + 1, 0:w]
    gy = P[2:w + 2, 1:w + 1] - P[0:w, 1:w + 1]
    m = window_weights(win).astype(LD)
    off = np.arange(w, dtype=LD) - win
    px, py = off[None, :], off[:, None]
    sxx, sxy, syy = np.sum(m * gx * gx), np.sum(m * gx * gy), np.sum(m * gy * gy)
    rx, ry = np.sum(m * (gx * gx * px + gx * gy * py)), np.sum(m * (gx * gy * px + gy * gy * py))
    det = sxx * syy - sxy * sxy
    if abs(det) <= DET_MIN:
        return None, None, det, sxx * syy, inside
    return LD(cx) + (syy * rx - sxy * ry) / det, LD(cy) + (sxx * ry - sxy * rx) / det, det, sxx * syy, inside


def iterate(img, x, y, win, max_iter, eps):
    """cornerSubPix on one point.  Returns a dict: x, y (float32), end ('det', 'left', 'cap' or 'eps'), iters (steps taken), reset (the
    final point lay more than win from the start and the start was kept), inside (per step), shift (max |final - start| before the
    reset rule, long double), err_margin (the smallest |err / eps^2 - 1| over the steps that tested it)"""
    rows, cols = img.shape
    max_iter = min(max(int(max_iter), 1), 100)
    eps2 = LD(max(eps, 0.0)) ** 2
    x0, y0 = np.float32(x), np.float32(y)
    cx, cy = x0, y0
    inside, margin, it, end = [], math.inf, 0, None
    while True:
        nx, ny, det, _, ins = step(img, cx, cy, win)
        inside.append(ins)
        if nx is None:
            end = "det"
            break
        nx, ny = np.float32(nx), np.float32(ny)
        err = (LD(nx) - LD(cx)) ** 2 + (LD(ny) - LD(cy)) ** 2
        cx, cy = nx, ny
        it += 1
        if cx < 0 or cx >= cols or cy < 0 or cy >= rows:
            end = "left"
            break
        if it >= max_iter:
            end = "cap"
            break
        if eps2 > 0:
            margin = min(margin, float(abs(err / eps2 - 1)))
        if not err > eps2:
            end = "eps"
            break
    shift = max(abs(LD(cx) - LD(x0)), abs(LD(cy) - LD(y0)))
    reset = bool(shift > win)
    if reset:
        cx, cy = x0, y0
    return dict(x=cx, y=cy, end=end, iters=it, reset=reset, inside=inside, shift=shift, err_margin=margin)


# ---- analytic images ---------------------------------------------------------------------------------------------------------------

def _phi(t):
    return 0.5 * (1.0 + _erf(np.asarray(t, np.float64) / math.sqrt(2.0)))


def _uv(rows, cols, x0, y0, angle):
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    c, s = math.cos(angle), math.sin(angle)
    return c * (xx - x0) + s * (yy - y0), -s * (xx - x0) + c * (yy - y0)


def _u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def corner_l(rows, cols, x0, y0, angle, sigma=1.0, lo=40.0, hi=210.0):
    """one dark quadrant with its apex at (x0, y0), turned by angle, blurred by a Gaussian of width sigma: the blur of an indicator of
    {u > 0, v > 0} in turned coordinates is Phi(u / sigma) Phi(v / sigma)"""
    u, v = _uv(rows, cols, x0, y0, angle)
    return _u8(hi - (hi - lo) * _phi(u / sigma) * _phi(v / sigma))


def corner_x(rows, cols, x0, y0, angle, sigma=1.0, lo=40.0, hi=210.0):
    """a checker saddle: the blur of sign(u) sign(v) is erf(u / (sigma sqrt 2)) erf(v / (sigma sqrt 2))"""
    u, v = _uv(rows, cols, x0, y0, angle)
    return _u8(0.5 * (hi + lo) + 0.5 * (hi - lo) * (2 * _phi(u / sigma) - 1) * (2 * _phi(v / sigma) - 1))


def edge(rows, cols, x0, y0, angle, sigma=1.0, lo=40.0, hi=210.0):
    """a straight blurred edge through (x0, y0): every gradient is parallel to one direction"""
    u, _ = _uv(rows, cols, x0, y0, angle)
    return _u8(hi - (hi - lo) * _phi(u / sigma))


def flat(rows, cols, value=128):
    return np.full((rows, cols), value, np.uint8)


def square(rows, cols, x0, y0, side, angle, sigma=1.0, lo=40.0, hi=210.0, base=None):
    """a dark square (first corner (x0, y0), sides along the turned axes) on `base` or a bright frame; its corners, in order"""
    u, v = _uv(rows, cols, x0, y0, angle)
    inside = (_phi(u / sigma) - _phi((u - side) / sigma)) * (_phi(v / sigma) - _phi((v - side) / sigma))
    bg = np.full((rows, cols), hi) if base is None else base.astype(np.float64)
    c, s = math.cos(angle), math.sin(angle)
    corners = np.array([[x0, y0], [x0 + side * c, y0 + side * s], [x0 + side * (c - s), y0 + side * (s + c)], [x0 - side * s, y0 + side * c]])
    return _u8(bg - (bg - lo) * inside), corners


def tiled_saddles(rows, cols, pitch, rng, sigma=0.7):
    """a frame cut into pitch x pitch tiles, each holding its own checker saddle (own sub-pixel centre, angle and contrast); the tile
    centres as a (tile rows, tile cols, 2) array of x, y"""
    tr, tc = rows // pitch, cols // pitch
    img = np.full((rows, cols), 128.0)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ty, tx = np.minimum(yy // pitch, tr - 1).astype(int), np.minimum(xx // pitch, tc - 1).astype(int)
    cx = (np.arange(tc) + 0.5) * pitch - 0.5 + rng.uniform(-0.4, 0.4, (tr, tc))
    cy = (np.arange(tr)[:, None] + 0.5) * pitch - 0.5 + rng.uniform(-0.4, 0.4, (tr, tc))
    ang = rng.uniform(0, math.pi, (tr, tc))
    amp = rng.uniform(40, 100, (tr, tc))
    c, s = np.cos(ang[ty, tx]), np.sin(ang[ty, tx])
    dx, dy = xx - cx[ty, tx], yy - cy[ty, tx]
    u, v = c * dx + s * dy, -s * dx + c * dy
    img = 128.0 + amp[ty, tx] * (2 * _phi(u / sigma) - 1) * (2 * _phi(v / sigma) - 1)
    return _u8(img), np.stack([cx, cy], -1)


def weak_cross(rows, cols, x0, y0, angle, sigma=2.0, weak=8.0, lo=40.0, hi=210.0):
    """a strong blurred edge through (x0, y0) crossed at right angles by one of only `weak` grey levels: the normal matrix is far from
    singular in exact arithmetic but nearly rank one, and the iteration hops along the strong edge for many steps"""
    u, v = _uv(rows, cols, x0, y0, angle)
    return _u8(hi - (hi - lo) * _phi(u / sigma) + weak * _phi(v / sigma))
