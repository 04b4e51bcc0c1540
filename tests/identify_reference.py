"""An exact restatement of marker identification (OpenCV 3.2 aruco.cpp::_extractBits, _getBorderErrors and
dictionary.cpp::Dictionary::identify), written from the OpenCV sources and independent of both the oracle and the kernels.

  - homography: the 8 x 8 system of getPerspectiveTransform from the float32 corners, solved in exact rationals, and its exact
    inverse; each sample position is then evaluated in long double (64-bit mantissa);
  - ambiguous pixels: an output pixel whose exact source coordinate lies within AMBIGUOUS px of a half-integer, inside or next to
    the frame.  Only there may a correct double-precision warp round either way; everywhere else its nearest pixel is unique;
  - sampling: nearest pixel, round half to even (cvRound); a position outside the frame reads 0 (BORDER_CONSTANT);
  - meanStdDev of the inner region (half a cell off every side): as OpenCV evaluates it (mean, sq * scale - mean^2 in double: the
    specification) and exactly in integers (n sq - sum^2 < n^2 minOtsuStdDev^2);
  - Otsu: the exact between-class criterion (N s0 - S n0)^2 / (n0 (N - n0)) for every split; its arg-max set;
  - cells: a cell is 1 when strictly more than floor(w^2 / 2) of its pixels (margin removed) exceed T;
  - _getBorderErrors, and Dictionary::identify over the four rotations np.rot90(marker, r), r = 0..3 (the lowest marker within
    int(maxCorrectionBits * errorCorrectionRate) wins; per marker the first minimal rotation).
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
EXACT_LD = np.finfo(LD).nmant >= 63          # the module needs an x87-style long double
AMBIGUOUS = 1e-9


def solve_exact(A, b):
    """Gaussian elimination in rationals (any nonzero pivot: the solution is exact)"""
    n = len(b)
    M = [list(A[i]) + [b[i]] for i in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[p] = M[p], M[c]
        for r in range(c + 1, n):
            if M[r][c] != 0:
                f = M[r][c] / M[c][c]
                M[r] = [x - f * y for x, y in zip(M[r], M[c])]
    x = [Fraction(0)] * n
    for i in range(n - 1, -1, -1):
        x[i] = (M[i][n] - sum(M[i][j] * x[j] for j in range(i + 1, n))) / M[i][i]
    return x


def homography(corners, S):
    """exact H (3 x 3 Fractions, H[2][2] = 1) with H (corner k) ~ (0,0), (S-1,0), (S-1,S-1), (0,S-1)"""
    c = np.asarray(corners, np.float32).reshape(4, 2)
    src = [(Fraction(float(x)), Fraction(float(y))) for x, y in c]
    dst = [(0, 0), (S - 1, 0), (S - 1, S - 1), (0, S - 1)]
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A.append([x, y, 1, 0, 0, 0, -x * u, -y * u]); b.append(Fraction(u))
    for (x, y), (u, v) in zip(src, dst):
        A.append([0, 0, 0, x, y, 1, -x * v, -y * v]); b.append(Fraction(v))
    h = solve_exact(A, b)
    return [h[0:3], h[3:6], [h[6], h[7], Fraction(1)]]


def adjugate(H):
    """the inverse of H up to a scale (the scale cancels in the projective division)"""
    (a, b, c), (d, e, f), (g, h, i) = H
    return [[e * i - f * h, c * h - b * i, b * f - c * e],
            [f * g - d * i, a * i - c * g, c * d - a * f],
            [d * h - e * g, b * g - a * h, a * e - b * d]]


def to_ld(q):
    """a Fraction rounded to long double (to within one ulp)"""
    q = Fraction(q)
    if q == 0:
        return LD(0)
    s = -1 if q < 0 else 1
    n, d = abs(q.numerator), q.denominator
    e = n.bit_length() - d.bit_length()
    m = (n << (64 - e)) // d if e <= 64 else n // (d << (e - 64))
    hi, lo = m >> 32, m & 0xFFFFFFFF
    return LD(s) * np.ldexp(LD(hi) * LD(2.0 ** 32) + LD(lo), e - 64)


def source_positions(corners, S):
    """exact-homography source coordinates (X, Y) of every output pixel, S x S long double arrays"""
    Minv = adjugate(homography(corners, S))
    m = [[to_ld(v) for v in row] for row in Minv]
    y, x = np.mgrid[0:S, 0:S]
    x, y = x.astype(LD), y.astype(LD)
    W = m[2][0] * x + m[2][1] * y + m[2][2]
    X = (m[0][0] * x + m[0][1] * y + m[0][2]) / W
    Y = (m[1][0] * x + m[1][1] * y + m[1][2]) / W
    return X, Y


class Result:
    pass


def warp(gray, corners, S):
    """(img S x S uint8, ambiguous S x S bool, outside S x S bool)"""
    rows, cols = gray.shape
    X, Y = source_positions(corners, S)
    near = (X > -2) & (X < cols + 1) & (Y > -2) & (Y < rows + 1)
    amb = near & ((np.abs(X - np.floor(X) - LD(0.5)) < AMBIGUOUS) | (np.abs(Y - np.floor(Y) - LD(0.5)) < AMBIGUOUS))
    big = LD(2.0 ** 40)                                  # far outside any frame: no rounding question, and no int overflow
    Xc, Yc = np.clip(X, -big, big), np.clip(Y, -big, big)
    Xi, Yi = np.rint(Xc).astype(np.int64), np.rint(Yc).astype(np.int64)     # rint: half to even
    inside = (Xi >= 0) & (Xi < cols) & (Yi >= 0) & (Yi < rows)
    img = np.zeros((S, S), np.uint8)
    img[inside] = gray[Yi[inside], Xi[inside]]
    return img, amb, ~inside


def otsu_argmax(img):
    """thresholds t whose split {<= t} / {> t} maximises the exact between-class criterion (empty when no split exists)"""
    h = np.bincount(img.reshape(-1), minlength=256).astype(object)
    N = int(img.size)
    Stot = sum(i * int(h[i]) for i in range(256))
    best, arg = None, []
    n0 = s0 = 0
    for t in range(256):
        n0 += int(h[t]); s0 += t * int(h[t])
        if n0 == 0 or n0 == N:
            continue
        crit = Fraction((N * s0 - Stot * n0) ** 2, n0 * (N - n0))
        if best is None or crit > best:
            best, arg = crit, [t]
        elif crit == best:
            arg.append(t)
    return arg


def cells_of(img, nc, cell, margin, T):
    """nc x nc cell bits: strictly more than floor(w^2 / 2) pixels above T"""
    w = cell - 2 * margin
    out = np.zeros((nc, nc), np.uint8)
    for cy in range(nc):
        for cx in range(nc):
            blk = img[cy * cell + margin: cy * cell + margin + w, cx * cell + margin: cx * cell + margin + w]
            out[cy, cx] = int((blk.astype(np.int64) > T).sum()) > (w * w) // 2
    return out


def border_errors(bits, ms, bb=1):
    n = ms + 2 * bb
    tot = 0
    for y in range(n):
        for k in range(bb):
            tot += int(bits[y, k] != 0) + int(bits[y, n - 1 - k] != 0)
    for x in range(bb, n - bb):
        for k in range(bb):
            tot += int(bits[k, x] != 0) + int(bits[n - 1 - k, x] != 0)
    return tot


def rotations(dict_bits):
    """n x 4 x ms x ms: rotation r of every marker, np.rot90(marker, r) (Dictionary::getByteListFromBits' channel r)"""
    return np.stack([np.stack([np.rot90(b, r) for r in range(4)]) for b in np.asarray(dict_bits, np.uint8)])


def identify_code(code, rots, max_corr):
    """Dictionary::identify: (id, rotation, distance of every marker's best rotation)"""
    d = (rots != np.asarray(code, np.uint8)[None, None]).sum(axis=(2, 3))          # n x 4
    best = d.min(axis=1)
    ok = np.nonzero(best <= max_corr)[0]
    if ok.size == 0:
        return -1, 0, best
    m = int(ok[0])
    return m, int(np.argmax(d[m] == best[m])), best


def identify(gray, corners, ms, rots, max_corr, cell=8, margin_rate=0.13, border_rate=0.35, min_std=5.0, bb=1):
    """everything _identifyOneCandidate decides, exactly; Result fields below"""
    r = Result()
    nc = ms + 2 * bb
    S = nc * cell
    margin = int(margin_rate * cell)
    img, amb, outside = warp(np.asarray(gray, np.uint8), corners, S)
    r.img, r.ambiguous, r.n_ambiguous, r.n_outside = img, bool(amb.any()), int(amb.sum()), int(outside.sum())
    lo, hi = cell // 2, S - cell // 2
    inner = img[lo:hi, lo:hi].astype(np.int64)
    n = int(inner.size)
    r.sum, r.sq = int(inner.sum()), int((inner * inner).sum())
    # the specification: OpenCV's double evaluation
    scale = 1.0 / (float(hi - lo) * (hi - lo))
    mean = r.sum * scale
    var = max(r.sq * scale - mean * mean, 0.0)
    uniform_double = float(np.sqrt(var)) < min_std
    uniform_exact = n * r.sq - r.sum * r.sum < Fraction(n * n) * Fraction(min_std) ** 2
    r.std_forms_disagree = uniform_double != uniform_exact
    r.stddev_exact_sq = Fraction(n * r.sq - r.sum * r.sum, n * n)
    r.mean_exact = Fraction(r.sum, n)
    r.otsu_set = []
    if uniform_double:
        r.branch = 2 if mean > 127 else 1
        r.T = 0
        r.bits = np.full((nc, nc), 1 if r.branch == 2 else 0, np.uint8)
    else:
        r.branch = 0
        r.otsu_set = otsu_argmax(img)
        r.T = r.otsu_set[0] if r.otsu_set else 0
        r.bits = cells_of(img, nc, cell, margin, r.T)
    # how many distinct binarisations the arg-max set allows (a run of empty bins splits the same way)
    flat = np.sort(img.reshape(-1))
    r.otsu_splits = len({int(np.searchsorted(flat, t, side="right")) for t in r.otsu_set})
    r.border_err = border_errors(r.bits, ms, bb)
    r.max_border_err = int(ms * ms * border_rate)
    r.id, r.rot, r.dist = -1, 0, None
    if r.border_err <= r.max_border_err:
        r.id, r.rot, r.dist = identify_code(r.bits[bb:nc - bb, bb:nc - bb], rots, max_corr)
    return r
