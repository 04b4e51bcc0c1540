"""k_identify (detect_identify.h) on injected quads, against the oracle and against the exact restatement in
tests/identify_reference.py.

aslam_debug_inject_candidates writes a slot's candidates; aslam_debug_run_identify launches the identification stage of a detection
call on them (the instrumented build of the same kernel body, which also records every decision) over the grey frame the slot's
last detection pass read.  Every candidate is checked twice:
  (a) against the oracle's _identifyOneCandidate (orc_identify_detail): cell bits, branch, Otsu threshold, border errors, inner
      sum and sum of squares, id and rotation, bit-exact;
  (b) against the reference, on every candidate without an ambiguous pixel (an exact source position within 1e-9 px of a
      half-integer): the cell bits, the branch (the double form of the stddev test, the specification), the Otsu threshold (in the
      exact arg-max set; where that set holds several distinct splits, the reference binarises with the kernel's threshold), the
      border errors, the id and the rotation.
Families: pixel-aligned candidates (a pure-translation warp: the test writes the warped image into the frame) placing every
decision boundary exactly and one step to each side, over marker sizes 3..7, 2..8 px per cell and 0..2 px cell margins; general
projective quads of rendered markers; quads beyond every edge of odd-sized frames and corners around +-3e9; batches of slots.
Each test counts what it reached and asserts a minimum, so that a later change cannot quietly stop a family reaching its case.
Runs on whichever library the session loads: the emulation here, the gfx950 build on the MI355X."""
import collections

import numpy as np
import pytest

import identify_reference as ir
from aruco_slam_amd import capi, synth
from oracle import pyoracle as orc

if not ir.EXACT_LD:
    pytest.skip("the exact reference needs a 64-bit-mantissa long double", allow_module_level=True)

K = np.array([[100.0, 0, 40], [0, 100, 40], [0, 0, 1]])
REACHED = collections.Counter()
DEFAULTS = dict(perspectiveRemovePixelPerCell=8, perspectiveRemoveIgnoredMarginPerCell=0.13, maxErroneousBitsInBorderRate=0.35,
                minOtsuStdDev=5.0, errorCorrectionRate=0.6)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nidentify cases reached: " + ", ".join(f"{k} {v}" for k, v in sorted(REACHED.items())))


@pytest.fixture(autouse=True)
def oracle_defaults():
    """every test leaves the oracle's free functions as it found them: DICT_ARUCO_ORIGINAL, default detector parameters"""
    yield
    orc.set_dictionary(None)
    orc.set_detector_params()


def margin_rate(cell, k):
    """a perspectiveRemoveIgnoredMarginPerCell with int(rate * cell) == k"""
    return 0.0 if k == 0 else (k + 0.5) / cell


def valid_margins(cell):
    return [k for k in (0, 1, 2) if cell - 2 * k >= 1 and (k == 0 or (k + 0.5) / cell < 0.5)]


class Setup:
    """one dictionary + detector parameters, on the library and on the oracle"""

    def __init__(self, dict_bits, maxcorr, builtin=False, **params):
        self.bits = np.asarray(dict_bits, np.uint8)
        self.ms = self.bits.shape[1]
        self.maxcorr = maxcorr
        self.builtin = builtin
        self.p = dict(DEFAULTS, **params)
        self.cell = int(self.p["perspectiveRemovePixelPerCell"])
        self.margin = int(self.p["perspectiveRemoveIgnoredMarginPerCell"] * self.cell)
        self.nc = self.ms + 2
        self.S = self.nc * self.cell
        self.max_corr = int(maxcorr * self.p["errorCorrectionRate"])
        self.max_border = int(self.ms * self.ms * self.p["maxErroneousBitsInBorderRate"])
        self.rots = ir.rotations(self.bits)

    def apply(self, ctx):
        if self.builtin:
            ctx.set_dictionary_bytes(synth.opencv_bytes_list(self.bits), 5, 0)
            orc.set_dictionary(None)
        else:
            ctx.set_dictionary(self.bits, self.maxcorr)
            orc.set_dictionary(self.bits, self.maxcorr)
        ctx.set_detector_params(**self.p)
        orc.set_detector_params(**self.p)

    def reference(self, gray, corners):
        return ir.identify(gray, corners, self.ms, self.rots, self.max_corr, cell=self.cell,
                           margin_rate=self.p["perspectiveRemoveIgnoredMarginPerCell"], border_rate=self.p["maxErroneousBitsInBorderRate"],
                           min_std=self.p["minOtsuStdDev"])


def context(rows, cols, batch):
    ctx = capi.Context(max_rows=rows, max_cols=cols, max_batch=batch, persistent_waves=4, max_landmarks=16)
    ctx.set_camera(K, np.zeros(5))
    return ctx


def run(ctx, setup, frames, cands, tally, ref_every=1, detect=False):
    """frames: n x rows x cols (gray, or bgr8 n x rows x cols x 3); cands[s]: m x 4 x 2 corners of slot s.  Checks every candidate
    against the oracle and (every ref_every-th of a slot) against the reference; returns the kernel's (ids, rots) per slot.
    detect: run a detection pass over the staged frames first (a gray slot is read as staged without one; a bgr8 slot needs it)."""
    setup.apply(ctx)
    frames = np.ascontiguousarray(frames, np.uint8)
    ctx.stage_frames(frames, 0)
    if detect:
        ctx.run_staged(0, len(frames), with_ekf=False)
        ctx.sync()
    if frames.ndim == 4:
        frames = np.stack([orc.bgr2gray(f) for f in frames])
    for s, c in enumerate(cands):
        c = np.asarray(c, np.float32).reshape(-1, 8)
        ctx.inject_candidates(s, np.full(len(c), 7, np.int32), np.full(len(c), 3, np.int32), c)
    ctx.run_identify(0, len(frames))
    out = []
    for s, c in enumerate(cands):
        c = np.asarray(c, np.float32).reshape(-1, 4, 2)
        ids, rots, cells, info = ctx.get_identified(s)
        assert len(ids) == len(c)
        assert np.array_equal(info[:, 5], ids) and np.array_equal(info[:, 6], rots), "record and candidate list disagree"
        for i in range(len(c)):
            check_one(setup, frames[s], c[i], ids[i], rots[i], cells[i], info[i], tally, f"slot {s} cand {i}", i % ref_every == 0)
        out.append((ids, rots))
    return out


def check_one(setup, gray, corners, kid, krot, kcells, info, tally, where, with_ref):
    branch, T, berr, ssum, ssq = (int(v) for v in info[:5])
    # (a) the oracle, field for field
    ob, od = orc.identify_detail(gray, corners)
    assert np.array_equal(kcells, ob), f"{where}: cell bits differ from the oracle"
    got = dict(branch=branch, T=T, border_err=berr, sum=ssum, sq=ssq, id=int(kid), rot=int(krot))
    assert got == od, f"{where}: kernel {got} != oracle {od}"
    tally["branch%d" % branch] += 1
    tally["ms%d" % setup.ms] += 1
    tally["cell%d" % setup.cell] += 1
    tally["margin%d" % setup.margin] += 1
    tally["identified" if kid >= 0 else "rejected"] += 1
    if setup.nc * setup.nc > 64 and kcells.reshape(-1)[64:].any():
        tally["upper ballot word set"] += 1
    if not with_ref:
        return
    # (b) the exact reference
    r = setup.reference(gray, corners)
    tally["checked"] += 1
    if r.n_outside:
        tally["outside samples"] += 1
    if r.std_forms_disagree:
        tally["stddev forms disagree"] += 1
    if r.ambiguous:
        tally["ambiguous"] += 1
        return
    assert branch == r.branch, f"{where}: branch {branch}, reference {r.branch}"
    assert (ssum, ssq) == (r.sum, r.sq), f"{where}: inner moments differ from the reference"
    bits = r.bits
    if branch == 0:
        assert T in r.otsu_set, f"{where}: Otsu threshold {T} outside the exact arg-max set {r.otsu_set}"
        if r.otsu_splits > 1:
            tally["otsu true tie"] += 1
            bits = ir.cells_of(r.img, setup.nc, setup.cell, setup.margin, T)
        elif len(r.otsu_set) > 1:
            tally["otsu tie over empty bins"] += 1
    assert np.array_equal(kcells, bits), f"{where}: cell bits differ from the reference"
    berr_ref = ir.border_errors(bits, setup.ms)
    assert berr == berr_ref, f"{where}: border errors {berr}, reference {berr_ref}"
    if berr == setup.max_border:
        tally["border errors at the limit"] += 1
    if berr == setup.max_border + 1:
        tally["border errors one over"] += 1
    rid, rrot = -1, 0
    if berr_ref <= setup.max_border:
        rid, rrot, dist = ir.identify_code(bits[1:-1, 1:-1], setup.rots, setup.max_corr)
        if (dist <= setup.max_corr).sum() > 1:
            tally["several entries in budget"] += 1
        dmin = int(dist.min())
        if dmin == setup.max_corr and setup.max_corr > 0:
            tally["distance at budget"] += 1
        if dmin == setup.max_corr + 1:
            tally["distance one over budget"] += 1
        if rid >= 0:
            d = (setup.rots[rid] != bits[1:-1, 1:-1][None]).sum(axis=(1, 2))
            if (d == d.min()).sum() > 1:
                tally["rotation tie"] += 1
    assert (int(kid), int(krot)) == (rid, rrot), f"{where}: id / rotation {(kid, krot)}, reference {(rid, rrot)}"


def need(tally, **mins):
    REACHED.update(tally)
    short = {k: (tally[k.replace("_", " ")], v) for k, v in mins.items() if tally[k.replace("_", " ")] < v}
    assert not short, f"cases not reached (got, wanted): {short}"


# ---- pixel-aligned candidates ---------------------------------------------------------------------------------------------------

LO, HI = 30, 220


def aligned_corners(x0, y0, S):
    return np.array([[x0, y0], [x0 + S - 1, y0], [x0 + S - 1, y0 + S - 1], [x0, y0 + S - 1]], np.float32)


def cell_image(cells, cell, lo=LO, hi=HI):
    return (np.kron(np.asarray(cells, np.int64), np.ones((cell, cell), np.int64)) * (hi - lo) + lo).astype(np.int64)


def marker_cells(code):
    ms = code.shape[0]
    c = np.zeros((ms + 2, ms + 2), np.uint8)
    c[1:-1, 1:-1] = code
    return c


def inner_slice(st):
    lo, hi = st.cell // 2, st.S - st.cell // 2
    return slice(lo, hi)


def aligned_images(st, rng):
    """warped images (S x S int) placing the decision boundaries of this setup"""
    ims = []
    ms, S, cell, w = st.ms, st.S, st.cell, st.cell - 2 * st.margin
    e = rng.randint(len(st.bits))
    for r in range(4):                                                # an entry in each rotation
        ims.append(cell_image(marker_cells(np.rot90(st.bits[(e + r) % len(st.bits)], r)), cell))
    # border errors: at the limit and one over (white border cells, bottom rows first: the upper ballot word of 9 x 9)
    border = [(y, x) for y in range(st.nc) for x in range(st.nc) if y in (0, st.nc - 1) or x in (0, st.nc - 1)][::-1]
    for k in (st.max_border, st.max_border + 1):
        cl = marker_cells(st.bits[e])
        for (y, x) in border[:k]:
            cl[y, x] = 1
        ims.append(cell_image(cl, cell))
    # Hamming distance max_corr and one over
    for k in sorted({st.max_corr, st.max_corr + 1}):
        code = st.bits[e].copy().reshape(-1)
        code[rng.permutation(ms * ms)[:k]] ^= 1
        ims.append(cell_image(marker_cells(code.reshape(ms, ms)), cell))
    # a cell with exactly floor(w^2 / 2) pixels above T (and the rest equal to T = LO), and one with one more
    for extra in (0, 1):
        cl = marker_cells(st.bits[e])
        im = cell_image(cl, cell)
        blk = [(y, x) for y in range(w) for x in range(w)]
        for cy, cx in ((0, 0), (st.nc - 1, st.nc - 1)):              # border cells (both ballot words at 9 x 9)
            for (y, x) in blk[:(w * w) // 2 + extra]:
                im[cy * cell + st.margin + y, cx * cell + st.margin + x] = HI
        ims.append(im)
    # stddev of the inner region exactly minOtsuStdDev (values m +- 5), and one step to each side
    sl = inner_slice(st)
    n = (sl.stop - sl.start) ** 2
    for step in ("on", "below", "above"):
        im = np.full((S, S), 100, np.int64)
        v = np.array([105 if i % 2 == 0 else 95 for i in range(n)], np.int64)
        if n % 2:
            v[-1] = 100
        if step == "below":
            v[0], v[1] = 100, 100
        elif step == "above":
            v[0], v[1] = 106, 94
        im[sl, sl] = v.reshape(sl.stop - sl.start, -1)
        ims.append(im)
    # uniform inner region at mean 127 / 128, a 127 + 1, a 126 / 128 alternation, and 127 inside a contrasting half-cell ring
    for inner, ring in ((127, 127), (128, 128), (127, 255), (128, 0), ("127+1", 127), ("126/128", 127)):
        im = np.full((S, S), ring, np.int64)
        if inner == "127+1":
            im[sl, sl] = 127
            im[sl.start, sl.start] = 128
        elif inner == "126/128":
            m = sl.stop - sl.start
            im[sl, sl] = np.where((np.add.outer(np.arange(m), np.arange(m)) % 2) == 0, 126, 128)
            if (m * m) % 2:
                im[sl.start, sl.start] = 127
        else:
            im[sl, sl] = inner
        ims.append(im)
    # Otsu: three levels with c0 == c2 (two distinct splits tie exactly)
    N = S * S
    lv = np.full(N, 120, np.int64)
    p = rng.permutation(N)
    lv[p[:N // 3]] = 40
    lv[p[N // 3: 2 * (N // 3)]] = 200
    ims.append(lv.reshape(S, S))
    return ims


def aligned_frame(im, size):
    f = np.full((size, size), 128, np.uint8)
    f[4:4 + im.shape[0], 4:4 + im.shape[1]] = np.clip(im, 0, 255)
    return f


def run_aligned(ctx, st, rng, tally, size=80):
    ims = aligned_images(st, rng)
    frames = np.stack([aligned_frame(im, size) for im in ims])
    cands = [aligned_corners(4, 4, st.S)[None] for _ in ims]
    run(ctx, st, frames, cands, tally)


def tie_dictionary(ms, rng, n=70, maxcorr=2):
    """entries 2, 5 and 66 all within 1 bit of one code (the lowest index wins; 2 and 66 share a lane); entry 7 is a
    rotation-symmetric pattern with one cell flipped, so the symmetric code lies 1 bit from all four of its rotations"""
    b = rng.randint(0, 2, (n, ms, ms)).astype(np.uint8)
    A = b[2].copy().reshape(-1)
    b[5] = A.copy().reshape(ms, ms); b[5].reshape(-1)[[0, 1]] ^= 1
    b[66] = A.copy().reshape(ms, ms); b[66].reshape(-1)[[0, 2]] ^= 1
    sym = rng.randint(0, 2, (ms, ms)).astype(np.uint8)
    for y in range(ms):
        for x in range(ms):
            orbit = [(y, x), (ms - 1 - x, y), (ms - 1 - y, ms - 1 - x), (x, ms - 1 - y)]
            sym[y, x] = sym[min(orbit)]
    b[7] = sym.copy()
    b[7][0, 1] ^= 1
    code_two = A.copy().reshape(ms, ms); code_two.reshape(-1)[0] ^= 1
    return b, maxcorr, code_two, sym


@pytest.mark.parametrize("ms", [3, 4, 5, 6, 7])
def test_aligned_boundaries(ms):
    """every decision boundary exactly on it and one step to each side, marker size ms, 2..8 px per cell, every margin"""
    rng = np.random.RandomState(ms)
    tally = collections.Counter()
    ctx = context(80, 80, 32)
    dist = {3: 3, 4: 5, 5: 7, 6: 9, 7: 13}[ms]
    bits, maxcorr = synth.random_dictionary(ms, 6, dist, seed=ms)
    for cell in range(2, 9):
        for k in valid_margins(cell):
            st = Setup(bits, maxcorr, perspectiveRemovePixelPerCell=cell, perspectiveRemoveIgnoredMarginPerCell=margin_rate(cell, k),
                       errorCorrectionRate=1.0)
            assert st.margin == k
            run_aligned(ctx, st, rng, tally)
    # ties in the dictionary: lowest index within budget, lowest rotation at equal distance
    tb, tmc, code_two, sym = tie_dictionary(ms, rng)
    st = Setup(tb, tmc, errorCorrectionRate=0.5)                       # int(2 * 0.5) = 1 bit
    ims = [cell_image(marker_cells(code_two), st.cell), cell_image(marker_cells(sym), st.cell)]
    ids = run(ctx, st, np.stack([aligned_frame(im, 80) for im in ims]), [aligned_corners(4, 4, st.S)[None]] * 2, tally)
    want_two = next(m for m in range(len(tb)) if (ir.rotations(tb)[m] != code_two[None]).sum(axis=(1, 2)).min() <= 1)
    assert int(ids[0][0][0]) == want_two
    need(tally, branch0=40, branch1=20, branch2=20, border_errors_at_the_limit=7, border_errors_one_over=7, distance_one_over_budget=7,
         several_entries_in_budget=1, rotation_tie=1, otsu_true_tie=1, otsu_tie_over_empty_bins=20, identified=30, rejected=30,
         **{f"cell{c}": 1 for c in range(2, 9)}, margin0=1, margin1=1, margin2=1)
    if ms == 7:
        need(tally, upper_ballot_word_set=10)


def test_aligned_72px_marker_fills_both_ballot_words():
    """7 x 7 markers at 8 px per cell: S = 72 > 64 (a warp row step of 0 rows per 64 pixels) and 81 cells"""
    rng = np.random.RandomState(72)
    tally = collections.Counter()
    bits, maxcorr = synth.random_dictionary(7, 8, 13, seed=72)
    st = Setup(bits, maxcorr)
    assert st.S == 72 and st.nc * st.nc == 81
    ctx = context(80, 80, 32)
    run_aligned(ctx, st, rng, tally)
    need(tally, upper_ballot_word_set=5, identified=4)


def test_aruco_original_dictionary_aligned():
    """the built-in DICT_ARUCO_ORIGINAL (1024 entries, no correction: 16 lanes' worth of entries per lane)"""
    bits = np.stack([synth.aruco_original_bits(i) for i in range(1024)])
    st = Setup(bits, 0, builtin=True)
    rng = np.random.RandomState(5)
    tally = collections.Counter()
    ctx = context(80, 80, 32)
    ids = [int(i) for i in rng.randint(0, 1024, 8)]
    ims = [cell_image(marker_cells(np.rot90(bits[i], r % 4)), 8) for r, i in enumerate(ids)]
    out = run(ctx, st, np.stack([aligned_frame(im, 80) for im in ims]), [aligned_corners(4, 4, 72 - 16)[None]] * len(ims), tally)
    assert [int(o[0][0]) for o in out] == ids and [int(o[1][0]) for o in out] == [r % 4 for r in range(len(ids))]
    run_aligned(ctx, st, rng, tally)
    need(tally, identified=10, rejected=5)


def test_error_budgets_at_exact_products():
    """maxErroneousBitsInBorderRate and errorCorrectionRate whose products land on integers: 0.04 * 25 = 1, 0.2 * 25 = 5, 0.6 * 5 = 3,
    0.7 * 10 = 7 (as float32 operands 6.9999998: a budget computed in float would be 6)"""
    rng = np.random.RandomState(9)
    tally = collections.Counter()
    ctx = context(80, 80, 32)
    for ms, maxcorr, ecr, brate in ((5, 5, 0.6, 0.04), (5, 5, 0.6, 0.2), (7, 10, 0.7, 0.35), (6, 10, 0.7, 0.04)):
        bits = rng.randint(0, 2, (4, ms, ms)).astype(np.uint8)
        st = Setup(bits, maxcorr, errorCorrectionRate=ecr, maxErroneousBitsInBorderRate=brate,
                   perspectiveRemovePixelPerCell=8 if ms < 7 else 8)
        assert st.max_corr == round(maxcorr * ecr) and st.max_border == round(ms * ms * brate)
        ims = []
        for k in (st.max_corr, st.max_corr + 1):
            code = bits[0].copy().reshape(-1)
            code[rng.permutation(ms * ms)[:k]] ^= 1
            d = (ir.rotations(bits) != code.reshape(ms, ms)[None, None]).sum(axis=(2, 3)).min()
            assert d == k or k > st.max_corr, "random entries too close for this case"
            ims.append(cell_image(marker_cells(code.reshape(ms, ms)), st.cell))
        run(ctx, st, np.stack([aligned_frame(im, 80) for im in ims]), [aligned_corners(4, 4, st.S)[None]] * 2, tally)
        run_aligned(ctx, st, rng, tally)
    need(tally, distance_at_budget=4, distance_one_over_budget=4, border_errors_at_the_limit=4, border_errors_one_over=4)


# ---- general quads of rendered markers ---------------------------------------------------------------------------------------

def render(frame, cells, quad, rng, ss=3, noise=0):
    """draw the nc x nc cell pattern (1 = white) into frame on the projective quad (corner 0 = the pattern's top-left, clockwise),
    ss x ss supersampled; noise: +- amplitude"""
    nc = cells.shape[0]
    src = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
    A = []
    for (u, v), (x, y) in zip(src, quad):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y, u])
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y, v])
    A = np.array(A)
    h = np.linalg.solve(A[:, :8], A[:, 8])
    Hm = np.append(h, 1).reshape(3, 3)                                # image -> marker unit square
    x0, y0 = np.floor(quad.min(axis=0)).astype(int) - 1
    x1, y1 = np.ceil(quad.max(axis=0)).astype(int) + 2
    x0, y0 = max(x0, 0), max(y0, 0)
    x1, y1 = min(x1, frame.shape[1]), min(y1, frame.shape[0])
    if x1 <= x0 or y1 <= y0:
        return
    yy, xx = np.mgrid[y0:y1, x0:x1]
    acc = np.zeros(yy.shape)
    cov = np.zeros(yy.shape)
    for sy in range(ss):
        for sx in range(ss):
            px, py = xx + (sx + 0.5) / ss - 0.5, yy + (sy + 0.5) / ss - 0.5
            w = Hm[2, 0] * px + Hm[2, 1] * py + Hm[2, 2]
            u = (Hm[0, 0] * px + Hm[0, 1] * py + Hm[0, 2]) / w
            v = (Hm[1, 0] * px + Hm[1, 1] * py + Hm[1, 2]) / w
            inside = (u >= 0) & (u < 1) & (v >= 0) & (v < 1)
            cu = np.clip((u * nc).astype(int), 0, nc - 1)
            cv = np.clip((v * nc).astype(int), 0, nc - 1)
            acc += np.where(inside, np.where(cells[cv, cu] > 0, 235.0, 20.0), 0.0)
            cov += inside
    sub = frame[y0:y1, x0:x1].astype(np.float64)
    val = np.where(cov > 0, (acc + sub * (ss * ss - cov)) / (ss * ss), sub)
    if noise:
        val = val + rng.randint(-noise, noise + 1, val.shape)
    frame[y0:y1, x0:x1] = np.clip(np.rint(val), 0, 255).astype(np.uint8)


def random_quad(rng, cx, cy, side, persp):
    """a convex quad around (cx, cy): a rotated square of the given side, corners moved by up to persp * side"""
    a = rng.uniform(0, 2 * np.pi)
    sq = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]) * side
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    while True:
        q = sq @ R.T + rng.uniform(-persp, persp, (4, 2)) * side + [cx, cy]
        d = np.roll(q, -1, axis=0) - q
        cr = d[:, 0] * np.roll(d, -1, axis=0)[:, 1] - d[:, 1] * np.roll(d, -1, axis=0)[:, 0]
        if (cr > 0).all() or (cr < 0).all():
            if (cr < 0).all():
                q = q[[0, 3, 2, 1]]
            return q


def general_case(st, rows, cols, rng, n, sides, noise):
    frame = np.full((rows, cols), 128, np.uint8)
    if noise:
        frame = np.clip(frame.astype(int) + rng.randint(-noise, noise + 1, frame.shape), 0, 255).astype(np.uint8)
    cands, placed = [], []
    for k in range(n):
        for _ in range(500):                                          # markers do not overlap (as many as fit)
            side = rng.uniform(*sides)
            cx, cy = rng.uniform(side * 0.6, cols - side * 0.6), rng.uniform(side * 0.6, rows - side * 0.6)
            if all(np.hypot(cx - px, cy - py) > 1.0 * (side + ps) for px, py, ps in placed):
                break
        else:
            break
        placed.append((cx, cy, side))
        q = random_quad(rng, cx, cy, side, 0.18)
        e = rng.randint(len(st.bits))
        render(frame, marker_cells(st.bits[e]), q, rng, noise=noise)
        r = k % 4
        cands.append(np.roll(q, -r, axis=0).astype(np.float32))      # the candidate starts at the marker's corner r
    return frame, np.array(cands)


@pytest.mark.parametrize("ms", [4, 5, 7])
def test_general_quads(ms):
    """rendered markers on random projective quads, all four corner rotations, sides from well under S to about 2.5 S, noise"""
    rng = np.random.RandomState(100 + ms)
    tally = collections.Counter()
    bits, maxcorr = synth.random_dictionary(ms, 8, {4: 5, 5: 7, 7: 13}[ms], seed=ms)
    rows, cols = 120, 160
    ctx = context(rows, cols, 4)
    for cell in (4, 8):
        st = Setup(bits, maxcorr, perspectiveRemovePixelPerCell=cell)
        frames, cands = [], []
        for s in range(4):
            f, c = general_case(st, rows, cols, rng, 6, (0.4 * st.S, min(2.5 * st.S, 100)), noise=6 if s % 2 else 0)
            frames.append(f); cands.append(c)
        run(ctx, st, np.stack(frames), cands, tally)
    general = tally["checked"]
    print(f"\ngeneral quads ms {ms}: {tally['ambiguous']} of {general} ambiguous")
    assert tally["ambiguous"] < 0.1 * general
    need(tally, identified=10)


def test_rotation_direction_against_a_turned_marker():
    """the same marker turned by 90 degrees in the image: the rotation found makes the rotated corners start at the marker's own
    top-left corner (as the oracle's rendered-marker test pins it)"""
    rng = np.random.RandomState(4)
    bits, maxcorr = synth.random_dictionary(5, 4, 7, seed=4)
    st = Setup(bits, maxcorr)
    tally = collections.Counter()
    ctx = context(120, 160, 4)
    frame = np.full((120, 160), 128, np.uint8)
    base = np.array([[30, 20], [100, 24], [96, 96], [26, 90]], np.float64)       # the marker's TL, TR, BR, BL
    render(frame, marker_cells(bits[1]), base, rng)
    for k in range(4):
        ids, rots = run(ctx, st, frame[None], [np.roll(base, -k, axis=0)[None]], tally, detect=True)[0]
        assert ids[0] == 1 and rots[0] == k
        assert np.array_equal(np.roll(np.roll(base, -k, axis=0), int(rots[0]), axis=0), base)
        r = st.reference(frame, np.roll(base, -k, axis=0).astype(np.float32))
        assert (r.id, r.rot) == (1, k)


# ---- beyond the frame ----------------------------------------------------------------------------------------------------------

def test_quads_beyond_the_frame():
    """quads partly or wholly beyond every edge of a 61 x 97 frame, a corner exactly on the last row / column, corners around
    +-3e9 (source positions beyond the int range)"""
    rows, cols = 61, 97
    rng = np.random.RandomState(61)
    tally = collections.Counter()
    bits, maxcorr = synth.random_dictionary(5, 6, 7, seed=61)
    ctx = context(64, 128, 3)
    for cell in (4, 8):
        st = Setup(bits, maxcorr, perspectiveRemovePixelPerCell=cell)
        frames, cands = [], []
        for s in range(3):
            f = np.full((rows, cols), 200, np.uint8)
            # (a marker whose outer border half lies beyond the left edge: the samples there read 0, a black border)
            render(f, marker_cells(bits[s]), np.array([[-4, 3], [52, 4], [51, 57], [-3, 56]], float), rng)
            render(f, marker_cells(bits[s + 1]), np.array([[60, 20], [120, 22], [118, 80], [58, 76]], float), rng)
            c = [[[-4, 3], [52, 4], [51, 57], [-3, 56]], [[60, 20], [120, 22], [118, 80], [58, 76]],
                 [[-20, -15], [40, -12], [44, 40], [-16, 36]],
                 [[-50, -40], [-5, -40], [-5, -3], [-50, -3]], [[100, 65], [150, 65], [150, 100], [100, 100]],
                 [[10, 30], [96, 30], [96, 60], [10, 60]], [[cols - 1, rows - 1], [cols + 40, rows - 1], [cols + 40, rows + 30], [cols - 1, rows + 30]],
                 [[-3e9, -3e9], [3e9, -3e9], [3e9, 3e9], [-3e9, 3e9]], [[0, 0], [3e9, 0], [3e9, 3e9], [0, 3e9]],
                 [[-3e9, 10], [40, 10], [40, 50], [-3e9, 50]], [[20, -3.1e9], [60, -3.1e9], [60, 40], [20, 40]]]
            c = [np.roll(np.array(q, np.float64), -s, axis=0) for q in c]
            for _ in range(4):
                c.append(random_quad(rng, rng.uniform(-30, cols + 30), rng.uniform(-30, rows + 30), rng.uniform(20, 90), 0.15))
            frames.append(f); cands.append(np.array(c, np.float32))
        run(ctx, st, np.stack(frames), cands, tally)
    need(tally, outside_samples=30, identified=2, rejected=20)


# ---- batches -------------------------------------------------------------------------------------------------------------------

def test_batch_of_slots_with_different_frames():
    """five bgr8 slots in one launch after a detection pass (k_threshold's grey planes), each frame different: a wrong per-frame
    grey offset or work-list order changes what is read"""
    rng = np.random.RandomState(12)
    tally = collections.Counter()
    bits, maxcorr = synth.random_dictionary(6, 10, 9, seed=12)
    st = Setup(bits, maxcorr)
    rows, cols = 120, 160
    ctx = context(rows, cols, 5)
    frames, cands = [], []
    for s in range(5):
        f, c = general_case(st, rows, cols, rng, 3 + s, (40, 90), noise=3)
        frames.append(f); cands.append(c)
    bgr = np.stack([np.stack([f, np.roll(f, 1, axis=1), f[::-1]], axis=-1) for f in frames])    # gray = mix of the three channels
    out = run(ctx, st, bgr, cands, tally, detect=True)
    assert sum(int((o[0] >= 0).sum()) for o in out) >= 0.7 * sum(len(c) for c in cands)
    need(tally, identified=5)


def test_full_slot_of_2048_candidates():
    """2048 candidates in one slot (every one checked against the oracle, every 16th against the reference); 2049 are refused"""
    rng = np.random.RandomState(2048)
    tally = collections.Counter()
    bits, maxcorr = synth.random_dictionary(5, 8, 7, seed=20)
    st = Setup(bits, maxcorr, perspectiveRemovePixelPerCell=4)
    rows, cols = 120, 160
    ctx = context(rows, cols, 2)
    f, c = general_case(st, rows, cols, rng, 6, (28, 44), noise=0)
    extra = np.array([random_quad(rng, rng.uniform(0, cols), rng.uniform(0, rows), rng.uniform(8, 120), 0.2) for _ in range(2048 - len(c))],
                     np.float32)
    allc = np.concatenate([c, extra])
    out = run(ctx, st, f[None], [allc], tally, ref_every=16)
    assert int((out[0][0][:len(c)] >= 0).sum()) >= 0.7 * len(c) and len(c) >= 2
    with pytest.raises(capi.AslamError):
        ctx.inject_candidates(0, np.full(2049, -1), np.zeros(2049), np.zeros((2049, 8), np.float32))
    need(tally, identified=2)


def test_run_identify_arguments_are_checked():
    ctx = context(64, 64, 2)
    with pytest.raises(capi.AslamError):
        ctx.run_identify(0, 1)                                     # no frame staged
    with pytest.raises(capi.AslamError):
        ctx.get_identified(0)                                      # nothing identified yet
    ctx.stage_frames(np.zeros((64, 64), np.uint8), 0)
    with pytest.raises(capi.AslamError):
        ctx.run_identify(1, 2)                                     # beyond max_batch
    with pytest.raises(capi.AslamError):
        ctx.run_identify(1, 1)                                     # slot 1 holds no frame of this shape


# ---- larger variants on the GPU -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ms", [3, 5, 6, 7])
def test_general_quads_full_frame(ms):
    """1280 x 720 frames, sides from 0.4 S to 600 px (strongly undersampled), all four rotations, noise; 8 slots per launch"""
    rng = np.random.RandomState(200 + ms)
    tally = collections.Counter()
    count, dist = {3: (6, 3), 5: (10, 7), 6: (10, 9), 7: (10, 13)}[ms]     # (3 x 3: what 9 bits can hold at distance 3)
    bits, maxcorr = synth.random_dictionary(ms, count, dist, seed=ms)
    rows, cols = 720, 1280
    ctx = context(rows, cols, 8)
    for cell in (2, 5, 8):
        st = Setup(bits, maxcorr, perspectiveRemovePixelPerCell=cell)
        frames, cands = [], []
        for s in range(8):
            f, c = general_case(st, rows, cols, rng, 8, (0.4 * st.S, 600), noise=8 if s % 2 else 0)
            frames.append(f); cands.append(c)
        run(ctx, st, np.stack(frames), cands, tally, ref_every=2)
    print(f"\nfull-frame quads ms {ms}: {tally['ambiguous']} of {tally['checked']} ambiguous")
    assert tally["ambiguous"] < 0.1 * tally["checked"]
    need(tally, identified=60)
