"""k_threshold, k_prefix, k_seg, k_link, k_link_serial and k_trace_write (detect.hip) on built images, against the oracle and against
the exact restatement in tests/contours_reference.py.

aslam_debug_run_contours launches the contour stage of a detection call on staged frames, with the cut lattice (32 / 64) and the
hand-over limit of k_link chosen by the test.  Every frame is checked three ways by equality of integers: the reference is first held
against its own invariants (contours_reference.check_invariants) and against the oracle (threshold decision and every border,
unfiltered), then the kernels against the reference: neighbour masks, the node list as a set of packed states, every node's (next,
steps, shoelace), n_starts, the kept contours (sizes, keys, points), the write tickets (they cover every point of every kept contour
exactly once; none of k_link's exceeds 64 points; every skip lies inside its segment) and which link form resolved the frame.
Every family runs at both lattices and through both link forms; only the cases built to land on one side of a hand-over limit, and the
300-frame batch, fix the form.  No case is skipped: capacities are sized
from the reference's counts (asserted before the kernels run) and overflow is met in the capacity tests only.  Runs on whichever
library the session loads: the emulation here, the gfx950 build on the MI355X.  The tally is printed at the end of the module (-s)."""
import collections

import numpy as np
import pytest

import contours_reference as cr
from aruco_slam_amd import capi
from oracle import pyoracle as orc

TALLY = collections.Counter()
MAXIMA = collections.Counter()
LINK_LDS_NODES, LINK_SLOTS, BLOCK_STARTS = 32000, 1536, 1024
NONE = cr.NONE
BRIGHT, DARK = 255, 0


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\ncontours tally: " + ", ".join(f"{k} {v}" for k, v in sorted(TALLY.items())))
    print("contours maxima: " + ", ".join(f"{k} {v}" for k, v in sorted(MAXIMA.items())))


def note_max(k, v):
    MAXIMA[k] = max(MAXIMA[k], int(v))


class Rig:
    """a context for frames of one shape, with one set of detector parameters on library, oracle calls and reference"""

    def __init__(self, rows, cols, batch=1, starts=1 << 14, contours=1 << 12, points=1 << 16, max_rows=None, max_cols=None, **dp):
        self.rows, self.cols, self.batch = rows, cols, batch
        self.caps = dict(nodes=starts, contours=contours, points=points)
        self.ctx = capi.Context(max_rows=max_rows or rows, max_cols=max_cols or cols, max_batch=batch, persistent_waves=4, max_landmarks=16,
                                cap_starts_per_frame=starts, cap_contours_per_frame=contours, cap_points_per_frame=points)
        self._ref = {}
        self.params(**dp)

    def params(self, **dp):
        self.dp = dict(adaptiveThreshWinSizeMin=3, adaptiveThreshWinSizeMax=23, adaptiveThreshWinSizeStep=10, adaptiveThreshConstant=7.0,
                       minMarkerPerimeterRate=0.03, maxMarkerPerimeterRate=4.0)
        self.dp.update(dp)
        self.ctx.set_detector_params(**self.dp)
        self.windows = cr.windows_of(self.dp["adaptiveThreshWinSizeMin"], self.dp["adaptiveThreshWinSizeMax"], self.dp["adaptiveThreshWinSizeStep"])
        self.C = self.dp["adaptiveThreshConstant"]
        self.lo, self.hi = cr.perim_limits(self.rows, self.cols, self.dp["minMarkerPerimeterRate"], self.dp["maxMarkerPerimeterRate"])
        return self

    def ref(self, img):
        """the reference's account of one frame, checked against its invariants and against the oracle, once"""
        gray = cr.bgr2gray(img) if img.ndim == 3 else img
        if img.ndim == 3:
            assert np.array_equal(gray, orc.bgr2gray(img)), "bgr8 -> gray: reference and oracle differ"
        key = (gray.tobytes(), tuple(self.windows), self.C, self.lo, self.hi)
        if key not in self._ref:
            f = cr.Frame(gray, self.windows, self.C, self.lo, self.hi)
            for sc, k in zip(f.scales, self.windows):
                th = orc.threshold(gray, k, self.C)
                assert np.array_equal(th > 0, sc.fg), f"window {k}: threshold decision of reference and oracle differ"
                sizes, keys, hole, pts = orc.find_contours(th, 1 << 16, 1 << 20)
                b = sc.borders[::-1]
                assert [len(x.pts) for x in b] == sizes.tolist() and [x.key for x in b] == keys.tolist() and [x.hole for x in b] == hole.tolist(), \
                    f"window {k}: borders of reference and oracle differ"
                assert np.array_equal(np.array([p for x in b for p in x.pts], np.int64).reshape(-1, 2), pts), f"window {k}: border points differ"
                TALLY["borders kept"] += len(sc.kept)
                TALLY["borders rejected: below min_perim"] += sum(len(x.pts) < self.lo or len(x.pts) == 1 for x in sc.borders)
                TALLY["borders rejected: above max_perim"] += sum(len(x.pts) > self.hi for x in sc.borders)
            TALLY["reference frames"] += 1
            self._ref[key] = f
        return self._ref[key]


def check_slot(rig, slot, f, grid, serial, todo=None):
    """one slot after run_contours against the reference frame f"""
    ctx, rows, cols = rig.ctx, rig.rows, rig.cols
    nsc = len(f.scales)
    nodes = f.nodes(grid)
    # neighbour masks
    for s in range(3):
        want = f.scales[s].m if s < nsc else np.zeros((rows, cols), np.int64)
        assert np.array_equal(ctx.debug_nbr(slot, s, rows, cols), want), f"slot {slot}: neighbour masks differ at scale {s}"
    # node list
    state, nxt, steps, area = ctx.debug_nodes(slot)
    live = state != NONE
    want_states = sorted(cr.pack(x, y, s, sc, t) for sc, (nd, _) in enumerate(nodes) for (x, y, s), t in nd.items())
    assert sorted(state[live].tolist()) == want_states, f"slot {slot}: node list differs (lattice {grid})"
    direct = sum(v > BLOCK_STARTS for v in f.tile_nodes(grid).values())
    fc = ctx.debug_frame_counts(slot)
    assert fc["nodes"] == len(state)
    if direct == 0:
        assert live.all() and fc["nodes"] == len(want_states), f"slot {slot}: n_starts differs from the reference's node count"
    TALLY["tiles on the direct path"] += direct
    TALLY["padding entries"] += int((~live).sum())
    assert np.all(nxt[~live] == NONE)
    index = {int(v) & 0x1FFFFFFF: i for i, v in enumerate(state.tolist()) if v != NONE}
    for i in np.nonzero(live)[0].tolist():
        v = int(state[i])
        sc = (v >> 27) & 3
        k = (v & 0xFFF, (v >> 12) & 0xFFF, (v >> 24) & 7)
        to, n, a = nodes[sc][1][k]
        if to is None:
            assert nxt[i] == NONE, f"slot {slot}: node {k} scale {sc}: the walk should have been cut"
            TALLY["segments cut"] += 1
        else:
            assert nxt[i] != NONE and nxt[i] < len(state), f"slot {slot}: node {k} scale {sc}: no next node"
            assert int(state[nxt[i]]) & 0x1FFFFFFF == cr.pack(*to, sc, 0), f"slot {slot}: node {k} scale {sc}: next node differs"
            assert (int(steps[i]), int(area[i])) == (n, a), f"slot {slot}: node {k} scale {sc}: steps / shoelace differ"
            note_max("longest segment", n)
        TALLY["nodes " + ("cut", "outer", "hole")[(v >> 29) & 3]] += 1
    # kept contours
    pos = []
    for s in range(3):
        kept = f.scales[s].kept if s < nsc else []
        # (buffers a little larger than the reference's lists: a longer list from the kernels is an error of the getter)
        gs, gk, gp = ctx.debug_contours(slot, s, len(kept) + 8, sum(len(b.pts) for b in kept) + 64)
        assert gs.tolist() == [len(b.pts) for b in kept], f"slot {slot}: contour sizes differ at scale {s} (lattice {grid}, serial {serial})"
        assert gk.tolist() == [b.key for b in kept], f"slot {slot}: contour keys differ at scale {s}"
        assert np.array_equal(gp, np.array([p for b in kept for p in b.pts], np.int64).reshape(-1, 2)), f"slot {slot}: contour points differ at scale {s}"
        pos.append({(x, y, d): (ib, ip) for ib, b in enumerate(kept) for ip, ((x, y), d) in enumerate(zip(b.pts, b.dirs))})
    cnts = f.counts()
    assert (fc["contours"], fc["points"]) == (cnts["contours"], cnts["points"])
    # write tickets
    tstate, tci, trel, tcnt = ctx.debug_write_tickets(slot)
    assert fc["write_tickets"] == len(tstate)
    cover = [[np.zeros(len(b.pts), np.int64) for b in f.scales[s].kept] for s in range(nsc)]
    owner = {}
    for v, ci, rel, cnt in zip(tstate.tolist(), tci.tolist(), trel.tolist(), tcnt.tolist()):
        if ci == NONE:
            assert serial, "an unused ticket from k_link"
            TALLY["tickets reserved, unused"] += 1
            continue
        sc = (v >> 27) & 3
        k = (v & 0xFFF, (v >> 12) & 0xFFF, (v >> 24) & 7)
        assert k in nodes[sc][0], f"slot {slot}: a ticket starts from a state that is no node"
        assert k in pos[sc], f"slot {slot}: a ticket on a border that is not kept"
        ib, ip = pos[sc][k]
        n = len(cover[sc][ib])
        skip, c = cnt >> 16, cnt & 0xFFFF
        assert owner.setdefault(ci, (sc, ib)) == (sc, ib), f"slot {slot}: contour index {ci} on two borders"
        assert rel < n and c >= 1 and (ip + skip) % n == rel, f"slot {slot}: ticket offset {rel} is not where its state and skip lead"
        if serial:
            assert skip == 0
        else:
            assert c <= 64 and skip < nodes[sc][1][k][1], f"slot {slot}: ticket of {c} points, skip {skip}"
        note_max("largest skip", skip)
        cover[sc][ib][(rel + np.arange(c)) % n] += 1
        TALLY["tickets"] += 1
    assert len(set(owner.values())) == len(owner) == cnts["contours"], f"slot {slot}: tickets name {len(owner)} contours of {cnts['contours']}"
    assert all((c == 1).all() for per in cover for c in per), f"slot {slot}: the tickets do not cover every point exactly once"
    # which form
    got = ctx.debug_link_todo(slot)
    if todo is None:
        todo = 1 if serial and len(want_states) > 0 else 0
    assert got == todo == fc["serial_link"], f"slot {slot}: link_todo {got}, expected {todo}"
    TALLY["frames resolved by " + ("k_link_serial" if got else "k_link")] += 1


def run_case(rig, imgs, grids=(32, 64), forms=(False, True), first=0, lds_nodes=None, todo=None):
    """stage imgs in slots first.., run the contour stage at every lattice and through both link forms, check every slot.
    lds_nodes / todo: a hand-over limit for the LDS form of this case and the link_todo it must give"""
    refs = [rig.ref(im) for im in imgs]
    for f in refs:                                                 # the capacities hold the reference's own counts: no overflow below
        c = f.counts(32)
        assert c["nodes"] + 16 <= rig.caps["nodes"] and c["contours"] <= rig.caps["contours"] and c["points"] <= rig.caps["points"], c
    rig.ctx.stage_frames(np.stack(imgs), first)
    for grid in grids:
        for serial in forms:
            rig.ctx.run_contours(first, len(imgs), grid, 0 if serial else (-1 if lds_nodes is None else lds_nodes))
            pitch = grid or (32 if len(imgs) == 1 else 64)          # 0: the lattice a detection call of that many frames takes
            for i, f in enumerate(refs):
                want = None if serial else todo
                if want == "by count":                              # the LDS form takes a frame of at most lds_nodes nodes
                    want = 1 if f.counts(pitch)["nodes"] > lds_nodes else 0
                check_slot(rig, first + i, f, pitch, serial or want == 1, want)
            TALLY["runs"] += 1
    return refs


# ---- image builders: 0 / 255 patterns without solid 3 x 3 dark blocks are reproduced exactly at every default scale -------------
def canvas(rows, cols):
    return np.full((rows, cols), BRIGHT, np.uint8)


def ring(img, x0, y0, w, h):
    img[y0, x0:x0 + w] = DARK; img[y0 + h - 1, x0:x0 + w] = DARK
    img[y0:y0 + h, x0] = DARK; img[y0:y0 + h, x0 + w - 1] = DARK


def checker(img, x0, y0, w, h):
    yy, xx = np.mgrid[y0:y0 + h, x0:x0 + w]
    img[y0:y0 + h, x0:x0 + w][(xx + yy) % 2 == 0] = DARK


def spiral(rows, cols, step, margin=2):
    img = canvas(rows, cols)
    x0, y0, x1, y1 = margin, margin, cols - 1 - margin, rows - 1 - margin
    while x1 - x0 > 2 * step and y1 - y0 > 2 * step:
        img[y0, x0:x1 + 1] = DARK
        img[y0:y1 + 1, x1] = DARK
        img[y1, x0 + step:x1 + 1] = DARK
        img[y0 + step:y1 + 1, x0 + step] = DARK
        img[y0 + step, x0 + step:x1 - step + 1] = DARK
        x0 += step; y0 += step; x1 -= step; y1 -= step
    return img


def comb(rows, cols, pitch=4):
    img = canvas(rows, cols)
    img[3:rows - 3, 2:cols - 2:pitch] = DARK
    img[3, 2:cols - 2] = DARK
    return img


def staircase(img, x0, y0, n, dx=1):
    for i in range(n):
        x, y = x0 + dx * i, y0 + i
        if 0 <= y < img.shape[0] and 0 <= x < img.shape[1]:
            img[y, x] = DARK
        if 0 <= y < img.shape[0] and 0 <= x + dx < img.shape[1] and i % 3 == 0:
            img[y, x + dx] = DARK


def edge_pattern(rows, cols):
    """touches all four edges and corners, runs along and across the tile seams (x = 64 k, y = 32 k) and just inside the halo"""
    img = canvas(rows, cols)
    img[0, :] = DARK; img[rows - 1, :] = DARK; img[:, 0] = DARK; img[:, cols - 1] = DARK      # frame ring: corners and edges
    for x in (63, 64, 11, 12, cols - 13):
        if 2 < x < cols - 3:
            img[2:rows - 2, x] = np.where(np.arange(2, rows - 2) % 7 == 0, BRIGHT, DARK)
    for y in (31, 32, 12, rows - 13):
        if 2 < y < rows - 3:
            img[y, 2:cols - 2] = np.where(np.arange(2, cols - 2) % 5 == 0, BRIGHT, DARK)
    if rows > 8 and cols > 8:
        staircase(img, 2, 2, min(rows, cols) - 4)
    # no solid 3 x 3 block may remain: punch the centre of any
    d = img == DARK
    p = np.pad(d, 1)
    solid = np.ones_like(d)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            solid &= p[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols]
    img[solid] = BRIGHT
    return img


# ---- frame and tile geometry -------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 70), (70, 1), (31, 63), (32, 64), (33, 65), (64, 128), (97, 129)])
def test_frame_and_tile_geometry(rows, cols):
    rig = Rig(rows, cols, batch=2, minMarkerPerimeterRate=0.03)
    a = edge_pattern(rows, cols)
    b = canvas(rows, cols)
    b[::2, ::3] = DARK                                              # isolated pixels
    if min(rows, cols) == 1:                                        # a one-pixel-wide frame: runs of 1, 2 and 3 pixels, the ends included
        a = canvas(rows, cols)
        if rows * cols > 1:
            a.reshape(-1)[[0, 1, 5, 6, 7, 20, 30, 31, 68, 69]] = DARK
    else:
        b[rows // 2, :] = DARK
    refs = run_case(rig, [a, b])
    if rows * cols > 1:
        assert refs[0].counts(32)["nodes"] > 0


# ---- input paths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [60, 61, 64, 66, 67, 68, 100])
def test_gray_input_paths(cols):
    """row steps that are and are not a multiple of 4 (dword path with its edge dword / byte path); on the dword path the last
    columns differ from their neighbours so that a dword read one short or one long shows; slot 1 of an odd-sized frame starts at an
    odd byte offset"""
    rows = 33
    rng = np.random.RandomState(cols)
    rig = Rig(rows, cols, batch=2)
    imgs = []
    for k in range(2):
        img = np.kron(rng.randint(0, 256, (rows // 3 + 1, cols // 3 + 1)), np.ones((3, 3))).astype(np.uint8)[:rows, :cols].copy()
        img[:, cols - 5:] = rng.randint(0, 256, (rows, 5))
        img[:, :5] = rng.randint(0, 256, (rows, 5))
        imgs.append(img)
    run_case(rig, imgs)
    TALLY["gray path " + ("dword" if cols % 4 == 0 else "byte")] += 1
    TALLY["slot at an odd byte offset"] += (rows * cols) % 2


def test_bgr_input():
    rows, cols = 33, 65
    rng = np.random.RandomState(3)
    rig = Rig(rows, cols, batch=2)
    imgs = [np.kron(rng.randint(0, 256, (rows // 3 + 1, cols // 3 + 1, 3)), np.ones((3, 3, 1))).astype(np.uint8)[:rows, :cols].copy() for _ in range(2)]
    assert not np.array_equal(imgs[0][..., 0], imgs[0][..., 1]) and not np.array_equal(imgs[0][..., 1], imgs[0][..., 2])
    # a weight swapped between channels shows on a frame that is bright in one channel only
    imgs[1][:, :20] = (255, 0, 0); imgs[1][:, 20:40] = (0, 255, 0); imgs[1][:, 40:] = (0, 0, 255)
    imgs[1][5:28:2, 3:60] //= 3
    run_case(rig, imgs)


# ---- the threshold decision on its limit -------------------------------------------------------------------
def limit_image(rows, cols, k, t, up, v):
    """a frame of value t whose k x k window around the centre pixel sums to k^2 t + (k^2 - 1) / 2 + up (mean t for up = 0, t + 1 for
    up = 1: t + 1/2 -+ 1 / (2 k^2) before rounding), centre value v; None where no window of 8-bit values has that sum"""
    img = np.full((rows, cols), min(t, 255), np.uint8)
    cy, cx, r = rows // 2, cols // 2, k // 2
    cells = [(y, x) for y in range(cy - r, cy + r + 1) for x in range(cx - r, cx + r + 1) if (y, x) != (cy, cx)]
    total = k * k * t + (k * k - 1) // 2 + up
    base, rem = divmod(total - v, len(cells))
    if base < 0 or base + (1 if rem else 0) > 255:
        return None
    for i, (y, x) in enumerate(cells):
        img[y, x] = base + (1 if i < rem else 0)
    img[cy, cx] = v
    assert int(img[cy - r:cy + r + 1, cx - r:cx + r + 1].astype(np.int64).sum()) == total
    return img


@pytest.mark.parametrize("C", [0.0, 7.0, 9.5, 254.9])
def test_threshold_on_the_limit(C):
    rows, cols = 33, 65
    ic = int(C // 1)
    t = 254 if ic > 200 else ic + 30
    reached = collections.Counter()
    for windows in ((3, 23, 10), (5, 5, 10)):
        rig = Rig(rows, cols, batch=16, adaptiveThreshWinSizeMin=windows[0], adaptiveThreshWinSizeMax=windows[1], adaptiveThreshWinSizeStep=windows[2],
                  adaptiveThreshConstant=C)
        batch = []
        for s, k in enumerate(rig.windows):
            imgs, wanted = [], []
            for up in (0, 1):
                mean = t + up
                for v in (mean - ic, mean - ic + 1):
                    img = limit_image(rows, cols, k, t, up, v) if 0 <= v <= 255 else None
                    if img is None:
                        # no 8-bit window has this sum: a centre that dark pulls the mean of a small window below v + C
                        assert not 0 <= v <= 255 or (k * k - 1) * 255 + v < k * k * t + (k * k - 1) // 2 + up, (k, t, up, v)
                        reached["no such window"] += 1
                        continue
                    imgs.append(img)
                    wanted.append(v - mean <= -ic)
            got = [bool(rig.ref(im).scales[s].fg[rows // 2, cols // 2]) for im in imgs]
            assert got == wanted, (k, C, got, wanted)
            reached["foreground"] += sum(got); reached["background"] += len(got) - sum(got)
            batch += imgs
        if batch:
            run_case(rig, batch)                                    # the cases of every window of the rig in one call per lattice and form
    TALLY["threshold limit cases"] += reached["foreground"] + reached["background"]
    assert reached["foreground"] >= 2 and reached["background"] >= 2, reached


def test_threshold_saturated_and_corners():
    rows, cols = 33, 65
    for C in (0.0, 7.0):
        rig = Rig(rows, cols, batch=4, adaptiveThreshConstant=C)
        z, o = np.zeros((rows, cols), np.uint8), np.full((rows, cols), 255, np.uint8)
        c = canvas(rows, cols)
        for y, x in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)):   # corners: the halo is all replication
            c[y, x] = 120
        c[0, 1] = 0; c[rows - 1, cols - 2] = 0; c[1, cols - 1] = 130
        d = canvas(rows, cols)
        d[:12, :12] = 100; d[0, 0] = 94; d[-12:, -12:] = 100; d[-1, -1] = 93
        run_case(rig, [z, o, c, d])


# ---- runtime windows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("wmin,wmax,step", [(7, 7, 10), (5, 15, 10), (5, 23, 9), (23, 23, 10), (3, 23, 20)])
def test_runtime_windows(wmin, wmax, step):
    rows, cols = 64, 128
    rng = np.random.RandomState(wmin * 100 + wmax)
    rig = Rig(rows, cols, batch=2, adaptiveThreshWinSizeMin=wmin, adaptiveThreshWinSizeMax=wmax, adaptiveThreshWinSizeStep=step)
    if (wmin, wmax, step) == (5, 23, 9):
        assert rig.windows == [5, 15, 23]                           # the even 14 is bumped to odd
    blobs = np.kron(rng.randint(0, 256, (rows // 8 + 1, cols // 8 + 1)), np.ones((8, 8))).astype(np.uint8)[:rows, :cols].copy()
    blobs[:, :3] = rng.randint(0, 256, (rows, 3)); blobs[-2:, :] = rng.randint(0, 256, (2, cols))
    run_case(rig, [blobs, edge_pattern(rows, cols)])
    TALLY["runtime window sets"] += 1


def test_window_25_is_refused():
    rig = Rig(33, 65)
    with pytest.raises(capi.AslamError) as e:
        rig.ctx.set_detector_params(adaptiveThreshWinSizeMin=25, adaptiveThreshWinSizeMax=25, adaptiveThreshWinSizeStep=10)
    assert e.value.code == -1
    with pytest.raises(capi.AslamError):
        rig.ctx.set_detector_params(adaptiveThreshWinSizeMin=5, adaptiveThreshWinSizeMax=24, adaptiveThreshWinSizeStep=19)   # 24 is bumped to 25
    run_case(rig, [edge_pattern(33, 65)])                              # the parameters in force are unchanged


# ---- lattice ---------------------------------------------------------------------------------------------
def lattice_image(rows, cols):
    img = canvas(rows, cols)
    img[64, 3:50] = DARK                                            # on a lattice line of both pitches for its whole length
    img[2:60, 32] = DARK                                            # on a line of pitch 32 only
    staircase(img, 70, 2, 50)                                       # crosses lines diagonally
    ring(img, 70, 70, 20, 10)                                       # touches no line of pitch 64, crosses none of pitch 32
    ring(img, 40, 33, 9, 9)                                         # never touches either lattice
    ring(img, 97, 70, 8, 27)                                        # touches y = 96 along one side, x = 96 nowhere
    img[90:93, 96] = DARK; img[89, 95] = DARK; img[89, 97] = DARK   # a stem on x = 96 with two arms off it
    for d in range(1, 4):                                           # a spur junction on the lattice crossing (64, 64): four diagonal arms
        img[64 - d, 64 - d] = DARK; img[64 - d, 64 + d] = DARK; img[64 + d, 64 - d] = DARK; img[64 + d, 64 + d] = DARK
    img[64, 64] = DARK
    ring(img, 30, 94, 5, 3)
    img[96, 32] = BRIGHT                                            # a ring that touches the lattice crossing (32, 96) in its gap only
    img[20, 62] = DARK; img[21, 63] = DARK; img[22, 64] = DARK; img[23, 63] = DARK; img[24, 62] = DARK   # touches x = 64 in one pixel
    return img


def test_lattice_families():
    rows, cols = 97, 129
    rig = Rig(rows, cols, batch=3)
    img = lattice_image(rows, cols)
    f = rig.ref(img)
    m = int(f.scales[0].m[64, 64])
    per_pixel = collections.Counter((x, y) for (x, y, s) in f.nodes(64)[0][0])
    note_max("nodes on one pixel", max(per_pixel.values()))
    assert per_pixel[(64, 64)] == 4 == max(per_pixel.values()), (bin(m), per_pixel[(64, 64)])   # alternating neighbours: the most a pixel can carry
    only_cands = canvas(rows, cols)
    ring(only_cands, 35, 35, 20, 20); ring(only_cands, 70, 5, 20, 20); only_cands[40:50, 40] = DARK
    g = rig.ref(only_cands)
    assert all(t != cr.CUT for nd, _ in g.nodes(32) for t in nd.values()), "a border that never touches the lattice has cut nodes"
    run_case(rig, [img, only_cands, comb(rows, cols)])


def test_border_across_many_lattice_lines():
    rows, cols = 40, 300
    rig = Rig(rows, cols, maxMarkerPerimeterRate=8.0)
    img = canvas(rows, cols)
    img[20, 2:298] = DARK                                           # crosses 9 lines of pitch 32
    staircase(img, 3, 3, 33, dx=8)
    f = rig.ref(img)
    assert sum(1 for (x, y, s), t in f.nodes(32)[0][0].items() if y == 20 and t == cr.CUT) >= 16
    run_case(rig, [img])


# ---- topology ---------------------------------------------------------------------------------------------
def topology_image(rows, cols):
    img = canvas(rows, cols)
    img[3, 3] = DARK                                                # single pixel: no border
    img[3, 8] = DARK; img[3, 9] = DARK                              # 2-pixel components: E, S, SE, SW neighbours
    img[3, 13] = DARK; img[4, 13] = DARK
    img[3, 17] = DARK; img[4, 18] = DARK
    img[3, 23] = DARK; img[4, 22] = DARK
    img[10, 3:20] = DARK; img[7:10, 8] = DARK; img[11, 14] = DARK   # a line with one-pixel spurs that double back
    ring(img, 30, 3, 25, 25); ring(img, 34, 7, 17, 17); ring(img, 38, 11, 9, 9); img[15, 42] = DARK   # holes in holes
    for i in range(12):                                             # 8-connected diagonals
        img[30 + i, 3 + i] = DARK; img[30 + i, 28 - i] = DARK
    ring(img, 60, 3, 12, 12); img[4:9, 65] = DARK; img[8, 61:65] = DARK      # a hole split in two; walls shared
    ring(img, 80, 3, 10, 10); img[4, 81] = DARK                     # spur inside the hole at its corner
    ring(img, 60, 20, 11, 11)
    for i in range(1, 10):                                          # a diagonal inside the ring: its holes touch the outer border in one pixel
        img[20 + i, 60 + i] = DARK
    ring(img, 80, 20, 9, 9); ring(img, 88, 24, 9, 9)                # two rings sharing one pixel column: an outer start on another's hole border
    ring(img, 100, 3, 7, 7); img[3, 100] = BRIGHT                   # a ring open at its corner (8-connected closure)
    checker(img, 3, 50, 30, 20)                                     # pixel checkerboard
    checker(img, 60, 45, 9, 9); ring(img, 58, 43, 13, 13)           # ... inside a ring
    img[60:80, 100:120:2] = DARK; img[60, 100:119] = DARK           # comb
    img[82:92:3, 3:40] = DARK; img[82:92, 3:40:3] = DARK            # a grid of one-pixel lines: many holes on shared walls
    return img


def test_topology():
    rows, cols = 97, 129
    rig = Rig(rows, cols)
    img = topology_image(rows, cols)
    f = rig.ref(img)
    b0 = f.scales[0].borders
    assert sum(len(b.pts) == 1 for b in b0) >= 1 and sum(len(b.pts) == 2 for b in b0) >= 4 and sum(b.hole for b in b0) >= 100
    run_case(rig, [img])


# ---- perimeter limits ---------------------------------------------------------------------------------------
def shapes_of_many_sizes(rows, cols):
    img = canvas(rows, cols)
    y = 2
    for L in range(2, 22):
        img[y, 3:3 + L] = DARK                                      # a line: 2 L - 2 points
        img[y, 40:40 + L] = DARK; img[y + 1, 40] = DARK             # ... with a corner pixel: an odd count
        w = 3 + L // 2
        if y + 1 < rows - 6:
            ring(img, 80, y, w, 3) if L % 2 else None
        y += 4
    return img


def test_perimeter_limits_exact():
    rows, cols = 97, 129
    rig = Rig(rows, cols, minMarkerPerimeterRate=0.1, maxMarkerPerimeterRate=0.25)
    assert (rig.lo, rig.hi) == (12, 32)
    img = shapes_of_many_sizes(rows, cols)
    f = rig.ref(img)
    sizes = {len(b.pts) for b in f.scales[0].borders}
    assert {rig.lo - 1, rig.lo, rig.hi, rig.hi + 1} <= sizes, sorted(sizes)
    kept = {len(b.pts) for b in f.scales[0].kept}
    assert rig.lo in kept and rig.hi in kept and rig.lo - 1 not in kept and rig.hi + 1 not in kept
    run_case(rig, [img])


def test_one_node_border_at_max_perim():
    """off-lattice lines, one outer node each: 2 L - 2 points.  With max_perim = 33 the line of 17 pixels (32 points) and a line with a
    corner pixel (33 points) close on their own node after max_perim steps or fewer; the line of 18 pixels (34 = max_perim + 1 points)
    is cut on its last step, where it stands on its own node again"""
    rows, cols = 40, 72
    rig = Rig(rows, cols, minMarkerPerimeterRate=2.5 / 72, maxMarkerPerimeterRate=33.5 / 72)
    assert (rig.lo, rig.hi) == (2, 33)
    img = canvas(rows, cols)
    img[5, 3:21] = DARK                                             # 34 points
    img[12, 3:20] = DARK                                            # 32 points
    img[19, 3:20] = DARK; img[20, 19] = DARK                        # 33 points (a corner pixel that is no start candidate)
    f = rig.ref(img)
    sizes = sorted(len(b.pts) for b in f.scales[0].borders)
    assert sizes == [32, 33, 34], sizes
    for grid in (32, 64):
        seg = f.nodes(grid)[0][1]
        assert len(seg) == 3 and sorted((to is None, n) for to, n, a in seg.values()) == [(False, 32), (False, 33), (True, 34)], seg
    before = TALLY["segments cut"]
    run_case(rig, [img])
    assert TALLY["segments cut"] == before + 3 * 4                  # one per scale, in each of the four runs


def test_long_border_cut_next_to_kept_ones():
    rows, cols = 97, 129
    rig = Rig(rows, cols, minMarkerPerimeterRate=0.05, maxMarkerPerimeterRate=0.5)
    img = spiral(rows, cols, 6, margin=10)
    for k in range(6):
        ring(img, 2 + 20 * k, 1, 8, 7)
    ring(img, 1, 30, 7, 9); ring(img, 120, 40, 8, 8)
    f = rig.ref(img)
    nodes = f.nodes(32)
    assert any(to is None for _, seg in nodes for to, n, a in seg.values()), "no walk is cut at max_perim"
    assert any(len(b.pts) > rig.hi for b in f.scales[0].borders) and len(f.scales[0].kept) >= 8
    before = TALLY["segments cut"]
    run_case(rig, [img])
    assert TALLY["segments cut"] > before


def test_largest_max_perim():
    rows, cols = 140, 256
    rate = 65534.0 / 256                                            # exact in binary: the largest rate set_detector_params accepts here
    rig = Rig(rows, cols, starts=1 << 15, contours=1 << 8, points=1 << 18, maxMarkerPerimeterRate=rate)
    assert rig.hi == 65534
    with pytest.raises(capi.AslamError):
        rig.ctx.set_detector_params(maxMarkerPerimeterRate=65534.5 / 256)
    img = spiral(rows, cols, 2, margin=1)
    f = rig.ref(img)
    longest = max(len(b.pts) for b in f.scales[0].borders)
    note_max("longest kept border", longest)
    assert 32768 < longest <= rig.hi and longest == max(len(b.pts) for b in f.scales[0].kept), longest
    run_case(rig, [img])


# ---- the per-tile staging limit ---------------------------------------------------------------------------
_TILES = {}


def tile_filled_to(target):
    """a 32 x 64 frame (one tile) whose nodes at lattice 64 number exactly `target`, by the reference's count: a pixel checkerboard
    (one hole-type node per dark pixel and scale) painted pixel by pixel, with up to two 3 x 3 grey blocks (a ring at window 3, solid
    at the others) to reach counts that are no multiple of 3"""
    rows, cols = 32, 64
    if "rig" not in _TILES:
        _TILES["rig"] = Rig(rows, cols, starts=1 << 12, contours=1 << 11, points=1 << 14)
    rig = _TILES["rig"]
    cells = [(y, x) for y in range(6, 31) for x in range(1, 63) if (x + y) % 2 == 0]
    for blocks in range(3):
        for n in range(target // 3 - 30, target // 3 + 10):
            img = canvas(rows, cols)
            for b in range(blocks):
                img[1:4, 2 + 5 * b:5 + 5 * b] = 100
            for y, x in cells[:n]:
                img[y, x] = DARK
            if cr.count_nodes(img, rig.windows, rig.C, 64) == target:
                return rig, img
    raise AssertionError(f"no image with exactly {target} nodes found")


@pytest.mark.parametrize("target,direct", [(1024, 0), (1025, 1), (1100, 1)])
def test_tile_staging_limit(target, direct):
    rig, img = tile_filled_to(target)
    f = rig.ref(img)
    assert f.counts(64)["nodes"] == target and f.tile_nodes(64)[(0, 0)] == target
    before = TALLY["tiles on the direct path"]
    run_case(rig, [img], grids=(64,))
    assert (TALLY["tiles on the direct path"] > before) == bool(direct)
    run_case(rig, [img], grids=(32,))


# ---- the LDS node limit and the slot limit ---------------------------------------------------------------------
def test_lds_node_limit_by_argument():
    rows, cols = 97, 129
    rig = Rig(rows, cols)
    img = topology_image(rows, cols)
    for grid in (32, 64):
        n = rig.ref(img).counts(grid)["nodes"]
        run_case(rig, [img], grids=(grid,), forms=(False,), lds_nodes=n, todo=0)
        run_case(rig, [img], grids=(grid,), forms=(False,), lds_nodes=n - 1, todo=1)


def test_lds_node_limit_at_the_constant():
    """exactly kLinkLdsNodes = 32 000 nodes and one piece more, by the reference's count: a checkerboard brings the count close, 2-pixel
    pieces (one outer node per scale) and grey 3 x 3 blocks (a ring at window 3, solid at the others: 4 nodes) make it exact"""
    rows, cols = 150, 200
    rig = Rig(rows, cols, starts=1 << 16, contours=1 << 15, points=1 << 18)
    assert rig.lo > 4                                               # the 4-point hole borders of the checkerboard are not kept: few slots
    count = lambda im: cr.count_nodes(im, rig.windows, rig.C, 64)
    for w in range(138, 120, -1):                                   # the widest checkerboard that leaves room for the pieces
        base = canvas(rows, cols)
        checker(base, 1, 1, w, rows - 2)
        deficit = LINK_LDS_NODES - count(base)
        if deficit >= 12:
            break
    assert 12 <= deficit <= 1200, deficit
    nb = deficit % 3
    na = (deficit - 4 * nb) // 3
    spots = [(x, y) for y in range(2, rows - 5, 4) for x in range(146, cols - 5, 5) if 3 < y % 64 < 59 and 3 < x % 64 < 58]
    assert len(spots) > na + nb + 1
    at = base.copy()
    for i, (x, y) in enumerate(spots[:na + nb]):
        if i < nb:
            at[y:y + 3, x:x + 3] = 100
        else:
            at[y, x] = DARK; at[y + 1, x] = DARK
    over = at.copy()
    x, y = spots[na + nb]
    over[y, x] = DARK; over[y + 1, x] = DARK
    assert count(at) == LINK_LDS_NODES and count(over) == LINK_LDS_NODES + 3
    run_case(rig, [at], grids=(64,), forms=(False,), todo=0)
    run_case(rig, [over], grids=(64,), forms=(False,), todo=1)


def ring_lattice(rows, cols, n_rings, extra_block, extra_line):
    img = canvas(rows, cols)
    k = 0
    for y in range(1, rows - 4, 4):
        for x in range(1, cols - 4, 4):
            if k < n_rings:
                ring(img, x, y, 3, 3)
            elif k < n_rings + extra_block:
                img[y:y + 3, x:x + 3] = 100
            elif k < n_rings + extra_block + extra_line:
                img[y, x:x + 3] = DARK
            k += 1
    assert k >= n_rings + extra_block + extra_line
    return img


def test_slot_limit():
    """exactly kLinkSlots = 1536 and 1537 kept borders (reference's count): a ring gives an outer and a hole border at each of the three
    scales, a grey 3 x 3 block a ring at window 3 and one border at the others, a short line one border per scale"""
    rows, cols = 97, 129
    rig = Rig(rows, cols, starts=1 << 15, contours=1 << 11, points=1 << 15, minMarkerPerimeterRate=0.03)
    assert rig.lo <= 4
    at = ring_lattice(rows, cols, 256, 0, 0)
    over = ring_lattice(rows, cols, 255, 1, 1)
    assert rig.ref(at).counts()["contours"] == LINK_SLOTS and rig.ref(over).counts()["contours"] == LINK_SLOTS + 1
    run_case(rig, [at], forms=(False,), todo=0)
    run_case(rig, [over], forms=(False,), todo=1)
    run_case(rig, [over], forms=(True,), grids=(64,))


# ---- batches ---------------------------------------------------------------------------------------------
def batch_images(rows, cols, n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        kind = i % 5
        if kind == 0:
            img = canvas(rows, cols)                                # blank
        elif kind == 1:
            img = comb(rows, cols, 3 + i % 3)
        elif kind == 2:
            img = spiral(rows, cols, 3 + i % 4)
        elif kind == 3:
            img = np.kron(rng.randint(0, 256, (rows // 4 + 1, cols // 4 + 1)), np.ones((4, 4))).astype(np.uint8)[:rows, :cols].copy()
        else:
            img = canvas(rows, cols)
            ring(img, 2 + i % 7, 3, 12, 9); ring(img, 30, 5 + i % 5, 6, 6)
        out.append(img)
    return out


@pytest.mark.parametrize("n,first", [(2, 0), (3, 1), (9, 2)])
def test_batches(n, first):
    """different content per slot, first > 0, blank frames first, last and between busy ones (equal entries in the prefix); every frame
    must equal what the reference says of it alone"""
    rows, cols = 40, 72
    rig = Rig(rows, cols, batch=12)
    imgs = batch_images(rows, cols, n, n)
    if n == 9:
        imgs[-1] = canvas(rows, cols); imgs[4] = canvas(rows, cols); imgs[5] = canvas(rows, cols)
    run_case(rig, imgs, first=first)


def test_batch_of_300_frames():
    """more than one frame per thread in k_prefix, and the ticket search over many frames; frames of more than 60 nodes go to the serial
    form, so both forms work side by side in one call"""
    rows, cols = 40, 72
    rig = Rig(rows, cols, batch=300, starts=1 << 11, contours=1 << 8, points=1 << 12)
    base = batch_images(rows, cols, 10, 7)
    imgs = [base[(i * 7) % 10] if i % 11 else canvas(rows, cols) for i in range(300)]
    before = (TALLY["frames resolved by k_link"], TALLY["frames resolved by k_link_serial"])
    run_case(rig, imgs, grids=(0,), forms=(False,), lds_nodes=60, todo="by count")
    assert TALLY["frames resolved by k_link"] >= before[0] + 50 and TALLY["frames resolved by k_link_serial"] >= before[1] + 50


# ---- capacities ---------------------------------------------------------------------------------------------
def overflow_then_exact(rig, bad, good, bit):
    rig.ctx.stage_frames(bad)
    for lds_nodes in (-1, 0):                                       # the overflow branches of k_link and of k_link_serial
        with pytest.raises(capi.AslamError) as e:
            rig.ctx.run_contours(0, 1, 64, lds_nodes)
        assert e.value.code == -4 and f"mask 0x{bit:x}" in str(e.value), str(e.value)
        if bit != 1:                                                # (a frame that overflows the node list is never linked)
            assert rig.ctx.debug_link_todo(0) == (1 if lds_nodes == 0 else 0)
    run_case(rig, [good], grids=(64,))                               # the mask was cleared when it was reported
    TALLY["capacity errors met"] += 1


def test_capacity_starts():
    rows, cols = 40, 72
    rig = Rig(rows, cols, starts=256, contours=1 << 10, points=1 << 14)
    bad = canvas(rows, cols); checker(bad, 1, 1, 60, 30)
    assert cr.Frame(bad).counts(64)["nodes"] > 256
    overflow_then_exact(rig, bad, comb(rows, cols, 8), 1)


def test_capacity_contours():
    rows, cols = 40, 72
    rig = Rig(rows, cols, starts=1 << 13, contours=32, points=1 << 14, minMarkerPerimeterRate=0.03)
    bad = ring_lattice(rows, cols, 40, 0, 0)
    c = cr.Frame(bad, min_perim=rig.lo, max_perim=rig.hi).counts(64)
    assert c["contours"] > 32 and c["nodes"] < 1 << 13 and c["points"] < 1 << 14
    good = canvas(rows, cols); ring(good, 5, 5, 20, 20)
    overflow_then_exact(rig, bad, good, 2)


def test_capacity_points():
    rows, cols = 40, 72
    rig = Rig(rows, cols, starts=1 << 13, contours=1 << 10, points=512, maxMarkerPerimeterRate=40.0)
    bad = spiral(rows, cols, 3)
    c = cr.Frame(bad, min_perim=rig.lo, max_perim=rig.hi).counts(64)
    assert c["points"] > 512 and c["contours"] < 1 << 10 and c["nodes"] < 1 << 13
    good = canvas(rows, cols); ring(good, 5, 5, 20, 20)
    overflow_then_exact(rig, bad, good, 4)


def test_run_contours_arguments():
    rig = Rig(33, 65, batch=2)
    with pytest.raises(capi.AslamError) as e:
        rig.ctx.run_contours(0, 1, 64, -1)                          # nothing staged
    assert e.value.code == -5
    rig.ctx.stage_frames(canvas(33, 65))
    for bad in (1, 16, 48, 128, -32):
        with pytest.raises(capi.AslamError) as e:
            rig.ctx.run_contours(0, 1, bad, -1)
        assert e.value.code == -1
    with pytest.raises(capi.AslamError):
        rig.ctx.run_contours(1, 2, 0, -1)
    rig.ctx.run_contours(0, 1, 0, -1)
    assert rig.ctx.debug_frame_counts(0)["nodes"] == 0 and rig.ctx.debug_link_todo(0) == 0


# ---- random ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blocky", "scribble", "blobs"])
def test_random(kind):
    rows, cols = 97, 129
    rng = np.random.RandomState({"blocky": 11, "scribble": 12, "blobs": 13}[kind])
    rig = Rig(rows, cols, batch=2, starts=1 << 15, contours=1 << 12, points=1 << 17, maxMarkerPerimeterRate=40.0)
    imgs = []
    for _ in range(2):
        if kind == "blocky":
            img = np.kron(rng.randint(0, 256, (rows // 3 + 1, cols // 3 + 1)), np.ones((3, 3))).astype(np.uint8)[:rows, :cols].copy()
        elif kind == "scribble":
            img = canvas(rows, cols)
            x, y = cols // 2, rows // 2
            for _ in range(3000):
                img[y, x] = DARK
                x = min(max(x + rng.randint(-1, 2), 0), cols - 1); y = min(max(y + rng.randint(-1, 2), 0), rows - 1)
        else:
            yy, xx = np.mgrid[:rows, :cols]
            v = np.zeros((rows, cols))
            for _ in range(12):
                cx, cy, r = rng.randint(0, cols), rng.randint(0, rows), rng.randint(4, 20)
                v += np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * r * r))
            img = (255 - np.clip(v * 200, 0, 255)).astype(np.uint8)
        imgs.append(img)
    run_case(rig, imgs)


# ---- a real shape, on the GPU ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_at_720p_against_the_oracle():
    """8 frames at 720 x 1280 through the batch lattice (64): comb, spiral, ring lattice, blobs, one blank.  Against the oracle only (the
    Python reference is too slow at this size; the small shapes above tie reference, oracle and kernels together)"""
    rows, cols = 720, 1280
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[:rows, :cols]
    v = np.zeros((rows, cols))
    for _ in range(40):
        cx, cy, r = rng.randint(0, cols), rng.randint(0, rows), rng.randint(10, 80)
        v += np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * r * r))
    blobs = (255 - np.clip(v * 200, 0, 255)).astype(np.uint8)
    rings = canvas(rows, cols)
    for y in range(4, rows - 40, 37):
        for x in range(4, cols - 40, 41):
            ring(rings, x, y, 30, 26)
    imgs = [comb(rows, cols, 9), canvas(rows, cols), spiral(rows, cols, 7), rings, blobs, canvas(rows, cols), spiral(rows, cols, 13), comb(rows, cols, 5)]
    lo, hi = cr.perim_limits(rows, cols, 0.03, 40.0)
    want = []
    tot = collections.Counter()
    for img in imgs:
        per = []
        for k in (3, 13, 23):
            th = orc.threshold(img, k, 7.0)
            sizes, keys, hole, pts = orc.find_contours(th, 1 << 18, 1 << 23)
            sel = (sizes >= max(lo, 2)) & (sizes <= hi)
            offs = np.concatenate([[0], np.cumsum(sizes)])
            p = np.concatenate([pts[offs[i]:offs[i + 1]] for i in np.nonzero(sel)[0]]) if sel.any() else np.zeros((0, 2), np.int32)
            per.append((th, sizes[sel], keys[sel], p))
        want.append(per)
        tot["contours"] = max(tot["contours"], sum(len(p[1]) for p in per)); tot["points"] = max(tot["points"], sum(len(p[3]) for p in per))
    assert tot["contours"] <= 1 << 15 and tot["points"] <= 1 << 21, tot          # the capacities hold the oracle's counts
    ctx = capi.Context(max_rows=rows, max_cols=cols, max_batch=8, max_landmarks=16, cap_starts_per_frame=1 << 19, cap_contours_per_frame=1 << 15,
                       cap_points_per_frame=1 << 21)
    ctx.set_detector_params(maxMarkerPerimeterRate=40.0)
    ctx.stage_frames(np.stack(imgs))
    from parity_common import nbr_from_binary
    for lds in (-1, 0):
        ctx.run_contours(0, 8, 0, lds)
        for i, per in enumerate(want):
            for s, (th, sizes, keys, p) in enumerate(per):
                if lds == -1:
                    assert np.array_equal(ctx.debug_nbr(i, s, rows, cols), nbr_from_binary(th > 0)), f"frame {i}: masks differ at scale {s}"
                gs, gk, gp = ctx.debug_contours(i, s, 1 << 15, 1 << 21)
                assert np.array_equal(gs, sizes) and np.array_equal(gk, keys) and np.array_equal(gp, p), f"frame {i}: contours differ at scale {s}"
            TALLY["720p frames resolved by " + ("k_link_serial" if ctx.debug_link_todo(i) else "k_link")] += 1
        TALLY["720p contours"] += sum(len(p[1]) for per in want for p in per)
