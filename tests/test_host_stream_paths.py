"""The host-fed stream (aslam_stream_open / _push / _acquire / _commit / _flush and ring_submit, capi.hip) path by path: which frame
the detector saw in which ring slot, bgr8 and padded rows through the ring, partial and empty flushes, halves reused many times,
push mixed with acquire + commit, reopening, the refusals.

Every frame of a case is different (another subset of 2 to 4 markers out of 8 ids at other poses, another encoder sample with
wl != wr), so a stale slot, a frame seen twice, a row copied at the wrong pitch or a sample taken from the wrong slot changes ids,
corners or mu.  Every case is checked three ways:
 1. against a twin context that is fed, submit by submit as tests/ring_reference.py predicts them, through stage_frames /
    stage_encoders / run_staged(slot0, n): ring_submit issues exactly that call, so state, observations, per-slot results and the
    window plan are equal to the bit;
 2. against the oracle's detection of the frame the model places in every live slot (ids and corners equal, poses to
    parity_common.check_poses);
 3. against oracle.ekf_literal.LiteralSlam fed the oracle's detections and poses in frame order (tolerances of test_camera_rig.py).

These tests run on whatever library the session uses.  The CPU emulation executes copies synchronously: there they check addressing,
bookkeeping and refusals, but not the ordering between the copy stream, the detection stream and the EKF streams (ev_up, ev_det,
ev_ekf).  On the gfx950 library the upload of one half does overlap the processing of the other; the 1280 x 720 case at the end is
where an ordering error would show."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from oracle import pyoracle as orc
from oracle.ekf_literal import LiteralSlam
import parity_common as pc
import ring_reference as rr

E_INVALID, E_STATE = -1, -5
IDS = synth.unambiguous_ids(8, start=5)
# four places in the image that never touch: (camera-frame position, yaw), jittered per frame
SPOTS = (((-0.45, -0.2, 1.3), 0.2), ((0.4, -0.15, 1.5), -0.25), ((-0.1, 0.25, 1.2), 0.4), ((0.35, 0.3, 1.6), -0.5))
# shape families: rows, cols, focal length, channels.  "odd" is off the 64-pixel pitch and off the tile grid, inside a 240 x 320 context
SHAPES = {"gray": (240, 320, 260.0, 1), "bgr": (240, 320, 260.0, 3), "odd": (203, 277, 225.0, 1),
          "tiny": (64, 64, 64.0, 1)}
POOL = 24                                                     # frames per family; no case needs more
D0 = np.zeros(5)
CHECKED = {}                                                  # case name -> frames checked against the oracle slot by slot


def frame_spec(key, i):
    """marker ids and poses of frame i"""
    if key == "tiny":                                         # two small markers side by side
        ids = [IDS[(3 * i) % 8], IDS[(3 * i + 1) % 8]]
        spots = [((-0.19 + 0.004 * math.sin(i), 0.01 * math.cos(i), 0.8), 0.2), ((0.19, -0.01 * math.sin(2.0 * i), 0.8 + 0.004 * math.cos(i)), -0.2)]
    else:
        n = 2 + i % 3
        ids = [IDS[(5 * i + k) % 8] for k in range(n)]
        spots = []
        for k in range(n):
            (x, y, z), yaw = SPOTS[(i + k) % 4]
            spots.append(((x + 0.03 * math.sin(1.7 * i + k), y + 0.02 * math.cos(2.3 * i + k), z + 0.04 * math.sin(0.9 * i + 2 * k)),
                          yaw + 0.1 * math.sin(1.3 * i + k)))
    poses = np.zeros((len(ids), 12))
    for k, (t, yaw) in enumerate(spots):
        R, tt = synth.marker_pose(t, yaw)
        poses[k, :9] = R.reshape(-1)
        poses[k, 9:] = tt
    return ids, poses


def encoder(i):
    return 2.0 + 0.13 * i, 1.5 - 0.07 * i, 0.03 + 0.001 * (i % 5)


def camera(key):
    rows, cols, f, _ = SHAPES[key]
    return synth.camera_matrix(rows, cols, f)


@functools.lru_cache(maxsize=None)
def renderer(max_rows, max_cols):
    return capi.Context(max_rows=max_rows, max_cols=max_cols, max_batch=1, persistent_waves=4)


def oracle_detect(img, K, D=D0):
    ids, corners = orc.detect(img)
    rv = np.zeros((len(ids), 3)); tv = np.zeros((len(ids), 3))
    for j in range(len(ids)):
        rv[j], tv[j], _ = orc.solve_pnp(corners[j], 0.27, K, D)
    return ids, corners, rv, tv


@functools.lru_cache(maxsize=None)
def pool(key):
    """the family's frames, rendered once, with the oracle's detections and poses: [(image, encoder sample, oracle result)].  The
    oracle finds at least 2 markers on every frame and consecutive frames' id sets differ, asserted before any library call of a case."""
    rows, cols, _, ch = SHAPES[key]
    K = camera(key)
    out = []
    for i in range(POOL):
        ids, poses = frame_spec(key, i)
        img = renderer(max(rows, 64), max(cols, 64)).synth_render(0, rows, cols, K, ids, poses, noise_amp=2, seed=100 + i)
        if ch == 3:                                           # three distinct channels, so that the gray conversion matters
            img = np.ascontiguousarray(np.stack([np.roll(img, 1, 0), img, np.roll(img, -1, 1)], -1))
        det = oracle_detect(img, K)
        # (a white bar inside a marker may be read as id 1023 besides: the library must find that too)
        assert len(set(det[0].tolist()) & set(ids)) >= 2, f"{key} frame {i}: the oracle finds {det[0]} of {ids}"
        assert not out or set(det[0].tolist()) != set(out[-1][2][0].tolist()), f"{key} frames {i - 1}, {i}: same ids"
        img.setflags(write=False)
        out.append((img, encoder(i), det))
    assert all(e[0] != e[1] for _, e, _ in out)
    return out


def padded(img, pad, seed):
    """the same frame as a view into an array whose rows are `pad` bytes longer, the padding filled with 255 or noise"""
    rows, row = img.shape[0], img[0].size
    wide = np.full((rows, row + pad), 255, np.uint8) if seed % 2 else np.random.RandomState(seed).randint(0, 256, (rows, row + pad)).astype(np.uint8)
    wide[:, :row] = img.reshape(rows, row)
    v = wide[:, :row].reshape(img.shape)
    assert np.shares_memory(v, wide) and v.strides[0] == row + pad and not v.flags["C_CONTIGUOUS"] and np.array_equal(v, img)
    return v


def make_context(max_rows, max_cols, max_batch, K, windows=True):
    kw = dict(max_rows=max_rows, max_cols=max_cols, max_batch=max_batch, max_landmarks=16, persistent_waves=4)
    if windows:
        c = capi.Context(**kw)
    else:
        os.environ["ASLAM_NO_WINDOWS"] = "1"
        try:
            c = capi.Context(**kw)
        finally:
            os.environ.pop("ASLAM_NO_WINDOWS", None)
    c.set_camera(K, D0)
    return c


def assert_twin(a, b, slots, where):
    for x, y, what in zip(a.get_state(), b.get_state(), ("mu", "Sigma")):
        assert np.array_equal(x, y), f"{where}: {what} differs from the staged twin by {np.abs(x - y).max() if x.shape == y.shape else 'its size'}"
    assert np.array_equal(a.get_landmark_ids(), b.get_landmark_ids()), f"{where}: landmark ids differ from the twin"
    for s in slots:
        for x, y in zip(a.get_slot_detections(s), b.get_slot_detections(s)):
            assert np.array_equal(x, y), f"{where}: slot {s} detections differ from the twin"
        for x, y in zip(a.get_slot_raw_observations(s), b.get_slot_raw_observations(s)):
            assert np.array_equal(x, y), f"{where}: slot {s} observations differ from the twin"
        assert np.array_equal(a.get_slot_ekf_stats(s, 1), b.get_slot_ekf_stats(s, 1)), f"{where}: slot {s} EKF step counts differ from the twin"
    for x, y in zip(a.get_observations(), b.get_observations()):
        assert np.array_equal(x, y), f"{where}: popped observations differ from the twin"
    assert a.plan_stats() == b.plan_stats(), f"{where}: {a.plan_stats()} vs {b.plan_stats()}"


def assert_oracle_slot(a, slot, frame, K, where):
    """the slot holds what the detector makes of `frame`"""
    o_ids, o_c = frame[2][:2]
    g_ids, g_c, g_rv, g_tv = a.get_slot_detections(slot)
    assert np.array_equal(o_ids, g_ids), f"{where}: slot {slot} holds ids {g_ids}, the frame placed there has {o_ids}"
    assert np.array_equal(o_c, g_c), f"{where}: slot {slot}: marker corners differ from the oracle's"
    pc.check_poses(g_ids, g_c, g_rv, g_tv, K, D0)


def assert_literal(a, frames, K, where):
    """LiteralSlam over the oracle's detections and poses of all frames in order, against the final state, id table and last pops"""
    ref = LiteralSlam()
    ref.K, ref.D = np.asarray(K, float), D0
    t_now = 0.0
    for _, (wl, wr, dt), (ids, corners, rv, tv) in frames:
        t_now += dt
        ref.add_encoder(wl, wr, t_now)
        ref.add_poses(ids, corners.reshape(len(ids), 8), rv, tv)
    mu_g, S_g = a.get_state()
    assert ref.mu.shape == mu_g.shape, f"{where}: state size differs from the literal EKF"
    assert np.allclose(ref.mu, mu_g, rtol=pc.POSE_RTOL, atol=1e-8), f"{where}: mu differs by {np.abs(ref.mu - mu_g).max()}"
    e_S = np.abs(ref.sigma - S_g).max() / max(np.abs(ref.sigma).max(), 1e-300)
    assert e_S < pc.POSE_RTOL, f"{where}: sigma differs by {e_S} (relative to max |sigma|)"
    assert np.array_equal(np.array(sorted(ref.id_map, key=ref.id_map.get), np.int32), a.get_landmark_ids()), f"{where}: landmark id table differs"
    gi, gx, ga, gz, _ = a.get_observations()
    assert np.array_equal(np.array([o["id"] for o in ref.last_observed], np.int32), gi), f"{where}: pop order (ids) differs"
    assert np.array_equal(np.array([e[1] for e in ref.log], np.int32), gx), f"{where}: landmark indices differ"
    assert np.array_equal(np.array([e[2] for e in ref.log], np.int32), ga), f"{where}: update / augment / stationary decisions differ"
    assert np.allclose(np.array([o["z"] for o in ref.last_observed]).reshape(-1, 3), gz, rtol=pc.POSE_RTOL, atol=1e-9), f"{where}: observations differ"
    assert mu_g.size > 3 and len(gi) >= 1


def drive(name, key, H, ops, context_shape=None, windows=True):
    """Run ops on a stream opened at family `key` with H frames per submit, mirrored on a staged twin.
    ops: ("push", pad) a frame through stream_push, its rows padded by pad bytes (0: tight); ("slot",) through stream_slot +
    stream_commit; ("slot2",) the same, asking for the slot twice; ("badpush",) aslam_stream_push with step one byte short of a
    row; ("flush",); ("open", H, key) reopen; ("call", f) f(stream context, model).  Frame i of the case is frame i of the pool of
    the family open at the time.  The last op must be a flush."""
    families = [key] + [op[2] for op in ops if op[0] == "open"]
    pools = {k: pool(k) for k in families}                   # (the oracle conditions hold before any library call of the case)
    K = camera(key)
    assert all(np.array_equal(camera(k), K) for k in families)
    rows, cols = context_shape or SHAPES[key][:2]
    max_batch = 2 * max([H] + [op[1] for op in ops if op[0] == "open"])
    a = make_context(rows, cols, max_batch, K, windows)
    b = make_context(rows, cols, max_batch, K, windows)
    model = rr.Ring(H)
    frames, checked = [], set()
    a.stream_open(*SHAPES[key][:2], SHAPES[key][3], H)
    assert ops[-1] == ("flush",)
    for n_op, op in enumerate(ops):
        where = f"{name} op {n_op} {op[0]}"
        sub, waited = None, False
        if op[0] in ("push", "slot", "slot2"):
            fr = pools[key][len(frames)]
            img, (wl, wr, dt) = fr[0], fr[1]
            if op[0] == "push":
                a.stream_push(padded(img, op[1], len(frames)) if op[1] else img, wl, wr, dt)
            else:
                r, c, _, ch = SHAPES[key]
                view = a.stream_slot(r, c, ch)
                assert view.shape == img.shape
                if op[0] == "slot2":                          # asking again before the commit gives the same memory
                    again = a.stream_slot(r, c, ch)
                    assert again.ctypes.data == view.ctypes.data and again.strides == view.strides
                view[:] = img
                a.stream_commit(wl, wr, dt)
            frames.append(fr)
            sub = model.commit()
        elif op[0] == "badpush":
            img = pools[key][len(frames)][0]
            rc = a.lib.aslam_stream_push(a.h, img.ctypes.data_as(C.c_void_p), img[0].size - 1, 1.0, 2.0, 0.1)
            assert rc == E_INVALID, rc
            with pytest.raises(capi.AslamError) as e:
                a._ck(rc)
            assert e.value.code == E_INVALID and "step" in str(e.value)
        elif op[0] == "flush":
            a.stream_flush()
            sub, waited = model.flush(), True
        elif op[0] == "open":
            a.stream_open(*SHAPES[op[2]][:2], SHAPES[op[2]][3], op[1])
            sub, waited = model.open(op[1]), True
            key = op[2]
        else:
            op[1](a, model)
        if sub:                                               # the twin: the same submit through the staged API
            _, slot0, n, idx = sub
            assert slot0 + n <= max_batch
            b.stage_frames(np.stack([frames[f][0] for f in idx]), slot0)
            b.stage_encoders([frames[f][1][0] for f in idx], [frames[f][1][1] for f in idx], [frames[f][1][2] for f in idx], slot0)
            b.run_staged(slot0, n, with_ekf=True)
        if waited:
            b.sync()
            assert_twin(a, b, sorted(model.frame_in), where)
            last = n_op == len(ops) - 1
            for s in (sorted(model.frame_in) if last or not sub else range(sub[1], sub[1] + sub[2])):
                assert_oracle_slot(a, s, frames[model.frame_in[s]], K, where)
                checked.add(model.frame_in[s])
    assert not model.pending and len(model.slot_of) == len(frames)
    assert_literal(a, frames, K, name)
    CHECKED[name] = (len(checked), len(frames))
    print(f"{name}: {len(frames)} frames, {len(model.submits)} submits, {len(checked)} frames checked against the oracle in their slots, "
          f"plan {a.plan_stats()}")
    return a, b, model


def cadence_ops(H, n, flush_each):
    ops = []
    for i in range(n):
        ops.append(("push", 0))
        if flush_each and (i + 1) % H == 0:
            ops.append(("flush",))                            # the half was just submitted: this flush waits, submits nothing, stays
    return ops + [("flush",)]


# ---- cadence: every half reused at least twice, the last submit partial -------------------------------------------------------------

@pytest.mark.parametrize("flush_each", [False, True], ids=["flush_at_end", "flush_each_submit"])
@pytest.mark.parametrize("H", [1, 2, 3, 5])
def test_cadence(H, flush_each):
    n = 7 if H == 1 else 4 * H + 1
    _, _, model = drive(f"cadence H={H} {'each' if flush_each else 'end'}", "gray", H, cadence_ops(H, n, flush_each))
    assert len(model.submits) == (7 if H == 1 else 5) and model.submits[-1][2] == 1
    assert sum(s[0] == 0 for s in model.submits) >= 3 and sum(s[0] == 1 for s in model.submits) >= 2
    if flush_each:
        assert CHECKED[f"cadence H={H} each"] == (n, n)      # every frame was live at some flush


def test_cadence_windows_off():
    a, _, _ = drive("cadence H=3 windows off", "gray", 3, cadence_ops(3, 13, False), windows=False)
    assert a.plan_stats()["windows"] == 0


# ---- partial and empty flushes ------------------------------------------------------------------------------------------------------

def test_partial_and_empty_flushes():
    """a flush at fill 1 of 3 in mid-stream, then two flushes in a row: the second submits nothing and stays on its half"""
    seen = []
    ops = [("push", 0), ("flush",), ("push", 0), ("push", 0), ("push", 0), ("push", 0), ("flush",),
           ("call", lambda a, m: seen.append((m.half, m.next_slot()))), ("flush",),
           ("call", lambda a, m: seen.append((m.half, m.next_slot()))), ("push", 0), ("push", 0), ("flush",), ("flush",), ("push", 0), ("flush",)]
    a, _, model = drive("partial flushes", "gray", 3, ops)
    assert seen[0] == seen[1] == (1, 3)
    assert [s[:3] for s in model.submits] == [(0, 0, 1), (1, 3, 3), (0, 0, 1), (1, 3, 2), (0, 0, 1)]
    assert model.slot_of == [rr.OVERWRITTEN, rr.OVERWRITTEN, rr.OVERWRITTEN, 5, rr.OVERWRITTEN, 3, 4, 0]


# ---- formats: bgr8, padded rows, a shape off the pitch and off the tile grid ---------------------------------------------------------

def test_bgr8_tight():
    drive("bgr8 tight", "bgr", 2, cadence_ops(2, 5, True))


@pytest.mark.parametrize("pad", [1, 13, 64])
@pytest.mark.parametrize("key", ["gray", "bgr"])
def test_padded_rows(key, pad):
    """views into wider arrays go through stream_push with their own strides[0]: the row-by-row copy of aslam_stream_push"""
    drive(f"{key} rows + {pad}", key, 2, [("push", pad)] * 2 + [("flush",)] + [("push", pad)] * 3 + [("flush",)])


def test_push_passes_a_padded_view_through():
    """Context.stream_push hands the library the caller's memory and strides[0] when the rows are contiguous in themselves, and
    copies only otherwise"""
    seen = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, k):
            return getattr(self._lib, k)

        def aslam_stream_push(self, h, px, step, wl, wr, dt):
            seen.append((px.value, step))
            return self._lib.aslam_stream_push(h, px, step, wl, wr, dt)

    img = pool("tiny")[0][0]
    c = make_context(64, 64, 8, camera("tiny"))
    c.lib = Spy(c.lib)
    c.stream_open(64, 64, 1, 4)
    v = padded(img, 13, 1)
    c.stream_push(v, 1.0, 2.0, 0.1)
    assert seen[-1] == (v.ctypes.data, 64 + 13)
    c.stream_push(img, 1.0, 2.0, 0.1)
    assert seen[-1] == (img.ctypes.data, 64)
    wide = np.zeros((64, 128), np.uint8)
    wide[:, ::2] = img
    c.stream_push(wide[:, ::2], 1.0, 2.0, 0.1)                # pixels not adjacent: copied
    assert seen[-1][1] == 64 and seen[-1][0] != wide.ctypes.data
    c.stream_push(img.astype(np.int32), 1.0, 2.0, 0.1)       # another type: converted
    assert seen[-1][1] == 64
    c.stream_flush()
    want = pool("tiny")[0][2][0]
    for s in range(4):
        assert np.array_equal(c.get_slot_detections(s)[0], want), s


def test_off_grid_shape():
    """203 x 277 in a 240 x 320 context, tight and padded"""
    drive("203 x 277", "odd", 2, [("push", 0), ("push", 13), ("push", 1), ("flush",), ("slot",), ("push", 64), ("push", 0), ("flush",)],
          context_shape=(240, 320))


# ---- zero copy ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["gray", "bgr"])
def test_zero_copy(key):
    drive(f"zero copy {key}", key, 2, [("slot",)] * 5 + [("flush",)])


def test_push_and_commit_mixed_in_one_half():
    ops = [("push", 0), ("slot2",), ("push", 13), ("slot",), ("push", 0), ("slot2",), ("push", 0), ("flush",)]
    _, _, model = drive("push / commit mixed", "gray", 3, ops)
    assert [s[:3] for s in model.submits] == [(0, 0, 3), (1, 3, 3), (0, 0, 1)]


# ---- reopening ----------------------------------------------------------------------------------------------------------------------

def test_reopen_after_flush_other_H_other_channels():
    """the stream carries on on the same filter: the twin and the literal EKF follow across the reopen"""
    ops = [("push", 0)] * 3 + [("flush",), ("open", 3, "bgr")] + [("push", 0)] * 4 + [("flush",), ("open", 1, "gray")] + [("push", 0)] * 2 + [("flush",)]
    _, _, model = drive("reopen", "gray", 2, ops)
    assert [s[:3] for s in model.submits] == [(0, 0, 2), (1, 2, 1), (0, 0, 3), (1, 3, 1), (0, 0, 1), (1, 1, 1)]


def test_reopen_with_committed_frames_keeps_them():
    """2 committed, unsubmitted frames at the reopen are submitted first: they are in the state, not lost.  An acquired slot that
    was not committed is dropped."""
    def acquire_only(a, m):
        a.stream_slot(240, 320)[:] = 0

    ops = [("push", 0)] * 2 + [("call", acquire_only), ("open", 2, "gray")] + [("push", 0)] * 3 + [("flush",)]
    a, _, model = drive("reopen with pending", "gray", 3, ops)
    assert [s[:3] for s in model.submits] == [(0, 0, 2), (0, 0, 2), (1, 2, 1)]
    with pytest.raises(capi.AslamError) as e:
        a.stream_commit(1.0, 2.0, 0.1)                        # nothing is acquired after the run either
    assert e.value.code == E_STATE


# ---- the frame shape changes behind an open stream ----------------------------------------------------------------------------------

@pytest.mark.parametrize("other", ["larger", "bgr8"])
def test_shape_change_refuses_the_stream_until_reopened(other):
    """The ring is sized and addressed by the shape of its aslam_stream_open.  A staged frame of another shape (128 x 128 gray, or
    64 x 64 bgr8: either is more bytes than a ring slot) reconfigures the context; every stream call then refuses with
    ASLAM_E_STATE and does nothing, and aslam_stream_open makes the stream usable again: the frame committed before is not lost."""
    foreign = np.zeros((128, 128), np.uint8) if other == "larger" else np.zeros((64, 64, 3), np.uint8)

    def change_and_check(a, m):
        view = a.stream_slot(64, 64)                          # acquired before the change: the commit must refuse on the shape
        view[:] = 7
        a.stage_frames(foreign, 3)
        img = pool("tiny")[5][0]
        for call in (lambda: a.stream_push(img, 1.0, 2.0, 0.1), lambda: a.stream_slot(64, 64), lambda: a.stream_commit(1.0, 2.0, 0.1),
                     a.stream_flush, lambda: a.stream_push(padded(img, 13, 0), 1.0, 2.0, 0.1)):
            with pytest.raises(capi.AslamError) as e:
                call()
            assert e.value.code == E_STATE and "frame shape changed" in str(e.value), str(e.value)

    ops = [("push", 0), ("call", change_and_check), ("open", 2, "tiny"), ("push", 0), ("push", 13), ("slot",), ("flush",)]
    a, _, model = drive(f"shape change {other}", "tiny", 2, ops, context_shape=(128, 128))
    assert [s[:3] for s in model.submits] == [(0, 0, 1), (0, 0, 2), (1, 2, 1)]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    c = make_context(64, 64, 4, camera("tiny"))
    for call in (c.stream_flush, lambda: c.stream_slot(64, 64), lambda: c.stream_commit(1.0, 2.0, 0.1)):
        with pytest.raises(capi.AslamError) as e:             # before stream_open
            call()
        assert e.value.code == E_STATE
    for bad in ((64, 64, 2, 2), (64, 64, 4, 2), (64, 64, 1, 0), (64, 64, 1, 3), (65, 64, 1, 2)):
        with pytest.raises(capi.AslamError) as e:             # channels 2 and 4, no frame, 2 * 3 > max_batch, rows > max_rows
            c.stream_open(*bad)
        assert e.value.code == E_INVALID, bad
    c.stream_open(64, 64, 1, 2)
    with pytest.raises(capi.AslamError) as e:
        c.stream_commit(1.0, 2.0, 0.1)                        # commit without acquire
    assert e.value.code == E_STATE and "acquire" in str(e.value)
    c.stream_flush()                                          # nothing pending: fine, nothing happens
    assert c.get_state()[0].size == 3


def test_short_step_push_consumes_no_slot():
    """aslam_stream_push with step one byte short of a row is refused with ASLAM_E_INVALID; the next valid push lands where the
    model says (drive() checks every live slot's detections against the frame the model places there)"""
    ops = [("push", 0), ("badpush",), ("push", 0), ("badpush",), ("push", 0), ("flush",)]
    _, _, model = drive("short step", "tiny", 2, ops)
    assert model.slot_of == [0, 1, 2]


# ---- on the MI355X at 1280 x 720: uploads overlap the other half's processing --------------------------------------------------------

@pytest.mark.gpu
def test_gpu_bgr8_padded_stream_1280x720():
    """cfg2 (20 markers in view), bgr8 with padded rows, H = 3, 20 frames, one flush at the end: an ordering error between ev_up,
    ev_det and ev_ekf (a half overwritten while the detector or the EKF still reads it) shows against the twin and the oracle"""
    cfg = synth.CONFIGS["cfg2"]
    w = synth.PanelWorld(cfg)
    H, n = 3, 20
    kw = dict(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=2 * H, max_landmarks=w.L + 8)
    a, b = capi.Context(**kw), capi.Context(**kw)
    frames = []
    try:
        for c in (a, b):
            c.set_camera(w.K, D0)
            synth.apply_detector(cfg, c, orc if c is a else None)
        for i in range(n):
            fr = w.frame(i)
            g = renderer(cfg.rows, cfg.cols).synth_render(0, cfg.rows, cfg.cols, w.K, fr.ids, fr.poses, noise_amp=2, seed=i)
            img = np.ascontiguousarray(np.stack([np.roll(g, 1, 0), g, np.roll(g, -1, 1)], -1))
            frames.append((img, (fr.wl + 0.05 * (i % 3 + 1), fr.wr - 0.03 * (i % 2 + 1), fr.dt + 0.001 * (i % 5))))
        model = rr.Ring(H)
        a.stream_open(cfg.rows, cfg.cols, 3, H)
        for i, (img, (wl, wr, dt)) in enumerate(frames):
            a.stream_push(padded(img, (1, 13, 64)[i % 3], i), wl, wr, dt)
            model.commit()
        a.stream_flush()
        model.flush()
        for _, slot0, cnt, idx in model.submits:
            b.stage_frames(np.stack([frames[f][0] for f in idx]), slot0)
            b.stage_encoders([frames[f][1][0] for f in idx], [frames[f][1][1] for f in idx], [frames[f][1][2] for f in idx], slot0)
            b.run_staged(slot0, cnt, with_ekf=True)
        b.sync()
        assert len(model.submits) == 7 and sorted(model.frame_in) == list(range(6))
        assert_twin(a, b, sorted(model.frame_in), "1280 x 720")
        for s, f in sorted(model.frame_in.items()):
            det = orc.detect(frames[f][0])
            assert len(det[0]) >= 10
            assert_oracle_slot(a, s, (None, None, det), w.K, "1280 x 720")
        assert len(a.get_landmark_ids()) >= 10
    finally:
        orc.set_detector_params()
