"""Map merge (aslam_merge_map_records / aslam_fleet_merge_maps, fleet_merge.h): N landmark maps in N frames aligned
into one anchor frame from the marker ids they share and fused per id, against the numpy restatement tests/merge_reference.py.

Tolerance against the reference: the project's bar for f64 state against a literal reference (assert_close of
tests/test_fleet_slam.py): 1e-9 absolute on means and transforms, 1e-9 relative to max|Sigma| on covariances; ids, n_seen and
rounds exact.  Marginals are random SPD matrices with eigenvalues in [1e-4, 1e-2], positions within +-3 m and headings away from
+-pi, which keeps the 3 x 3 inverses and the short transform chains far inside that bar."""
import ctypes as C
import math

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from tests import merge_reference as ref
from tests.merge_reference import MAP_DTYPE
from tests.test_localize import E_INVALID, E_STATE, emu_context, inject, observe, random_map

TOL = 1e-9


def spd(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q @ np.diag(10.0 ** rng.uniform(-4, -2, 3)) @ q.T


def into_frame(xyth, frame):
    """world landmarks (n x 3) seen from a map frame whose origin has world pose frame = (x, y, theta)"""
    c, s = math.cos(frame[2]), math.sin(frame[2])
    d = xyth[:, :2] - frame[:2]
    return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], xyth[:, 2] - frame[2]], 1)


def relative(frame, anchor):
    """T = (tx, ty, phi) taking coordinates in `frame` to coordinates in `anchor`"""
    c, s = math.cos(anchor[2]), math.sin(anchor[2])
    d = frame[:2] - anchor[:2]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], frame[2] - anchor[2]])


def make_records(rng, ids, xyth, frames, subsets, per_map, noise):
    """one map per frame: the landmarks subsets[m] (positions into ids) in frame m, shuffled, noisy, with random SPD marginals"""
    rec = np.zeros((len(frames), per_map), MAP_DTYPE)
    rec["id"] = -1
    rec["index"] = -1
    for m, (frame, sub) in enumerate(zip(frames, subsets)):
        sub = rng.permutation(sub)
        local = into_frame(xyth[sub], frame) + noise * rng.normal(size=(len(sub), 3))
        rec["id"][m, :len(sub)] = ids[sub]
        rec["index"][m, :len(sub)] = np.arange(len(sub))
        rec["x"][m, :len(sub)], rec["y"][m, :len(sub)], rec["theta"][m, :len(sub)] = local.T
        rec["S"][m, :len(sub)] = [spd(rng).reshape(9) for _ in sub]
    return rec


def random_frames(rng, n):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(-0.6, 0.6, n)], 1)


def world(rng, n, id_pool=1024):
    """n markers: random ids, positions in +-3 m, headings in +-1 rad (with frames in +-0.6 rad no heading comes near +-pi)"""
    ids = np.sort(rng.permutation(id_pool)[:n]).astype(np.int32)
    return ids, np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-1, 1, n)], 1)


CHAIN = [list(range(0, 5)), list(range(3, 8)), list(range(6, 10)), list(range(8, 12))]      # 0-1-2-3: neighbours share two markers


def chain_case(seed, noise):
    rng = np.random.RandomState(seed)
    ids, xyth = world(rng, 12)
    frames = random_frames(rng, 4)
    return ids, xyth, frames, make_records(rng, ids, xyth, frames, CHAIN, 7, noise)


def leveled_case(seed, n_maps, per_map, levels, group, noise=0.01):
    """an overlap graph of depth `levels`: marker group g is first held by the maps of level g; a map of level g >= 1 shares 4 markers
    of group g - 1 with the maps of level g - 1 and none with lower levels.  Map 0 is level 0; the first map of every level holds
    its whole group.  Ids 0 and 1023 are in the world."""
    rng = np.random.RandomState(seed)
    ids, xyth = world(rng, (levels + 1) * group)
    ids[0], ids[-1] = 0, 1023
    order = rng.permutation(ids.size)
    groups = [order[g * group:(g + 1) * group] for g in range(levels + 1)]
    level = [0] + [1 + (m - 1) % levels for m in range(1, n_maps)]
    subsets, first = [], set()
    for m in range(n_maps):
        g = level[m]
        own = groups[g] if g not in first else rng.permutation(groups[g])[:rng.randint(3, per_map - 4 + 1)]
        first.add(g)
        subsets.append(list(own) + (list(rng.permutation(groups[g - 1])[:4]) if g else []))
    frames = random_frames(rng, n_maps)
    return ids, xyth, frames, make_records(rng, ids, xyth, frames, subsets, per_map, noise)


def assert_merge_close(got, want, where):
    ids, xyth, sig, seen, rounds, T = got
    r_ids, r_xyth, r_sig, r_seen, r_rounds, r_T = want
    assert np.array_equal(rounds, r_rounds), f"{where}: rounds {rounds} vs {r_rounds}"
    assert np.array_equal(ids, r_ids) and np.array_equal(seen, r_seen), f"{where}: ids / n_seen differ"
    e_m, e_T = np.abs(xyth - r_xyth).max(), np.abs(T - r_T).max()
    e_S = np.abs(sig - r_sig).max() / max(np.abs(r_sig).max(), 1e-300)
    print(f"{where}: |d xyth| {e_m:.2e}  |d T| {e_T:.2e}  |d Sigma| / max {e_S:.2e}")
    assert e_m <= TOL and e_T <= TOL, f"{where}: means differ by {e_m}, transforms by {e_T}"
    assert e_S <= TOL, f"{where}: covariances differ by {e_S} of max|Sigma|"


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def device_copy(rec, on_emulation):
    """address of a device copy of the records, and what keeps it alive (the emulation's device memory is host memory)"""
    if on_emulation:
        keep = np.ascontiguousarray(rec).copy()
        return keep.ctypes.data, keep
    import torch
    keep = torch.from_numpy(np.frombuffer(np.ascontiguousarray(rec).tobytes(), np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return keep.data_ptr(), keep


@pytest.fixture(scope="module")
def ctx():
    return emu_context(4, max_landmarks=16)


def check_host_and_device(ctx, rec, on_emulation, where, **kw):
    n_maps, per_map = rec.shape
    got = ctx.merge_map_records(rec, n_maps, per_map, **kw)
    ptr, keep = device_copy(rec, on_emulation)
    dev = ctx.merge_map_records(ptr, n_maps, per_map, on_device=True, **kw)
    assert same_bits(got, dev), f"{where}: host records and device records give different bits"
    assert same_bits(got, ctx.merge_map_records(rec, n_maps, per_map, **kw)), f"{where}: two runs differ"
    want = ref.merge(rec, n_maps, per_map, **kw)
    assert_merge_close(got, want, where)
    return got, want


# ---- 1, 2: synthetic records ----------------------------------------------------------------------------------------------------------

def test_chain_of_four_noisy_maps_against_reference(ctx, on_emulation):
    ids, xyth, frames, rec = chain_case(1, 0.01)
    got, _ = check_host_and_device(ctx, rec, on_emulation, "chain")
    assert got[4].tolist() == [0, 1, 2, 3]
    assert np.array_equal(got[0], ids) and got[3].tolist() == [1, 1, 1, 2, 2, 1, 2, 2, 2, 2, 1, 1]


@pytest.mark.parametrize("anchor,rounds", [(0, [0, 1, 2, 3]), (2, [2, 1, 0, 1])])
def test_zero_noise_recovers_truth_and_frames(ctx, on_emulation, anchor, rounds):
    ids, xyth, frames, rec = chain_case(2, 0.0)
    got, _ = check_host_and_device(ctx, rec, on_emulation, f"anchor {anchor}", anchor=anchor)
    m_ids, m_xyth, _, _, m_rounds, T = got
    assert m_rounds.tolist() == rounds and np.array_equal(m_ids, ids)
    assert np.abs(m_xyth - into_frame(xyth, frames[anchor])).max() <= TOL
    for m in range(4):
        assert np.abs(T[m] - relative(frames[m], frames[anchor])).max() <= TOL, f"map {m}"
    assert np.array_equal(T[anchor], np.zeros(3))


# ---- 3: rules -------------------------------------------------------------------------------------------------------------------------

def records(rows, per_map):
    """rows: per map a list of (id, x, y, theta, S or None = identity * 1e-3)"""
    rec = np.zeros((len(rows), per_map), MAP_DTYPE)
    rec["id"] = -1
    rec["index"] = -1
    for m, row in enumerate(rows):
        for i, (lid, x, y, th, S) in enumerate(row):
            rec[m, i] = (lid, i, x, y, th, (np.eye(3) * 1e-3 if S is None else np.asarray(S, float)).reshape(9))
    return rec


def test_too_few_common_ids_and_coincident_landmarks_stay_unaligned(ctx):
    a = [(5, 0.0, 0.0, 0.1, None), (9, 1.0, 0.0, 0.2, None), (11, 0.0, 2.0, 0.3, None), (20, 1.0, 1.0, 0.0, None)]
    one_common = [(9, 0.5, 0.5, 0.0, None), (30, 2.0, 2.0, 0.0, None), (31, 2.5, 2.0, 0.0, None)]
    coincide = [(5, 0.7, -0.3, 0.0, None), (11, 0.7, -0.3, 0.5, None), (40, 1.0, 1.0, 0.0, None)]      # both common ids on one point
    rec = records([a, one_common, coincide], 5)
    got = ctx.merge_map_records(rec, 3, 5)
    assert_merge_close(got, ref.merge(rec, 3, 5), "unaligned maps")
    assert got[4].tolist() == [0, -1, -1] and np.array_equal(got[5], np.zeros((3, 3)))
    assert got[0].tolist() == [5, 9, 11, 20] and got[3].tolist() == [1, 1, 1, 1]
    # two common ids align with min_common = 2 but not with 3, and a map that waited aligns once a later round brings its ids
    two = [(5, 1.0, 1.0, 0.1, None), (9, 2.0, 1.0, 0.2, None), (50, 3.0, 3.0, 0.0, None), (51, 3.0, 4.0, 0.0, None)]
    late = [(50, 0.0, 0.0, 0.0, None), (51, 0.0, 1.0, 0.0, None), (60, 5.0, 5.0, 0.0, None)]
    rec = records([a, late, two], 5)
    got = ctx.merge_map_records(rec, 3, 5)
    assert_merge_close(got, ref.merge(rec, 3, 5), "late map")
    assert got[4].tolist() == [0, 2, 1] and got[0].tolist() == [5, 9, 11, 20, 50, 51, 60]
    got = ctx.merge_map_records(rec, 3, 5, min_common=3)
    assert_merge_close(got, ref.merge(rec, 3, 5, min_common=3), "min_common 3")
    assert got[4].tolist() == [0, -1, -1] and got[0].tolist() == [5, 9, 11, 20]


def test_duplicate_ids_unusable_marginals_and_ids_out_of_range(ctx):
    indefinite = np.diag([1e-3, -1e-3, 1e-3])
    saddle = np.array([[1e-3, 2e-3, 0.0], [2e-3, 1e-3, 0.0], [0.0, 0.0, 1e-3]])
    nan = np.full((3, 3), np.nan)
    a = [(7, 1.0, 2.0, 0.3, None), (7, -5.0, -5.0, 1.0, None),          # the same id twice: the first counts
         (8, 0.0, 1.0, 0.0, np.zeros((3, 3))),                          # its only marginal is zero: n_seen 0
         (9, 2.0, 0.0, -0.2, indefinite), (1024, 9.0, 9.0, 0.0, None), (-7, 9.0, 9.0, 0.0, None), (5000, 9.0, 9.0, 0.0, None),
         (12, -1.0, -1.0, 0.4, None)]
    b = [(9, 2.1, 0.1, -0.1, None), (7, 1.1, 2.1, 0.4, saddle), (12, -0.9, -0.9, 0.5, nan), (8, 0.1, 1.1, 0.1, None),
         (1024, 0.0, 0.0, 0.0, None), (13, 4.0, 4.0, 0.0, np.zeros((3, 3)))]
    rec = records([a, b], 8)
    got = ctx.merge_map_records(rec, 2, 8)
    want = ref.merge(rec, 2, 8)
    assert_merge_close(got, want, "rules")
    ids, xyth, sig, seen, rounds, T = got
    assert ids.tolist() == [7, 8, 9, 12, 13] and rounds.tolist() == [0, 1]
    assert seen.tolist() == [1, 1, 1, 1, 0]
    assert np.array_equal(xyth[0], [1.0, 2.0, 0.3]), "the record at the lower position counts, and a lone contribution is the mean"
    assert np.array_equal(sig[4], np.zeros((3, 3))), "no usable contribution: zero covariance"
    # alone, the anchor keeps the table's mean for ids without a usable marginal
    got = ctx.merge_map_records(rec[:1], 1, 8)
    assert_merge_close(got, ref.merge(rec[:1], 1, 8), "one map")
    assert got[0].tolist() == [7, 8, 9, 12] and got[3].tolist() == [1, 0, 0, 1] and got[4].tolist() == [0]
    assert np.array_equal(got[1][1], [0.0, 1.0, 0.0]) and np.array_equal(got[2][1], np.zeros((3, 3)))


def raw_merge(ctx, rec, n_maps, per_map, anchor=0, min_common=2, max_=1024, null_rec=False, **out):
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None      # noqa: E731
    n = out.get("n")
    return ctx.lib.aslam_merge_map_records(ctx.h, None if null_rec else rec.ctypes.data_as(C.c_void_p), 0, n_maps, per_map, anchor,
                                           min_common, max_, C.byref(n) if n is not None else None, p(out.get("ids"), capi._ip),
                                           p(out.get("xyth"), capi._dp), p(out.get("sigmas"), capi._dp), p(out.get("seen"), capi._ip),
                                           p(out.get("rounds"), capi._ip), p(out.get("T"), capi._dp))


def test_truncation_null_outputs_and_argument_errors(ctx):
    ids, xyth, frames, rec = chain_case(3, 0.01)
    full = ctx.merge_map_records(rec, 4, 7)
    n = C.c_int(-1)
    o = dict(ids=np.full(12, -9, np.int32), xyth=np.full((12, 3), -9.0), sigmas=np.full((12, 9), -9.0), seen=np.full(12, -9, np.int32))
    assert raw_merge(ctx, rec, 4, 7, max_=3, n=n, **o) == 0
    assert n.value == 12, "*n is the number available"
    assert np.array_equal(o["ids"][:3], full[0][:3]) and np.array_equal(o["xyth"][:3], full[1][:3])
    assert np.array_equal(o["sigmas"][:3].reshape(3, 3, 3), full[2][:3]) and np.array_equal(o["seen"][:3], full[3][:3])
    assert np.all(o["ids"][3:] == -9) and np.all(o["xyth"][3:] == -9) and np.all(o["sigmas"][3:] == -9) and np.all(o["seen"][3:] == -9)
    n = C.c_int(-1)
    assert raw_merge(ctx, rec, 4, 7, max_=0, n=n) == 0 and n.value == 12
    assert raw_merge(ctx, rec, 4, 7) == 0                               # every output NULL
    rounds, T = np.zeros(4, np.int32), np.zeros((4, 3))
    assert raw_merge(ctx, rec, 4, 7, rounds=rounds, T=T) == 0
    assert np.array_equal(rounds, full[4]) and np.array_equal(T, full[5])
    big = np.zeros((257, 2), MAP_DTYPE)
    wide = np.zeros((1, 1025), MAP_DTYPE)
    bad = [dict(null_rec=True), dict(n_maps=0), dict(per_map=0), dict(anchor=-1), dict(anchor=4), dict(min_common=1),
           dict(min_common=1025), dict(max_=-1)]
    for kw in bad:
        args = dict(n_maps=4, per_map=7)
        args.update(kw)
        assert raw_merge(ctx, rec, **args) == E_INVALID, kw
    assert raw_merge(ctx, big, 257, 2) == E_INVALID and raw_merge(ctx, wide, 1, 1025) == E_INVALID
    assert ctx.lib.aslam_merge_map_records(None, rec.ctypes.data_as(C.c_void_p), 0, 4, 7, 0, 2, 0, None, None, None, None, None, None,
                                           None) == E_INVALID
    assert raw_merge(ctx, rec, 4, 7, min_common=1024) == 0
    with pytest.raises(ValueError):
        ctx.merge_map_records(rec, 4, 6)


CAM = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))


def raw_fleet_merge(c, anchor=0, min_common=2, max_=1024, null_ctx=False):
    return c.lib.aslam_fleet_merge_maps(None if null_ctx else c.h, anchor, min_common, max_, None, None, None, None, None, None, None)


def test_fleet_merge_needs_a_slam_fleet():
    c = emu_context(2, max_landmarks=8)
    with pytest.raises(capi.AslamError) as e:
        c.fleet_merge_maps()
    assert e.value.code == E_STATE
    c.fleet_begin([CAM] * 2, [3, 4], np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.zeros((2, 3)), np.stack([np.eye(3) * 1e-3] * 2))
    with pytest.raises(capi.AslamError) as e:
        c.fleet_merge_maps()
    assert e.value.code == E_STATE
    c.fleet_slam_begin([CAM] * 2)
    for kw in (dict(anchor=2), dict(anchor=-1), dict(min_common=1), dict(min_common=1025), dict(max_=-1), dict(null_ctx=True)):
        assert raw_fleet_merge(c, **kw) == E_INVALID, kw
    assert raw_fleet_merge(c) == 0 and raw_fleet_merge(c, anchor=1, min_common=1024, max_=0) == 0      # every output NULL
    got = c.fleet_merge_maps()                                          # empty maps: nothing to merge, robot 1 never aligned
    assert got[0].size == 0 and got[4].tolist() == [0, -1]
    c.fleet_end()
    with pytest.raises(capi.AslamError) as e:
        c.fleet_merge_maps()
    assert e.value.code == E_STATE


def test_scratch_is_allocated_by_the_first_merge_and_freed_by_fleet_end():
    c = emu_context(2, max_landmarks=8)
    rec = chain_case(3, 0.01)[3]
    assert c.merge_scratch_bytes() == 0
    assert c.merge_map_records(rec, 4, 7)[4].tolist() == [0, 1, 2, 3]
    tables = c.merge_scratch_bytes() - 4 * 7 * capi.MAP_RECORD_BYTES
    assert tables > 256 * 1024 * 4, "the id -> position tables of 256 maps alone are 1 MB"
    # ending localization is no fleet call: the single filter's calls leave the merge scratch alone
    c.localize_begin([3], np.array([[1.0, 0.0, 0.0]]), np.zeros(3), np.eye(3) * 1e-3)
    c.localize_end()
    assert c.merge_scratch_bytes() == tables + 4 * 7 * capi.MAP_RECORD_BYTES
    c.fleet_slam_begin([CAM] * 2)
    c.fleet_merge_maps()
    assert c.merge_scratch_bytes() == tables + 4 * 7 * capi.MAP_RECORD_BYTES, "2 x 8 records fit the buffer of 4 x 7"
    c.fleet_end()
    assert c.merge_scratch_bytes() == 0
    assert c.merge_map_records(rec, 4, 7)[4].tolist() == [0, 1, 2, 3]    # and the next merge allocates again
    assert c.merge_scratch_bytes() == tables + 4 * 7 * capi.MAP_RECORD_BYTES


def test_fleet_of_more_than_1024_landmark_slots_merges():
    """per_map <= 1024 limits aslam_merge_map_records only: a fleet's capacity is not the caller's argument"""
    L = 1030
    c = emu_context(2, max_landmarks=L)
    c.fleet_slam_begin([CAM] * 2)
    rng = np.random.RandomState(21)
    ids, xyth = world(rng, 5)
    frames = random_frames(rng, 2)
    rec = make_records(rng, ids, xyth, frames, [[0, 1, 2, 3], [4, 3, 1, 2]], 4, 0.01)
    for r in range(2):
        S = np.zeros((15, 15))
        for i in range(4):
            S[3 + 3 * i:6 + 3 * i, 3 + 3 * i:6 + 3 * i] = rec["S"][r, i].reshape(3, 3)
        mu = np.concatenate([[0.0, 0.0, 0.0], np.stack([rec["x"][r], rec["y"][r], rec["theta"][r]], 1).reshape(-1)])
        c.fleet_set_state(r, mu, S, rec["id"][r])
    got = c.fleet_merge_maps()
    assert_merge_close(got, ref.merge(rec, 2, 4), "capacity 1030")
    assert np.array_equal(got[0], ids) and got[4].tolist() == [0, 1] and got[3].tolist() == [1, 2, 2, 2, 1]
    assert c.merge_scratch_bytes() > 2 * L * capi.MAP_RECORD_BYTES


# ---- 4: size limits -------------------------------------------------------------------------------------------------------------------

def test_256_maps_of_40_records_depth_4(ctx, on_emulation):
    ids, xyth, frames, rec = leveled_case(4, 256, 40, 4, 30)
    got, want = check_host_and_device(ctx, rec, on_emulation, "256 x 40")
    assert got[4].max() == 4 and got[4].min() == 0 and (got[4] == 0).sum() == 1
    assert got[0][0] == 0 and got[0][-1] == 1023 and got[0].size == 150
    assert got[3].max() > 20


def test_two_maps_of_1024_records(ctx, on_emulation):
    rng = np.random.RandomState(5)
    ids, xyth = world(rng, 1024)
    frames = random_frames(rng, 2)
    second = list(rng.permutation(1024)[:900])
    rec = make_records(rng, ids, xyth, frames, [list(range(1024)), second], 1024, 0.01)
    rec[1, 900:] = rec[1, :124]                                         # a full second map whose tail repeats ids of its head
    rec["x"][1, 900:] += 1.0
    got, _ = check_host_and_device(ctx, rec, on_emulation, "2 x 1024")
    assert got[0].size == 1024 and got[4].tolist() == [0, 1] and (got[3] == 2).sum() == 900


# ---- 5, 6: the fleet path on injected observations ------------------------------------------------------------------------------------

def drive(pose, wl, wr, dt, kl=0.05, kr=0.05, b=0.09):
    sl, sr = kl * dt * wl, kr * dt * wr
    dth, ds = (sr - sl) / (2 * b), 0.5 * (sr + sl)
    return np.array([pose[0] + ds * math.cos(pose[2] + 0.5 * dth), pose[1] + ds * math.sin(pose[2] + 0.5 * dth), pose[2] + dth])


def fleet_frames(seed, starts, views, ids, xyth, n_frames):
    """per frame and robot (wl, wr, dt, obs): robot r starts at world pose starts[r] and observes the markers views[r] every frame"""
    rng = np.random.RandomState(seed)
    poses = [np.array(s, float) for s in starts]
    out = []
    for f in range(n_frames):
        row = []
        for r in range(len(starts)):
            wl, wr, dt = rng.uniform(1, 3), rng.uniform(1, 3), 0.05
            if f:
                poses[r] = drive(poses[r], wl, wr, dt)
            row.append((wl, wr, dt, [(int(ids[k]), 1, observe(poses[r], xyth[k], rng), rng.uniform(0.01, 0.05, 3)) for k in views[r]]))
        out.append(row)
    return out, poses


def run_fleet_frames(fleet, frames, with_ekf=2):
    R = len(frames[0])
    for row in frames:
        for r, fr in enumerate(row):
            inject(fleet, r, fr[3])
        fleet.stage_encoders([fr[0] for fr in row], [fr[1] for fr in row], [fr[2] for fr in row])
        fleet.fleet_run_staged(0, list(range(R)), with_ekf=with_ekf)
        fleet.sync()


def host_records(fleet, R):
    """the robots' maps as records, from the host getters"""
    per_map = int(fleet.init.max_landmarks)
    rec = np.zeros((R, per_map), MAP_DTYPE)
    rec["id"] = -1
    rec["index"] = -1
    for r in range(R):
        mu, S = fleet.fleet_get_state(r)
        for i, lid in enumerate(fleet.fleet_get_landmark_ids(r)):
            li = 3 + 3 * i
            rec[r, i] = (lid, i, mu[li], mu[li + 1], mu[li + 2], S[li:li + 3, li:li + 3].reshape(9))
    return rec


STARTS = [(0.0, 0.0, 0.0), (1.0, -0.5, 0.4), (-0.5, 1.0, -0.3)]
VIEWS = [range(0, 6), range(3, 9), range(5, 10)]


@pytest.fixture(scope="module")
def surveyed():
    rng = np.random.RandomState(11)
    ids, xyth = random_map(rng, 10)
    xyth[:, 2] = rng.uniform(-1, 1, 10)
    frames, poses = fleet_frames(12, STARTS, VIEWS, ids, xyth, 9)
    fleet = emu_context(3, max_landmarks=12)
    fleet.fleet_slam_begin([CAM] * 3)
    run_fleet_frames(fleet, frames)
    return fleet, ids, xyth, poses


def test_fleet_merge_equals_host_records_and_reference(surveyed):
    fleet, ids, xyth, _ = surveyed
    before = [fleet.fleet_get_state(r) + (fleet.fleet_get_landmark_ids(r),) for r in range(3)]
    assert all(b[2].size == len(v) for b, v in zip(before, VIEWS))
    rec = host_records(fleet, 3)
    for anchor in (0, 1):
        got = fleet.fleet_merge_maps(anchor=anchor)
        assert same_bits(got, fleet.merge_map_records(rec, 3, 12, anchor=anchor)), "fleet export != records from the host getters"
        assert_merge_close(got, ref.merge(rec, 3, 12, anchor=anchor), f"fleet, anchor {anchor}")
        assert np.array_equal(got[0], np.sort(ids)) and got[4].min() >= 0 and got[3].max() == 3
    after = [fleet.fleet_get_state(r) + (fleet.fleet_get_landmark_ids(r),) for r in range(3)]
    for r in range(3):
        assert same_bits(before[r], after[r]), f"robot {r}: the merge changed its filter"
    # the merged map is the surveyed world seen from robot 0's start frame, to the filters' accuracy
    got = fleet.fleet_merge_maps()
    order = np.argsort(ids)
    assert np.abs(got[1] - into_frame(xyth[order], np.array(STARTS[0]))).max() < 0.1


def test_merged_map_localizes_the_fleet(surveyed):
    slam, ids, xyth, true_poses = surveyed
    m_ids, m_xyth, _, _, rounds, T = slam.fleet_merge_maps()
    poses, sig = slam.fleet_get_poses()
    moved = np.zeros((3, 3))
    for r in range(3):                                                  # each robot's pose estimate, through its map's T
        c, s = math.cos(T[r, 2]), math.sin(T[r, 2])
        moved[r] = [c * poses[r, 0] - s * poses[r, 1] + T[r, 0], s * poses[r, 0] + c * poses[r, 1] + T[r, 1], ref.wrap(poses[r, 2] + T[r, 2])]
    loc = emu_context(3, max_landmarks=12)
    loc.fleet_begin([CAM] * 3, m_ids, m_xyth, moved, 0.5 * (sig + sig.transpose(0, 2, 1)) + np.eye(3) * 1e-4)
    assert loc.is_fleet() == 3 and not loc.is_fleet_slam()
    rng = np.random.RandomState(13)
    for r in range(3):
        inject(loc, r, [(int(ids[k]), 1, observe(true_poses[r], xyth[k], rng), np.full(3, 0.02)) for k in VIEWS[r]])
    loc.stage_encoders([1.0] * 3, [1.0] * 3, [0.05] * 3)
    loc.fleet_run_staged(0, [0, 1, 2], with_ekf=2)
    loc.sync()
    stats = loc.get_slot_ekf_stats(0, 3)
    assert np.all(stats[:, 2] >= 1), f"a robot fused no correction against the merged map: {stats.tolist()}"
    assert np.array_equal(stats[:, 0], [len(v) for v in VIEWS])
    after, _ = loc.fleet_get_poses()
    world_in_anchor = [relative(np.array(p), np.array(STARTS[0])) for p in true_poses]
    assert np.abs(after - np.array(world_in_anchor)).max() < 0.2, "the fleet localizes in the anchor's frame"


# ---- 7: on the MI355X -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_64_maps_of_64_records(on_emulation):
    c = capi.Context(max_rows=64, max_cols=64, max_batch=2, max_landmarks=16)
    ids, xyth, frames, rec = leveled_case(6, 64, 64, 5, 40)
    got, _ = check_host_and_device(c, rec, on_emulation, "64 x 64")
    assert got[4].max() == 5 and got[4].min() == 0 and got[0].size == 240


@pytest.mark.gpu
def test_gpu_fleet_of_8_on_rendered_ring():
    from tests.test_fleet import ring_cams, render_fleet
    from tests.test_localize import small_ring
    w = synth.RingWorld(small_ring())
    cfg = w.cfg
    R, T = 8, 30
    cams = ring_cams(w, [260.0, 240.0] * 4, [(0.12, 0.02, 0.0), (0.1, -0.03, 0.0)] * 4)
    fleet = capi.Context(max_rows=cfg.rows, max_cols=cfg.cols, max_batch=R * T, max_landmarks=w.L + 8)
    synth.apply_detector(cfg, ctx=fleet)
    fleet.fleet_slam_begin(cams)
    frames = render_fleet(fleet, w, cams, [15 * r for r in range(R)], T)
    fleet.stage_frames(np.stack([frames[t][r][0] for t in range(T) for r in range(R)]))
    fleet.stage_encoders(*[[getattr(frames[t][r][1], k) for t in range(T) for r in range(R)] for k in ("wl", "wr", "dt")])
    fleet.fleet_run_staged(0, [r for t in range(T) for r in range(R)])
    fleet.sync()
    before = [fleet.fleet_get_state(r) for r in range(R)]
    rec = host_records(fleet, R)
    got = fleet.fleet_merge_maps()
    per_map = int(fleet.init.max_landmarks)
    assert same_bits(got, fleet.merge_map_records(rec, R, per_map))
    assert_merge_close(got, ref.merge(rec, R, per_map), "rendered fleet")
    assert got[4].min() >= 0 and got[4].max() >= 1 and got[0].size > max((rec["id"][r] >= 0).sum() for r in range(R))
    for r in range(R):
        assert same_bits(before[r], fleet.fleet_get_state(r)), f"robot {r}"


@pytest.mark.gpu
def test_gpu_one_rank_gather_then_merge_on_device():
    import torch
    from aruco_slam_amd.dist import MAP_DTYPE as DIST_DTYPE
    L = 16
    c = capi.Context(max_rows=64, max_cols=64, max_batch=2, max_landmarks=L)
    rng = np.random.RandomState(8)
    ids, xyth = world(rng, 9, id_pool=400)
    mu = np.concatenate([[0.1, 0.2, 0.3], xyth.reshape(-1)])
    S = np.zeros((mu.size, mu.size))
    for i in range(9):
        S[3 + 3 * i:6 + 3 * i, 3 + 3 * i:6 + 3 * i] = spd(rng)
    order = rng.permutation(9)
    c.set_state(np.concatenate([mu[:3], xyth[order].reshape(-1)]), S, ids[order])
    c.comm_create(capi.Context.comm_unique_id(), 1, 0)
    dst = torch.zeros(L * capi.MAP_RECORD_BYTES, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    c.comm_gather_maps_to_device(dst.data_ptr())
    got = c.merge_map_records(dst.data_ptr(), 1, L, on_device=True)
    own = np.frombuffer(c.export_map().tobytes(), dtype=DIST_DTYPE)
    c.comm_destroy()
    assert np.array_equal(np.frombuffer(dst.cpu().numpy().tobytes(), dtype=DIST_DTYPE), own)
    assert_merge_close(got, ref.merge(own, 1, L), "one rank")
    assert got[4].tolist() == [0] and np.array_equal(got[5], np.zeros((1, 3)))
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], xyth) and got[3].tolist() == [1] * 9


def test_map_gather_merges_its_own_buffer():
    """dist.MapGather.merge on the buffer its gather filled (one rank, host tensors): this rank's map, identity transform"""
    from aruco_slam_amd.dist import MapGather
    c = emu_context(2, max_landmarks=6)
    rng = np.random.RandomState(9)
    ids, xyth = world(rng, 4, id_pool=300)
    S = np.zeros((15, 15))
    for i in range(4):
        S[3 + 3 * i:6 + 3 * i, 3 + 3 * i:6 + 3 * i] = spd(rng)
    c.set_state(np.concatenate([[0.0, 0.0, 0.0], xyth[::-1].reshape(-1)]), S, ids[::-1])
    g = MapGather(c)
    g.gather()
    got = g.merge()
    assert_merge_close(got, ref.merge(g.records(), 1, 6), "gathered")
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], xyth) and got[4].tolist() == [0]
