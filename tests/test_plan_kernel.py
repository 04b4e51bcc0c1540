"""k_ekf_plan (csrc/ekf.hip) at the edges of its observation list, and the host's mirror of it (the window planner in csrc/capi.hip),
against the exact reference of the plan stage in tests/plan_reference.py.

Each case is one arming sample, then one or more frames of injected observations on an injected dense state, every frame through
run_staged(..., with_ekf=2) in a context without windows: the pop list (id, index, action, detection position), L, the landmark
ids, the per-slot statistics and the overflow mask are compared with ==, mu and Sigma at the bounds of tests/test_ekf_sizes.py
(mu rtol 1e-9 / atol 1e-11, Sigma 1e-9 relative).  The lists have 1, 2, 63, 64, 65, 127 and 128 entries (one and two wavefronts of
the kernel's ballots); what they are made of is in each builder below, which also asserts the coverage it claims on the reference's
result (the device's equals it).  Every multi-frame case runs again with windows on, followed by 8 clean frames, so that the host
planner has to continue from the device's tables or from its own; three of them run as the three robots of one fleet round.
Runs on the emulation build without a GPU and again, marked gpu, on the real library."""
import functools
import os
import re

import numpy as np
import pytest

from aruco_slam_amd import capi, synth
from ekf_reference import CHAIN_KERNELS, chain_of, ekf_kernels_run, rel_err
from plan_reference import DT, ID_TABLE, OVF_LANDMARKS, OVF_UPDATES, WL, WR, PlanReference, dense_state, make_frame

E_CAPACITY = -4
LENGTHS = (1, 2, 63, 64, 65, 127, 128)


def context(cap, ML, batch, windows=False):
    kw = dict(max_rows=64, max_cols=64, max_batch=batch, persistent_waves=4, max_landmarks=ML, max_updates_per_frame=cap)
    if windows:
        return capi.Context(**kw)
    os.environ["ASLAM_NO_WINDOWS"] = "1"
    try:
        return capi.Context(**kw)
    finally:
        os.environ.pop("ASLAM_NO_WINDOWS", None)


def sync_mask(ctx):
    """sync; the overflow mask it reports (0: none)"""
    try:
        ctx.sync()
    except capi.AslamError as e:
        assert e.code == E_CAPACITY, e
        return int(re.search(r"mask 0x([0-9a-f]+)", str(e)).group(1), 16)
    return 0


def inject(ctx, slot, obs):
    ctx.inject_observations(slot, [o[0] for o in obs], [o[1] for o in obs], np.array([o[2] for o in obs]).reshape(-1, 3),
                            np.array([o[3] for o in obs]).reshape(-1, 3))


def arrange(rng, pinned, rest):
    """a detection order: pinned = {position: entry}, the rest shuffled into the other positions"""
    out = [None] * (len(pinned) + len(rest))
    for pos, e in pinned.items():
        out[pos] = e
    it = iter([rest[i] for i in rng.permutation(len(rest))])
    return [e if e is not None else next(it) for e in out]


class Case:
    """an injected state, its frames and what the reference makes of them (built once, on the CPU, shared by every test of the case)"""

    def __init__(self, name, seed, L0, ML, cap, numerics=True):
        self.name, self.ML, self.cap, self.numerics = name, ML, cap, numerics
        self.rng, self.mu0, self.S0 = dense_state(seed, L0)
        perm = self.rng.permutation(ID_TABLE)
        self.ids0 = perm[:L0].astype(np.int32)
        self.spare = [int(i) for i in perm[L0:]]
        self.ref = PlanReference(self.mu0, self.S0, self.ids0, ML, cap)
        self.frames, self.exp, self.states = [], [], []
        self.n_data = None

    def fresh(self, n):
        out, self.spare = self.spare[:n], self.spare[n:]
        return out

    def add(self, spec, shift=0.0):
        obs = make_frame(self.rng, self.ref, spec, self.frames[-1] if self.frames else [], shift)
        e = self.ref.frame(obs)
        self.frames.append(obs); self.exp.append(e); self.states.append(self.ref.state())
        return e

    def add_clean(self, n=8, k=12):
        """n frames that see one fixed set of k landmarks, each under an id the table maps to it"""
        self.n_data = len(self.frames)
        cands = sorted(set(self.ref.table.values()))
        seen = [int(i) for i in self.rng.choice(cands, min(k, len(cands)), replace=False)]
        for k in range(n):
            e = self.add(arrange(self.rng, {}, [("known", i) for i in seen]), shift=0.06 * (-1) ** k)
            assert e["stats"] == [len(seen), 0, len(seen), 0] and e["mask"] == 0
        return self

    def data_frames(self):
        return len(self.frames) if self.n_data is None else self.n_data

    def kinds(self, f):
        """detection positions of frame f by kind: new, update, stationary, gated"""
        out = dict(new=[], update=[], stationary=[], gated=[k for k, o in enumerate(self.frames[f]) if not o[1]])
        for _, _, action, det in self.exp[f]["pop"]:
            out[("new", "update", "stationary")[action]].append(det)
        return out

    def both_waves(self, f, kinds):
        k = self.kinds(f)
        for name in kinds:
            assert min(k[name]) < 64 <= max(k[name]), f"{self.name}: no {name} entry on both sides of detection position 63 / 64"


# ---- the cases -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def all_new(nM, L0, clean=False):
    """nM new ids in one shuffled frame: the heap order among up to 128 equal keys decides the landmark indices; then a frame
    (or 8, for the host planner) that observes some of them under those indices"""
    c = Case(f"all new nM {nM} L0 {L0}", 100 + nM + L0, L0, L0 + 128, (24, 64, 128)[nM % 3])
    e = c.add(arrange(c.rng, {}, [("new", i) for i in c.fresh(nM)]))
    assert e["stats"] == [nM, nM, 0, 0] and e["mask"] == 0 and e["L"] == L0 + nM
    assert [p[2] for p in e["pop"]] == [0] * nM and sorted(p[3] for p in e["pop"]) == list(range(nM))
    if nM > 2:
        assert [p[3] for p in e["pop"]] != list(range(nM)), "the heap order equals the detection order: nothing is tested"
    if nM >= 65:
        c.both_waves(0, ["new"])
    if clean:
        return c.add_clean()
    seen = [int(i) for i in c.rng.choice(e["L"], min(e["L"], 12), replace=False)]
    e = c.add(arrange(c.rng, {}, [("known", i) for i in seen]))
    assert e["stats"] == [len(seen), 0, len(seen), 0]
    return c


@functools.lru_cache(maxsize=None)
def known_gated(nM):
    """known, distinct ids (the rank path), with gated entries at detection positions 0, 63, 64 and nM - 1"""
    L = nM + 19
    c = Case(f"known + gated nM {nM}", 200 + nM, L, L + 1, 128)
    gated = sorted({0, 63, 64, nM - 1} & set(range(nM)))
    idx = [int(i) for i in c.rng.choice(L, nM, replace=False)]
    pinned = {g: ("gated", int(c.ids0[idx[k]])) for k, g in enumerate(gated)}
    e = c.add(arrange(c.rng, pinned, [("known", i) for i in idx[len(gated):]]))
    m = nM - len(gated)
    assert c.kinds(0)["gated"] == gated and e["stats"] == [nM, 0, m, 0] and e["mask"] == 0
    assert [p[1] for p in e["pop"]] == sorted(idx[len(gated):]) and all(p[2] == 1 for p in e["pop"])
    if nM >= 127:
        c.both_waves(0, ["update", "gated"])
    return c


@functools.lru_cache(maxsize=None)
def mixed(nM, clean=False):
    """new, known, stationary and gated entries on both sides of detection position 63 / 64; in pop order the new ones end below
    position 64 and the fused updates lie on both sides of it (the ballot prefix across the two wavefronts)"""
    L0, n_new, n_gated, n_stat, n_first = 100, 30, 8, 20, 40
    c = Case(f"mixed nM {nM}", 300 + nM, L0, 160, 128)
    first = [int(i) for i in c.rng.choice(L0, n_first, replace=False)]
    e = c.add(arrange(c.rng, {}, [("known", i) for i in first]))
    assert e["stats"] == [n_first, 0, n_first, 0]
    stat = first[:n_stat]
    n_upd = nM - n_new - n_gated - n_stat
    upd = [int(i) for i in c.rng.choice(sorted(set(range(L0)) - set(stat)), n_upd, replace=False)]
    entries = ([("new", i) for i in c.fresh(n_new)] + [("gated", int(c.ids0[i])) for i in c.rng.choice(L0, n_gated, replace=False)] +
               [("repeat", int(c.ids0[i])) for i in stat] + [("known", i) for i in upd])
    by_kind = {k: [x for x in entries if x[0] == k] for k in ("new", "gated", "repeat", "known")}
    pinned, rest = {}, []
    for j, k in enumerate(("new", "gated", "repeat", "known")):
        pinned[j] = by_kind[k][0]; pinned[64 + j] = by_kind[k][1]
        rest += by_kind[k][2:]
    e = c.add(arrange(c.rng, pinned, rest))
    assert e["stats"] == [nM, n_new, n_upd, n_stat] and e["mask"] == 0
    assert [[p[2] for p in e["pop"]].count(a) for a in (0, 1, 2)] == [n_new, n_upd, n_stat]
    c.both_waves(1, ["new", "update", "stationary", "gated"])
    fused = [q for q, p in enumerate(e["pop"]) if p[2] == 1]
    assert min(fused) < 64 <= max(fused), "the fused updates do not cross pop position 64"
    return c.add_clean() if clean else c


@functools.lru_cache(maxsize=None)
def known_repeated(copies):
    """one known id two / three times with the copies in different wavefronts and nothing new: the heap path with zero new entries;
    every copy is fused, in heap order"""
    nM, pos = {2: (65, (3, 64)), 3: (128, (10, 64, 127))}[copies]
    L = nM + 10
    c = Case(f"known id x{copies}", 400 + copies, L, L, 128)
    idx = [int(i) for i in c.rng.choice(L, nM - copies + 1, replace=False)]
    t = sorted(idx)[len(idx) // 2]
    e = c.add(arrange(c.rng, {p: ("known", t) for p in pos}, [("known", i) for i in idx if i != t]))
    assert e["stats"] == [nM, 0, nM, 0] and e["mask"] == 0
    run = [p for p in e["pop"] if p[1] == t]
    assert len(run) == copies and sorted(p[3] for p in run) == list(pos) and all(p[2] == 1 for p in run)
    assert [p[1] for p in e["pop"]] == sorted(p[1] for p in e["pop"])
    return c


@functools.lru_cache(maxsize=None)
def new_repeated(nM, pos):
    """a new id twice in one frame: two landmarks with one id, the id table keeps the first; the next frame corrects that one"""
    L0 = 10
    c = Case(f"new id twice nM {nM}", 500 + nM, L0, L0 + nM + 2, 24 if nM < 24 else 64)
    a = c.fresh(1)[0]
    n_known = min((nM - 2) // 2, L0)
    rest = [("known", int(i)) for i in c.rng.choice(L0, n_known, replace=False)] + [("new", i) for i in c.fresh(nM - 2 - n_known)]
    e = c.add(arrange(c.rng, {p: ("new", a) for p in pos}, rest))
    n_new = nM - n_known
    assert e["stats"] == [nM, n_new, n_known, 0] and e["mask"] == 0 and e["ids"].count(a) == 2
    i0 = e["ids"].index(a)
    assert c.ref.table[a] == i0
    e = c.add(arrange(c.rng, {}, [("known", i0)] + [("known", int(i)) for i in c.rng.choice(L0, 3, replace=False)]))
    assert (a, i0, 1) in [p[:3] for p in e["pop"]] and e["stats"] == [4, 0, 4, 0]
    return c.add_clean()


def _prev_dup(swap):
    L = 12
    c = Case(f"previous list holds an id twice ({'ab'[swap]})", 600, L, L, 24)
    x = 5
    xid = int(c.ids0[x])
    others = [i for i in range(L) if i != x]
    c.add(arrange(c.rng, {}, [("known", x)] + [("known", i) for i in others[:5]]))
    two = [("repeat", xid), ("known", x)]
    e = c.add(arrange(c.rng, {1: two[swap], 4: two[1 - swap]}, [("known", i) for i in others[3:7]]))
    run = [p for p in e["pop"] if p[0] == xid]
    assert sorted(p[2] for p in run) == [1, 2] and e["stats"] == [6, 0, 5, 1]
    upd_det = next(p[3] for p in run if p[2] == 1)
    first = "update" if run[0][2] == 1 else "stationary"
    e = c.add(arrange(c.rng, {}, [("repeat", (xid, upd_det))] + [("known", i) for i in others[6:9]]))
    # std::find takes the first entry with the id: the update's z (the same z: stationary) or the stationary entry's NaN (an update)
    assert next(p[2] for p in e["pop"] if p[0] == xid) == (2 if first == "update" else 1)
    return first, c


@functools.lru_cache(maxsize=None)
def prev_dup(first):
    """the previous frame's list holds an id twice, once as an update and once as stationary, with `first` popped first"""
    found = {}
    for swap in (0, 1):
        f, c = _prev_dup(swap)
        found[f] = c
    assert set(found) == {"update", "stationary"}, "swapping the two copies did not swap their pop order"
    return found[first].add_clean()


@functools.lru_cache(maxsize=None)
def capacity(n_new, room, clean=False):
    """n_new new ids and known ids in a frame with room for `room` landmarks: the first `room` new observations in pop order go in,
    the rest are popped with action 0 and index -1; the next frame sees a dropped id as new again"""
    if n_new == 2:
        L0, n_known, cap = 20, 10, 24
        ML = L0 + room
    else:
        ML, n_known, cap = 160, 20, 128
        L0 = ML - room
    c = Case(f"capacity n_new {n_new} room {room}", 700 + 10 * n_new + room + 50 * clean, L0, ML, cap)
    new = c.fresh(n_new)
    known = [int(i) for i in c.rng.choice(L0, n_known, replace=False)]
    e = c.add(arrange(c.rng, {}, [("new", i) for i in new] + [("known", i) for i in known]))
    went_in = min(room, n_new)
    pops = e["pop"]
    assert [p[2] for p in pops[:n_new]] == [0] * n_new and all(p[1] == -1 for p in pops[:n_new])
    assert e["L"] == ML and e["ids"][L0:] == [p[0] for p in pops[:went_in]]
    assert e["mask"] == (OVF_LANDMARKS if room < n_new else 0) and e["stats"] == [n_new + n_known, went_in, n_known, 0]
    assert [p[1] for p in pops[n_new:]] == sorted(known) and all(p[2] == 1 for p in pops[n_new:])
    if n_new == 65:
        c.both_waves(0, ["new", "update"])
    some = [("known", int(i)) for i in c.rng.choice(L0, 5, replace=False)]
    if room < n_new:
        dropped = pops[went_in][0]
        e = c.add(arrange(c.rng, {}, [("new", dropped)] + some))
        assert e["pop"][0][:3] == (dropped, -1, 0) and e["mask"] == OVF_LANDMARKS and e["stats"] == [6, 0, 5, 0] and e["L"] == ML
    else:
        e = c.add(arrange(c.rng, {}, [("known", L0)] + some))
        assert e["pop"][-1][:3] == (pops[0][0], L0, 1) and e["mask"] == 0 and e["stats"] == [6, 0, 6, 0]
    return c.add_clean() if clean else c


@functools.lru_cache(maxsize=None)
def update_cap(cap, clean=False):
    """cap + 1 corrections and three new landmarks in one frame: reported (mask 0x40 alone), the predict and the augments applied,
    no correction applied, the statistics count 0 fused updates; the last-observed list is written as if they had been fused"""
    L0 = cap + 10
    c = Case(f"update cap {cap}", 800 + cap, L0, L0 + 5, cap)
    known = [int(i) for i in c.rng.choice(L0, cap + 1, replace=False)]
    e = c.add(arrange(c.rng, {}, [("new", i) for i in c.fresh(3)] + [("known", i) for i in known]))
    assert e["mask"] == OVF_UPDATES and e["stats"] == [cap + 4, 3, 0, 0] and e["L"] == L0 + 3
    assert [p[2] for p in e["pop"]] == [0] * 3 + [1] * (cap + 1)
    mu_pred = PlanReference(c.mu0, c.S0, c.ids0, c.ML, cap)
    mu_pred.frame([])
    assert np.array_equal(c.states[0][0][:3 + 3 * L0], mu_pred.state()[0]), "a correction was applied"
    e = c.add(arrange(c.rng, {}, [("repeat", int(c.ids0[known[0]]))] + [("known", i) for i in known[1:6]]))
    assert e["mask"] == 0 and e["stats"] == [6, 0, 5, 1]
    return c.add_clean() if clean else c


@functools.lru_cache(maxsize=None)
def out_of_range():
    """ids outside [0, 1024) (only the injection call can deliver them): new in every frame, never in the id table, reported by the
    landmark id list.  (Pinned on the integer outputs only: the reference's std::map would remember such an id.)"""
    L0 = 8
    c = Case("ids outside the table", 900, L0, 20, 24, numerics=False)
    odd = [1024, 5000, -3]
    e = c.add(arrange(c.rng, {}, [("new", i) for i in odd] + [("known", i) for i in (0, 3, 5, 7)]))
    first = [p[0] for p in e["pop"][:3]]
    assert sorted(first) == sorted(odd) and e["stats"] == [7, 3, 4, 0] and e["mask"] == 0
    e = c.add(arrange(c.rng, {}, [("new", i) for i in odd] + [("known", i) for i in (1, 2, 6)]))
    assert [p[:3] for p in e["pop"][:3]] == [(p[0], -1, 0) for p in e["pop"][:3]] and e["stats"] == [6, 3, 3, 0]
    assert e["ids"][L0:L0 + 3] == first and sorted(e["ids"][L0 + 3:]) == sorted(odd) and e["L"] == L0 + 6
    return c.add_clean()


@functools.lru_cache(maxsize=None)
def new_only_in_second_wave():
    """every new id at a detection position >= 64, known ids everywhere else: the second wavefront's count of new entries alone
    decides that the frame has any"""
    L0 = 80
    c = Case("new ids only past detection position 63", 950, L0, 90, 128)
    known = [int(i) for i in c.rng.choice(L0, 66, replace=False)]
    e = c.add(arrange(c.rng, {64 + k: ("new", i) for k, i in enumerate(c.fresh(4))}, [("known", i) for i in known]))
    assert min(c.kinds(0)["new"]) >= 64 and e["stats"] == [70, 4, 66, 0] and e["mask"] == 0 and e["L"] == L0 + 4
    return c


@functools.lru_cache(maxsize=None)
def window_after_arming(L):
    """two clean frames and nothing before them: with windows on, a window of two frames directly behind the arming sample.  (On the
    emulation build the replay workgroups of such a short window used to publish their step count before every lane of the storing
    wave had stored: the Psi workgroups then read unwritten steps, and Sigma outside the window's set came back corrupt.)"""
    return Case(f"window after arming L {L}", 1, L, 30, 24).add_clean(2, 12)


# ---- running them ------------------------------------------------------------------------------------------------------------------

def check_state(c, f, mu, S, ids, where):
    e = c.exp[f]
    assert ids.tolist() == e["ids"], f"{where}: landmark ids"
    assert mu.shape == (3 + 3 * e["L"],), f"{where}: L"
    if not c.numerics:
        assert np.isfinite(mu).all() and np.isfinite(S).all()
        return 0.0, 0.0
    mu_r, S_r = c.states[f]
    e_mu, e_S = float(np.abs(mu - mu_r).max()), rel_err(S, S_r)
    assert np.allclose(mu, mu_r, rtol=1e-9, atol=1e-11), f"{where}: mu differs by {e_mu}"
    assert e_S <= 1e-9, f"{where}: Sigma differs by {e_S} (relative)"
    return e_mu, e_S


def run_case(c, n_frames=None):
    """every frame on the per-frame chain of a context without windows, checked after each; returns the final (mu, Sigma, ids)"""
    n = len(c.frames) if n_frames is None else n_frames
    ctx = context(c.cap, c.ML, n + 1)
    ctx.set_state(c.mu0, c.S0, c.ids0)
    ctx.stage_encoders([0.0] + [WL] * n, [0.0] + [WR] * n, [0.0] + [DT] * n)
    inject(ctx, 0, [])
    for f in range(n):
        inject(ctx, f + 1, c.frames[f])
    ctx.profile_enable(True)
    worst = [0.0, 0.0]
    for f in range(n):
        e, obs, where = c.exp[f], c.frames[f], f"{c.name}, frame {f}"
        ctx.profile_reset()
        ctx.run_staged(*((0, 2) if f == 0 else (f + 1, 1)), with_ekf=2)
        assert sync_mask(ctx) == e["mask"], f"{where}: overflow mask"
        assert ekf_kernels_run(ctx.profile_get()) == CHAIN_KERNELS[chain_of(c.cap)], where
        gi, gx, ga, gz, gR = ctx.get_observations()
        pop = e["pop"]
        assert np.stack([gi, gx, ga], 1).tolist() == [list(p[:3]) for p in pop], f"{where}: pop list (id, index, action)"
        assert np.array_equal(gz, np.array([obs[p[3]][2] for p in pop]).reshape(-1, 3)) and \
            np.array_equal(gR, np.array([obs[p[3]][3] for p in pop]).reshape(-1, 3)), f"{where}: detection positions of the pops"
        assert ctx.get_slot_ekf_stats(f + 1, 1)[0].tolist() == e["stats"], f"{where}: statistics"
        mu, S = ctx.get_state()
        ids = ctx.get_landmark_ids()
        err = check_state(c, f, mu, S, ids, where)
        worst = [max(a, b) for a, b in zip(worst, err)]
    print(f"{c.name}: {n} frames, cap {c.cap}, max_landmarks {c.ML}: worst |dmu| {worst[0]:.3g}, Sigma {worst[1]:.3g} relative")
    return mu, S, ids


def host_unclean(c, f):
    """frames the host planner must leave to the device: an id twice, an id outside the table, a new landmark past the capacity"""
    ids = [o[0] for o in c.frames[f] if o[1]]
    return len(ids) != len(set(ids)) or any(not 0 <= i < ID_TABLE for i in ids) or bool(c.exp[f]["mask"] & OVF_LANDMARKS)


def run_planner(c):
    """the case with windows on: the data frames in one staged call, together with the 8 clean frames when the host can plan them all
    (its own index assignment then serves the window), else the clean frames in a call of their own (from the device's tables)"""
    n, nd = len(c.frames), c.n_data
    bad = [f for f in range(nd) if host_unclean(c, f)]
    ctx = context(c.cap, c.ML, n + 1, windows=True)
    ctx.set_state(c.mu0, c.S0, c.ids0)
    ctx.stage_encoders([0.0] + [WL] * n, [0.0] + [WR] * n, [0.0] + [DT] * n)
    inject(ctx, 0, [])
    for f in range(n):
        inject(ctx, f + 1, c.frames[f])
    ctx.profile_enable(True)
    ctx.profile_reset()
    calls = [(0, n + 1)] if not bad else [(0, nd + 1), (nd + 1, n - nd)]
    for first, count in calls:
        ctx.run_staged(first, count, with_ekf=2)
        mask = 0
        for f in range(max(first - 1, 0), first + count - 1):
            mask |= c.exp[f]["mask"]
        assert sync_mask(ctx) == mask, f"{c.name}: overflow mask of slots {first} .. {first + count - 1}"
    ps = ctx.plan_stats()
    assert ps["windows"] >= 1 and ps["frames_in_windows"] >= 2, f"{c.name}: no window formed ({ps})"
    assert ps["frames_device_planned"] == (nd - bad[0] if bad else 0), f"{c.name}: frames left to the device ({ps}, unclean {bad})"
    assert ctx.profile_get()["k_ekf_win_step"][0] > 0
    mu, S = ctx.get_state()
    e_mu, e_S = check_state(c, n - 1, mu, S, ctx.get_landmark_ids(), f"{c.name}, windows on")
    print(f"{c.name}, windows on: {ps}: |dmu| {e_mu:.3g}, Sigma {e_S:.3g} relative")


KERNEL_CASES = ([(all_new, (nM, L0)) for nM in LENGTHS for L0 in (0, 5)] + [(known_gated, (nM,)) for nM in LENGTHS] +
                [(mixed, (127,)), (mixed, (128,)), (known_repeated, (2,)), (known_repeated, (3,)),
                 (new_repeated, (5, (1, 3))), (new_repeated, (66, (2, 65))), (prev_dup, ("update",)), (prev_dup, ("stationary",))] +
                [(capacity, (2, r)) for r in (0, 1, 2)] + [(capacity, (65, r)) for r in (0, 1, 64, 65)] +
                [(update_cap, (24,)), (update_cap, (64,)), (out_of_range, ()), (new_only_in_second_wave, ())])
# every multi-frame case again with windows on, and the window that follows the arming sample directly
PLANNER_CASES = ([(all_new, (nM, L0, True)) for nM in LENGTHS for L0 in (0, 5)] + [(mixed, (127, True)), (mixed, (128, True)),
                 (new_repeated, (5, (1, 3))), (new_repeated, (66, (2, 65))), (prev_dup, ("update",)), (prev_dup, ("stationary",))] +
                 [(capacity, (2, r, True)) for r in (0, 1, 2)] + [(capacity, (65, r, True)) for r in (0, 1, 64, 65)] +
                 [(update_cap, (24, True)), (update_cap, (64, True)), (out_of_range, ()), (window_after_arming, (20,)),
                  (window_after_arming, (24,))])


def _id(case):
    fn, args = case
    return fn.__wrapped__.__name__ + "".join(f"-{a}" for a in args).replace(" ", "").replace("(", "").replace(")", "").replace(",", "_")


@pytest.mark.parametrize("case", KERNEL_CASES, ids=_id)
def test_plan_against_reference(case):
    run_case(case[0](*case[1]))


@pytest.mark.parametrize("case", PLANNER_CASES, ids=_id)
def test_host_planner_continues_the_plan(case):
    run_planner(case[0](*case[1]))


def test_lengths_and_compositions_are_covered():
    """the list lengths of the issue, each composition at the lengths where it can occur"""
    for fn in (all_new, known_gated):
        assert {a[0] for f, a in KERNEL_CASES if f is fn} == set(LENGTHS)
    assert {a for f, a in KERNEL_CASES if f is capacity} == {(n, r) for n in (2, 65) for r in (0, 1, n - 1, n)}
    multi = {(f, a) for f, a in KERNEL_CASES if f not in (known_gated, known_repeated, new_only_in_second_wave)}
    assert multi <= {(f, a[:-1] if a and a[-1] is True else a) for f, a in PLANNER_CASES}, "a multi-frame case does not run with windows on"
    assert {a[0] for f, a in KERNEL_CASES if f is update_cap} == {24, 64}


def fleet_round(order):
    """three robots in one context: an empty list, the 128-entry mixed list and a capacity case, frame by frame in one round each;
    returns every robot's final (mu, Sigma, ids) and the masks the syncs reported"""
    cases = fleet_cases()
    cam = (synth.camera_matrix(64, 64, 60.0), np.zeros(5), (0.0, 0.0, 0.0))
    fleet = capi.Context(max_rows=64, max_cols=64, max_batch=3, persistent_waves=4, max_landmarks=160, max_updates_per_frame=128)
    fleet.fleet_slam_begin([cam] * 3)
    for r, (c, frames) in enumerate(cases):
        fleet.fleet_set_state(r, c.mu0, c.S0, c.ids0)
    masks = []
    for f in range(-1, 2):                               # the arming samples, then the two frames
        for s, r in enumerate(order):
            inject(fleet, s, cases[r][1][f] if f >= 0 else [])
        fleet.stage_encoders(*[[v if f >= 0 else 0.0] * 3 for v in (WL, WR, DT)])
        fleet.fleet_run_staged(0, order, with_ekf=2)
        masks.append(sync_mask(fleet))
        if f >= 0:
            stats = fleet.get_slot_ekf_stats(0, 3)
            for s, r in enumerate(order):
                c = cases[r][0]
                assert stats[s].tolist() == (c.exp[f]["stats"] if c.exp else [0, 0, 0, 0]), f"robot {r}, frame {f}: statistics"
    return [(*fleet.fleet_get_state(r), fleet.fleet_get_landmark_ids(r)) for r in range(3)], masks


@functools.lru_cache(maxsize=None)
def fleet_cases():
    empty = Case("empty list", 1000, 3, 160, 128)
    m, cp = mixed(128), capacity(65, 64)
    assert (m.ML, m.cap) == (cp.ML, cp.cap) == (160, 128)
    return ((empty, [[], []]), (m, m.frames[:2]), (cp, cp.frames[:2]))


def _fleet_equals_single_contexts():
    cases = fleet_cases()
    got, masks = fleet_round([0, 1, 2])
    assert masks == [0, cases[2][0].exp[0]["mask"], cases[2][0].exp[1]["mask"]] and masks[1] == OVF_LANDMARKS, "robot three's capacity error"
    for r, (c, frames) in enumerate(cases):
        if c.exp:
            mu, S, ids = run_case(c, 2)
        else:                                            # the empty list: arming, then two predictions
            one = context(128, 160, 3)
            one.set_state(c.mu0, c.S0, c.ids0)
            one.stage_encoders([0.0, WL, WL], [0.0, WR, WR], [0.0, DT, DT])
            for s in range(3):
                inject(one, s, [])
            one.run_staged(0, 3, with_ekf=2)
            one.sync()
            (mu, S), ids = one.get_state(), one.get_landmark_ids()
            assert not np.array_equal(mu[:3], c.mu0[:3]) and np.array_equal(mu[3:], c.mu0[3:])
        assert np.array_equal(got[r][0], mu) and np.array_equal(got[r][1], S) and np.array_equal(got[r][2], ids), \
            f"robot {r} ({c.name}) differs from its own context"
    again, masks2 = fleet_round([2, 0, 1])
    assert masks2 == masks
    for r in range(3):
        for a, b in zip(got[r], again[r]):
            assert np.array_equal(a, b), f"robot {r} changed with the order of the robots in the call"


def test_fleet_round_equals_single_contexts():
    _fleet_equals_single_contexts()


# ---- the same on the real library ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", KERNEL_CASES, ids=_id)
def test_plan_against_reference_on_gpu(case):
    run_case(case[0](*case[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLANNER_CASES, ids=_id)
def test_host_planner_continues_the_plan_on_gpu(case):
    run_planner(case[0](*case[1]))


@pytest.mark.gpu
def test_fleet_round_equals_single_contexts_on_gpu():
    _fleet_equals_single_contexts()
