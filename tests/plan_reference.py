"""Exact reference of the plan stage of one EKF frame (k_ekf_plan in csrc/ekf.hip, and its host mirror, the window planner in
csrc/capi.hip), and the generator of the frames tests/test_plan_kernel.py drives through it (a plain helper module).

The plan is what the reference does between the detections and the arithmetic (aruco_slam.cpp:88-263, as oracle/ekf_literal.py
states it): checkLandmark on every detection that passed the gates, obs_.push in detection order, pops in the order of libstdc++'s
std::priority_queue (new markers first, then ascending landmark index; equal keys in heap order), an augment per new marker, and
per mapped marker the "stationary" test against the first entry with its id in the previous frame's list.  The pop order comes
from the real std::priority_queue (oracle.pyoracle.heap_order); oracle/ekf_literal.py::_Heap is asserted to agree on every list.
There is no shortcut for lists of distinct keys.  What the device adds to the reference is stated here, not taken from the kernel's
text: the landmark cap (a new marker that finds the map full is popped with action 0 and index -1 and reported, mask 0x20), the
cap on fused corrections (a frame above it keeps its predict and its augments, fuses nothing and is reported, mask 0x40) and the
id table of 1024 entries (an id outside [0, 1024) is never remembered).

The numbers come from LiteralSlam's own correct / augment, called in exactly that pop order on the pre-frame mean."""
import math

import numpy as np

from ekf_reference import LD, observe, predicted_pose, random_state, wrap_once
from oracle import pyoracle as orc
from oracle.ekf_literal import LiteralSlam, _Heap

ID_TABLE = 1024
OVF_LANDMARKS, OVF_UPDATES = 0x20, 0x40
WL, WR, DT = 2.0, 2.3, 1 / 30.0


def pop_order(keys):
    """pop order (positions in the push sequence) of std::priority_queue for the pushed aruco_index_ values; both opinions agree"""
    keys = [int(k) for k in keys]
    if not keys:
        return []
    real = orc.heap_order(keys).tolist()
    q = _Heap()
    for i, k in enumerate(keys):
        q.push(dict(index=k, pos=i))
    second = []
    while q.c:
        second.append(q.pop()["pos"])
    assert real == second, "oracle/ekf_literal.py::_Heap and std::priority_queue disagree"
    return real


class PlanReference:
    """the filter between frames: mu, Sigma (in a LiteralSlam), the landmark ids in index order, the id table (first index per
    id) and the previous frame's last-observed list [(id, z or None)]"""

    def __init__(self, mu, S, ids, max_landmarks, cap, last=()):
        self.lit = LiteralSlam()
        self.lit.mu, self.lit.sigma = np.array(mu, float), np.array(S, float)
        self.ids = [int(i) for i in ids]
        self.table = {}
        for k, i in enumerate(self.ids):
            if 0 <= i < ID_TABLE:
                self.table.setdefault(i, k)
        self.max_landmarks, self.cap = int(max_landmarks), int(cap)
        self.last = list(last)
        self.t = 0.0
        self.lit.add_encoder(0.0, 0.0, 0.0)                  # the arming sample

    @property
    def L(self):
        return len(self.ids)

    def state(self):
        return self.lit.mu.copy(), self.lit.sigma.copy()

    def frame(self, obs, wl=WL, wr=WR, dt=DT):
        """predict, then the frame obs = [(id, valid, z, Rdiag)] in detection order.  Returns dict(pop = [(id, index, action,
        detection position)], L, ids, stats = [nM, augments, fused updates, stationary], mask, last = the next last-observed list)"""
        lit = self.lit
        self.t += dt
        lit.add_encoder(wl, wr, self.t)
        mu0 = lit.mu.copy()                                  # every observation is linearised at the pre-frame mean
        pushed = []                                          # (detection position, id, index) of what passed the gates
        for det, (lid, valid, z, r) in enumerate(obs):
            if valid:
                pushed.append((det, int(lid), self.table.get(int(lid), -1) if 0 <= int(lid) < ID_TABLE else -1))
        pops = [pushed[k] for k in pop_order([p[2] for p in pushed])]
        assert [p[2] for p in pops] == sorted(p[2] for p in pops), "new markers first, then ascending index"
        prev = {}                                            # std::find: the first entry with the id
        for lid, z in self.last:
            prev.setdefault(lid, z)
        mask, plan = 0, []
        for det, lid, index in pops:
            z = np.asarray(obs[det][2], float)
            if index < 0:
                action = 0
                if self.L >= self.max_landmarks:
                    mask |= OVF_LANDMARKS
                    plan.append((lid, -1, 0, det, False))
                    continue
                plan.append((lid, -1, 0, det, True))
                if 0 <= lid < ID_TABLE:
                    self.table.setdefault(lid, self.L)      # std::map::insert keeps the first
                self.ids.append(lid)
            else:
                zl = prev.get(lid)
                stationary = zl is not None and float(np.linalg.norm(np.asarray(zl, float) - z)) < 0.01
                plan.append((lid, index, 2 if stationary else 1, det, not stationary))
        m = sum(1 for p in plan if p[2] == 1)
        if m > self.cap:
            mask |= OVF_UPDATES
        # the numbers: LiteralSlam's own branches in this pop order
        observed, nxt = [], []
        for lid, index, action, det, applied in plan:
            z, r = np.asarray(obs[det][2], float), np.asarray(obs[det][3], float)
            ob = dict(id=lid, index=index, z=z, R=np.diag(r), last=np.full(3, np.nan))
            if action == 0:
                if applied:
                    assert lit.augment(ob, mu0) == 0
            elif mask & OVF_UPDATES:
                if action == 1:
                    ob["last"] = z                           # the list is written as if the frame had been fused
            else:
                assert lit.correct(ob, mu0) == action, "LiteralSlam takes the other branch of the stationary rule"
            observed.append(ob)
            nxt.append((lid, z.copy() if action == 1 else None))
        lit.last_observed = observed
        self.last = nxt
        assert lit.mu.size == 3 + 3 * self.L
        n_stat = sum(1 for p in plan if p[2] == 2)
        n_aug = sum(1 for p in plan if p[2] == 0 and p[4])
        return dict(pop=[p[:4] for p in plan], L=self.L, ids=list(self.ids), stats=[len(obs), n_aug, 0 if mask & OVF_UPDATES else m, n_stat],
                    mask=mask, last=list(nxt))


# ---- frames --------------------------------------------------------------------------------------------------------------------

def new_z(rng):
    return np.array([rng.uniform(0.5, 2), rng.uniform(-1, 1), rng.uniform(-3, 3)])


def make_frame(rng, ref, spec, prev_obs, shift=0.0, kl=0.05, kr=0.05, b=0.09):
    """one frame from spec = [(kind, what)] in detection order, observed from the reference's current state:
    ("new", id): an observation of an id (mapped or not) at a random place; ("known", index): a noisy observation of that landmark
    under its id; ("repeat", id or (id, detection position there)): the previous frame's observation of the id again;
    ("gated", id): an observation that did not pass the gates (valid = 0).  shift moves the x of the "known" observations (frames that alternate it are never "stationary").  Asserts the margins that keep the reference's own decisions away from rounding."""
    mu = ref.lit.mu
    pose = predicted_pose(mu, WL, WR, DT, kl=kl, kr=kr, b=b)
    obs = []
    for kind, what in spec:
        if kind == "known":
            _, z, r = observe(rng, mu, [what], post_predict=pose)[0]
            z[0] += shift
            obs.append((ref.ids[what], 1, z, r))
        elif kind == "repeat":
            if isinstance(what, tuple):                      # (id, detection position in the previous frame)
                what, z = what[0], prev_obs[what[1]][2]
            else:
                z = next(o[2] for o in prev_obs if o[0] == what and o[1])
            obs.append((int(what), 1, z.copy(), rng.uniform(0.02, 0.2, 3)))
        elif kind == "new":
            obs.append((int(what), 1, new_z(rng), rng.uniform(0.02, 0.2, 3)))
        else:
            assert kind == "gated"
            obs.append((int(what), 0, new_z(rng), rng.uniform(0.02, 0.2, 3)))
    dth = (kr * DT * WR - kl * DT * WL) / (2 * b)
    assert abs(abs(float(mu[2]) + dth) - math.pi) > 1e-6, "the predicted heading is within 1e-6 of +-pi before its wrap"
    check_margins(ref, obs, prev_obs, pose)
    return obs


def check_margins(ref, obs, prev_obs, pose):
    zs = [tuple(o[2]) for o in obs]
    assert len(set(zs)) == len(zs), "two observations of a frame with the same z: the detection position would be ambiguous"
    for lid, valid, z, _ in obs:
        if not valid:
            continue
        for plid, pvalid, pz, _ in prev_obs:
            if pvalid and plid == lid:
                d = float(np.linalg.norm(np.asarray(pz) - z))
                assert not 0.009 <= d <= 0.011, f"id {lid}: {d} from its previous observation, at the stationary threshold"
        index = ref.table.get(lid, -1) if 0 <= lid < ID_TABLE else -1
        if index >= 0:
            rel = float(ref.lit.mu[5 + 3 * index] - pose[2])
            inno = float(z[2] - float(wrap_once(LD(rel))))
            angles = (rel, inno)
        else:
            angles = (float(pose[2] + z[2]),)
        for a in angles:
            assert abs(abs(a) - math.pi) > 1e-6, f"id {lid}: an angle within 1e-6 of +-pi before its wrap"


def dense_state(seed, L):
    rng = np.random.RandomState(seed)
    mu, S = random_state(rng, L)
    return rng, mu, S
