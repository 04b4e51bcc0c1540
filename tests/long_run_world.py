"""The small ring world of the long runs (tests/test_long_runs.py), its observation streams and their references; a plain helper module.

The world: L landmarks on a circle of radius 3 m, ids (37 i + 5) mod 1024, random headings.  The robot turns nearly in place (wl = -2.0,
wr = 2.3, dt = 1/30: 0.0398 rad per frame, about 158 frames per lap), so its heading wraps once per lap, in the predict, in the
innovations and in the augments.  Every frame sees the m landmarks nearest in bearing, in a shuffled detection order, with measurement
noise (2e-3, 2e-3, 1e-3) and R = diag(0.05, 0.05, 0.01).  The pose starts at 0, where the filter starts; `phase` turns the world
about it, so that streams of different phase meet the landmarks in another order and build another map.

reference_run drives tests/plan_reference.PlanReference (LiteralSlam's own augment / correct: double, dense literal products) from
the empty map; gated_reference_run does the same with tests/slam_gate_reference.GatedLiteralSlam.  long_double_tail restates the
corrections behind the map build with ekf_reference.reference_step in long double: the distance between the two is the floor that
any bound on the device's error is judged against.  Results are cached on their arguments: the cases of one stream share them.

consistent_reference_run, consistent_gated_reference_run and consistent_long_double_tail are the same three with consistent
innovations (tests/consistent_reference.py: ConsistentPlanReference, ConsistentLiteral, consistent_step), for
tests/test_long_runs_consistent.py; with consistent = False the two runs are reference_run and gated_reference_run bit for bit.
HONEST_R is the variance of the noise the sightings carry (NOISE squared): with it the gains are of order one."""
import functools
import math

import numpy as np

from consistent_reference import ConsistentLiteral, ConsistentPlanReference, consistent_step
from ekf_reference import LD, predicted_pose, reference_step, rel_err, wrap_once
from plan_reference import PlanReference
from slam_gate_reference import GatedLiteralSlam, gated_reference_step

WL, WR, DT = -2.0, 2.3, 1 / 30.0
RADIUS = 3.0
NOISE = (2e-3, 2e-3, 1e-3)
RDIAG = (0.05, 0.05, 0.01)
HONEST_R = tuple(n * n for n in NOISE)               # (4e-6, 4e-6, 1e-6)
SCHEDULE = (1, 7, 64, 33, 2, 50)                     # batch lengths of the calls, cycled; max_batch = 64
MAX_BATCH = 64
LAP = 160                                            # frames: 2 pi / 0.0398 = 157.8 rounded up
OUTLIER_SHIFT = 0.5                                  # metres added to z[0] of a planted outlier
OUTLIER_FROM = 106                                   # two thirds of a lap: the map of the gated case is complete after frame 105
REPEAT_MARGIN = 0.05                                 # 5 x the "stationary" rule's 0.01


class Stream(tuple):
    """frames = ((wl, wr, dt), [(id, valid, z, Rdiag)] in detection order); hashed by the arguments that made it"""

    def __new__(cls, frames, key, outliers, wraps=(), ids=None, world=None):
        self = super().__new__(cls, frames)
        self.key, self.outliers = key, outliers      # outliers: {frame: id of the displaced sighting}
        self.wraps = tuple(wraps)                    # the frames whose predict takes the true heading across +-pi
        self.ids, self.world = ids, world            # the true map: marker ids and (x, y, theta), in landmark order
        return self

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return isinstance(other, Stream) and self.key == other.key

    def __ne__(self, other):
        return not self == other


def batches_of(frames, schedule=SCHEDULE):
    """((first frame, count), ...) of the calls: the schedule cycled until `frames` frames are spent"""
    out, f, k = [], 0, 0
    while f < frames:
        n = min(schedule[k % len(schedule)], frames - f)
        out.append((f, n))
        f += n; k += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ring_stream(L, m, frames, seed, phase=0.0, outlier_every=0, R=RDIAG, start=0.0):
    """the stream of `frames` frames.  outlier_every = k > 0: from frame OUTLIER_FROM on, every k-th frame's first sighting (detection
    order) has z[0] moved by OUTLIER_SHIFT; the random draws do not depend on it, so the stream is otherwise the one without outliers.
    R: the Rdiag every sighting carries (the draws do not depend on it either).  start: the true heading before frame 0 (robots that
    share one world, and so one map, start at different headings; a filter on such a stream starts at (0, 0, start))"""
    rng = np.random.RandomState(seed)
    ang = np.linspace(0, 2 * math.pi, L, endpoint=False) + phase
    world = np.stack([RADIUS * np.cos(ang), RADIUS * np.sin(ang), rng.uniform(-3, 3, L)], 1)
    ids = (37 * np.arange(L) + 5) % 1024
    assert len(set(ids.tolist())) == L
    pose = np.array([0.0, 0.0, start])
    out, outliers, wraps, prev = [], {}, [], {}
    for f in range(frames):
        new = predicted_pose(pose, WL, WR, DT)
        if abs(new[2] - pose[2]) > 3:
            wraps.append(f)
        pose = new
        rel = (np.arctan2(world[:, 1] - pose[1], world[:, 0] - pose[0]) - pose[2] + math.pi) % (2 * math.pi) - math.pi
        seen = rng.permutation(np.argsort(np.abs(rel), kind="stable")[:m])
        c, s = math.cos(pose[2]), math.sin(pose[2])
        obs, now = [], {}
        for k, i in enumerate(seen):
            dx, dy = world[i, 0] - pose[0], world[i, 1] - pose[1]
            z = np.array([dx * c + dy * s, -dx * s + dy * c, float(wrap_once(LD(world[i, 2] - pose[2])))]) + rng.normal(0, NOISE)
            if outlier_every and k == 0 and f >= OUTLIER_FROM and f % outlier_every == 0:
                z[0] += OUTLIER_SHIFT
                outliers[f] = int(ids[i])
            z[2] = float(wrap_once(LD(z[2])))
            lid = int(ids[i])
            if lid in prev:
                d = float(np.linalg.norm(prev[lid] - z))
                assert d > REPEAT_MARGIN, f"frame {f}: id {lid} is sighted {d} from its previous sighting (the stationary rule's 0.01)"
            now[lid] = z
            obs.append((lid, 1, z, np.array(R)))
        prev = now
        out.append(((WL, WR, DT), obs))
    for f0 in range(0, frames - LAP + 1, LAP):
        assert any(f0 <= w < f0 + LAP for w in wraps), f"the heading does not cross +-pi in frames {f0} .. {f0 + LAP - 1}"
    return Stream(out, (L, m, frames, seed, phase, outlier_every, tuple(R), start), outliers, wraps, ids.astype(np.int32), world)


def _exact_dt(lit):
    lit.last_time = 0.0                              # every sample's dt is DT exactly (t_now - last_time of a running clock is not)


@functools.lru_cache(maxsize=None)
def reference_run(stream, max_landmarks, cap, batches):
    """PlanReference from mu = 0(3), Sigma = 0(3 x 3), no ids.  Returns dict(states = [(mu, Sigma)], ids = [[id]], mask = [int],
    pops = [[(id, index, action)]] at the end of every batch (pops: of its last frame), stats = [[4 ints]] of every frame,
    complete = the frame after which the map holds every landmark)"""
    return _plan_run(PlanReference(np.zeros(3), np.zeros((3, 3)), [], max_landmarks, cap), stream, batches)


def _plan_run(ref, stream, batches):
    res = dict(states=[], ids=[], mask=[], pops=[], stats=[], complete=None)
    L = len({o[0] for _, obs in stream for o in obs})
    for first, count in batches:
        mask = 0
        for f in range(first, first + count):
            (wl, wr, dt), obs = stream[f]
            ref.t = 0.0
            _exact_dt(ref.lit)
            r = ref.frame(obs, wl, wr, dt)
            mask |= r["mask"]
            res["stats"].append(r["stats"])
            if res["complete"] is None and r["L"] == L:
                res["complete"] = f
        res["states"].append(ref.state()); res["ids"].append(list(ref.ids)); res["mask"].append(mask)
        res["pops"].append([p[:3] for p in r["pop"]])
    return res


@functools.lru_cache(maxsize=None)
def gated_reference_run(stream, batches, gate_d2):
    """GatedLiteralSlam from the empty map under the SLAM gate: reference_run's results (mask: none, the literal filter has no caps)
    plus health = the slot record of every frame, track = the track record at the end of every batch, rejected = {frame: [id]}"""
    lit = GatedLiteralSlam(gate=dict(gate_d2=gate_d2))
    res = _gated_run(lit, stream, batches)
    lit.assert_margins()
    return res


def _gated_run(lit, stream, batches):
    lit.add_encoder(0.0, 0.0, 0.0)                   # the arming sample
    lit.add_frame([])
    res = dict(states=[], ids=[], mask=[], pops=[], stats=[], health=[], track=[], rejected={}, complete=None)
    L = len({o[0] for _, obs in stream for o in obs})
    for first, count in batches:
        for f in range(first, first + count):
            (wl, wr, dt), obs = stream[f]
            _exact_dt(lit)
            lit.add_encoder(wl, wr, dt)
            lit.add_frame([(o[0], o[2], o[3]) for o in obs])
            res["stats"].append(list(lit.stats)); res["health"].append(dict(lit.health))
            rej = [i for i, _, a in lit.log if a == 3]
            if rej:
                res["rejected"][f] = rej
            if res["complete"] is None and len(lit.id_map) == L:
                res["complete"] = f
        res["states"].append((lit.mu.copy(), lit.sigma.copy()))
        res["ids"].append(sorted(lit.id_map, key=lit.id_map.get)); res["mask"].append(0)
        res["pops"].append(list(lit.log)); res["track"].append(dict(lit.track))
    return res


@functools.lru_cache(maxsize=None)
def consistent_reference_run(stream, max_landmarks, cap, batches, consistent=True):
    """reference_run with consistent innovations (ConsistentPlanReference); consistent = False is reference_run bit for bit"""
    return _plan_run(ConsistentPlanReference(np.zeros(3), np.zeros((3, 3)), [], max_landmarks, cap, consistent=consistent), stream, batches)


@functools.lru_cache(maxsize=None)
def consistent_gated_reference_run(stream, batches, gate_d2, consistent=True):
    """gated_reference_run with consistent innovations (ConsistentLiteral; gate_d2 = +inf: the ungated filter with records), plus
    d2 = every d2 it compared with the gate; consistent = False is gated_reference_run bit for bit (its margins are then not asserted:
    that run is only what the consistent one is told apart from)"""
    lit = ConsistentLiteral(gate=dict(gate_d2=gate_d2), consistent=consistent)
    res = _gated_run(lit, stream, batches)
    if consistent:
        lit.assert_margins()
    res["d2"] = list(lit.d2_seen)
    return res


def first_complete_batch(ref, batches):
    """index of the first batch that ends with the whole map built"""
    return next(k for k, (first, count) in enumerate(batches) if first + count - 1 >= ref["complete"])


@functools.lru_cache(maxsize=None)
def long_double_tail(stream, max_landmarks, cap, batches, gate_d2=None):
    """How far the double reference is from exact arithmetic: reference_step in long double, started from the literal state at the
    end of the first batch that holds the whole map and fed the same stream.  Returns {batch: (max |dmu|, Sigma relative)} for the
    batches behind that one.  (With gate_d2: the gated step against gated_reference_run.)"""
    ref = reference_run(stream, max_landmarks, cap, batches) if gate_d2 is None else gated_reference_run(stream, batches, gate_d2)
    k0 = first_complete_batch(ref, batches)
    index = {lid: k for k, lid in enumerate(ref["ids"][k0])}
    mu, S = (a.astype(LD) for a in ref["states"][k0])
    out = {}
    for k in range(k0 + 1, len(batches)):
        first, count = batches[k]
        for f in range(first, first + count):
            (wl, wr, dt), obs = stream[f]
            pops = sorted((index[o[0]], o[2], o[3]) for o in obs)          # distinct mapped ids pop in ascending index
            if gate_d2 is None:
                mu, S = reference_step(mu, S, wl, wr, dt, pops, dtype=LD)
            else:
                mu, S, _ = gated_reference_step(mu, S, wl, wr, dt, pops, gate_d2, dtype=LD)
        mu_r, S_r = ref["states"][k]
        out[k] = (float(np.abs(mu_r - mu).max()), rel_err(S_r, S))
    return out


@functools.lru_cache(maxsize=None)
def consistent_long_double_tail(stream, max_landmarks, cap, batches, gate_d2=None):
    """long_double_tail with consistent innovations: consistent_reference.consistent_step in long double, started from the consistent
    literal state at the end of the first batch that holds the whole map.  Returns {batch: (max |dmu|, Sigma relative)}"""
    ref = (consistent_reference_run(stream, max_landmarks, cap, batches) if gate_d2 is None else
           consistent_gated_reference_run(stream, batches, gate_d2))
    k0 = first_complete_batch(ref, batches)
    index = {lid: k for k, lid in enumerate(ref["ids"][k0])}
    mu, S = (a.astype(LD) for a in ref["states"][k0])
    out = {}
    for k in range(k0 + 1, len(batches)):
        first, count = batches[k]
        for f in range(first, first + count):
            (wl, wr, dt), obs = stream[f]
            pops = sorted((index[o[0]], o[2], o[3]) for o in obs)          # distinct mapped ids pop in ascending index
            mu, S, _ = consistent_step(mu, S, wl, wr, dt, pops, math.inf if gate_d2 is None else gate_d2, dtype=LD)
        mu_r, S_r = ref["states"][k]
        out[k] = (float(np.abs(mu_r - mu).max()), rel_err(S_r, S))
    return out


def asymmetry(S):
    """max |Sigma - Sigma^T| / max |Sigma|"""
    return float(np.abs(S - S.T).max() / np.abs(S).max())


def min_eig(S):
    """the smallest eigenvalue of (Sigma + Sigma^T) / 2"""
    return float(np.linalg.eigvalsh((S + S.T) / 2).min())
