"""The innovation gate of the SLAM chains, restated sequentially (include/aruco_slam_hip.h); a plain helper module.

gated_reference_step is ekf_reference.reference_step, the same long-double sequential step, with d2 = ze^T Sk^-1 ze formed from its
own Sk and ze between a correction's gain and its fusion, the skip on rejection (the reference's commented-out `continue`,
aruco_slam.cpp:156-175) and the slot's health counts.  GatedLiteralSlam is the literal transcription (oracle/ekf_literal.py) on
injected observations with the same gate, for sequences: augments, the "stationary" test, the last-observed list without the
rejected observations, the track record.  Both keep every d2 and every ||ze|| they compared, so that a test can assert that none
lies close enough to its threshold for rounding to decide (assert_margins) before it compares anything discrete."""
import math

import numpy as np

from ekf_reference import LD, _inv3, wrap_once
from oracle.ekf_literal import LiteralSlam, _Heap, norm_angle

DEFAULTS = dict(gate_d2=16.266, min_attempted=2, min_accept_percent=50, lost_after=3)
TRACK_ZERO = dict(frames=0, accepted_total=0, rejected_total=0, bad_streak=0, lost=0)
OUTLIER = np.array([2.7, -2.1, 0.0])                # what a planted outlier adds to a true sighting


def rejects(gate_d2, d2):
    return math.isfinite(gate_d2) and not (d2 <= gate_d2)          # a NaN d2 rejects


def new_health():
    return dict(attempted=0, accepted=0, rejected=0, ref_flagged=0, nis_sum=0.0, d2_max=0.0, worst_id=-1, have_max=False)


def note_correction(h, d2, n_ze, rejected, marker_id):
    """one attempted correction into the slot record h (pop order)"""
    h["attempted"] += 1
    if n_ze >= 1.0:                                               # the ||ze|| half of aruco_slam.cpp:156; the chains never form K
        h["ref_flagged"] += 1
    if not math.isnan(d2) and (not h["have_max"] or d2 > h["d2_max"]):
        h["have_max"] = True
        h["d2_max"], h["worst_id"] = d2, int(marker_id)
    if rejected:
        h["rejected"] += 1
    else:
        h["accepted"] += 1
        h["nis_sum"] += d2


def advance_track(t, h, gate):
    """§19's integer streak rule"""
    t["frames"] += 1
    t["accepted_total"] += h["accepted"]
    t["rejected_total"] += h["rejected"]
    if h["attempted"] >= gate["min_attempted"]:
        bad = 100 * h["accepted"] < gate["min_accept_percent"] * h["attempted"]
        t["bad_streak"] = t["bad_streak"] + 1 if bad else 0
    t["lost"] = int(t["bad_streak"] >= gate["lost_after"])


def assert_margins(gate_d2, d2s, norms, rel=1e-6):
    """no d2 within `rel` (relative) of the gate, no ||ze|| within `rel` of 1: conditions on the inputs, not tolerances"""
    if math.isfinite(gate_d2):
        for d2 in d2s:
            assert math.isnan(d2) or abs(d2 - gate_d2) > rel * gate_d2, f"d2 {d2} too close to the gate {gate_d2}"
    for n in norms:
        assert math.isnan(n) or abs(n - 1.0) > rel, f"|ze| {n} too close to 1"


def gated_reference_step(mu, S, wl, wr, dt, obs, gate_d2, ids=None, kl=0.05, kr=0.05, b=0.09, Qk=0.01, dtype=LD):
    """predict, then the corrections obs = [(index, z(3), Rdiag(3))] in pop order under the gate; returns (mu, Sigma, info) with
    info = dict(d2=[...], rejected=[...], norms=[...], health={...}); ids[index] = the landmark's marker id (worst_id)"""
    mu = np.array(mu, dtype=dtype); S = np.array(S, dtype=dtype)
    wl, wr, dt = dtype(wl), dtype(wr), dtype(dt)
    dsl, dsr = dtype(kl) * (dt * wl), dtype(kr) * (dt * wr)
    dth = (dsr - dsl) / (2 * dtype(b)); ds = (dsr + dsl) / 2
    th = mu[2] + dth / 2
    c, s = np.cos(th), np.sin(th)
    mu[0] += ds * c; mu[1] += ds * s; mu[2] = wrap_once(mu[2] + dth)
    H = np.array([[1, 0, -ds * s], [0, 1, ds * c], [0, 0, 1]], dtype=dtype)
    f = dtype(kl) * dt / 2
    wkh = np.array([[f * c, f * c], [f * s, f * s], [f / dtype(b), -f / dtype(b)]], dtype=dtype)
    Q = wkh @ np.diag(np.array([dtype(Qk) * abs(wl), dtype(Qk) * abs(wr)], dtype=dtype)) @ wkh.T
    S[:3, :] = H @ S[:3, :]
    S[:, :3] = S[:, :3] @ H.T
    S[:3, :3] += Q
    mu0 = mu.copy()                                           # every correction is linearised at the pre-frame mean (Q1)
    st, ct = np.sin(mu0[2]), np.cos(mu0[2])
    h = new_health()
    info = dict(d2=[], rejected=[], norms=[], health=h)
    for idx, z, Rd in obs:
        li = 3 + 3 * idx
        dx, dy = mu0[li] - mu0[0], mu0[li + 1] - mu0[1]
        zh = np.array([dx * ct + dy * st, -dx * st + dy * ct, wrap_once(mu0[li + 2] - mu0[2])], dtype=dtype)
        ze = np.array(z, dtype=dtype) - zh
        ze[2] = wrap_once(ze[2])
        G = np.array([[-ct, -st, -dx * st + dy * ct, ct, st, 0], [st, -ct, -dx * ct - dy * st, -st, ct, 0], [0, 0, -1, 0, 0, 1]],
                     dtype=dtype)
        cols = [0, 1, 2, li, li + 1, li + 2]
        GS = G @ S[cols, :]                                    # Gx * sigma_   (3 x N)
        Sk = GS[:, cols] @ G.T + np.diag(np.array(Rd, dtype=dtype))
        Si = _inv3(Sk) if dtype is LD else np.linalg.inv(Sk)
        d2 = float(ze @ Si @ ze)
        n_ze = float(np.sqrt((ze * ze).sum()))
        rej = rejects(gate_d2, d2)
        info["d2"].append(d2); info["rejected"].append(rej); info["norms"].append(n_ze)
        note_correction(h, d2, n_ze, rej, idx if ids is None else ids[idx])
        if rej:
            continue                                           # the reference's commented-out `continue`: mu and Sigma stay
        K = (S[:, cols] @ G.T) @ Si                            # sigma_ * Gx^T * S^-1
        mu += K @ ze
        if dtype is LD:
            for r in range(3):                                 # S -= K GS as three outer products (no long double BLAS)
                S -= np.outer(K[:, r], GS[r])
        else:
            S -= K @ GS
    return mu, S, info


class GatedLiteralSlam(LiteralSlam):
    """LiteralSlam on ready observations (add_frame) with the SLAM gate: d2 from the literal Gx sigma Gx^T + Rk, the skip, the
    last-observed list without the rejected observations, the slot record (health) and the track record (track)"""

    def __init__(self, gate=None, **kw):
        super().__init__(**kw)
        self.gate = {**DEFAULTS, **(gate or {})}
        self.track = dict(TRACK_ZERO)
        self.health = None
        self.stats = None
        self.d2_seen, self.norms_seen = [], []

    def seat(self, mu, sigma, ids):
        """aslam_set_state: state and id map replaced, the last-observed list emptied, the track record cleared"""
        self.mu, self.sigma = np.array(mu, float), np.array(sigma, float)
        self.id_map = {int(i): k for k, i in enumerate(ids)}
        self.last_observed = []
        self.track = dict(TRACK_ZERO)

    def add_frame(self, obs):
        """obs = [(id, z(3), Rdiag(3))] in detection order"""
        q = _Heap()
        for lid, z, r in obs:
            q.push(dict(id=int(lid), index=self.id_map.get(int(lid), -1), z=np.asarray(z, float), R=np.diag(r), last=np.full(3, np.nan)))
        mu = self.mu.copy()
        observed, self.log = [], []
        self.health = new_health()
        n_aug = n_stat = 0
        while q.c:
            ob = q.pop()
            action = self.correct(ob, mu) if ob["index"] >= 0 else self.augment(ob, mu)
            n_aug += action == 0
            n_stat += action == 2
            if action != 3:
                observed.append(ob)                               # a rejected observation leaves the list
            self.log.append((ob["id"], ob["index"], action))
        self.last_observed = observed
        self.stats = [len(obs), int(n_aug), self.health["accepted"], int(n_stat)]
        advance_track(self.track, self.health, self.gate)

    def correct(self, ob, mu):
        Rk = ob["R"]
        N = self.mu.size
        i3 = 3 + 3 * ob["index"]
        F = np.zeros((6, N)); F[:3, :3] = np.eye(3); F[3:, i3:i3 + 3] = np.eye(3)
        mx, my, mth = mu[i3], mu[i3 + 1], mu[i3 + 2]
        x, y, th = mu[0], mu[1], mu[2]
        s, c = math.sin(th), math.cos(th)
        gdx, gdy = mx - x, my - y
        gdth = norm_angle(mth - th)
        z = ob["z"].copy()
        ze = z - np.array([gdx * c + gdy * s, -gdx * s + gdy * c, gdth])
        ze[2] = norm_angle(ze[2])
        Gxm = np.array([[-c, -s, -gdx * s + gdy * c, c, s, 0], [s, -c, -gdx * c - gdy * s, -s, c, 0], [0, 0, -1, 0, 0, 1]], float)
        Gx = Gxm @ F
        last = next((o for o in self.last_observed if o["id"] == ob["id"]), None)
        if last is not None and np.linalg.norm(last["last"] - z) < 0.01:
            return 2                                              # a no-op: neither attempted nor gated
        with np.errstate(all="ignore"):
            Si = np.linalg.inv(Gx @ self.sigma @ Gx.T + Rk)
            d2 = float(ze @ Si @ ze)
            n_ze = float(np.sqrt((ze * ze).sum()))
        rej = rejects(self.gate["gate_d2"], d2)
        self.d2_seen.append(d2); self.norms_seen.append(n_ze)
        note_correction(self.health, d2, n_ze, rej, ob["id"])
        if rej:
            return 3
        ob["last"] = z
        Kg = self.sigma @ Gx.T @ Si
        self.mu = self.mu + Kg @ ze
        self.sigma = (np.eye(N) - Kg @ Gx) @ self.sigma
        return 1

    def assert_margins(self, rel=1e-6):
        assert_margins(self.gate["gate_d2"], self.d2_seen, self.norms_seen, rel)


def check_slot_health(got, want, where, rtol=1e-9):
    """a SLOT_HEALTH_DTYPE record against a reference record: counts and the id exact, the two sums to rtol"""
    for k in ("attempted", "accepted", "rejected", "ref_flagged", "worst_id"):
        assert int(got[k]) == want[k], f"{where}: {k} {int(got[k])} != {want[k]}"
    for k in ("nis_sum", "d2_max"):
        a, b = float(got[k]), float(want[k])
        assert a == b or abs(a - b) <= rtol * abs(b), f"{where}: {k} {a} != {b}"


def check_track(got, want, where):
    for k in TRACK_ZERO:
        assert int(got[k]) == want[k], f"{where}: {k} {int(got[k])} != {want[k]}"
