"""The innovation gate of the localization steps, restated literally in numpy (include/aruco_slam_hip.h).

GatedLocalizer is tests.test_localize.FrozenMapLocalizer with the gate between a correction's gain and its fusion: d2 = ze^T S^-1 ze,
the reference's logged test (aruco_slam.cpp:156), the skip, the list that leaves the rejected observations out, the slot's health
record and the filter's track record.  It also keeps every d2 and every norm it compared, so that a test can assert that none lies
close enough to its threshold for rounding to decide (assert_margins)."""
import math

import numpy as np

from oracle.ekf_literal import _Heap, norm_angle
from tests.test_localize import FrozenMapLocalizer

DEFAULTS = dict(gate_d2=16.266, min_attempted=2, min_accept_percent=50, lost_after=3)
TRACK_ZERO = dict(frames=0, accepted_total=0, rejected_total=0, bad_streak=0, lost=0)


class GatedLocalizer(FrozenMapLocalizer):
    def __init__(self, ids, xyth, pose, pose_sigma, gate=None, **kw):
        super().__init__(ids, xyth, pose, pose_sigma, **kw)
        self.gate = {**DEFAULTS, **(gate or {})}
        self.track = dict(TRACK_ZERO)
        self.health = None                              # the last step's slot record
        self.d2_seen, self.norms_seen = [], []          # everything compared with a threshold so far
        self.d2_step = []                               # the last step's d2, in pop order

    def seat(self, pose, pose_sigma):
        """aslam_fleet_set_pose / a solved relocalize with apply: pose, Sigma_xx, empty list, disarmed, track record cleared"""
        self.mu = np.asarray(pose, float).copy()
        self.P = np.asarray(pose_sigma, float).reshape(3, 3).copy()
        self.last = []
        self.is_init = False
        self.track = dict(TRACK_ZERO)

    def add_observations(self, obs):
        g = self.gate
        q = _Heap()
        for k, (lid, valid, z, r) in enumerate(obs):
            if valid and int(lid) in self.index:
                q.push(dict(id=int(lid), index=self.index[int(lid)], z=np.asarray(z, float), R=np.diag(r), det=k))
        x, y, th = self.mu                              # every correction's operands come from the frame-start pose
        s, c = math.sin(th), math.cos(th)
        self.log, nxt, nstat = [], [], 0
        h = dict(attempted=0, accepted=0, rejected=0, ref_flagged=0, nis_sum=0.0, d2_max=0.0, worst_id=-1)
        have_max = False
        self.d2_step = []
        while q.c:
            ob = q.pop()
            mx, my, mth = self.xyth[ob["index"]]
            last = next((l for l in self.last if l[0] == ob["id"]), None)
            if last is not None and np.linalg.norm(last[1] - ob["z"]) < 0.01:
                act = 2                                 # a no-op: neither attempted nor gated
                nstat += 1
                nxt.append((ob["id"], np.full(3, np.nan)))
            else:
                h["attempted"] += 1
                gdx, gdy = mx - x, my - y
                gdth = norm_angle(mth - th)
                ze = ob["z"] - np.array([gdx * c + gdy * s, -gdx * s + gdy * c, gdth])
                ze[2] = norm_angle(ze[2])
                H = np.array([[-c, -s, -gdx * s + gdy * c], [s, -c, -gdx * c - gdy * s], [0.0, 0.0, -1.0]])
                with np.errstate(all="ignore"):
                    try:
                        Si = np.linalg.inv(H @ self.P @ H.T + ob["R"])
                    except np.linalg.LinAlgError:
                        Si = np.full((3, 3), np.nan)
                    K = self.P @ H.T @ Si
                    d2 = float(ze @ Si @ ze)
                    n_ze, n_K = float(np.sqrt((ze * ze).sum())), float(np.sqrt((K * K).sum()))
                self.d2_step.append(d2)
                self.d2_seen.append(d2)
                self.norms_seen.append((n_ze, n_K))
                if n_ze >= 1.0 or n_K >= 10.0:          # aruco_slam.cpp:156
                    h["ref_flagged"] += 1
                if not math.isnan(d2) and (not have_max or d2 > h["d2_max"]):
                    have_max = True
                    h["d2_max"], h["worst_id"] = d2, ob["id"]
                if math.isfinite(g["gate_d2"]) and not (d2 <= g["gate_d2"]):
                    act = 3                             # rejected: pose, P and the list stay as they are
                    h["rejected"] += 1
                else:
                    act = 1
                    h["accepted"] += 1
                    h["nis_sum"] += d2
                    self.mu = self.mu + K @ ze
                    self.P = (np.eye(3) - K @ H) @ self.P
                    nxt.append((ob["id"], ob["z"].copy()))
            self.log.append((ob["id"], ob["index"], act))
        self.last = nxt
        self.stats = [len(obs), 0, h["accepted"], nstat]
        self.health = h
        t = self.track
        t["frames"] += 1
        t["accepted_total"] += h["accepted"]
        t["rejected_total"] += h["rejected"]
        if h["attempted"] >= g["min_attempted"]:
            bad = 100 * h["accepted"] < g["min_accept_percent"] * h["attempted"]
            t["bad_streak"] = t["bad_streak"] + 1 if bad else 0
        t["lost"] = int(t["bad_streak"] >= g["lost_after"])

    def assert_margins(self, rel=1e-6):
        """no d2 within `rel` (relative) of the gate, no norm within `rel` of the reference test's 1 and 10"""
        gd = self.gate["gate_d2"]
        if math.isfinite(gd):
            for d2 in self.d2_seen:
                assert math.isnan(d2) or abs(d2 - gd) > rel * gd, f"d2 {d2} too close to the gate {gd}"
        for n_ze, n_K in self.norms_seen:
            assert math.isnan(n_ze) or abs(n_ze - 1.0) > rel, f"|ze| {n_ze} too close to 1"
            assert math.isnan(n_K) or abs(n_K - 10.0) > rel * 10.0, f"|K| {n_K} too close to 10"


def check_slot_health(got, want, where, rtol=1e-9):
    """a SLOT_HEALTH_DTYPE record against a GatedLocalizer.health: counts and the id exact, the two sums to rtol"""
    for k in ("attempted", "accepted", "rejected", "ref_flagged", "worst_id"):
        assert int(got[k]) == want[k], f"{where}: {k} {int(got[k])} != {want[k]}"
    for k in ("nis_sum", "d2_max"):
        a, b = float(got[k]), want[k]
        assert (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= rtol * abs(b), f"{where}: {k} {a} != {b}"


def check_track(got, want, where):
    for k in TRACK_ZERO:
        assert int(got[k]) == want[k], f"{where}: {k} {int(got[k])} != {want[k]}"
