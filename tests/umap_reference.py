"""Localization on an uncertain map (Schmidt-Kalman steps; include/aruco_slam_hip.h), restated in numpy long double and
in a different formulation from the kernels.

UncertainMapLocalizer keeps the dense (3 + 3L)^2 covariance and the full 3 x (3 + 3L) Jacobian of every correction, forms the
reference's gain K = Sigma H^T S^-1 (aruco_slam.cpp:145-160) with its landmark rows zeroed and updates the whole dense covariance in
the Joseph form (I - K H) Sigma (I - K H)^T + K R K^T, which is the covariance of the estimate for ANY gain.  The kernels instead carry the 3 x (3 + 3L)
strip [Sigma_xx | Sigma_xl] and subtract K (H Sigma) from it.  Pop order, the "stationary" rule, the gate and the health records are
tests.gate_reference.GatedLocalizer's (a gate of +inf monitors only: the run is the ungated one)."""
import math

import numpy as np

from oracle.ekf_literal import _Heap, norm_angle
from tests.gate_reference import TRACK_ZERO, GatedLocalizer

LD = np.longdouble


def inv3(S):
    """3 x 3 inverse by the adjugate, in the precision of S; a singular S gives inf / NaN as the kernel's does"""
    a, b, c, d, e, f, g, h, i = S.reshape(-1)
    co = np.array([[e * i - f * h, c * h - b * i, b * f - c * e],
                   [f * g - d * i, a * i - c * g, c * d - a * f],
                   [d * h - e * g, b * g - a * h, a * e - b * d]], S.dtype)
    with np.errstate(all="ignore"):
        return co / (a * co[0, 0] + b * co[1, 0] + c * co[2, 0])


def sym_blocks(map_sigmas):
    s = np.asarray(map_sigmas, float).reshape(-1, 3, 3)
    return 0.5 * (s + s.transpose(0, 2, 1))


class UncertainMapLocalizer(GatedLocalizer):
    """mu_x (3) and the dense Sigma of [pose, map] with fixed block-diagonal Sigma_ll, in long double (or in `dtype`)"""

    def __init__(self, ids, xyth, map_sigmas, pose, pose_sigma, gate=None, cross=True, dtype=LD, **kw):
        self.dtype = LD = dtype                         # np.float64: the double form, to show that a case is well conditioned
        super().__init__(ids, xyth, pose, pose_sigma, gate if gate is not None else dict(gate_d2=math.inf), **kw)
        L = self.xyth.shape[0]
        self.L, self.N = L, 3 + 3 * L
        self.C = sym_blocks(map_sigmas)
        self.x = np.asarray(pose, LD).copy()
        self.S = np.zeros((self.N, self.N), LD)
        self.S[:3, :3] = np.asarray(pose_sigma, LD).reshape(3, 3)
        for i in range(L):
            self.S[3 + 3 * i:6 + 3 * i, 3 + 3 * i:6 + 3 * i] = self.C[i]
        self.cross_on = cross                           # False: the comparison filter that only inflates R by Hl C Hl^T

    # what the device comparisons read, in f64
    mu = property(lambda self: self.x.astype(float), lambda self, v: None)
    P = property(lambda self: self.S[:3, :3].astype(float), lambda self, v: None)
    cross = property(lambda self: self.S[:3, 3:].astype(float))

    def full_sigma(self):
        return self.S.astype(float)

    def seat(self, pose, pose_sigma):
        """a seat of the pose drops its correlation with the map"""
        LD = self.dtype
        self.x = np.asarray(pose, LD).copy()
        self.S[:3, :3] = np.asarray(pose_sigma, LD).reshape(3, 3)
        self.S[:3, 3:] = 0
        self.S[3:, :3] = 0
        self.last = []
        self.is_init = False
        self.track = dict(TRACK_ZERO)

    def predict(self, wl, wr, dt):
        LD = self.dtype
        wl, wr, dt = LD(wl), LD(wr), LD(dt)
        kl, kr, b, Qk = LD(self.kl), LD(self.kr), LD(self.b), LD(self.Q_k)
        delta_sl, delta_sr = kl * (dt * wl), kr * (dt * wr)
        delta_theta = (delta_sr - delta_sl) / (2 * b)
        delta_s = LD(0.5) * (delta_sr + delta_sl)
        tmp = self.x[2] + LD(0.5) * delta_theta
        c, s = np.cos(tmp), np.sin(tmp)
        self.x[0] += delta_s * c
        self.x[1] += delta_s * s
        self.x[2] = norm_angle(self.x[2] + delta_theta)
        f02, f12 = -delta_s * s, delta_s * c             # F = blockdiag(D, I), D = I but for (0,2) and (1,2)
        wkh = (LD(0.5) * kl * dt) * np.array([[c, c], [s, s], [1 / b, -1 / b]], LD)
        Q = wkh @ np.diag(np.array([Qk * abs(wl), Qk * abs(wr)], LD)) @ wkh.T
        S = self.S                                      # F Sigma F^T on the dense matrix: rows, then columns
        S[0, :] += f02 * S[2, :]
        S[1, :] += f12 * S[2, :]
        S[:, 0] += f02 * S[:, 2]
        S[:, 1] += f12 * S[:, 2]
        S[:3, :3] += Q

    def add_observations(self, obs):
        LD = self.dtype
        g = self.gate
        q = _Heap()
        for k, (lid, valid, z, r) in enumerate(obs):
            if valid and int(lid) in self.index:
                q.push(dict(id=int(lid), index=self.index[int(lid)], z=np.asarray(z, float), R=np.asarray(r, float), det=k))
        x, y, th = self.x                               # every correction's operands come from the frame-start pose
        s, c = np.sin(th), np.cos(th)
        self.log, nxt, nstat = [], [], 0
        h = dict(attempted=0, accepted=0, rejected=0, ref_flagged=0, nis_sum=0.0, d2_max=0.0, worst_id=-1)
        have_max = False
        self.d2_step = []
        while q.c:
            ob = q.pop()
            li = ob["index"]
            mx, my, mth = (LD(v) for v in self.xyth[li])
            last = next((l for l in self.last if l[0] == ob["id"]), None)
            if last is not None and np.linalg.norm(last[1] - ob["z"]) < 0.01:
                act = 2
                nstat += 1
                nxt.append((ob["id"], np.full(3, np.nan)))
            else:
                h["attempted"] += 1
                gdx, gdy = mx - x, my - y
                gdth = norm_angle(mth - th)
                z = ob["z"].astype(LD)
                ze = z - np.array([gdx * c + gdy * s, -gdx * s + gdy * c, gdth], LD)
                ze[2] = norm_angle(ze[2])
                H = np.zeros((3, self.N), LD)
                H[:, :3] = np.array([[-c, -s, -gdx * s + gdy * c], [s, -c, -gdx * c - gdy * s], [0, 0, -1]], LD)
                Hl = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], LD)
                R = np.diag(ob["R"].astype(LD))
                if self.cross_on:
                    H[:, 3 + 3 * li:6 + 3 * li] = Hl
                else:
                    R = R + Hl @ self.C[li].astype(LD) @ Hl.T
                # (products with H, K and their transposes skip the columns of H and the rows of K that are zero: cost, not form)
                nz = np.r_[0:3, 3 + 3 * li:6 + 3 * li] if self.cross_on else np.r_[0:3]
                Hn = H[:, nz]
                with np.errstate(all="ignore"):
                    Si = inv3(Hn @ self.S[np.ix_(nz, nz)] @ Hn.T + R)
                    K = np.zeros((self.N, 3), LD)
                    K[:3] = (self.S[:3][:, nz] @ Hn.T) @ Si     # Sigma H^T S^-1 with the landmark rows zeroed: the landmarks are
                                                                # considered, not estimated
                    d2 = float(ze @ Si @ ze)
                    n_ze, n_K = float(np.sqrt((ze * ze).sum())), float(np.sqrt((K * K).sum()))
                self.d2_step.append(d2)
                self.d2_seen.append(d2)
                self.norms_seen.append((n_ze, n_K))
                if n_ze >= 1.0 or n_K >= 10.0:
                    h["ref_flagged"] += 1
                if not math.isnan(d2) and (not have_max or d2 > h["d2_max"]):
                    have_max = True
                    h["d2_max"], h["worst_id"] = d2, ob["id"]
                if math.isfinite(g["gate_d2"]) and not (d2 <= g["gate_d2"]):
                    act = 3
                    h["rejected"] += 1
                else:
                    act = 1
                    h["accepted"] += 1
                    h["nis_sum"] += d2
                    with np.errstate(all="ignore"):
                        self.x = self.x + (K @ ze)[:3]
                        S = self.S
                        S[:3, :] -= K[:3] @ (Hn @ S[nz, :])                  # (I - K H) Sigma
                        S[:, :3] -= (S[:, nz] @ Hn.T) @ K[:3].T              # ... (I - K H)^T
                        S[:3, :3] += K[:3] @ R @ K[:3].T                     # ... + K R K^T
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
