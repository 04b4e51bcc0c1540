"""Consistent innovations (aslam_set_consistent_innovations, include/aruco_slam_hip.h), restated sequentially; a plain
helper module.

consistent_step is slam_gate_reference.gated_reference_step (and, with the gate at +inf, ekf_reference.reference_step): the same
long-double sequential step, every correction's ze and Jacobian formed at the frame's predicted mean mu_0 as the reference forms them,
with the one change the switch makes,
    e_i = ze_i - H_i (mu_{i-1} - mu_0)          mu_i = mu_{i-1} + K_i e_i
a plain difference with no angle wrap.  d2, the verdict, nis_sum, d2_max and worst_id are formed from e_i; ref_flagged stays the
reference's logged test on ze_i.  joint_mean is the other formulation of the same mean, mu_0 + Sigma_0 H^T (H Sigma_0 H^T +
blockdiag R)^-1 ze in one solve.  ConsistentLocalizer and ConsistentUmapLocalizer are gate_reference.GatedLocalizer and
umap_reference.UncertainMapLocalizer with the same change (on an uncertain map only the pose columns of H enter: the landmarks are not
estimated).  ConsistentLiteral is the literal transcription on ready observations (slam_gate_reference.GatedLiteralSlam: double, dense
literal products, augments, the "stationary" test, the gate, the records) with e_i in place of ze_i, the one literal that builds a map
with the switch on; ConsistentPlanReference is plan_reference.PlanReference (landmark cap, cap on fused corrections, pop order) on it.
Everything compared with a threshold is kept, so that a test can assert that no decision hangs on rounding."""
import math

import numpy as np

from ekf_reference import LD, _inv3, wrap_once
from oracle.ekf_literal import _Heap, norm_angle
from plan_reference import PlanReference
from slam_gate_reference import GatedLiteralSlam, new_health, note_correction, rejects
from tests.gate_reference import GatedLocalizer
from tests.umap_reference import UncertainMapLocalizer, inv3


def _predict(mu, S, wl, wr, dt, kl, kr, b, Qk, dtype):
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


def _linearise(mu0, idx, z, dtype):
    """the reference's ze and Gxm of one sighting at the frozen mean mu0 (aruco_slam.cpp:116-143)"""
    st, ct = np.sin(mu0[2]), np.cos(mu0[2])
    li = 3 + 3 * idx
    dx, dy = mu0[li] - mu0[0], mu0[li + 1] - mu0[1]
    zh = np.array([dx * ct + dy * st, -dx * st + dy * ct, wrap_once(mu0[li + 2] - mu0[2])], dtype=dtype)
    ze = np.array(z, dtype=dtype) - zh
    ze[2] = wrap_once(ze[2])
    G = np.array([[-ct, -st, -dx * st + dy * ct, ct, st, 0], [st, -ct, -dx * ct - dy * st, -st, ct, 0], [0, 0, -1, 0, 0, 1]], dtype=dtype)
    return ze, G, [0, 1, 2, li, li + 1, li + 2]


def consistent_step(mu, S, wl, wr, dt, obs, gate_d2=math.inf, ids=None, consistent=True, predict=True, kl=0.05, kr=0.05, b=0.09, Qk=0.01,
                    dtype=LD):
    """predict, then the corrections obs = [(index, z(3), Rdiag(3))] in pop order, each from the mean the previous one left, under the
    gate (+inf: none).  consistent = False is gated_reference_step.  Returns (mu, Sigma, info); info = dict(d2, rejected, norms (||ze||),
    health, mu0 (the predicted mean), S0 (the predicted covariance))"""
    mu = np.array(mu, dtype=dtype); S = np.array(S, dtype=dtype)
    if predict:
        _predict(mu, S, wl, wr, dt, kl, kr, b, Qk, dtype)
    mu0 = mu.copy()
    h = new_health()
    info = dict(d2=[], rejected=[], norms=[], health=h, mu0=mu0, S0=S.copy())
    for idx, z, Rd in obs:
        ze, G, cols = _linearise(mu0, idx, z, dtype)
        e = ze - G @ (mu[cols] - mu0[cols]) if consistent else ze       # plain difference, no wrap
        GS = G @ S[cols, :]
        Sk = GS[:, cols] @ G.T + np.diag(np.array(Rd, dtype=dtype))
        Si = _inv3(Sk) if dtype is LD else np.linalg.inv(Sk)
        d2 = float(e @ Si @ e)
        n_ze = float(np.sqrt((ze * ze).sum()))
        rej = rejects(gate_d2, d2)
        info["d2"].append(d2); info["rejected"].append(rej); info["norms"].append(n_ze)
        note_correction(h, d2, n_ze, rej, idx if ids is None else ids[idx])
        if rej:
            continue
        K = (S[:, cols] @ G.T) @ Si
        mu += K @ e
        if dtype is LD:
            for r in range(3):
                S -= np.outer(K[:, r], GS[r])
        else:
            S -= K @ GS
    return mu, S, info


def _solve(A, b):
    """A x = b by Gaussian elimination with partial pivoting, in the precision of A (np.linalg does not take long double)"""
    A = A.copy(); x = b.copy()
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]; x[[k, p]] = x[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= np.outer(f, A[k, k:])
        x[k + 1:] -= f * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def joint_mean(mu0, S0, obs, dtype=LD):
    """mu_0 + Sigma_0 H^T (H Sigma_0 H^T + blockdiag R)^-1 ze over obs, every row of H and ze formed at mu_0"""
    mu0 = np.array(mu0, dtype=dtype); S0 = np.array(S0, dtype=dtype)
    N, m = mu0.size, len(obs)
    H = np.zeros((3 * m, N), dtype); ze = np.zeros(3 * m, dtype); R = np.zeros(3 * m, dtype)
    for k, (idx, z, Rd) in enumerate(obs):
        e, G, cols = _linearise(mu0, idx, z, dtype)
        H[3 * k:3 * k + 3, cols] = G
        ze[3 * k:3 * k + 3] = e
        R[3 * k:3 * k + 3] = np.array(Rd, dtype)
    SH = S0 @ H.T
    return mu0 + SH @ _solve(H @ SH + np.diag(R), ze)


class ConsistentLocalizer(GatedLocalizer):
    """GatedLocalizer with every correction formed at the running pose: e = ze - H (mu - mu_0); a gate of +inf is the ungated filter"""

    def __init__(self, ids, xyth, pose, pose_sigma, gate=None, **kw):
        super().__init__(ids, xyth, pose, pose_sigma, gate if gate is not None else dict(gate_d2=math.inf), **kw)

    def add_observations(self, obs):
        g = self.gate
        q = _Heap()
        for k, (lid, valid, z, r) in enumerate(obs):
            if valid and int(lid) in self.index:
                q.push(dict(id=int(lid), index=self.index[int(lid)], z=np.asarray(z, float), R=np.diag(r), det=k))
        mu0 = self.mu.copy()                            # every correction's operands come from the frame-start pose
        x, y, th = mu0
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
                act = 2
                nstat += 1
                nxt.append((ob["id"], np.full(3, np.nan)))
            else:
                h["attempted"] += 1
                gdx, gdy = mx - x, my - y
                gdth = norm_angle(mth - th)
                ze = ob["z"] - np.array([gdx * c + gdy * s, -gdx * s + gdy * c, gdth])
                ze[2] = norm_angle(ze[2])
                H = np.array([[-c, -s, -gdx * s + gdy * c], [s, -c, -gdx * c - gdy * s], [0.0, 0.0, -1.0]])
                e = ze - H @ (self.mu - mu0)            # plain difference, no wrap
                with np.errstate(all="ignore"):
                    try:
                        Si = np.linalg.inv(H @ self.P @ H.T + ob["R"])
                    except np.linalg.LinAlgError:
                        Si = np.full((3, 3), np.nan)
                    K = self.P @ H.T @ Si
                    d2 = float(e @ Si @ e)
                    n_ze, n_K = float(np.sqrt((ze * ze).sum())), float(np.sqrt((K * K).sum()))
                self.d2_step.append(d2)
                self.d2_seen.append(d2)
                self.norms_seen.append((n_ze, n_K))
                if n_ze >= 1.0 or n_K >= 10.0:          # aruco_slam.cpp:156, on ze: what the reference would have logged
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
                    self.mu = self.mu + K @ e
                    self.P = (np.eye(3) - K @ H) @ self.P
                    nxt.append((ob["id"], ob["z"].copy()))
            self.log.append((ob["id"], ob["index"], act))
        self.last = nxt
        self.stats = [len(obs), 0, h["accepted"], nstat]
        self.health = h
        _advance(self.track, h, g)


def _advance(t, h, g):
    t["frames"] += 1
    t["accepted_total"] += h["accepted"]
    t["rejected_total"] += h["rejected"]
    if h["attempted"] >= g["min_attempted"]:
        bad = 100 * h["accepted"] < g["min_accept_percent"] * h["attempted"]
        t["bad_streak"] = t["bad_streak"] + 1 if bad else 0
    t["lost"] = int(t["bad_streak"] >= g["lost_after"])


class ConsistentUmapLocalizer(UncertainMapLocalizer):
    """UncertainMapLocalizer with e = ze - Hx (x - x_0): the landmarks are considered, not estimated, so only the pose columns enter"""

    def add_observations(self, obs):
        LD = self.dtype
        g = self.gate
        q = _Heap()
        for k, (lid, valid, z, r) in enumerate(obs):
            if valid and int(lid) in self.index:
                q.push(dict(id=int(lid), index=self.index[int(lid)], z=np.asarray(z, float), R=np.asarray(r, float), det=k))
        x0 = self.x.copy()
        x, y, th = x0
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
                ze = ob["z"].astype(LD) - np.array([gdx * c + gdy * s, -gdx * s + gdy * c, gdth], LD)
                ze[2] = norm_angle(ze[2])
                Hx = np.array([[-c, -s, -gdx * s + gdy * c], [s, -c, -gdx * c - gdy * s], [0, 0, -1]], LD)
                Hl = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], LD)
                e = ze - Hx @ (self.x - x0)             # plain difference, no wrap
                R = np.diag(ob["R"].astype(LD))
                nz = np.r_[0:3, 3 + 3 * li:6 + 3 * li]
                Hn = np.concatenate([Hx, Hl], 1)
                with np.errstate(all="ignore"):
                    Si = inv3(Hn @ self.S[np.ix_(nz, nz)] @ Hn.T + R)
                    Kx = (self.S[:3][:, nz] @ Hn.T) @ Si
                    d2 = float(e @ Si @ e)
                    n_ze, n_K = float(np.sqrt((ze * ze).sum())), float(np.sqrt((Kx * Kx).sum()))
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
                        self.x = self.x + Kx @ e
                        S = self.S
                        S[:3, :] -= Kx @ (Hn @ S[nz, :])
                        S[:, :3] -= (S[:, nz] @ Hn.T) @ Kx.T
                        S[:3, :3] += Kx @ R @ Kx.T
                    nxt.append((ob["id"], ob["z"].copy()))
            self.log.append((ob["id"], ob["index"], act))
        self.last = nxt
        self.stats = [len(obs), 0, h["accepted"], nstat]
        self.health = h
        _advance(self.track, h, g)


class ConsistentLiteral(GatedLiteralSlam):
    """GatedLiteralSlam with every correction formed at the running mean: e = ze - Gx (mu - mu_0), mu_0 = the mean at the start of the
    frame (the `mu` both drivers hand to correct).  d2, the verdict, nis_sum, d2_max and worst_id are formed from e; ref_flagged stays
    the reference's logged test on ||ze||; a rejected sighting leaves the last-observed list and moves nothing.  No gate (or +inf) is
    the ungated filter with records; consistent = False is GatedLiteralSlam itself"""

    def __init__(self, gate=None, consistent=True, **kw):
        super().__init__(gate=gate if gate is not None else dict(gate_d2=math.inf), **kw)
        self.consistent = consistent

    def add_frame(self, obs):
        """obs = [(id, z, Rdiag)] or [(id, valid, z, Rdiag)] in detection order"""
        super().add_frame([(o[0], o[2], o[3]) for o in obs if o[1]] if obs and len(obs[0]) == 4 else obs)

    def correct(self, ob, mu):
        if not self.consistent:
            return super().correct(ob, mu)
        N = self.mu.size
        i3 = 3 + 3 * ob["index"]
        F = np.zeros((6, N)); F[:3, :3] = np.eye(3); F[3:, i3:i3 + 3] = np.eye(3)
        x, y, th = mu[0], mu[1], mu[2]
        s, c = math.sin(th), math.cos(th)
        gdx, gdy = mu[i3] - x, mu[i3 + 1] - y
        gdth = norm_angle(mu[i3 + 2] - th)
        z = ob["z"].copy()
        ze = z - np.array([gdx * c + gdy * s, -gdx * s + gdy * c, gdth])
        ze[2] = norm_angle(ze[2])
        Gx = np.array([[-c, -s, -gdx * s + gdy * c, c, s, 0], [s, -c, -gdx * c - gdy * s, -s, c, 0], [0, 0, -1, 0, 0, 1]], float) @ F
        last = next((o for o in self.last_observed if o["id"] == ob["id"]), None)
        if last is not None and np.linalg.norm(last["last"] - z) < 0.01:
            return 2                                              # a no-op: neither attempted nor gated
        n0 = mu.size                                              # landmarks appended in this frame were not in mu_0: they have not moved
        d = self.mu.copy(); d[:n0] -= mu; d[n0:] = 0.0
        e = ze - Gx @ d                                           # plain difference, no wrap
        with np.errstate(all="ignore"):
            Si = np.linalg.inv(Gx @ self.sigma @ Gx.T + ob["R"])
            d2 = float(e @ Si @ e)
            n_ze = float(np.sqrt((ze * ze).sum()))
        rej = rejects(self.gate["gate_d2"], d2)
        self.d2_seen.append(d2); self.norms_seen.append(n_ze)
        note_correction(self.health, d2, n_ze, rej, ob["id"])
        if rej:
            return 3
        ob["last"] = z
        Kg = self.sigma @ Gx.T @ Si
        self.mu = self.mu + Kg @ e
        self.sigma = (np.eye(N) - Kg @ Gx) @ self.sigma
        return 1


class ConsistentPlanReference(PlanReference):
    """PlanReference with ConsistentLiteral's correct behind its plan: frame() hands every correction the mean at the start of the
    frame, which is mu_0.  No gate: the records are kept and not read"""

    def __init__(self, mu, S, ids, max_landmarks, cap, last=(), consistent=True):
        super().__init__(mu, S, ids, max_landmarks, cap, last)
        plain, self.lit = self.lit, ConsistentLiteral(consistent=consistent)
        self.lit.mu, self.lit.sigma = plain.mu, plain.sigma
        self.lit.is_init, self.lit.last_time = plain.is_init, plain.last_time

    def frame(self, obs, *a, **kw):
        self.lit.health = new_health()
        return super().frame(obs, *a, **kw)
