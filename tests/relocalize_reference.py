"""Plain numpy (f64) restatement of relocalization (include/aruco_slam_hip.h "relocalization"): the yardstick of
tests/test_relocalize.py.  Python loops, math.cos / math.sin and np.linalg.inv; shares no code with the library."""
import math

import numpy as np

ID_TABLE = 1024
MARKER_MAX = 128
PI = math.pi
DEFAULTS = dict(tol_xy=0.25, tol_th=0.2, min_inliers=2)


def wrap(a):
    """the library's single angle wrap (ArucoSlam::normAngle)"""
    if a >= PI:
        a -= 2 * PI
    if a < -PI:
        a += 2 * PI
    return a


def candidates(map_ids, map_xyth, obs):
    """obs: (id, valid, z, Rdiag) in list order -> [(list position, hypothesis (3), observation z, r)]"""
    index = {}
    for i, lid in enumerate(map_ids):
        index.setdefault(int(lid), i)
    out = []
    for j, (lid, valid, z, r) in enumerate(obs[:MARKER_MAX]):
        z, r = np.asarray(z, float), np.asarray(r, float)
        if not valid or not 0 <= int(lid) < ID_TABLE or int(lid) not in index:
            continue
        if not (np.all(np.isfinite(z)) and np.all(np.isfinite(r)) and np.all(r > 0)):
            continue
        lx, ly, lt = map_xyth[index[int(lid)]]
        th = wrap(lt - z[2])
        c, s = math.cos(th), math.sin(th)
        out.append((j, np.array([lx - (c * z[0] - s * z[1]), ly - (s * z[0] + c * z[1]), th]), z, r))
    return out


def distance(hk, hj):
    """(squared planar distance, |wrapped heading difference|) of two hypotheses"""
    return (hk[0] - hj[0]) ** 2 + (hk[1] - hj[1]) ** 2, abs(wrap(hk[2] - hj[2]))


def supports(hk, hj, tol_xy, tol_th):
    d2, dt = distance(hk, hj)
    return d2 <= tol_xy * tol_xy and dt <= tol_th


def margin(map_ids, map_xyth, obs, tol_xy=0.25, tol_th=0.2, **_):
    """how far the nearest pair of candidate hypotheses stays from a threshold: min over pairs of | d^2 - tol_xy^2 | and
    | |dtheta| - tol_th | (inf without a pair): a test asserts this before it compares discrete results"""
    cs = candidates(map_ids, map_xyth, obs)
    m = math.inf
    for a in range(len(cs)):
        for b in range(a + 1, len(cs)):
            d2, dt = distance(cs[a][1], cs[b][1])
            m = min(m, abs(d2 - tol_xy * tol_xy), abs(dt - tol_th))
    return m


def relocalize(map_ids, map_xyth, obs, tol_xy=0.25, tol_th=0.2, min_inliers=2):
    """-> dict(status, n_candidates, n_inliers, runner_up, best, pose (3), sigma (3 x 3), inliers = list positions fused)"""
    map_xyth = np.asarray(map_xyth, float).reshape(-1, 3)
    out = dict(status=1, n_candidates=0, n_inliers=0, runner_up=0, best=-1, pose=np.zeros(3), sigma=np.zeros((3, 3)), inliers=[])
    cs = candidates(map_ids, map_xyth, obs)
    if not cs:
        return out
    sup = [[supports(ck[1], cj[1], tol_xy, tol_th) for ck in cs] for cj in cs]      # sup[j][k]: k supports j
    counts = [sum(row) for row in sup]
    b = max(range(len(cs)), key=lambda j: (counts[j], -cs[j][0]))
    out.update(n_candidates=len(cs), n_inliers=counts[b], best=cs[b][0],
               runner_up=max([counts[j] for j in range(len(cs)) if not sup[b][j]], default=0))
    if counts[b] < min_inliers:
        out["status"] = 2
        return out
    m0 = cs[b][1]
    Lam, eta = np.zeros((3, 3)), np.zeros(3)
    for k in range(len(cs)):                                 # ascending list position
        if not sup[b][k]:
            continue
        _, h, z, r = cs[k]
        c, s = math.cos(h[2]), math.sin(h[2])
        J = np.array([[-c, s, -(s * z[0] + c * z[1])], [-s, -c, c * z[0] - s * z[1]], [0.0, 0.0, -1.0]])
        W = np.linalg.inv(J @ np.diag(r) @ J.T)
        d = h - m0
        d[2] = wrap(d[2])
        Lam += W
        eta += W @ d
        out["inliers"].append(cs[k][0])
    P = np.linalg.inv(Lam)
    m = m0 + P @ eta
    m[2] = wrap(m[2])
    out.update(status=0, pose=m, sigma=P)
    return out
