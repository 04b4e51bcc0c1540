"""Dense long-double restatement of SLAM relocalization (include/aruco_slam_hip.h "SLAM relocalization"): the
yardstick of tests/test_slam_relocalize.py.  Steps 1-4 (candidates, hypotheses, consensus, status) are those of
tests/relocalize_reference.py with the filter's own mu as the map; the fusion, the covariance and the seat are written out here on
the full N x N matrix with Python loops and a cofactor inverse.  Shares no code with the library."""
import math

import numpy as np

from tests import relocalize_reference as ref

LD = np.longdouble
PI = LD(math.pi)                                 # the library's constant, not a better pi


def wrap(a):
    if a >= PI:
        a = a - 2 * PI
    if a < -PI:
        a = a + 2 * PI
    return a


def inv3(A):
    a, b, c, d, e, f, g, h, i = [A[r, k] for r in range(3) for k in range(3)]
    co = np.array([[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
                   [d * h - e * g, b * g - a * h, a * e - b * d]], dtype=LD)
    return co / (a * co[0, 0] + b * co[1, 0] + c * co[2, 0])


def mirrored(A):
    """the upper triangle of A, mirrored"""
    U = np.triu(A)
    return U + np.triu(A, 1).T


def relocalize(mu, Sigma, ids, obs, tol_xy=0.25, tol_th=0.2, min_inliers=2):
    """mu (N), Sigma (N x N), ids (L, in landmark order), obs = [(id, valid, z, Rdiag)] in list order ->
    dict(status, n_candidates, n_inliers, runner_up, best, pose, sigma, inliers; mu_new, Sigma_new: the state an apply != 0 leaves
    (the state itself when unsolved); strip: Sigma_lx' (N - 3 x 3) or None)"""
    mu = np.asarray(mu, float)
    Sigma = np.asarray(Sigma, float)
    N = mu.size
    assert Sigma.shape == (N, N) and (N - 3) % 3 == 0 and len(ids) == (N - 3) // 3
    xyth = mu[3:].reshape(-1, 3)
    out = ref.relocalize(ids, xyth, obs, tol_xy=tol_xy, tol_th=tol_th, min_inliers=min_inliers)      # steps 1-4, word for word
    out.update(pose=np.zeros(3), sigma=np.zeros((3, 3)), mu_new=mu.copy(), Sigma_new=Sigma.copy(), strip=None)
    if out["status"] != 0:
        return out
    index = {}
    for i, lid in enumerate(ids):
        index.setdefault(int(lid), i)
    S = Sigma.astype(LD)

    def parts(j):
        """supporter at list position j: landmark index, hypothesis, J, G, R"""
        lid, _, z, r = obs[j]
        i = index[int(lid)]
        lm = mu[3 + 3 * i: 6 + 3 * i].astype(LD)
        x, y, t = [LD(v) for v in z]
        th = wrap(lm[2] - t)
        c, s = np.cos(th), np.sin(th)
        h = np.array([lm[0] - (c * x - s * y), lm[1] - (s * x + c * y), th], dtype=LD)
        J = np.array([[-c, s, -(s * x + c * y)], [-s, -c, c * x - s * y], [0, 0, -1]], dtype=LD)
        G = np.array([[1, 0, s * x + c * y], [0, 1, -(c * x - s * y)], [0, 0, 1]], dtype=LD)
        return i, h, J, G, np.diag(np.asarray(r, float).astype(LD))

    m0 = parts(out["best"])[1]
    Lam, eta, sup = np.zeros((3, 3), LD), np.zeros(3, LD), []
    for j in out["inliers"]:                                     # ascending list position
        i, h, J, G, R = parts(j)
        P = mirrored(S[3 + 3 * i: 6 + 3 * i, 3 + 3 * i: 6 + 3 * i])
        Cm = J @ R @ J.T
        W = inv3(mirrored(Cm + G @ P @ G.T))
        d = h - m0
        d[2] = wrap(d[2])
        Lam += W
        eta += W @ d
        sup.append((i, W, G, Cm))
    Pm = inv3(Lam)
    m = m0 + Pm @ eta
    m[2] = wrap(m[2])
    B = np.zeros((3, N), LD)
    meas = np.zeros((3, 3), LD)
    for i, W, G, Cm in sup:
        A = Pm @ W
        B[:, 3 + 3 * i: 6 + 3 * i] += A @ G                        # an id sighted twice adds twice
        meas += A @ Cm @ A.T
    strip = S[3:, 3:] @ B[:, 3:].T                                 # Sigma_ll B^T
    Sxx = mirrored(meas + B[:, 3:] @ strip)
    mu_new, S_new = mu.astype(LD), S.copy()
    mu_new[:3] = m
    S_new[:3, :3] = Sxx
    S_new[3:, :3] = strip
    S_new[:3, 3:] = strip.T
    out.update(pose=m.astype(float), sigma=Sxx.astype(float), mu_new=mu_new.astype(float), Sigma_new=S_new.astype(float),
               strip=strip.astype(float))
    return out
