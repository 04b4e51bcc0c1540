"""What k_pose_cov computes, restated in numpy long double on top of tests/pose_reference.py: the Jacobian J of the
projection by the complex step, N = J^T J, the observation Jacobian G by the complex step of the observation formula, the covariance
sigma2 M G N^-1 G^T M^T by long-double elimination, the rule that turns it into R, flags and valid, and the slot sums.  Every function
takes a batch: the leading axis is markers."""
import numpy as np

import pose_reference as pr

LD, CLD = pr.LD, pr.CLD
DEFAULTS = dict(sigma_px=0.5, scale=1.0, floor_xy=1e-6, floor_th=1e-6, gate_norm=1.0, use_residual=1)


def solve_ld(A, B):
    """A X = B for one system, Gaussian elimination with partial pivoting in long double (numpy has no long-double solver)"""
    A, B = np.array(A, dtype=LD), np.array(B, dtype=LD)
    n = A.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]] = A[[p, c]]
            B[[c, p]] = B[[p, c]]
        for r in range(c + 1, n):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            B[r] -= f * B[c]
    X = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - A[i, i + 1:] @ X[i + 1:]) / A[i, i]
    return X


def observation_jacobian(rvec, tvec):
    """G (n, 3, 6): d (t_z, -t_x, atan2(-R02, R22)) / d (r, t) in the camera's frame, by the complex step.  atan2 is not analytic in
    numpy's complex arithmetic: with a = -R02 and b = R22 the heading's imaginary part is (b Im a - a Im b) / (a^2 + b^2)"""
    p = np.concatenate([np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD)], -1).astype(CLD)
    cols = []
    for j in range(6):
        q = p.copy()
        q[..., j] += 1j * pr.STEP
        R = pr.rodrigues(q[..., :3])
        a, b = -R[..., 0, 2], R[..., 2, 2]
        th = (b.real * a.imag - a.real * b.imag) / (a.real * a.real + b.real * b.real)
        cols.append(np.stack([q[..., 5].imag, -q[..., 3].imag, th], -1) / pr.STEP)
    return np.stack(cols, -1)


def mount_matrix(mount):
    psi = LD(float(mount[2]))
    c, s = np.cos(psi), np.sin(psi)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=LD)


def covariance(rvec, tvec, corners, K, D, L, mount=(0.0, 0.0, 0.0), sigma_px=0.5, use_residual=1, **_):
    """(cov (n, 3, 3), sigma2 (n), e2 (n), N (n, 6, 6)) at the poses (rvec, tvec): cov = sigma2 M G N^-1 G^T M^T"""
    rvec, tvec = np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD)
    n = rvec.shape[0]
    corners = np.asarray(corners, np.float32).reshape(n, 4, 2)
    J = pr.jacobian(rvec, tvec, corners, K, D, L)
    N = np.einsum("...ri,...rj->...ij", J, J)
    e2 = pr.cost(rvec, tvec, corners, K, D, L)
    sigma2 = LD(float(sigma_px)) ** 2 + (e2 / 8 if use_residual else 0 * e2)
    G = observation_jacobian(rvec, tvec)
    M = mount_matrix(mount)
    cov = np.zeros((n, 3, 3), dtype=LD)
    with np.errstate(all="ignore"):
        for i in range(n):
            X = solve_ld(N[i], G[i].T)
            C = M @ (G[i] @ X) @ M.T
            cov[i] = sigma2[i] * (C + C.T) / 2
    return cov, sigma2, e2, N


def degenerate(cov):
    """flag 1: an entry of cov non-finite or a diagonal entry <= 0"""
    c = np.asarray(cov, np.float64).reshape(-1, 9)
    return ~np.isfinite(c).all(axis=1) | (c[:, 0] <= 0) | (c[:, 4] <= 0) | (c[:, 8] <= 0)


def kappa2(N):
    return np.linalg.cond(np.asarray(N, np.float64))


def rule(cov, flag1, tvec, threshold, scale=1.0, floor_xy=1e-6, floor_th=1e-6, gate_norm=1.0, **_):
    """the rule on a record's own doubles: (r (n, 3) in float64 with the kernel's expressions, flags).  Rows with flag 1 have r = nan:
    there R keeps the pose stage's values and flag 2 is not evaluated"""
    c = np.asarray(cov, np.float64).reshape(-1, 9)
    flag1 = np.asarray(flag1, bool)
    r = np.stack([np.float64(scale) * c[:, 0] + np.float64(floor_xy), np.float64(scale) * c[:, 4] + np.float64(floor_xy),
                  np.float64(scale) * c[:, 8] + np.float64(floor_th)], 1)
    t = np.asarray(tvec, np.float64)
    nt = np.sqrt(t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1] + t[:, 2] * t[:, 2])
    far = nt.astype(np.float32) > np.float32(threshold)
    with np.errstate(all="ignore"):
        gated = ~flag1 & (np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]) > np.float64(gate_norm))
    r[flag1] = np.nan
    return r, flag1 * 1 + gated * 2 + far * 4


def slot_sum(fl):
    fl = np.asarray(fl)
    return len(fl), int(np.sum((fl & 1) != 0)), int(np.sum((fl & 2) != 0))


def observation_at(R, t, mount):
    """(x, y, theta) of a marker at rotation matrix R and translation t: the noise-free truth of a generated case"""
    R, t = np.asarray(R, dtype=LD), np.asarray(t, dtype=LD)
    mx, my, psi = (LD(float(v)) for v in mount)
    x0, y0 = t[..., 2], -t[..., 0]
    th0 = pr.norm_angle(np.arctan2(-R[..., 0, 2], R[..., 2, 2]))
    c, s = np.cos(psi), np.sin(psi)
    return np.stack([c * x0 - s * y0 + mx, s * x0 + c * y0 + my, pr.norm_angle(th0 + psi)], -1)


def mahalanobis(obs, truth, cov):
    """d^2 = e^T cov^-1 e per marker, e = obs - truth with theta wrapped; cov (n, 3, 3), or (n, 3) for a diagonal"""
    e = np.asarray(obs, np.float64) - np.asarray(truth, np.float64)
    e[:, 2] = (e[:, 2] + np.pi) % (2 * np.pi) - np.pi
    cov = np.asarray(cov, np.float64)
    if cov.ndim == 2:
        return np.sum(e * e / cov, axis=1)
    return np.einsum("ni,ni->n", e, np.linalg.solve(cov, e[:, :, None])[:, :, 0])
