"""What k_pose_alt computes, restated in numpy long double on top of tests/pose_reference.py: the mirrored start, the
damped iteration of solvePnP with its stopping rule, undamped Gauss-Newton continued to full convergence (the second minimum
itself), the alternate observation, the flag rule and the slot sums.  Every function takes a batch: the leading axis is markers."""
import numpy as np

import pose_reference as pr

LD = pr.LD
FLT_EPSILON = LD(float(np.finfo(np.float32).eps))


def rodrigues_inv(R):
    """rotation matrices (n, 3, 3) -> rotation vectors with angle in [0, pi], through the unit quaternion (the largest of w, x, y, z
    first: exact near angle pi, where a facing marker lies)"""
    R = np.asarray(R, dtype=LD)
    out = np.zeros(R.shape[:-2] + (3,), dtype=LD)
    for n in np.ndindex(R.shape[:-2]):
        m = R[n]
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        cand = [tr, m[0, 0] - m[1, 1] - m[2, 2], m[1, 1] - m[0, 0] - m[2, 2], m[2, 2] - m[0, 0] - m[1, 1]]
        i = int(np.argmax(np.array(cand, dtype=np.float64)))
        s = np.sqrt(1 + cand[i]) * 2
        if i == 0:
            q = [s / 4, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
        elif i == 1:
            q = [(m[2, 1] - m[1, 2]) / s, s / 4, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
        elif i == 2:
            q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, s / 4, (m[1, 2] + m[2, 1]) / s]
        else:
            q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, s / 4]
        q = np.array(q, dtype=LD)
        if q[0] < 0:
            q = -q
        nv = np.sqrt(np.sum(q[1:] * q[1:]))
        if nv == 0:
            continue
        out[n] = q[1:] / nv * (2 * np.arctan2(nv, q[0]))
    return out


def mirrored_start(rvec, tvec):
    """(r, t) of the start of the second solve: R' = (I - 2 v v^T) R1 diag(1, 1, -1), v = t1 / |t1| - the marker's normal reflected about
    the line of sight, the in-plane axes kept (det R' = +1) - and t1 itself"""
    rvec, tvec = np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD)
    R1 = pr.rodrigues(rvec)
    v = tvec / np.sqrt(np.sum(tvec * tvec, axis=-1))[..., None]
    H = np.eye(3, dtype=LD) - 2 * v[..., :, None] * v[..., None, :]
    Rm = (H @ R1) * np.array([1, 1, -1], dtype=LD)
    return rodrigues_inv(Rm), tvec.copy()


def _normal_equations(p, corners, K, D, L):
    e = pr.residuals(p[..., :3], p[..., 3:], corners, K, D, L)
    J = pr.jacobian(p[..., :3], p[..., 3:], corners, K, D, L)
    return np.einsum("...ri,...rj->...ij", J, J), np.einsum("...ri,...r->...i", J, e), np.sum(e * e, axis=-1)


def _solve(A, b):
    """long-double systems solved in double (numpy has no long-double solver): the iterations below only need a step, and their fixed
    point is set by the long-double gradient b"""
    return np.linalg.solve(np.asarray(A, np.float64), np.asarray(b, np.float64)[..., None])[..., 0].astype(LD)


def refine(rvec, tvec, corners, K, D, L):
    """solvePnP's damped iteration from (rvec, tvec): Levenberg-Marquardt on the 8 residuals, (J^T J with its diagonal times 1 + lambda)
    x = J^T e, lambda = 10^k from k = -3, a worse trial raises k (up to 16) and is retried, an accepted one lowers it; at most 20 accepted
    steps, stop when |dp| / |p| < FLT_EPSILON.  Returns (r, t, cost, accepted steps)"""
    p = np.concatenate([np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD)], -1)
    n = p.shape[0]
    corners = np.asarray(corners, np.float32).reshape(n, 4, 2)
    JtJ, Jte, c = _normal_equations(p, corners, K, D, L)
    prev_err = np.sqrt(c)
    lg = np.full(n, -3)
    iters = np.zeros(n, int)
    done = np.zeros(n, bool)
    eye = np.eye(6, dtype=LD)
    for _ in range(64):
        if done.all():
            break
        lam = LD(10) ** lg.astype(LD)
        A = JtJ * (1 + eye * lam[:, None, None])
        trial = p - _solve(A, Jte)
        tJ, tg, tc = _normal_equations(trial, corners, K, D, L)
        err = np.sqrt(tc)
        for i in np.nonzero(~done)[0]:
            if err[i] > prev_err[i]:
                lg[i] += 1
                if lg[i] <= 16:
                    continue
            lg[i] = max(lg[i] - 1, -16)
            d = trial[i] - p[i]
            iters[i] += 1
            if iters[i] >= 20 or np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(p[i] * p[i])) < FLT_EPSILON:
                done[i] = True
            p[i], JtJ[i], Jte[i], c[i], prev_err[i] = trial[i], tJ[i], tg[i], tc[i], err[i]
    return p[:, :3], p[:, 3:], c, iters


def converge(rvec, tvec, corners, K, D, L, tol=1e-15, max_iter=400):
    """undamped Gauss-Newton from (rvec, tvec) until |dp| / |p| < tol: the minimum itself.  Returns (r, t, last step per marker)"""
    p = np.concatenate([np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD)], -1).copy()
    n = p.shape[0]
    corners = np.asarray(corners, np.float32).reshape(n, 4, 2)
    step = np.full(n, np.inf)
    for _ in range(max_iter):
        live = step >= tol
        if not live.any():
            break
        JtJ, Jte, _ = _normal_equations(p[live], corners[live], K, D, L)
        dp = _solve(JtJ, Jte)
        step[live] = np.asarray(np.sqrt(np.sum(dp * dp, axis=-1)) / np.sqrt(np.sum(p[live] * p[live], axis=-1)), np.float64)
        p[live] = p[live] - dp
    return p[:, :3], p[:, 3:], step


def second_pose(rvec, tvec, corners, K, D, L):
    """the whole second solve from the primary pose: (r_stop, t_stop, cost, iters) of the damped iteration and (r_min, t_min, step) of
    the minimum it was heading for"""
    r0, t0 = mirrored_start(rvec, tvec)
    r, t, c, it = refine(r0, t0, corners, K, D, L)
    rm, tm, step = converge(r, t, corners, K, D, L)
    return (r, t, c, it), (rm, tm, step)


def dtheta(th_alt, th_obs):
    """|wrap(th_alt - th_obs)|"""
    return np.abs(pr.norm_angle(np.asarray(th_alt, dtype=LD) - np.asarray(th_obs, dtype=LD)))


def flags(rms, rms_alt, dth, valid, finite, ratio, floor_px, min_dtheta, reject):
    """the rule on a record's own doubles: 1 ambiguous, 2 rejected, 4 non-finite"""
    rms, rms_alt, dth = (np.asarray(a, np.float64) for a in (rms, rms_alt, dth))
    finite = np.asarray(finite, bool)
    amb = finite & (rms_alt <= np.maximum(np.float64(ratio) * rms, np.float64(floor_px))) & (dth > np.float64(min_dtheta))
    rej = amb & bool(reject) & (np.asarray(valid) != 0)
    return amb * 1 + rej * 2 + (~finite) * 4


def slot_sum(fl):
    fl = np.asarray(fl)
    return len(fl), int(np.sum((fl & 1) != 0)), int(np.sum((fl & 2) != 0))
