"""Long-double restatement of one EKF step of the reference on an already-mapped state, and the random states the size tests
draw (a plain helper module, imported by the tests).

reference_step is addEncoder + addImage for landmarks that are already in the map (aruco_slam.cpp:35-73, 108-207), written in its
rank-3 form: sigma <- sigma - K (Gx sigma), the same products the reference forms with dense N x N matrices.  Every correction of a
frame is linearised at the pre-frame mean (quirk Q1), sigma follows them one by one in pop order.  Angles wrap once
(aruco_slam.cpp:412-421) around the double value of pi the device uses."""
import math

import numpy as np

LD = np.longdouble
PI = LD(math.pi)

# kernels that run for one per-frame EKF step on each chain (capi.hip: run_ekf_frame), by the context's max_updates_per_frame
CHAIN_KERNELS = {
    "fast": {"k_ekf_plan", "k_ekf_mid", "k_ekf_apply"},                                      # cap <= 24
    "mid": {"k_ekf_plan", "k_ekf_mid64", "k_ekf_T", "k_ekf_update_mfma"},                     # 24 < cap <= 64
    "general": {"k_ekf_plan", "k_ekf_gather", "k_ekf_small", "k_ekf_T", "k_ekf_update_mfma"},  # cap > 64
}
CHAIN_CAP = {"fast": 24, "mid": 64, "general": 128}


def chain_of(cap):
    return "fast" if cap <= 24 else "mid" if cap <= 64 else "general"


def ekf_kernels_run(prof):
    """names of the EKF kernels with at least one call in a profile_get() dictionary"""
    return {k for k, (calls, _) in prof.items() if k.startswith("k_ekf") and calls > 0}


def wrap_once(a):
    if a >= PI:
        a -= 2 * PI
    if a < -PI:
        a += 2 * PI
    return a


def _inv3(A):
    """inverse of a 3 x 3 matrix by cofactors (np.linalg does not take long double)"""
    a, b, c = A[0]; d, e, f = A[1]; g, h, i = A[2]
    C = np.array([[e * i - f * h, c * h - b * i, b * f - c * e],
                  [f * g - d * i, a * i - c * g, c * d - a * f],
                  [d * h - e * g, b * g - a * h, a * e - b * d]], dtype=LD)
    return C / (a * C[0, 0] + b * C[1, 0] + c * C[2, 0])


def reference_step(mu, S, wl, wr, dt, obs, kl=0.05, kr=0.05, b=0.09, Qk=0.01, dtype=LD, predict=True):
    """predict, then the corrections obs = [(index, z(3), Rdiag(3))] in pop order; returns (mu, Sigma) in `dtype`.  predict = False:
    the corrections alone, on a state that a predict of the caller's has left"""
    mu = np.array(mu, dtype=dtype); S = np.array(S, dtype=dtype)
    if predict:
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
        K = (S[:, cols] @ G.T) @ (_inv3(Sk) if dtype is LD else np.linalg.inv(Sk))     # sigma_ * Gx^T * S^-1
        mu += K @ ze
        if dtype is LD:
            for r in range(3):                                 # S -= K GS as three outer products (no long double BLAS)
                S -= np.outer(K[:, r], GS[r])
        else:
            S -= K @ GS
    return mu, S


def random_state(rng, L, heading=None, rank=24):
    """mu (3 + 3L) and a dense symmetric positive definite Sigma.  The pose heading (default: just below pi, so that the predict
    wraps it) is where a quarter of the landmarks sit at a relative heading within 0.02 of +-pi (their measurements fall on either
    side of the cut: the innovation wraps both ways); another quarter has absolute headings within 0.05 of +-pi."""
    N = 3 + 3 * L
    mu = np.zeros(N)
    h = math.pi - 0.0009 if heading is None else heading
    mu[:3] = [0.3, -0.2, h]
    ang = rng.uniform(0, 2 * math.pi, L); rad = rng.uniform(1.0, 6.0, L)
    mu[3::3] = rad * np.cos(ang); mu[4::3] = rad * np.sin(ang)
    th = rng.uniform(-math.pi + 1e-3, math.pi - 1e-3, L)
    k = rng.permutation(L)
    k1, k2 = k[: (L + 3) // 4], k[(L + 3) // 4: (L + 1) // 2]
    sg = np.where(rng.rand(L) < 0.5, -1.0, 1.0)
    th[k1] = [float(wrap_once(LD(h + sg[i] * (math.pi - rng.uniform(1e-3, 0.02))))) for i in k1]
    th[k2] = sg[k2] * rng.uniform(math.pi - 0.05, math.pi - 1e-3, k2.size)
    mu[5::3] = th
    A = rng.standard_normal((N, rank)) * 0.05
    S = A @ A.T + np.diag(rng.uniform(0.01, 0.05, N))
    return mu, S


def observe(rng, mu, seen, noise=0.03, post_predict=None):
    """observations of the landmarks `seen` from the pose post_predict (default mu[:3]): the true measurement plus noise, its
    heading wrapped once, so that measurements of landmarks seen near +-pi land on the other side of the cut"""
    x, y, th = mu[:3] if post_predict is None else post_predict
    ct, st = math.cos(th), math.sin(th)
    out = []
    for idx in seen:
        li = 3 + 3 * int(idx)
        dx, dy = mu[li] - x, mu[li + 1] - y
        z = np.array([dx * ct + dy * st, -dx * st + dy * ct, mu[li + 2] - th]) + rng.normal(0, noise, 3)
        z[2] = float(wrap_once(LD(z[2])))
        out.append((int(idx), z, rng.uniform(0.02, 0.2, 3)))
    return out


def predicted_pose(mu, wl, wr, dt, kl=0.05, kr=0.05, b=0.09):
    dsl, dsr = kl * dt * wl, kr * dt * wr
    dth = (dsr - dsl) / (2 * b); ds = 0.5 * (dsr + dsl)
    th = mu[2] + 0.5 * dth
    return np.array([mu[0] + ds * math.cos(th), mu[1] + ds * math.sin(th), float(wrap_once(LD(mu[2] + dth)))])


def rel_err(a, ref):
    """max |a - ref| / max |ref| in double"""
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(a, dtype=LD) - ref).max() / np.abs(ref).max())
