"""The medium EKF chain (k_ekf_mid64 -> k_ekf_T -> k_ekf_update_mfma) at a state size where the update really is a dense
contraction (N = 1503 / 3003 is what cfg3 runs at): one predict + 50 fused corrections against a numpy restatement of the
reference's sequential recursion (aruco_slam.cpp:35-73, 108-207) written in its rank-3 form
(tests/ekf_reference.py: sigma <- sigma - K (Gx sigma), the same products the reference forms with dense N x N matrices)."""
import math

import numpy as np
import pytest

from aruco_slam_amd import capi
from ekf_reference import reference_step, wrap_once

pytestmark = pytest.mark.gpu


def wrap(a):
    return float(wrap_once(a))


@pytest.mark.parametrize("L,M", [(500, 50), (1000, 40)])
def test_medium_chain_at_dense_update_size(L, M):
    rng = np.random.RandomState(L)
    N = 3 + 3 * L
    mu = np.zeros(N)
    mu[:3] = [0.3, -0.2, 0.4]
    ang = rng.uniform(0, 2 * math.pi, L); rad = rng.uniform(1.0, 6.0, L)
    mu[3::3] = rad * np.cos(ang); mu[4::3] = rad * np.sin(ang); mu[5::3] = rng.uniform(-3, 3, L)
    A = rng.standard_normal((N, 24)) * 0.05
    S = A @ A.T + np.diag(rng.uniform(0.01, 0.05, N))          # dense, symmetric positive definite
    ids = np.arange(L, dtype=np.int32)
    ctx = capi.Context(max_rows=64, max_cols=64, max_batch=2, max_landmarks=L + 4, max_updates_per_frame=64, persistent_waves=64)
    ctx.set_state(mu, S, ids)
    seen = np.sort(rng.choice(L, M, replace=False))
    obs = []
    ct, st = math.cos(mu[2]), math.sin(mu[2])
    for idx in seen:
        li = 3 + 3 * idx
        dx, dy = mu[li] - mu[0], mu[li + 1] - mu[1]
        z = np.array([dx * ct + dy * st, -dx * st + dy * ct, wrap(mu[li + 2] - mu[2])]) + rng.normal(0, 0.03, 3)
        obs.append((int(idx), z, rng.uniform(0.02, 0.2, 3)))
    # first sample only arms the filter (dt ignored), the second one predicts
    ctx.stage_encoders([0.0, 2.0], [0.0, 2.3], [0.0, 1 / 30.0])
    ctx.inject_observations(0, [], [], np.zeros((0, 3)), np.zeros((0, 3)))
    ctx.inject_observations(1, [int(o[0]) for o in obs], [1] * M, np.array([o[1] for o in obs]), np.array([o[2] for o in obs]))
    ctx.run_staged(0, 2, with_ekf=2)
    ctx.sync()
    mu_g, S_g = ctx.get_state()
    mu_r, S_r = reference_step(mu, S, 2.0, 2.3, 1 / 30.0, obs, dtype=np.float64)
    gi, gx, ga, _, _ = ctx.get_observations()
    assert np.array_equal(gx, seen) and (ga == 1).all()
    assert np.allclose(mu_g, mu_r, rtol=1e-9, atol=1e-11)
    assert np.abs(S_g - S_r).max() <= 1e-9 * np.abs(S_r).max()
