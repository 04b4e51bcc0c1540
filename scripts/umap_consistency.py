"""Consistency evidence for localization on an uncertain map, CPU only, recorded and not asserted: the mean pose
NEES e^T Sigma_xx^-1 e (3 for a consistent filter) of the fixed-map reference (tests.test_localize.FrozenMapLocalizer) and of the
uncertain-map reference (tests.umap_reference.UncertainMapLocalizer) on the same sightings, when the landmarks really stand where
a draw from the map's C_i puts them.

    python scripts/umap_consistency.py [--runs 200] [--frames 30] [--landmarks 12] [--sigma 0.05]

Per run: true landmarks = map means + N(0, C_i), true start pose = POSE0 + N(0, SIG0), the true pose then moves by the filter's own
motion model on exact encoder samples; every frame sights 4 landmarks with noise drawn from each observation's own R."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests.test_innovation_gate import Truth, sight  # noqa: E402
from tests.test_localize import POSE0, SIG0, FrozenMapLocalizer, random_map  # noqa: E402
from tests.umap_reference import UncertainMapLocalizer  # noqa: E402


def nees(m, truth):
    e = m.mu - truth
    e[2] = (e[2] + math.pi) % (2 * math.pi) - math.pi
    return float(e @ np.linalg.solve(m.P, e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--landmarks", type=int, default=12)
    ap.add_argument("--sigma", type=float, default=0.05)
    a = ap.parse_args()
    rng = np.random.RandomState(2024)
    ids, xyth = random_map(rng, a.landmarks)
    A = rng.normal(0, a.sigma, (a.landmarks, 3, 3))
    C = A @ A.transpose(0, 2, 1)
    chol = np.linalg.cholesky(C + 1e-15 * np.eye(3))
    chol0 = np.linalg.cholesky(SIG0)
    acc = dict(fixed=[], umap=[])
    last = dict(fixed=[], umap=[])
    for run in range(a.runs):
        true_map = xyth + np.einsum("nij,nj->ni", chol, rng.normal(0, 1, (a.landmarks, 3)))
        truth = Truth(ids, true_map, POSE0 + chol0 @ rng.normal(0, 1, 3))
        filters = dict(fixed=FrozenMapLocalizer(ids, xyth, POSE0, SIG0), umap=UncertainMapLocalizer(ids, xyth, C, POSE0, SIG0))
        for f in range(a.frames):
            wl, wr, dt = rng.uniform(1, 4), rng.uniform(1, 4), 0.05
            pose = truth.step(wl, wr, dt)
            obs = sight(pose, ids, true_map, rng.permutation(a.landmarks)[:4].tolist(), rng)
            for k, m in filters.items():
                m.add_encoder(wl, wr, dt)
                m.add_observations(obs)
                acc[k].append(nees(m, pose))
        for k, m in filters.items():
            last[k].append(nees(m, pose))
    print(json.dumps(dict(runs=a.runs, frames=a.frames, landmarks=a.landmarks, landmark_sigma=a.sigma, sightings_per_frame=4,
                          mean_nees_all_frames={k: round(float(np.mean(v)), 3) for k, v in acc.items()},
                          mean_nees_last_frame={k: round(float(np.mean(v)), 3) for k, v in last.items()}, consistent=3.0)))


if __name__ == "__main__":
    main()
