"""Windowed EKF over several laps of the benchmark scenes (aruco_slam_amd/csrc/ekf_window.hip): observations injected from the
cfg2 panel world and the cfg2 sliding ring world (no detector), three laps each, with chain pieces of 1 and 8 frames.  Mean and
covariance are compared with the per-frame chain (ASLAM_NO_WINDOWS) after every lap.  The runs are longer than any case of
tests/test_ekf_window.py: the prepare wave of the chain carries the pose rows of P in its own registers through a whole piece,
and any drift of those rows from the accumulators would show here.  Runs on the emulation build here and on the MI355X."""
import math
import os

import numpy as np
import pytest

from aruco_slam_amd import capi, synth

LAPS = 3


def observations(world, fr, rng):
    px, py, phi = fr.true_pose
    c, s = math.cos(phi), math.sin(phi)
    out = []
    for li in fr.landmark_index:
        wx, wy, wth = world.world[li]
        dx, dy = wx - px, wy - py
        th = (wth - phi + math.pi) % (2 * math.pi) - math.pi
        out.append((dx * c + dy * s + rng.normal(0, 2e-3), -dx * s + dy * c + rng.normal(0, 2e-3), th + rng.normal(0, 1e-3)))
    return np.array(out).reshape(-1, 3)


def run_laps(name, frames_per_lap, windows, piece, monkeypatch):
    """mu, Sigma after each of LAPS laps of `frames_per_lap` frames of the scene, and the planner's statistics"""
    cfg = synth.CONFIGS[name]
    w = synth.make_world(cfg)
    lap = min(frames_per_lap, w.lap_length())
    with monkeypatch.context() as m:
        if windows:
            m.setenv("ASLAM_WIN_PIECE", str(piece))
            m.delenv("ASLAM_NO_WINDOWS", raising=False)
        else:
            m.setenv("ASLAM_NO_WINDOWS", "1")
        ctx = capi.Context(max_rows=64, max_cols=64, max_batch=lap, max_landmarks=w.L + 8,
                           max_updates_per_frame=24 if w.M <= 24 else 64)
    ctx.set_camera(synth.camera_matrix(64, 64, 50.0), np.zeros(5))
    rng = np.random.RandomState(7)
    frames = [w.frame(i) for i in range(lap)]
    turn = w.frame(lap)
    ctx.profile_enable(True)
    ctx.profile_reset()
    out = []
    for k in range(LAPS):
        enc = [(f.wl, f.wr, f.dt) for f in frames]
        if k:
            enc[0] = (turn.wl, turn.wr, turn.dt)
        ctx.stage_encoders([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc])
        for i, f in enumerate(frames):
            ctx.inject_observations(i, f.ids, np.ones(len(f.ids), np.int32), observations(w, f, rng),
                                    np.tile([0.05, 0.05, 0.01], (len(f.ids), 1)))
        ctx.run_staged(0, lap, with_ekf=2)
        ctx.sync()
        out.append(ctx.get_state())
    stats = ctx.plan_stats()
    ctx.close()
    return out, stats


def check_laps(name, frames_per_lap, piece, monkeypatch):
    win, st = run_laps(name, frames_per_lap, True, piece, monkeypatch)
    ref, st_ref = run_laps(name, frames_per_lap, False, piece, monkeypatch)
    assert st_ref["frames_in_windows"] == 0
    # the first lap builds the map (new landmarks end windows); the later laps must run almost entirely inside windows
    assert st["windows"] > 0 and st["frames_in_windows"] >= (LAPS - 1) * 0.9 * min(frames_per_lap, synth.make_world(synth.CONFIGS[name]).lap_length())
    for k, ((mu, S), (mu_r, S_r)) in enumerate(zip(win, ref)):
        assert mu.shape == mu_r.shape and mu.size > 3
        assert np.allclose(mu, mu_r, rtol=1e-10, atol=1e-12), f"lap {k}: mu differs by {np.abs(mu - mu_r).max()}"
        e = np.abs(S - S_r).max() / np.abs(S_r).max()
        assert e <= 1e-10, f"lap {k}: Sigma differs by {e} (relative)"


# the emulation runs a shortened lap (every kernel thread is a coroutine on the CPU); the GPU runs the whole lap
EMU_FRAMES = 40


@pytest.mark.parametrize("piece", [1, 8])
@pytest.mark.parametrize("name", ["cfg2", "cfg2_sliding"])
def test_laps_match_the_per_frame_chain(name, piece, monkeypatch):
    check_laps(name, EMU_FRAMES, piece, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [1, 8])
@pytest.mark.parametrize("name", ["cfg2", "cfg2_sliding"])
def test_laps_match_the_per_frame_chain_on_gpu(name, piece, monkeypatch):
    check_laps(name, 10 ** 6, piece, monkeypatch)
