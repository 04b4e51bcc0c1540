"""One launch per window (aruco_slam_amd/csrc/ekf_window.hip, k_ekf_win_step with ONE = true): the chain, the replay of its log and
the Psi product of a whole window run in one launch and follow each other through in-launch counters.  The steps are those of the
piece schedule (ASLAM_WIN_PIECE) in the same order; the one difference: a piece reloads the prepare wave's pose rows from the
accumulators' P image, while the one launch carries them in the prepare wave's registers through the window (as a piece does between
its own frames), so mu and Sigma agree to rounding (1e-12 relative) and the landmark ids, the pop lists and the per-slot statistics
exactly.  A wait that gives up makes the call fail (sync reads the window error word, clears it and returns ASLAM_E_HIP), so
these runs also show that no workgroup timed out.  Runs on the emulation build and on the real library on the MI355X.  The
emulation starts a launch's workgroups in index order, so there the replay and Psi roles mostly find the whole log published and
replay it in one batch; the partial counts and the batch-by-batch hand-off are exercised by the -m gpu runs."""
import ctypes as C
import os

import numpy as np
import pytest

from aruco_slam_amd import capi
from test_ekf_window import CASES, WIDE, D, K, make_case


def run(frames, batch, env, max_landmarks=40, max_updates=24):
    """the frames through the windowed filter under the environment knobs `env`; everything the filter leaves behind, per batch"""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        nfr = len(frames)
        ctx = capi.Context(max_rows=64, max_cols=64, max_batch=nfr, persistent_waves=4, max_landmarks=max_landmarks, r2c_t=(0.1, -0.05, 0.0),
                           max_updates_per_frame=max_updates)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx.set_camera(K, D)
    t = [fr["t"] for fr in frames]
    ctx.stage_encoders([fr["wl"] for fr in frames], [fr["wr"] for fr in frames], [0.0] + [t[i] - t[i - 1] for i in range(1, nfr)])
    for f, fr in enumerate(frames):
        obs = fr["obs"]
        ctx.inject_observations(f, fr["ids"], [0 if o is None else 1 for o in obs],
                                np.array([np.zeros(3) if o is None else o["z"] for o in obs]).reshape(-1, 3),
                                np.array([np.ones(3) if o is None else np.diag(o["R"]) for o in obs]).reshape(-1, 3))
    ctx.profile_enable(True)
    ctx.profile_reset()
    out = []
    for f0 in range(0, nfr, batch):
        nb = min(batch, nfr - f0)
        ctx.run_staged(f0, nb, with_ekf=2)
        ctx.sync()                         # (raises if a workgroup of a window launch gave up waiting: see the docstring)
        words = np.zeros(8, np.uint32)       # ... so the word read back here is zero whenever sync returned
        assert ctx.lib.aslam_debug_get_counters(ctx.h, words.ctypes.data_as(C.c_void_p)) == 0
        assert words[6] == 0, f"window error word {words[6]}"
        mu, S = ctx.get_state()
        out.append(dict(mu=mu, S=S, ids=ctx.get_landmark_ids(), obs=ctx.get_observations(), stats=ctx.get_slot_ekf_stats(f0, nb)))
    return out, ctx.profile_get()


def same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x["mu"].shape == y["mu"].shape and x["S"].shape == y["S"].shape
        assert np.allclose(x["mu"], y["mu"], rtol=1e-12, atol=1e-14), f"batch {i}: mu differs by {np.abs(x['mu'] - y['mu']).max()}"
        e = np.abs(x["S"] - y["S"]).max() / np.abs(y["S"]).max()
        assert e <= 1e-12, f"batch {i}: Sigma differs by {e} (relative)"
        assert np.array_equal(x["ids"], y["ids"]), f"batch {i}: landmark ids differ"
        for p, q in zip(x["obs"], y["obs"]):
            assert np.array_equal(p, q) if p.dtype.kind == "i" else np.allclose(p, q, rtol=1e-12, atol=1e-14), f"batch {i}: pop list differs"
        assert np.array_equal(x["stats"], y["stats"]), f"batch {i}: per-slot statistics differ"


def compare(case, batch, extra=None, **kw):
    seed, groups, n_land = case
    frames, _ = make_case(seed, groups, n_land)
    env = dict(extra or {})
    one, prof = run(frames, batch, env, **kw)
    pieces, _ = run(frames, batch, dict(env, ASLAM_WIN_PIECE="8"), **kw)
    same(one, pieces)
    assert prof["k_ekf_win_step"][0] > 0, "no window was formed"
    return one, prof


# a cfg2-like 64-wide window (20 landmarks, 20 corrections per frame, 32 frames), the sliding 128-wide ring, a 64-frame window,
# 1-frame windows (every other frame leaves the set), stationary and subset frames inside a window, window -> window hand-over
ONE_CASES = {
    "cfg2_like_64_wide": (11, [(32, list(range(20)), False)], 20),
    "sliding_128": CASES["sliding_set"],
    "frames_64": (12, [(2, [0, 1, 2], False), (66, [0, 1, 2, 3], False)], 4),
    "one_frame_windows": (13, [(1, [0, 1], False), (1, [2, 3], False)] * 5, 4),
    "stationary_inside": CASES["stationary_inside"],
    "subset_frames": CASES["subset_frames"],
    "window_to_window": CASES["window_to_window"],
}


@pytest.mark.parametrize("name", sorted(ONE_CASES))
def test_one_launch_equals_the_piece_schedule(name):
    compare(ONE_CASES[name], batch=10_000)


@pytest.mark.parametrize("name", ["window_to_window", "sliding_128"])
def test_one_launch_hand_over_without_early_start(name):
    compare(ONE_CASES[name], batch=10_000, extra={"ASLAM_WIN_NO_EARLY": "1"})


def test_one_launch_small_batches():
    compare(ONE_CASES["window_to_window"], batch=7)


def test_one_launch_192_wide_50_corrections():
    compare(WIDE, batch=10_000, max_landmarks=60, max_updates=50)


def test_one_launch_matches_the_literal_transcription():
    from test_ekf_window import run_device
    seed, groups, n_land = CASES["window_to_window"]
    frames, exp = make_case(seed, groups, n_land)
    _, prof, worst = run_device(frames, exp, batch=len(frames))     # checks every frame at 1e-9
    assert prof["k_ekf_win_step"][0] > 0 and worst <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ONE_CASES))
def test_one_launch_equals_the_piece_schedule_on_gpu(name):
    compare(ONE_CASES[name], batch=10_000)


@pytest.mark.gpu
def test_one_launch_192_wide_on_gpu():
    compare(WIDE, batch=10_000, max_landmarks=60, max_updates=50)


@pytest.mark.gpu
def test_one_launch_hand_over_without_early_start_on_gpu():
    compare(ONE_CASES["window_to_window"], batch=10_000, extra={"ASLAM_WIN_NO_EARLY": "1"})
