"""The logger wave of the one-launch window (aruco_slam_amd/csrc/ekf_window.hip, win_chain_role with ONE = true): one wave of the chain
workgroup copies every step's operand rows and header from the parity buffers in LDS to the log and publishes the step count
(every kWinPubEvery = 4 steps, for the steps kWinPubLag = 4 or more behind; the whole count at the end), and the prepare wave reads
its own A operand at the next step's row indices in front of the step barrier.  The cases are the smallest shapes at which the
publication or the hoisted reads can go wrong.  Every case
  - equals the piece schedule (ASLAM_WIN_PIECE, where worker waves store the log and nothing is published inside a launch) under
    same()'s bounds: 1e-12 relative, landmark ids, pop lists and per-slot statistics exactly;
  - equals the numpy literal transcription of the reference at 1e-9 after every call;
  - leaves the window error word 0 (checked by run() after every call);
  - launches k_ekf_win_step exactly once per window the case is built to form.
A window never spans calls and the planner gives a lone eligible frame to the per-frame chain (capi.hip, close_window: "a lone
frame: the per-frame chain is as good"), so the smallest window has two frames: the cases cut their windows with the batch size, and
"windows in a row on different sets" are 2-frame windows.  The first call of every case adds the landmarks (no window)."""
import functools

import pytest

from test_ekf_window import make_case, run_device
from test_ekf_window_one_launch import compare

# name: ((seed, groups, n_land), batch, windows, context arguments)
LOGGER_CASES = {
    # windows of 2, 4, 5, 8 and 9 steps (a frame with m corrections is 1 + m steps): below kWinPubLag, at it, one past it, at a
    # multiple of kWinPubEvery (all of these publish only the final count) and one past it (the first publication inside the loop)
    "short_windows": ((21, [(2, [0, 1, 2, 3], False), (2, [], False), (2, [0], False), (1, [0], False), (1, [0, 1], False),
                            (2, [0, 1, 2], False), (1, [0, 1, 2], False), (1, [0, 1, 2, 3], False)], 4), 2, 5, {}),
    # a frame that fuses nothing between two that fuse: a predict prepared after a predict (depth-4 operands read ahead, the
    # fourth depth row written, then zeroed by the next correction in that buffer)
    "predict_after_predict": ((22, [(3, [0, 1, 2], False), (1, [0, 1, 2], False), (1, [], False), (1, [0, 2], False)], 3), 3, 2, {}),
    # a frame whose observations are all "stationary" (popped, not fused) inside a window
    "stationary_inside": ((23, [(4, [0, 1, 2, 3], False), (4, [0, 1, 2, 3], True)], 4), 4, 2, {}),
    # the wider images: 21 landmarks = 128 wide (T = 8: 7 log stores per step), 42 landmarks = 192 wide (T = 12: 10 per step)
    "two_frames_128_wide": ((24, [(2, list(range(21)), False), (2, list(range(21)), False)], 21), 2, 1, {}),
    "two_frames_192_wide": ((25, [(2, list(range(42)), False), (2, list(range(42)), False)], 42), 2, 1, dict(max_landmarks=60, max_updates=50)),
    # three windows in a row on different sets: the counters carry the window's epoch and are never reset
    "different_sets_in_a_row": ((26, [(2, list(range(6)), False), (2, [0, 1], False), (2, [2, 3], False), (2, [4, 5], False)], 6), 2, 3, {}),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the frames and the literal transcription's state after each of them: computed once per case"""
    return make_case(*LOGGER_CASES[name][0])


def check(name):
    case, batch, windows, kw = LOGGER_CASES[name]
    _, prof = compare(case, batch, **kw)                             # one launch == piece schedule; error word 0 after every call
    assert prof["k_ekf_win_step"][0] == windows, f"{prof['k_ekf_win_step'][0]} window launches, the case is built for {windows}"
    frames, exp = reference(name)
    _, prof, worst = run_device(frames, exp, batch=batch, **kw)      # every call's last frame against the literal transcription at 1e-9
    print(f"{name}: worst relative Sigma error against the literal transcription {worst:.2e}")
    assert prof["k_ekf_win_step"][0] == windows and worst <= 1e-9


@pytest.mark.parametrize("name", sorted(LOGGER_CASES))
def test_logger_wave(name):
    check(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LOGGER_CASES))
def test_logger_wave_on_gpu(name):
    check(name)
