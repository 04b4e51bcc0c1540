"""Step control and header records of the window chain (aruco_slam_amd/csrc/ekf_window.hip, win_chain_role): the prepare wave counts
its steps in wave-uniform registers (frame, corrections of the frame, next correction; a step is a predict when the frame's
corrections are exhausted) and takes a correction's landmark position from the lane that loaded it at the frame's predict, instead
of looking both up in the step tables; and it writes the per-frame part of a correction's log header (ze, g02, g12) once per frame
into a record table by frame parity, from which the wave that stores the header (the logger wave; in the piece schedule worker
wave 0) composes it with type and position from the step tables.  The cases are the smallest shapes at which the counters or the
composition can go wrong.  Every case
  - equals the piece schedule (ASLAM_WIN_PIECE: the same role code, the header composed by worker wave 0 instead of the logger wave)
    under same()'s bounds: 1e-12 relative, landmark ids, pop lists and per-slot statistics exactly;
  - equals the numpy literal transcription of the reference at 1e-9 after every call (the independent reference);
  - leaves the window error word 0 (checked by run() after every call);
  - launches k_ekf_win_step exactly once per window the case is built to form.
The smallest window has two frames and a window never spans calls (see test_ekf_window_logger.py): the cases cut their windows with
the batch size, and the first call of every case adds the landmarks (frame 0; what follows it in that call may form a window)."""
import functools

import pytest

from test_ekf_window import make_case, run_device
from test_ekf_window_one_launch import compare

# name: ((seed, groups, n_land), batch, windows, context arguments)
STEPCTL_CASES = {
    # two-frame windows fusing 0 / m, m / 0 and 0 / 0 corrections, then m / m again: a predict after a predict, the counters at
    # m = 0 at either end of a window, nothing left over from an empty window
    "empty_frames": ((41, [(2, [0, 1, 2], False), (1, [], False), (1, [0, 1, 2], False), (1, [0, 1, 2], False), (1, [], False),
                           (2, [], False), (1, [0, 2], False), (1, [1], False)], 3), 2, 4, {}),
    # an empty frame between two that fuse: frames k and k + 2 share a parity of the record table, and the predict of k + 2 is
    # prepared while the lone predict of k + 1 is stored
    "empty_between": ((42, [(3, [0, 1, 2], False), (1, [0, 1, 2], False), (1, [], False), (1, [0, 2], False)], 3), 3, 2, {}),
    # m = 4, 1, 3 in consecutive frames: the correction count and the running index are re-armed at every predict
    "m_4_1_3": ((43, [(3, [0, 1, 2, 3], False), (1, [0, 1, 2, 3], False), (1, [2], False), (1, [0, 1, 3], False)], 4), 3, 2, {}),
    # frames fusing non-contiguous, differing subsets of S = {0, 1, 2, 3}: the position of correction a is not a
    "non_contiguous_subsets": ((44, [(2, [0, 1, 2, 3], False), (1, [0, 2, 3], False), (1, [1, 3], False)], 4), 2, 1, {}),
    # a frame whose observations are all "stationary" (popped, not fused) inside a window: m = 0 < npop
    "stationary_inside": ((45, [(4, [0, 1, 2, 3], False), (4, [0, 1, 2, 3], True)], 4), 4, 2, {}),
    # the planner's correction limit (kWinCorrMax = kWinSMax = 63, admitted when the context allows 63 updates per frame): lane 62
    # holds a position and a record, on the 192-wide image
    "correction_limit_192_wide": ((46, [(2, list(range(63)), False), (2, list(range(63)), False)], 63), 2, 1,
                                  dict(max_landmarks=64, max_updates=64)),
    # 23 landmarks = 128 wide: positions 21 and 22 have their rows in the second chunk of 64 columns (lrow = 66, 69)
    "two_frames_128_wide": ((47, [(2, list(range(23)), False), (2, list(range(23)), False)], 23), 2, 1, {}),
    # three windows in a row on different sets with different counts: neither the counters nor the record table leak
    "different_sets_in_a_row": ((48, [(2, list(range(6)), False), (2, [0, 1, 2], False), (2, [4], False), (2, [3, 5], False)], 6), 2, 3, {}),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the frames and the literal transcription's state after each of them: computed once per case"""
    return make_case(*STEPCTL_CASES[name][0])


def check(name):
    case, batch, windows, kw = STEPCTL_CASES[name]
    _, prof = compare(case, batch, **kw)                             # one launch == piece schedule; error word 0 after every call
    print(f"{name}: {prof['k_ekf_win_step'][0]} window launches, built for {windows}")
    assert prof["k_ekf_win_step"][0] == windows
    frames, exp = reference(name)
    _, prof, worst = run_device(frames, exp, batch=batch, **kw)      # every call's last frame against the literal transcription at 1e-9
    print(f"{name}: worst relative Sigma error against the literal transcription {worst:.2e}")
    assert prof["k_ekf_win_step"][0] == windows and worst <= 1e-9


@pytest.mark.parametrize("name", sorted(STEPCTL_CASES))
def test_step_control(name):
    check(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STEPCTL_CASES))
def test_step_control_on_gpu(name):
    check(name)
