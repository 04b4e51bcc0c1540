"""The hand-over between two windows and the prepare wave's predict (aruco_slam_amd/csrc/ekf_window.hip).

Hand-over: k_ekf_win_next forms the next window's P and mu_S images from the previous window's small results in ONE launch; the
four launches it replaced (gather, thin products, Sigma pass on the miniature state, fix) stay behind ASLAM_WIN_NEXT_SPLIT.  Every
entry goes through the same matrix-core sequence in both, so everything the filter leaves behind must be EQUAL (largest absolute
difference 0): mu, Sigma, landmark ids, pop lists, slot statistics.  A hand-over happens only between two windows with no frame
on the per-frame chain between them, so every landmark of a case is introduced by its first frames; of the cases taken from the
other files only `window_to_window` hands over (in `two_groups` and `WIDE` a frame with new landmarks separates the windows, and
`sliding_set` widens its one window: they run here for the count 0 and the equality of everything else).  The cases below force
what those lack:
width changes 64 -> 128, 128 -> 64 (disjoint sets: only the pose rows in common), 192 -> 192 and 192 -> 64 (kWinWidenFrames,
s_cap in win_plan.h: a window of 16 frames or more is closed rather than widened, and so is one whose union would pass
s_cap landmarks), a next window with one landmark (s' = 6), and next sets whose s' = 3 + 3 nS' is no multiple of 16 (all but
`s48`, whose 15 landmarks make s' = 48 = 3 tiles exactly).

Predict: the slot statistics are stored by the table-building threads, the next frame's observations are fetched through an LDS
table of detection indices, and in the one-launch window the logger wave leaves the last frame's pop list behind; the piece
schedule (ASLAM_WIN_PIECE) keeps the pop list in the prepare wave.  Both must agree as in test_ekf_window_one_launch.py."""
import functools

import numpy as np
import pytest

from aruco_slam_amd import capi
from test_ekf_window import CASES, WIDE, make_case
from test_ekf_window_one_launch import ONE_CASES, compare, run

R = lambda a, b: list(range(a, b))  # noqa: E731
# name: (case, Context arguments, windows, hand-overs)
HAND = {
    "window_to_window": (CASES["window_to_window"], {}, 3, 2),
    "two_groups": (CASES["two_groups"], {}, 3, 0),
    "sliding_set": (CASES["sliding_set"], {}, 1, 0),
    "WIDE": (WIDE, dict(max_landmarks=60, max_updates=50), 2, 0),
    # 54 landmarks introduced by 3 frames; 17 frames on 20 (64 wide, closed rather than widened), 3 on 24 that overlap it in 10
    # (128 wide), 3 on a disjoint 20 (the union of 44 passes s_cap = 41: closed; 64 wide)
    "64_128_64": ((21, [(1, R(0, 18), False), (1, R(18, 36), False), (1, R(36, 54), False), (17, R(0, 20), False), (3, R(10, 34), False),
                        (3, R(34, 54), False)], 54), dict(max_landmarks=60), 3, 2),
    # 66 landmarks; 3 frames on 45 (192 wide), 3 on 46 that overlap it in 25 (union 66 > s_cap = 63: closed; 192 wide), 3 on 20 of
    # which 2 lie in the previous set (union 64: closed; 64 wide)
    "192_192_64": ((22, [(1, R(0, 33), False), (1, R(33, 66), False), (3, R(0, 45), False), (3, R(20, 66), False), (3, R(2, 22), False)], 66),
                   dict(max_landmarks=70, max_updates=50), 3, 2),
    # 17 frames on 20, then 3 frames on ONE landmark outside them: s' = 6
    "one_landmark": ((23, [(1, R(0, 13), False), (1, R(13, 26), False), (17, R(0, 20), False), (3, [25], False)], 26), {}, 2, 1),
    # the next set has 15 landmarks, 5 of them in the previous set: s' = 48, three full tiles of the 64-wide image
    "s48": ((24, [(1, R(0, 18), False), (1, R(18, 36), False), (17, R(0, 20), False), (3, R(15, 30), False)], 36), {}, 2, 1),
}


@functools.lru_cache(maxsize=None)
def frames_of(name):
    seed, groups, n_land = HAND[name][0]
    return make_case(seed, groups, n_land)[0]


def run_with_plan(frames, env, **kw):
    """`run` of test_ekf_window_one_launch.py, and the plan statistics of the context it made"""
    made = []

    class Recording(capi.Context):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    orig = capi.Context
    capi.Context = Recording
    try:
        out, prof = run(frames, 10_000, env, **kw)
    finally:
        capi.Context = orig
    return out, prof, made[0].plan_stats()


def equal(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x["mu"].shape == y["mu"].shape and x["S"].shape == y["S"].shape
        assert np.abs(x["mu"] - y["mu"]).max() == 0, f"batch {i}: mu differs by {np.abs(x['mu'] - y['mu']).max()}"
        assert np.abs(x["S"] - y["S"]).max() == 0, f"batch {i}: Sigma differs by {np.abs(x['S'] - y['S']).max()}"
        assert np.array_equal(x["ids"], y["ids"]), f"batch {i}: landmark ids differ"
        assert len(x["obs"]) == len(y["obs"])
        for p, q in zip(x["obs"], y["obs"]):
            assert np.array_equal(p, q), f"batch {i}: pop list differs"
        assert np.array_equal(x["stats"], y["stats"]), f"batch {i}: per-slot statistics differ"


def fused_against_split(name):
    _, kw, windows, hand_overs = HAND[name]
    frames = frames_of(name)
    fused, prof, plan = run_with_plan(frames, {}, **kw)
    split, prof2, plan2 = run_with_plan(frames, {"ASLAM_WIN_NEXT_SPLIT": "1"}, **kw)
    print(name, "plan", plan, "k_ekf_win_next", prof["k_ekf_win_next"][0], "k_ekf_win_step", prof["k_ekf_win_step"][0])
    assert plan == plan2 and prof["k_ekf_win_next"][0] == prof2["k_ekf_win_next"][0] and prof["k_ekf_win_step"][0] == prof2["k_ekf_win_step"][0]
    assert plan["frames_device_planned"] == 0
    assert plan["windows"] == windows, plan
    assert prof["k_ekf_win_next"][0] == hand_overs, "k_ekf_win_next must run once per hand-over"
    assert prof["k_ekf_win_step"][0] == plan["windows"]             # one launch per window
    equal(fused, split)
    return fused


@pytest.mark.parametrize("name", sorted(HAND))
def test_fused_hand_over_equals_the_four_launches(name):
    fused_against_split(name)


@pytest.mark.parametrize("name", ["64_128_64", "192_192_64"])
def test_hand_over_across_widths_equals_waiting_for_the_flush(name):
    """the image the fused kernel leaves is what the flush would have left in Sigma (ASLAM_WIN_NO_EARLY: every window waits for
    its own flush and loads P from Sigma): to rounding, as in test_ekf_window.py"""
    _, kw, _, _ = HAND[name]
    frames = frames_of(name)
    early, _, _ = run_with_plan(frames, {}, **kw)
    late, prof, _ = run_with_plan(frames, {"ASLAM_WIN_NO_EARLY": "1"}, **kw)
    assert prof["k_ekf_win_next"][0] == 0
    for x, y in zip(early, late):
        assert np.allclose(x["mu"], y["mu"], rtol=1e-10, atol=1e-12) and np.abs(x["S"] - y["S"]).max() <= 1e-10 * np.abs(y["S"]).max()


# `empty_frame` has two predicts back to back: the observations fetched during the first are consumed one step later
PREDICT_CASES = {
    "cfg2_like_64_wide": ONE_CASES["cfg2_like_64_wide"],
    "stationary_inside": CASES["stationary_inside"],
    "subset_frames": CASES["subset_frames"],
    "empty_frame": CASES["empty_frame"],
}


@pytest.mark.parametrize("name", sorted(PREDICT_CASES))
def test_one_launch_bookkeeping_equals_the_piece_schedule(name):
    compare(PREDICT_CASES[name], batch=10_000)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_fused_hand_over_equals_the_four_launches_on_gpu(name):
    fused_against_split(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PREDICT_CASES))
def test_one_launch_bookkeeping_equals_the_piece_schedule_on_gpu(name):
    compare(PREDICT_CASES[name], batch=10_000)
