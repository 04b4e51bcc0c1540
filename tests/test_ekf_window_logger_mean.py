"""The logger wave's share of a correction (aruco_slam_amd/csrc/ekf_window.hip, win_chain_role with ONE = true): in the one-launch
window the logger wave forms the log header's S^-1 itself, from the step's c rows in LDS and the frame's records, and carries mu_S:
it applies mu += K ze per accepted correction (K = the negated A operand), takes a predict's pose from the prepare wave and hands
its mean to the prepare wave for every predict, which adds the one step the logger has not seen yet.  The prepare wave's own form
(it writes S^-1 into the header buffer and carries the mean) stays selectable at context creation: ASLAM_WIN_LOGGER_PARTS = 0; 1 and
2 move one of the two parts alone.  Both forms use the same expressions on the same inputs, so every case asserts
  - that everything the filter leaves behind after every call is EQUAL TO THE BIT between the default and the comparison path, and
    between each part alone and the comparison path: mu, Sigma, landmark ids, pop lists, slot statistics (gated cases: also the
    slot health records and the track record);
  - that the default path equals the numpy literal transcription of the reference (oracle/ekf_literal.py; gated cases: the gated
    transcription of tests/slam_gate_reference.py) at the 1e-9 of tests/test_ekf_window.py;
  - that the window error word is 0 after every call (run() and sync check it) and that the windows the case is built for are formed.
The cases are the smallest shapes at which the two hand-overs of the mean (logger -> prepare wave at a predict, pose -> logger) and
the logger's S^-1 inputs (landmark row, R records, the frame's cos / sin) can go wrong.  A window never spans calls and the planner
gives a lone eligible frame to the per-frame chain (win_plan.h, close_window), so the smallest window has two frames: "the frame's
last correction is its first" is a window of two frames with one correction each.  The first call of every case adds the landmarks."""
import functools

import numpy as np
import pytest

from test_ekf_window import make_case, run_device
from test_ekf_window_handover import equal
from test_ekf_window_one_launch import ONE_CASES, run
from test_ekf_window_stepctl import STEPCTL_CASES

KNOB = "ASLAM_WIN_LOGGER_PARTS"
R = lambda a, b: list(range(a, b))  # noqa: E731

# name: ((seed, groups, n_land), batch, windows, hand-overs (k_ekf_win_next launches), context arguments)
CASES = {
    # calls of three frames.  Call 2 is a window that BEGINS with two empty frames (the logger's mean for step 1 is written before
    # any step; two predicts in a row: the pose hand-over's parity, the mean row's parity), call 3 has an empty frame in the
    # middle, call 4 ends with one (the window's last step is a lone predict: the mean image takes its pose)
    "empty_frames": ((61, [(3, [0, 1, 2], False), (2, [], False), (1, [0, 1, 2], False), (1, [0, 1, 2], False), (1, [], False), (1, [0, 2], False),
                           (1, [0, 1], False), (1, [2], False), (1, [], False)], 3), 3, 4, 0, {}),
    # two frames with one correction each: the frame's last correction is its first, every correction is followed by a predict
    "m_1": ((62, [(2, [0, 1], False), (2, [1], False)], 2), 2, 1, 0, {}),
    "m_4_1_3": STEPCTL_CASES["m_4_1_3"][:3] + (0, {}),
    "stationary_inside": STEPCTL_CASES["stationary_inside"][:3] + (0, {}),
    # positions in S that are not the correction's index (lrow from the step table), every marker with an R of its own
    "subsets_distinct_R": STEPCTL_CASES["non_contiguous_subsets"][:3] + (0, {}),
    # 63 corrections per frame on the 192-wide image (three chunks of the mean; record lane 62), and the 128-wide image with
    # landmark rows in the second chunk
    "m_63_192_wide": STEPCTL_CASES["correction_limit_192_wide"][:3] + (0, STEPCTL_CASES["correction_limit_192_wide"][3]),
    "rows_past_64_128_wide": STEPCTL_CASES["two_frames_128_wide"][:3] + (0, {}),
    # a window of 64 frames (the frame left over goes to the per-frame chain)
    "frames_64": (ONE_CASES["frames_64"], 10_000, 1, 0, {}),
    # three windows in a row on different sets, handed over window to window: k_ekf_win_next reads the mean image the logger wrote
    # (sets of 20 landmarks fill the 64-wide image: a window of 16 frames or more is closed rather than widened to take the next
    # set), and k_ekf_win_fix puts it back into the state
    "windows_in_a_row": ((63, [(1, R(0, 11), False), (1, R(11, 22), False), (16, R(0, 20), False), (16, R(2, 22), False), (3, [0, 1], False)], 22),
                         10_000, 3, 2, {}),
    # 30 landmarks with 4 of them in S: Sigma[R, R] and mu_R depend on the logged S^-1 through the replay
    "large_state": ((64, [(1, R(0, 15), False), (1, R(15, 30), False), (4, [3, 11, 18, 27], False)], 30), 10_000, 1, 0, {}),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the frames and the literal transcription's state after each of them: computed once per case"""
    return make_case(*CASES[name][0])


def check(name):
    _, batch, windows, hand_overs, kw = CASES[name]
    frames, exp = reference(name)
    if name == "subsets_distinct_R":
        for fr in frames:
            rs = [tuple(np.diag(o["R"])) for o in fr["obs"]]
            assert len(set(rs)) == len(rs), "the case is built on a different R for every marker of a frame"
    old, prof0 = run(frames, batch, {KNOB: "0"}, **kw)
    for parts in ("3", "1", "2"):
        new, prof = run(frames, batch, {KNOB: parts} if parts != "3" else {}, **kw)
        assert prof["k_ekf_win_step"][0] == windows and prof["k_ekf_win_next"][0] == hand_overs, \
            f"{prof['k_ekf_win_step'][0]} windows, {prof['k_ekf_win_next'][0]} hand-overs: the case is built for {windows}, {hand_overs}"
        equal(new, old)
    assert prof0["k_ekf_win_step"][0] == windows
    _, prof, worst = run_device(frames, exp, batch=batch, **kw)      # every call's last frame against the literal transcription at 1e-9
    print(f"{name}: worst relative Sigma error against the literal transcription {worst:.2e}")
    assert prof["k_ekf_win_step"][0] == windows and worst <= 1e-9


@pytest.mark.parametrize("name", sorted(CASES))
def test_logger_mean(name):
    check(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_logger_mean_on_gpu(name):
    check(name)


# ---- gated windows -------------------------------------------------------------------------------------------------------------------
# Sequences and references as in tests/test_slam_gate_windows.py (gate_d2 = 1; an outlier is a true sighting displaced by OUTLIER; the
# reference alone is asserted to reject exactly the planted sightings, with margins).  Every fourth correction of the window is an
# outlier, about a quarter of its steps.  name: (landmarks, frames, updates per frame, a NaN z[0] at (window frame, position) or None)
GATED = {
    "quarter_64_wide": (5, 6, 24, None),
    "quarter_and_nan_64_wide": (5, 6, 24, (2, 0)),
    "quarter_and_nan_128_wide": (25, 3, 64, (1, 23)),
}


@functools.lru_cache(maxsize=None)
def gated_case(name):
    import test_slam_gate_windows as gw
    L, K, cap, nan = GATED[name]
    rng = np.random.RandomState(700 + sorted(GATED).index(name))
    mu, S = gw.random_state(rng, L, heading=0.4)
    ids = rng.permutation(gw.ID_TABLE)[:L].astype(np.int32)
    out = {(j // L, j % L) for j in range(1, K * L, 4)}
    assert nan is None or nan not in out
    plan = [([], set())] + [(list(range(L)), {a for k, a in out if k == f}) for f in range(K)]
    frames, marks = gw.make_frames(rng, mu, ids, plan, nan=set() if nan is None else {(1 + nan[0], nan[1])})
    gw.assert_repeats_decidable(frames)
    lit, per = gw.reference(mu, S, ids, frames, marks=marks)
    return dict(mu=mu, S=S, ids=ids, frames=frames, lit=lit, per=per, n_out=len(out) + (nan is not None), cap=cap)


def gated_results(c, gate, parts, monkeypatch):
    """a gated context on the case (the knob is read at context creation): everything it leaves behind, as bytes where floats may be NaN"""
    import test_slam_gate_windows as gw
    if parts is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, parts)
    run_ = gw.Run(c["mu"], c["S"], c["ids"], c["frames"], gate=gate, cap=c["cap"], ML=len(c["ids"]))
    res = run_.results()
    assert res["prof"]["k_ekf_win_step"][0] == 1 and res["prof"][gw.WIN_FINISH][0] == 1
    mu, S = res["state"]
    bits = dict(mu=mu.tobytes(), S=S.tobytes(), ids=res["ids"].tobytes(), stats=res["stats"].tobytes(), health=res["health"].tobytes(),
                track=res["track"].tobytes(), pops={f: p.tobytes() for f, p in run_.pops.items()})
    return run_, res, bits


def check_gated(name, monkeypatch):
    import test_slam_gate_windows as gw
    c = gated_case(name)
    gates = (gw.GATE,) if GATED[name][3] is not None else (gw.GATE, gw.INF)      # (at +inf a NaN sighting would be fused)
    for gate in gates:
        _, _, old = gated_results(c, gate, "0", monkeypatch)
        for parts in (None, "1", "2"):
            run_, res, new = gated_results(c, gate, parts, monkeypatch)
            for k in old:
                assert new[k] == old[k], f"{name}, gate {gate}, parts {parts or 3}: {k} differs from the comparison path"
            if parts is None and gate == gw.GATE:
                gw.check_against_reference(run_, c["lit"], c["per"], name)      # 1e-9, every discrete result exactly
                assert int(res["health"]["rejected"].sum()) == c["n_out"]
            if parts is None and gate == gw.INF:
                assert int(res["health"]["rejected"].sum()) == 0


@pytest.mark.parametrize("name", sorted(GATED))
def test_logger_mean_gated(name, monkeypatch):
    check_gated(name, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GATED))
def test_logger_mean_gated_on_gpu(name, monkeypatch):
    check_gated(name, monkeypatch)
