"""How the window chain's worker waves publish the landmark rows of the step after next (aruco_slam_amd/csrc/ekf_window.hip:
win_publish_at and the worker loop of win_chain_role).  Two forms, each a bit of ASLAM_WIN_WORKER_PUBLISH (read at context
creation; 0 is the comparison path, the form the workers had before; unset, every width runs its own default):
  1  the published rows are stored packed (column 16 t + li at element 32 (t >> 1) + 2 li + (t & 1) of its 64-column chunk), written 16
     bytes at a time, and read by the prepare wave at a lane offset of its own;
  2  the workers read the step table's entry a phase ahead.
None of them changes an operand or the order of a floating-point operation, so every case asserts
  - that each form alone (1, 2), both together (3) and the defaults (unset) leave IDENTICAL BYTES to the comparison path after every call: mu, Sigma,
    landmark ids, pop lists, slot statistics (the gated window: also the slot health records and the track record);
  - that the default equals the numpy literal transcription of the reference (oracle/ekf_literal.py; the gated window: the gated
    transcription of tests/slam_gate_reference.py) at the 1e-9 of tests/test_ekf_window.py;
  - that the window error word is 0 after every call (run() checks it) and that the windows the case is built for are formed.
The piece schedule (ASLAM_WIN_PIECE) runs the same worker loop and the same rows: two cases repeat the comparison under it.

What the cases are built on.  A correction at position pos of the window's set S publishes rows p = 3 + 3 pos .. p + 2 of the
image; tile row g = row >> 4 belongs to worker g >> 1 (two tile rows per worker at every width, so no worker owns fewer), the lanes
that write a row are chosen by row & 3, the accumulator register by (row >> 2) & 3, and the instance of the switch by p & 15.
  - 16 landmarks, all fused: pos = 0 .. 15 gives every value of p mod 16; pos = 4 is p = 15 (rows 15, 16, 17: both tile rows of worker
    0) and pos = 9 is p = 30 (rows 30, 31, 32: workers 0 and 1).  A second frame fuses a subset, so that a position is followed by
    one of another tile row and of another worker.
  - 23 landmarks (128 wide): pos = 20 is p = 63 (workers 1 and 2), pos = 21, 22 are rows past column 64 (the second chunk of the
    packed row; the prepare wave's second read).
  - 63 landmarks, 63 corrections per frame (192 wide, six workers, three chunks).
  - windows that begin with two empty frames, have one in the middle or end with one: nothing is published for a predict, and the
    entry read ahead is a predict's; m = 1 in a window of two frames (every publication is followed by none); m = 4, 1, 3 in a row;
    three windows handed over in a row (the first publication of a window is made in front of its loop); a window of 64 frames.
A window never spans calls and a lone frame goes to the per-frame chain, so the smallest window has two frames; the first call of
every case adds the landmarks."""
import functools

import pytest

from test_ekf_window import make_case, run_device
from test_ekf_window_logger_mean import CASES as LOGGER_CASES, gated_case
from test_ekf_window_one_launch import run

KNOB = "ASLAM_WIN_WORKER_PUBLISH"
FORMS = ("1", "2", "3", None)         # each form alone, both together, every width's default (the knob unset)
R = lambda a, b: list(range(a, b))  # noqa: E731

# name: ((seed, groups, n_land), batch, windows, hand-overs (k_ekf_win_next launches), context arguments)
CASES = {
    # calls of two frames: the first adds the 16 landmarks, the second is a window of all 16 positions and then a subset of them
    # (pos 0, 4, 5, 9, 10, 15: tile rows 0, 0 / 1, 1, 1 / 2, 2, 3), the third a window that starts on the subset
    "sixteen_positions": ((71, [(3, R(0, 16), False), (1, [0, 4, 5, 9, 10, 15], False), (1, [4, 9, 15], False), (1, R(0, 16), False)], 16),
                          2, 2, 0, {}),
    "p_63_and_past_64_128_wide": LOGGER_CASES["rows_past_64_128_wide"],
    "m_63_192_wide": LOGGER_CASES["m_63_192_wide"],
    "empty_frames": LOGGER_CASES["empty_frames"],
    "m_1": LOGGER_CASES["m_1"],
    "m_4_1_3": LOGGER_CASES["m_4_1_3"],
    "windows_in_a_row": LOGGER_CASES["windows_in_a_row"],
    "frames_64": LOGGER_CASES["frames_64"],
}
# under the piece schedule: pieces of one frame (every piece's first publication is made in front of its loop) and of three
PIECE_CASES = {"sixteen_positions": "1", "empty_frames": "3", "p_63_and_past_64_128_wide": "3"}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the frames and the literal transcription's state after each of them: computed once per case"""
    return make_case(*CASES[name][0])


def identical(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for k in ("mu", "S", "ids", "stats"):
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), f"{what}, call {i}: {k} differs"
        assert len(x["obs"]) == len(y["obs"])
        for p, q in zip(x["obs"], y["obs"]):
            assert p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes(), f"{what}, call {i}: the pop list differs"


def check(name):
    _, batch, windows, hand_overs, kw = CASES[name]
    frames, exp = reference(name)
    old, prof0 = run(frames, batch, {KNOB: "0"}, **kw)
    assert prof0["k_ekf_win_step"][0] == windows and prof0["k_ekf_win_next"][0] == hand_overs, \
        f"{prof0['k_ekf_win_step'][0]} windows, {prof0['k_ekf_win_next'][0]} hand-overs: the case is built for {windows}, {hand_overs}"
    for form in FORMS:
        new, prof = run(frames, batch, {} if form is None else {KNOB: form}, **kw)
        assert prof["k_ekf_win_step"][0] == windows and prof["k_ekf_win_next"][0] == hand_overs
        identical(new, old, f"{name}, form {form}")
    _, prof, worst = run_device(frames, exp, batch=batch, **kw)      # the default: every call's last frame against the literal transcription
    print(f"{name}: worst relative Sigma error against the literal transcription {worst:.2e}")
    assert prof["k_ekf_win_step"][0] == windows and worst <= 1e-9


def check_pieces(name):
    _, batch, windows, _, kw = CASES[name]
    frames, _ = reference(name)
    piece = {"ASLAM_WIN_PIECE": PIECE_CASES[name]}
    old, prof0 = run(frames, batch, dict(piece, **{KNOB: "0"}), **kw)
    assert prof0["k_ekf_win_step"][0] > windows, "the windows were not cut into pieces"
    for form in FORMS:
        new, prof = run(frames, batch, dict(piece) if form is None else dict(piece, **{KNOB: form}), **kw)
        assert prof["k_ekf_win_step"][0] == prof0["k_ekf_win_step"][0]
        identical(new, old, f"{name}, pieces of {PIECE_CASES[name]}, form {form}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_worker_publish(name):
    check(name)


@pytest.mark.parametrize("name", sorted(PIECE_CASES))
def test_worker_publish_pieces(name):
    check_pieces(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_worker_publish_on_gpu(name):
    check(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PIECE_CASES))
def test_worker_publish_pieces_on_gpu(name):
    check_pieces(name)


# ---- a gated window that rejects steps ------------------------------------------------------------------------------------------------
# Sequence and reference of tests/test_ekf_window_logger_mean.py ("quarter_64_wide": every fourth correction of the window is an
# outlier at gate_d2 = 1).  A rejected step is a step with zero A operand rows: the rows published around it must not move.
def gated_bits(c, form, monkeypatch):
    import test_slam_gate_windows as gw
    if form is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, form)
    run_ = gw.Run(c["mu"], c["S"], c["ids"], c["frames"], gate=gw.GATE, cap=c["cap"], ML=len(c["ids"]))
    res = run_.results()
    assert res["prof"]["k_ekf_win_step"][0] == 1 and res["prof"][gw.WIN_FINISH][0] == 1
    mu, S = res["state"]
    bits = dict(mu=mu.tobytes(), S=S.tobytes(), ids=res["ids"].tobytes(), stats=res["stats"].tobytes(), health=res["health"].tobytes(),
                track=res["track"].tobytes(), pops={f: p.tobytes() for f, p in run_.pops.items()})
    return run_, res, bits


def check_gated(monkeypatch):
    import test_slam_gate_windows as gw
    c = gated_case("quarter_64_wide")
    _, _, old = gated_bits(c, "0", monkeypatch)
    for form in FORMS:
        run_, res, new = gated_bits(c, form, monkeypatch)
        for k in old:
            assert new[k] == old[k], f"gated window, form {form or 'default'}: {k} differs from the comparison path"
    gw.check_against_reference(run_, c["lit"], c["per"], "quarter_64_wide")      # the default: 1e-9, every discrete result exactly
    assert int(res["health"]["rejected"].sum()) == c["n_out"] > 0


def test_worker_publish_gated(monkeypatch):
    check_gated(monkeypatch)


@pytest.mark.gpu
def test_worker_publish_gated_on_gpu(monkeypatch):
    check_gated(monkeypatch)
