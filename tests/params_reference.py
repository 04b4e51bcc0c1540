"""Filter parameters away from the defaults of aslam_init, the motions at which a predict can go wrong, and the mutants that show a
case set can tell a wrong predict from the right one (a plain helper module, imported by tests/test_filter_params.py).

The device holds three hand-written copies of the reference's addEncoder (aruco_slam.cpp:35-73): predict_block (ekf.hip), the prepare
wave of the window chain (ekf_window.hip) and loc_steps (ekf_localize.h).  At kl == kr a whole class of mistakes in them changes no
bit of any result, so the cases here use

    A   kl 0.03   kr 0.08   b 0.2    Q_k 0.5
    B   kl 0.11   kr 0.04   b 0.05   Q_k 0.2

beside the defaults as the control.  predict_terms is the predict written once more, with one formula changed on request:

    swap_k       kl <-> kr in the arc lengths delta_sl / delta_sr
    kr_noise     kr in the noise's second column (the reference uses kl for both wheels, quirk Q7)
    2b_noise     2 b for b in the noise's heading row
    b_dtheta     b for 2 b in delta_theta
    Qk_default   Q_k at its default

The mutant classes run the project's references (LiteralSlam, GatedLiteralSlam, FrozenMapLocalizer, GatedLocalizer,
UncertainMapLocalizer) with that predict.  No tolerance is taken from them: moved() measures how far a mutant moves a reference's
result, and a case set must move by FLOOR = 1e-6, a thousand times the 1e-9 the device is held to."""
import math

import numpy as np

from ekf_reference import LD, rel_err, reference_step, wrap_once
from oracle.ekf_literal import LiteralSlam
from slam_gate_reference import GatedLiteralSlam
from tests.gate_reference import GatedLocalizer
from tests.test_localize import FrozenMapLocalizer
from tests.umap_reference import UncertainMapLocalizer

DEFAULTS = dict(kl=0.05, kr=0.05, b=0.09, Q_k=0.01)
SETS = {"defaults": DEFAULTS,
        "A": dict(kl=0.03, kr=0.08, b=0.2, Q_k=0.5),
        "B": dict(kl=0.11, kr=0.04, b=0.05, Q_k=0.2)}
MUTANTS = ("swap_k", "kr_noise", "2b_noise", "b_dtheta", "Qk_default")
FLOOR = 1e-6                                        # what a mutant must move a reference's result by
AGREE = 1e-12                                       # double against long double form of a reference
HEADINGS = (math.pi - 0.0009, -math.pi + 0.0009)   # the predict wraps the first downwards under a left turn, the second upwards

# (wl, wr, dt)
MOTIONS = {
    "forward": (2.0, 2.3, 0.1),
    "reverse": (-3.0, -1.5, 0.1),
    "spin": (2.5, -2.5, 0.08),                      # delta_s != 0 only because kl != kr
    "left_only": (4.0, 0.0, 0.1),                   # blind to a kr in the second noise column; right_only is not
    "right_only": (0.0, 4.0, 0.1),
    "standstill": (0.0, 0.0, 0.05),
}
LARGE_TURN = (40.0, -35.0, 0.5)                     # under B: delta_theta = -29, the single wrap leaves the heading near -19.6


def straight(p, dt=0.1):
    """wheel speeds with kl (dt wl) == kr (dt wr) in double, wl != wr unless kl == kr: delta_theta = 0 exactly"""
    if p["kl"] == p["kr"]:
        return (2.5, 2.5, dt)
    for k in range(8, 40):                          # wl = 2, 2.25, ...: wr = the double next to kl wl / kr at which the products are equal
        wl = k / 4.0
        wr = p["kl"] * wl / p["kr"]
        for cand in (wr, np.nextafter(wr, 0.0), np.nextafter(wr, 99.0)):
            if p["kl"] * (dt * wl) == p["kr"] * (dt * float(cand)):
                return (wl, float(cand), dt)
    raise AssertionError("no exactly straight pair of wheel speeds")


def motions(name):
    """the motions a case under parameter set `name` cycles through, by name"""
    m = dict(MOTIONS, straight=straight(SETS[name]))
    if name == "B":
        m["large_turn"] = LARGE_TURN
    return m


def cycle(name, n, start=0, skip=("standstill",)):
    """n motions (wl, wr, dt) of the set's cycle, from position `start` on"""
    seq = [v for k, v in motions(name).items() if k not in skip]
    return [seq[(start + i) % len(seq)] for i in range(n)]


def ctx_params(name):
    """the set as keyword arguments of capi.Context / LiteralSlam / FrozenMapLocalizer"""
    return dict(SETS[name])


def step_params(name):
    """the set as keyword arguments of reference_step / gated_reference_step / predicted_pose"""
    p = SETS[name]
    return dict(kl=p["kl"], kr=p["kr"], b=p["b"], Qk=p["Q_k"])


def predict_terms(th0, wl, wr, dt, p, mutant=None, dtype=LD):
    """addEncoder's quantities at heading th0: (delta_s, delta_theta, cos, sin of the mid-step heading, Q 3 x 3)"""
    assert mutant is None or mutant in MUTANTS
    T = dtype
    kl, kr, b, Qk = T(p["kl"]), T(p["kr"]), T(p["b"]), T(p["Q_k"])
    wl, wr, dt = T(wl), T(wr), T(dt)
    if mutant == "swap_k":
        dsl, dsr = kr * (dt * wl), kl * (dt * wr)
    else:
        dsl, dsr = kl * (dt * wl), kr * (dt * wr)
    dth = (dsr - dsl) / (b if mutant == "b_dtheta" else 2 * b)
    ds = (dsr + dsl) / 2
    th = T(th0) + dth / 2
    c, s = np.cos(th), np.sin(th)
    f0 = kl * dt / 2
    f1 = (kr if mutant == "kr_noise" else kl) * dt / 2
    bn = 2 * b if mutant == "2b_noise" else b
    if mutant == "Qk_default":
        Qk = T(DEFAULTS["Q_k"])
    wkh = np.array([[f0 * c, f1 * c], [f0 * s, f1 * s], [f0 / bn, -f1 / bn]], dtype=T)
    Q = wkh @ np.diag(np.array([Qk * abs(wl), Qk * abs(wr)], dtype=T)) @ wkh.T
    return ds, dth, c, s, Q


def dense_predict(mu, S, wl, wr, dt, p, mutant=None, dtype=LD):
    """the predict on a dense state (copies): Sigma <- Hx Sigma Hx^T + F Q F^T by rows, then columns"""
    mu = np.array(mu, dtype=dtype); S = np.array(S, dtype=dtype)
    ds, dth, c, s, Q = predict_terms(mu[2], wl, wr, dt, p, mutant, dtype)
    mu[0] += ds * c; mu[1] += ds * s
    mu[2] = wrap(mu[2] + dth, dtype)
    f02, f12 = -ds * s, ds * c
    S[0, :] += f02 * S[2, :]; S[1, :] += f12 * S[2, :]
    S[:, 0] += f02 * S[:, 2]; S[:, 1] += f12 * S[:, 2]
    S[:3, :3] += Q
    return mu, S


def wrap(a, dtype=LD):
    """one wrap around the double value of pi (aruco_slam.cpp:412-421), in dtype"""
    if dtype is LD:
        return wrap_once(a)
    if a >= math.pi:
        a -= 2 * math.pi
    if a < -math.pi:
        a += 2 * math.pi
    return a


def step(mu, S, wl, wr, dt, obs, p, mutant=None, dtype=LD):
    """reference_step with the predict of predict_terms: the predict here, the corrections by reference_step"""
    mu, S = dense_predict(mu, S, wl, wr, dt, p, mutant, dtype)
    return reference_step(mu, S, 0.0, 0.0, 0.0, obs, dtype=dtype, predict=False)


def _literal_family(base):
    class Mutant(base):
        """add_encoder with the predict of predict_terms in double; mutant = None is the class itself to rounding"""

        def __init__(self, *a, mutant=None, **kw):
            super().__init__(*a, **kw)
            self.mutant = mutant

        def add_encoder(self, wl, wr, t_now):
            if not self.is_init:
                self.last_time, self.is_init = t_now, True
                return
            dt = t_now - self.last_time
            self.last_time = t_now
            p = dict(kl=self.kl, kr=self.kr, b=self.b, Q_k=self.Q_k)
            self.mu, self.sigma = dense_predict(self.mu, self.sigma, wl, wr, dt, p, self.mutant, np.float64)
    return Mutant


def _localizer_family(base):
    class Mutant(base):
        def __init__(self, *a, mutant=None, **kw):
            super().__init__(*a, **kw)
            self.mutant = mutant

        def predict(self, wl, wr, dt):
            p = dict(kl=self.kl, kr=self.kr, b=self.b, Q_k=self.Q_k)
            if isinstance(self, UncertainMapLocalizer):
                self.x, S = dense_predict(self.x, self.S, wl, wr, dt, p, self.mutant, self.dtype)
                self.S[:] = S
            else:
                self.mu, self.P = dense_predict(self.mu, self.P, wl, wr, dt, p, self.mutant, np.float64)
    return Mutant


MutantLiteral = _literal_family(LiteralSlam)
MutantGatedLiteral = _literal_family(GatedLiteralSlam)
MutantFrozen = _localizer_family(FrozenMapLocalizer)
MutantGated = _localizer_family(GatedLocalizer)
MutantUncertain = _localizer_family(UncertainMapLocalizer)


def moved(mu, S, mu_ref, S_ref):
    """how far (mu, Sigma) lies from a reference's: the larger of max |d mu| and max |d Sigma| / max |Sigma|; a result of another
    size (a mutant that changed a discrete decision) counts as moved without bound"""
    if np.shape(mu) != np.shape(mu_ref):
        return math.inf
    d = max(float(np.abs(np.asarray(mu, LD) - np.asarray(mu_ref, LD)).max()), rel_err(S, S_ref))
    return math.inf if math.isnan(d) else d


def agree(mu, S, mu_ref, S_ref, where):
    """the double form of a reference against its long-double form: the case is well conditioned"""
    assert np.shape(mu) == np.shape(mu_ref)
    e_mu, e_S = float(np.abs(np.asarray(mu, LD) - np.asarray(mu_ref, LD)).max()), rel_err(S, S_ref)
    assert e_mu <= AGREE and e_S <= AGREE, f"{where}: the double reference is {e_mu} (mu), {e_S} (Sigma, relative) from the long-double one"
    return e_mu, e_S


def check_floor(path, per_mutant):
    """per_mutant: {mutant: [moved() of every case of the path]}.  Every mutant must move at least one case by FLOOR."""
    assert set(per_mutant) == set(MUTANTS), f"{path}: mutants {sorted(per_mutant)}"
    for m, ds in per_mutant.items():
        assert ds and max(ds) >= FLOOR, f"{path}: no case tells the mutant {m} from the reference (moves {ds})"
    return {m: max(ds) for m, ds in per_mutant.items()}


def augment(mu, S, pose, z, Rd, dtype=LD):
    """a new landmark from the observation z at the frame-start pose (aruco_slam.cpp:208-260; its sine and cosine are floats)"""
    T = dtype
    z = np.array(z, dtype=T)
    sn, cs = T(np.float32(np.sin(pose[2]))), T(np.float32(np.cos(pose[2])))
    mx, my = pose[0] + cs * z[0] - sn * z[1], pose[1] + sn * z[0] + cs * z[1]
    dx, dy = mx - pose[0], my - pose[1]
    Gsk = np.array([[-cs, -sn, -sn * dx + cs * dy], [sn, -cs, -dx * cs - dy * sn], [0, 0, -1]], dtype=T)
    Gmi = np.array([[cs, sn, 0], [-sn, cs, 0], [0, 0, 1]], dtype=T)
    N = mu.size
    S2 = np.zeros((N + 3, N + 3), dtype=T)
    S2[:N, :N] = S
    S2[N:, :N] = -Gmi @ Gsk @ S[:3, :]
    S2[:N, N:] = S2[N:, :N].T
    S2[N:, N:] = Gmi @ (Gsk @ S[:3, :3] @ Gsk.T + np.diag(np.array(Rd, dtype=T))).T @ Gmi.T
    return np.concatenate([mu, np.array([mx, my, wrap(pose[2] + z[2], T)], dtype=T)]), S2


def slam_frame(mu, S, wl, wr, dt, new, known, p, mutant=None, dtype=LD, arm=False):
    """one SLAM frame in pop order: the predict (none for the arming sample), the new landmarks new = [(z, Rdiag)], then the
    corrections known = [(index, z, Rdiag)], every one of them at the mean the predict left (quirk Q1)"""
    mu = np.array(mu, dtype=dtype); S = np.array(S, dtype=dtype)
    if not arm:
        mu, S = dense_predict(mu, S, wl, wr, dt, p, mutant, dtype)
    pose = mu[:3].copy()
    for z, Rd in new:
        mu, S = augment(mu, S, pose, z, Rd, dtype)
    return reference_step(mu, S, 0.0, 0.0, 0.0, known, dtype=dtype, predict=False)


def replay_make_case(frames, exp, p, mutant=None, dtype=LD):
    """the frames of tests/test_ekf_window.make_case through slam_frame, in the pop order and with the branches the literal
    transcription logged (its observations depend on no state); the first sample arms the filter"""
    mu, S = np.zeros(3, dtype=dtype), np.zeros((3, 3), dtype=dtype)
    t = None
    for fr, e in zip(frames, exp):
        by_id = {int(i): o for i, o in zip(fr["ids"], fr["obs"])}
        new = [(by_id[int(i)]["z"], np.diag(by_id[int(i)]["R"])) for i, _, a in e["log"] if a == 0]
        known = [(int(x), by_id[int(i)]["z"], np.diag(by_id[int(i)]["R"])) for i, x, a in e["log"] if a == 1]
        mu, S = slam_frame(mu, S, fr["wl"], fr["wr"], 0.0 if t is None else fr["t"] - t, new, known, p, mutant, dtype, arm=t is None)
        t = fr["t"]
    return mu, S
