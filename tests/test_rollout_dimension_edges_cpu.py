"""The inputs of tests/test_gpu_rollout_dimension_edges.py, judged from the oracle alone (no GPU).

That module holds the fused roll-out to the oracle at the edges of the dimension sets it accepts (csrc/rollout_plugin.hip
rollout_plugin_dims: n = 2, L in 2..44, N in 2..40, q in {1, 2, L}) and at two sets it refuses (L2q2, max); this one owns the case table, the inputs of every case and the
oracle's step, and proves that the inputs can carry such a comparison.  Every case: B = 32 trajectories (initial_states seed 3), 5 steps
from iteration 99 with the plant switch at 102, model = offline_edmd of the oracle's lift (set through set_model), the estimator started
afresh.
    MLP   random_mlp_weights(2, 100, 3, L, seed=5), Duffing plant, y = C x (q rows of C), box +-2, Rw = 1, r = [1; 0][:q]
    psi   the same lift, y = psi (q = L), box +-6, default weights, r = psi([1; 0])
    RBF   thin plates "rbf", L centres drawn from the Van der Pol offline samples (RandomState(0)), Van der Pol plant, y = C x, box +-2,
          Rw = 1, r = [1; 0]
(With the default Rw = 1e-4 every input sits at a bound in 50-85 % of the steps of the y = C x cases: they run with Rw = 1.)

Per-trajectory OracleController(rls="gain") free-running on the oracle's plant.  A step is LEFT OUT when cond(H) >= 1e9 or qp_exact does
not terminate: it has no minimiser to hold 1e-6 against (the controller then goes on with the clipped least-squares point).  Asserted
over the 160 trajectory-steps of every case:
    left out          at most 1/16 (MLP and psi cases), 1/8 (RBF cases)
    box active        some variable of the minimiser at a bound in at least 1/4 of the steps
    all at bounds     every variable at a bound in at most 1/2 of the steps

Measured here (printed by `python -m pytest tests/test_rollout_dimension_edges_cpu.py -s`), of 160:
    case     (L, N, q)      left out   box active   all at bounds
    N2       (8, 2, 2)      0          80           51
    N3       (8, 3, 2)      0          92           47
    N15      (9, 15, 2)     0          114          30
    N17      (8, 17, 2)     0          117          27
    N29      (12, 29, 2)    0          121          24
    N31      (12, 31, 2)    0          121          24
    v2max    (30, 32, 2)    1          118          23
    L2q1     (2, 6, 1)      0          108          53
    L2q2     (2, 6, 2)      0          95           33
    L29q1    (29, 17, 1)    0          132          43
    L31      (31, 12, 2)    0          112          31
    L31N24   (31, 24, 2)    1          114          20
    L31N25   (31, 25, 2)    1          116          21
    N33      (30, 33, 2)    1          118          22
    L33      (33, 16, 2)    0          112          37
    L44q1    (44, 12, 1)    0          121          49
    max      (44, 45, 2)    6          113          14
    max40    (44, 40, 2)    3          116          17
    psi9     (9, 11, 9)     0          92           37
    psi16    (16, 25, 16)   0          52           9
    psi31    (31, 13, 31)   0          75           29
    rbf23    (23, 33, 2)    8          134          25
    rbf24    (24, 33, 2)    9          133          24
"""
import functools

import numpy as np
import pytest

from oracle import koopman_oracle as ko

B, STEPS, STEP0, SWITCH = 32, 5, 99, 102
COND_MAX = 1e9  # as tests/test_gpu_round6.py's plug-in test: beyond, H is numerically singular

# id -> (L, N, q, kind); the edge each one straddles is named in tests/test_gpu_rollout_dimension_edges.py
CASES = {
    "N2": (8, 2, 2, "mlp"),
    "N3": (8, 3, 2, "mlp"),
    "N15": (9, 15, 2, "mlp"),
    "N17": (8, 17, 2, "mlp"),
    "N29": (12, 29, 2, "mlp"),
    "N31": (12, 31, 2, "mlp"),
    "v2max": (30, 32, 2, "mlp"),
    "L2q1": (2, 6, 1, "mlp"),
    "L2q2": (2, 6, 2, "mlp"),
    "L29q1": (29, 17, 1, "mlp"),
    "L31": (31, 12, 2, "mlp"),
    "L31N24": (31, 24, 2, "mlp"),
    "L31N25": (31, 25, 2, "mlp"),
    "N33": (30, 33, 2, "mlp"),
    "L33": (33, 16, 2, "mlp"),
    "L44q1": (44, 12, 1, "mlp"),
    "max": (44, 45, 2, "mlp"),
    "max40": (44, 40, 2, "mlp"),  # (the nearest set to `max` that runs fused: horizons above 40 are per-step launches)
    "psi9": (9, 11, 9, "psi"),
    "psi16": (16, 25, 16, "psi"),
    "psi31": (31, 13, 31, "psi"),
    "rbf23": (23, 33, 2, "rbf"),
    "rbf24": (24, 33, 2, "rbf"),
}
LEFT_OUT_CAP = {"mlp": 1.0 / 16.0, "psi": 1.0 / 16.0, "rbf": 1.0 / 8.0}
ACTIVE_MIN = 1.0 / 4.0
ALL_AT_BOUNDS_MAX = 1.0 / 2.0


class Inputs:
    """What a case hands to both sides: the lift, the offline model, the reference, the initial states, the controller options."""

    def __init__(self, case):
        from koopmpc.synth import duffing_rk4, initial_states, offline_data, offline_edmd, random_mlp_weights, vdp_rk4

        self.case = case
        self.L, self.N, self.q, self.kind = CASES[case]
        L, N, q = self.L, self.N, self.q
        self.weights = self.centres = None
        if self.kind == "rbf":
            Xo = offline_data(plant=vdp_rk4)[0]
            self.centres = Xo[:, np.random.RandomState(0).choice(Xo.shape[1], L, replace=False)].T.copy()
            self.lift = lambda x: ko.rbf_lift(x, self.centres)
            self.plant, offline_plant = "vdp", vdp_rk4
        else:
            self.weights = random_mlp_weights(2, 100, 3, L, seed=5)
            self.lift = lambda x: ko.mlp_lift(self.weights, x)
            self.plant, offline_plant = "duffing", duffing_rk4
        self.A0, self.B0, self.C0 = offline_edmd(self.lift, plant=offline_plant)
        if self.kind == "psi":
            assert q == L
            self.output, self.bound, self.weights_kw = "lift", 6.0, {}
            self.r = np.tile(self.lift(np.array([[1.0], [0.0]])), (1, N))
        else:
            assert q in (1, 2)
            self.output, self.bound, self.weights_kw = "Cx", 2.0, dict(Rw=1.0)
            self.r = np.tile(np.array([[1.0], [0.0]])[:q], (1, N))
        self.X0 = initial_states(B, seed=3)

    def handle_kw(self):
        """Keyword arguments of KoopmanMPC for this case."""
        kw = dict(n=2, L=self.L, N=self.N, batch=B, output=self.output, lb=-self.bound, ub=self.bound, **self.weights_kw)
        if self.kind == "rbf":
            kw.update(lift="rbf", centres=self.centres)
        else:
            kw.update(weights=self.weights)
        if self.output == "Cx" and self.q != 2:
            kw.update(out_rows=self.q, out_row0=0)
        return kw

    def controller(self):
        return ko.OracleController(self.lift, self.L, 2, self.N, -self.bound, self.bound, self.A0, self.B0, self.C0, rls="gain",
                                   output=self.output, **self.weights_kw)

    def switched(self, k):
        return STEP0 + k >= SWITCH


@functools.lru_cache(maxsize=None)
def inputs_of(case):
    return Inputs(case)


def oracle_qp(inp, ctl, x):
    """The oracle's step up to the QP: lift, the gain-form update with the transition that ended in x (ctl.prev), condense.
    Returns (psi, H, f, U): U the exact minimiser, or None where the step is left out."""
    psi = inp.lift(np.reshape(x, (2, 1))).reshape(-1)
    if ctl.prev is not None:
        ppsi, pu = ctl.prev
        ctl.gK, ctl.gP = ko.rls_update_gain(ctl.gK, ctl.gP, np.concatenate([ppsi, [pu]]), psi)
        ctl.gC, ctl.gQ = ko.rls_update_gain(ctl.gC, ctl.gQ, ppsi, np.reshape(x, -1))
        ctl.A, ctl.B, ctl.C = ctl.gK[:, :-1].copy(), ctl.gK[:, -1:].copy(), ctl.gC.copy()
    Co = None if inp.output == "lift" else ctl.C[:inp.q]
    _, _, H, f, _ = ko.condense(ctl.A, ctl.B, Co, psi, inp.r, inp.N, ctl.Qw, ctl.Rw)
    U = None
    if np.isfinite(H).all() and np.linalg.cond(H) < COND_MAX:
        try:
            U, _ = ko.qp_exact(H, f, -inp.bound, inp.bound)
        except (RuntimeError, np.linalg.LinAlgError):
            U = None
    return psi, H, f, U


@functools.lru_cache(maxsize=None)
def oracle_alone(case):
    """The case free-running on the oracle: (left out, box active, all variables at bounds) of B * STEPS trajectory-steps."""
    inp = inputs_of(case)
    left_out = active = all_at = 0
    for b in range(B):
        ctl = inp.controller()
        x = inp.X0[:, b].copy()
        for k in range(STEPS):
            psi, H, f, U = oracle_qp(inp, ctl, x)
            if U is None:
                left_out += 1
                u = float(np.clip(np.linalg.lstsq(2.0 * H, -f, rcond=None)[0][0], -inp.bound, inp.bound))
            else:
                at = np.abs(U) == inp.bound
                active += int(at.any())
                all_at += int(at.all())
                u = float(U[0])
            ctl.prev = (psi, u)
            x = ko.plant_step(inp.plant, x, u, switched=inp.switched(k))
    return left_out, active, all_at


@pytest.mark.parametrize("case", list(CASES))
def test_inputs_meet_the_conditions(case):
    kind = CASES[case][3]
    total = B * STEPS
    left_out, active, all_at = oracle_alone(case)
    print("%s %s: left out %d / %d, box active %d, all variables at bounds %d" % (case, CASES[case][:3], left_out, total, active, all_at))
    assert left_out <= LEFT_OUT_CAP[kind] * total
    assert active >= ACTIVE_MIN * total
    assert all_at <= ALL_AT_BOUNDS_MAX * total


def test_the_table_covers_the_limits_of_the_plugin_dimension_sets():
    """The table's own claims: the smallest and largest L and N a plug-in is made for, both parities of N on each side of every
    threshold it names, and every q."""
    Ls = {c[0] for c in CASES.values()}
    Ns = {c[1] for c in CASES.values()}
    assert min(Ls) == 2 and max(Ls) == 44 and min(Ns) == 2 and max(Ns) == 45
    assert (44 + 1) ** 2 <= 2048 < (45 + 1) ** 2 and 45 ** 2 <= 2048 < 46 ** 2
    assert {15, 17} <= Ns and {29, 31} <= Ns and {24, 25} <= Ns and {32, 33} <= Ns
    assert {30, 31} <= Ls and {23, 24} <= {c[0] for c in CASES.values() if c[3] == "rbf"}
    assert {c[2] for c in CASES.values() if c[3] != "psi"} == {1, 2}
    assert all(c[2] == c[0] for c in CASES.values() if c[3] == "psi")
