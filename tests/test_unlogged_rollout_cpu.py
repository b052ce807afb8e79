"""The inputs of tests/test_gpu_unlogged_rollout.py, judged from the oracle alone (no GPU).

The logged oracle comparisons of the suite run with the default weights and box, where the oracle alone puts the first input ON the box
in 520 of 576 trajectory-steps at (20, 20) and in 248 of 280 at (8, 30): they mostly compare clip with clip.  The four cases below use
weights and boxes for which a large share of the first inputs is strictly interior; each case states its condition and this module
proves it: per-trajectory OracleController(rls="gain") free-running on the oracle's plant over the launches of the case, counting the
first inputs strictly inside the box and those on it, the largest cond(H) of the condensed QPs, and the model bound.

The model bound is what the GPU module allows between the kernel's final A, B, C and the oracle's: 8 x the deviation between the oracle's
own two RLS forms (the gain form the kernels evaluate and the form as the reference writes it, K_A inv_K_G) on the same transitions,
relative to max(1, |.|max), floor 1e-12.  It must stay below 1e-6 or the inputs are unfit for a model comparison.

Measured here (printed by `python -m pytest tests/test_unlogged_rollout_cpu.py -s`):
    case            set                   plant    box    weights          B   launches        interior   on the box   max cond(H)   model bound
    cfg2_mixed      (20, 20, 2) MLP       duffing  +-2    Rw = 1           32  6 + 6 + 6 @ 94  223 / 576  353          6.0e2         1.4e-10
    cfg2_interior   (20, 20, 2) MLP       duffing  +-2    Qw = 1, Rw = 1   32  6 + 6 + 6 @ 94  565 / 576  11           6.7e3         1.4e-10
    cfg3_mixed      (8, 30, 2) RBF, y=Cx  vdp      +-6    default          20  5 + 5 + 4 @ 0   114 / 280  166          5.5e2         2.4e-10
    cfg3_interior   (8, 30, 2) RBF, y=Cx  vdp      +-20   Rw = 1           20  5 + 5 + 4 @ 0   272 / 280  8            1.3e1         4.0e-10
The mixed cases must have at least 1/3 of the first inputs strictly interior AND at least 1/5 on the box, the interior cases at least
0.9 interior; cond(H) <= 1e6 everywhere.
"""
import functools

import numpy as np
import pytest

from oracle import koopman_oracle as ko

# name -> set, plant, box, controller weights, batch, launches, step0, switch step, required shares (interior, on the box)
CASES = {
    "cfg2_mixed": dict(set="cfg2", plant="duffing", lb=-2.0, ub=2.0, kw=dict(Rw=1.0), B=32, launches=(6, 6, 6), step0=94, switch=102,
                       interior=1.0 / 3.0, on_box=1.0 / 5.0),
    "cfg2_interior": dict(set="cfg2", plant="duffing", lb=-2.0, ub=2.0, kw=dict(Qw=1.0, Rw=1.0), B=32, launches=(6, 6, 6), step0=94,
                          switch=102, interior=0.9, on_box=0.0),
    "cfg3_mixed": dict(set="cfg3", plant="vdp", lb=-6.0, ub=6.0, kw=dict(), B=20, launches=(5, 5, 4), step0=0, switch=7,
                       interior=1.0 / 3.0, on_box=1.0 / 5.0),
    "cfg3_interior": dict(set="cfg3", plant="vdp", lb=-20.0, ub=20.0, kw=dict(Rw=1.0), B=20, launches=(5, 5, 4), step0=0, switch=7,
                          interior=0.9, on_box=0.0),
}
COND_MAX = 1e6          # cond(H) of every QP of a case: the minimiser is then unique to far below the 1e-6 bound on the inputs
MODEL_BOUND_MAX = 1e-6  # a model bound above this says nothing: the inputs would be unfit
MODEL_FLOOR = 1e-12
MARGIN = 8.0            # what tests/test_gpu_float32.py gives a kernel over a restatement

SETS = {"cfg2": (20, 20), "cfg3": (8, 30)}


def rel(a, b):
    """max |a - b| relative to max(1, max |b|): the measure of tests/test_gpu_parity.py's model comparisons."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) / max(1.0, float(np.abs(b).max()))


def cfg2_weights():
    from koopmpc.synth import random_mlp_weights

    return random_mlp_weights(2, 100, 3, 20, seed=5)


def cfg3_offline():
    """Centres and offline samples exactly as tests/test_gpu_round2.py::test_rollout_vs_oracle_across_the_switch takes them."""
    from koopmpc.synth import offline_data, vdp_rk4

    Xo, Yo, Uo = offline_data(plant=vdp_rk4)
    cx = Xo[:, np.random.RandomState(0).choice(Xo.shape[1], 8, replace=False)].T.copy()
    return cx, Xo, Yo, Uo


def storage_start(lift_fn, Xo, Yo, Uo):
    """Both RLS forms of the least-squares fit over the offline samples (offline_fit(init_rls=True), Koopman_update.m:258-278):
    gain form (gK, gP, gC, gQ) and the reference's accumulators (K_A, bar_X; inv_K_G = gP, bar_Q = gQ)."""
    PX, PY = lift_fn(Xo), lift_fn(Yo)
    Z = np.concatenate([PX, Uo[None, :]], 0)
    gP = np.linalg.inv(Z @ Z.T)
    gQ = np.linalg.inv(PX @ PX.T)
    K_A, bar_X = PY @ Z.T, Xo @ PX.T
    return dict(gK=K_A @ gP, gP=gP, gC=bar_X @ gQ, gQ=gQ, K_A=K_A, bar_X=bar_X)


def make_controller(case, lift_fn, L, N, A0, B0, C0, start=None):
    c = CASES[case]
    ctl = ko.OracleController(lift_fn, L, 2, N, c["lb"], c["ub"], A0, B0, C0, rls="gain", **c["kw"])
    if start is not None:
        ctl.gK, ctl.gP, ctl.gC, ctl.gQ = start["gK"].copy(), start["gP"].copy(), start["gC"].copy(), start["gQ"].copy()
    return ctl


def make_reference_rls(L, start=None):
    """The estimator in the form the reference writes (K_A inv_K_G), to be fed the transitions a gain-form controller saw."""
    st = ko.RlsStateRef(L, 1, 2)
    if start is not None:
        st.K_A, st.P, st.bar_X, st.bar_Q = start["K_A"].copy(), start["gP"].copy(), start["bar_X"].copy(), start["gQ"].copy()
    return st


def model_deviation(ctl, st):
    """Deviation of the reference-form model from the gain-form controller's after the same transitions (0 before any)."""
    if not st.K.any():
        return 0.0
    L = ctl.L
    return max(rel(ctl.A, st.K[:, :L]), rel(ctl.B, st.K[:, L:]), rel(ctl.C, st.C))


def model_bound(dev):
    return max(MARGIN * dev, MODEL_FLOOR)


@functools.lru_cache(maxsize=None)
def oracle_alone(case):
    """The case free-running on the oracle: counts of first inputs, max cond(H), model bound."""
    from koopmpc.synth import duffing_rk4, initial_states, offline_edmd

    c = CASES[case]
    L, N = SETS[c["set"]]
    start = None
    if c["set"] == "cfg2":
        w = cfg2_weights()
        lift_fn = lambda x: ko.mlp_lift(w, x)
        A0, B0, C0 = offline_edmd(lift_fn, plant=duffing_rk4)
    else:
        cx, Xo, Yo, Uo = cfg3_offline()
        lift_fn = lambda x: ko.rbf_lift(x, cx)
        start = storage_start(lift_fn, Xo, Yo, Uo)
        A0, B0, C0 = start["gK"][:, :-1].copy(), start["gK"][:, -1:].copy(), start["gC"].copy()
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = initial_states(c["B"], seed=3)
    steps = sum(c["launches"])
    interior = on_box = 0
    cond = dev = 0.0
    for b in range(c["B"]):
        ctl = make_controller(case, lift_fn, L, N, A0, B0, C0, start)
        st = make_reference_rls(L, start)
        x = X0[:, b].copy()
        for k in range(steps):
            prev = ctl.prev
            u, _, psi = ctl.step(x, r)
            if prev is not None:
                ko.rls_update_reference(st, prev[0], prev[1], psi, x)
            H = ko.condense(ctl.A, ctl.B, ctl.C, psi, r, N, ctl.Qw, ctl.Rw)[2]
            cond = max(cond, float(np.linalg.cond(H)))
            if c["lb"] < u < c["ub"]:
                interior += 1
            else:
                assert u == c["lb"] or u == c["ub"]
                on_box += 1
            x = ko.plant_step(c["plant"], x, u, switched=(c["step0"] + k >= c["switch"]))
        dev = max(dev, model_deviation(ctl, st))
    return dict(total=c["B"] * steps, interior=interior, on_box=on_box, cond=cond, model_bound=model_bound(dev))


@pytest.mark.parametrize("case", sorted(CASES))
def test_inputs_meet_the_condition_of_the_case(case):
    c, res = CASES[case], oracle_alone(case)
    print("%s: %d / %d first inputs strictly interior, %d on the box, max cond(H) = %.2e, model bound %.2e"
          % (case, res["interior"], res["total"], res["on_box"], res["cond"], res["model_bound"]))
    assert res["interior"] + res["on_box"] == res["total"] == c["B"] * sum(c["launches"])
    assert res["interior"] >= c["interior"] * res["total"]
    assert res["on_box"] >= c["on_box"] * res["total"]
    assert res["cond"] <= COND_MAX
    assert res["model_bound"] < MODEL_BOUND_MAX
