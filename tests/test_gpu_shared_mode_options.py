"""Shared-model mode (kmpc_shared_local_gram / kmpc_shared_solve[_plant] / kmpc_shared_rollout) against the oracle with lambda < 1, y = psi
and a reference that moves along the horizon, across rows and from step to step, on every model route of csrc/api.hip shared_solve_impl.
Runs on the MI355X box:  python -m pytest tests/test_gpu_shared_mode_options.py -m gpu

The cases, their routes and the proof that their inputs are fit (mix of interior / on-box QPs, cond(H), the model bound, and that ignoring
lambda or misplacing the reference by one horizon step moves some input by >= 1e-2) are in tests/test_shared_mode_cases_cpu.py; the oracle
side (SharedOracle) is imported from there and runs in lockstep on the device's states and inputs.

  stages    shared_step(X, r_k) for 8 steps, plant switched from step 5 on.  After every step: shared_model() within the case's model
            bound of SharedEdmd(lam).model() (C left out for y = psi), Useq of every trajectory within 1e-6 of qp_exact of the oracle's
            condensed QP, every status 0 (du_tank: the filter of test_shared_model_delta_u_tank_vs_oracle, status 0 and cond(H) < 1e10,
            at least 3 B QPs compared).
  roll-out  shared_rollout(plant, X, r_0, 8, step0=0, switch_step=5, log=True), the horizon-varying reference of step 0 held over the
            call; U_log / X_log replayed through the oracle: inputs 1e-6, final shared_model() within the bound, states 1e-9 against
            ko.plant_step / ko.tank_step on the logged input.
  terminal  m2_17 and psi8 once more with set_terminal_weight(P_N) against ko.condense(..., PN=P_N): the Wt terms of F and f0 read the
            last Gamma block and reference column N - 1 in each of the three kernels that build the condensed QP.
  route     m2_17, m2_33 and du_tank once more under KMPC_SHARED_MODEL_R3 (read per call): lambda in the round-3 kernel at shapes the
            sixteen-wave kernel takes otherwise.
  refusal   y = psi at (30, 30): the condensed QP needs 252 240 bytes of LDS.  After three step() calls shared_step raises KmpcError (-3)
            naming y = psi, the condensed QP of the shared model and the LDS; the checkpoint is byte for byte what it was and the handle
            goes on with step() exactly as a twin that never saw the refused call.

Bounds: inputs 1e-6 (the project's bound for this comparison at cond(H) ~ 1e8; here cond(H) <= 1e6), states 1e-9, model: per case,
8 x max(two-form deviation, cond(G + I/P0) eps) < 1e-7 (tests/test_shared_mode_cases_cpu.py).

Measured on the card (worst deviations, printed with -s), model (its bound) / inputs (bound 1e-6); roll-out states <= 4.4e-16 (bound 1e-9):
    case      stages                          roll-out                        terminal block        KMPC_SHARED_MODEL_R3
    m2_17     1.5e-12 (1.9e-9) / 1.5e-11      1.4e-12 (1.9e-9) / 1.3e-11      1.3e-12 / 2.4e-11     1.4e-12 / 5.3e-11
    m2_33     2.9e-12 (2.4e-9) / 6.7e-11      2.1e-12 (2.4e-9) / 1.9e-10                            3.4e-12 / 9.0e-11
    m2_33w    5.6e-12 (2.8e-9) / 7.5e-11      6.3e-12 (3.4e-9) / 1.2e-10
    r3_short  1.8e-12 (1.4e-10) / 6.0e-10     4.2e-12 (1.4e-10) / 3.4e-10
    r3_wide   1.7e-11 (4.7e-9) / 2.7e-10      3.0e-11 (4.4e-9) / 1.7e-10
    psi8      9.8e-13 (6.7e-11) / 7.8e-11     1.3e-12 (6.9e-11) / 3.8e-11     3.7e-12 / 1.3e-10
    psi20     2.3e-12 (2.5e-9) / 4.7e-11      1.2e-12 (2.5e-9) / 1.7e-11
    L64       1.4e-9 (5.6e-8) / 2.9e-9        1.2e-9 (5.7e-8) / 2.1e-9
    du_tank   1.1e-11 (5.3e-10) / 2.5e-11     4.1e-12 (8.6e-10) / 2.4e-11                           8.7e-12 / 2.6e-11
Every status 0, all 192 (128) QPs of every case compared.

What the cases found.  L64 missed the input bound with the library as it was: model 1.3e-9 (inside its bound), inputs 1.6e-6.  Condensed QP
and box QPs reproduced the oracle's on the device's own model to 5e-13; the model was [A B] = (Y Z') P with the explicit inverse P of the
swept Gram matrix, whose error cond eps lies in every direction, where a solve leaves it in the directions the samples hardly excite
(NumPy's two forms differ by 9e-10 in the model and 1e-9 in the inputs).  shared_solve_kernel now adds one step of iterative refinement
to both solves of the shared-model step; psi8 went from 1.0e-9 to 7.8e-11 and psi20 from 1.7e-10 to 4.7e-11 with it.
The refusal: before the up-front check the (30, 30) handle came back from shared_step with -1001 ("launch_shared_condense<T>(...): invalid
argument") after G <- lambda G + delta and the model solve had run, and with its shared-model blocks allocated.
"""
import os
import sys

import numpy as np
import pytest

from oracle import koopman_oracle as ko

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_shared_mode_cases_cpu as inputs  # noqa: E402  (the case table, the oracle side and the model bound)

pytestmark = pytest.mark.gpu

STATE_BOUND = 1e-9


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def KM(torch_mod):
    from koopmpc import KoopmanMPC

    return KoopmanMPC


def make(KM, case, PN=None):
    mpc = KM(**inputs.handle_options(case))
    mpc.set_model(*inputs.setup(case)[2])
    if PN is not None:
        mpc.set_terminal_weight(PN)
    return mpc


def device_model(mpc):
    A, Bm, C = mpc.shared_model()
    return A.cpu().numpy(), Bm.cpu().numpy(), None if C is None else C.cpu().numpy()


def stages(KM, case, label, PN=None, monkeypatch=None):
    """shared_step in lockstep with the oracle on the device's states and inputs; monkeypatch: every call under KMPC_SHARED_MODEL_R3."""
    c = inputs.CASES[case]
    B = c["B"]
    bound = inputs.oracle_alone(case, terminal=PN is not None)["model_bound"]
    mpc, orc = make(KM, case, PN), inputs.SharedOracle(case, PN)
    X = inputs.setup(case)[3].copy()
    worst_m = worst_u = worst_cond = 0.0
    compared = 0
    for k in range(inputs.STEPS):
        r = orc.reference(k)
        if monkeypatch is not None:
            monkeypatch.setenv("KMPC_SHARED_MODEL_R3", "1")
        try:
            u = mpc.shared_step(X, r).cpu().numpy()
        finally:
            if monkeypatch is not None:
                monkeypatch.delenv("KMPC_SHARED_MODEL_R3", raising=False)
        Useq, st = mpc.Useq.cpu().numpy(), mpc.status.cpu().numpy()
        H, Uo = orc.solve(X, r)
        cond = float(np.linalg.cond(H))
        if orc.samples:
            worst_m = max(worst_m, inputs.model_deviation(device_model(mpc), orc.model))
        if orc.du:
            assert (st <= 1).all(), (k, st)
            ok = (st == 0) if cond < inputs.COND_DU else np.zeros(B, bool)
        else:
            assert (st == 0).all(), (k, st)
            assert cond <= inputs.COND_MAX
            ok = np.ones(B, bool)
        worst_cond = max(worst_cond, cond)
        if ok.any():
            worst_u = max(worst_u, float(np.abs(Useq[:, ok] - Uo[:, ok]).max()), float(np.abs(u[ok] - orc.first_inputs(Uo)[ok]).max()))
        compared += int(ok.sum())
        orc.commit(u)  # both sides regress on the input the device applied
        X = orc.plant_step(X, u, k)
    print("%-22s %-8s model %.2e (bound %.2e), inputs %.2e (bound %.0e), %d / %d QPs compared, max cond(H) %.1e"
          % (label, case, worst_m, bound, worst_u, inputs.INPUT_BOUND, compared, B * inputs.STEPS, worst_cond))
    assert compared >= (3 * B if orc.du else B * inputs.STEPS)
    assert worst_m <= bound
    assert worst_u <= inputs.INPUT_BOUND


@pytest.mark.parametrize("case", list(inputs.CASES))
def test_stages_vs_oracle(torch_mod, KM, case):
    stages(KM, case, "stages")


@pytest.mark.parametrize("case", ["m2_17", "psi8"])
def test_terminal_block_with_a_moving_reference(torch_mod, KM, case):
    stages(KM, case, "terminal block", PN=inputs.terminal_block(case))


@pytest.mark.parametrize("case", ["m2_17", "m2_33", "du_tank"])
def test_round3_model_kernel_at_sixteen_wave_shapes(torch_mod, KM, monkeypatch, case):
    stages(KM, case, "KMPC_SHARED_MODEL_R3", monkeypatch=monkeypatch)


@pytest.mark.parametrize("case", list(inputs.CASES))
def test_rollout_vs_oracle(torch_mod, KM, case):
    torch = torch_mod
    c = inputs.CASES[case]
    B, S = c["B"], inputs.STEPS
    bound = inputs.oracle_alone(case, held=True)["model_bound"]
    mpc, orc = make(KM, case), inputs.SharedOracle(case)
    X0 = inputs.setup(case)[3].copy()
    r0 = orc.reference(0)
    X = torch.tensor(X0, dtype=torch.float64, device="cuda:0").contiguous()
    Ul, Xl = mpc.shared_rollout(c["plant"], X, r0, S, step0=0, switch_step=inputs.SWITCH, log=True)
    Ul, Xl, Useq, st = Ul.cpu().numpy(), Xl.cpu().numpy(), mpc.Useq.cpu().numpy(), mpc.status.cpu().numpy()
    assert np.array_equal(X.cpu().numpy(), Xl[-1]) and np.array_equal(mpc.U0.cpu().numpy(), Ul[-1])
    if orc.du:
        assert (st <= 1).all(), st
        ok = st == 0  # (the worst status of a trajectory over the call)
    else:
        assert (st == 0).all(), st
        ok = np.ones(B, bool)
    assert ok.sum() * S >= (3 * B if orc.du else B * S)
    worst_u = worst_x = 0.0
    Xk = X0
    for k in range(S):
        H, Uo = orc.solve(Xk, r0)
        assert float(np.linalg.cond(H)) <= (inputs.COND_DU if orc.du else inputs.COND_MAX)
        worst_u = max(worst_u, float(np.abs(Ul[k][ok] - orc.first_inputs(Uo)[ok]).max()))
        if k == S - 1:
            worst_u = max(worst_u, float(np.abs(Useq[:, ok] - Uo[:, ok]).max()))
        worst_x = max(worst_x, float(np.abs(Xl[k] - orc.plant_step(Xk, Ul[k], k)).max()))
        orc.commit(Ul[k])
        Xk = Xl[k]
    worst_m = inputs.model_deviation(device_model(mpc), orc.model)
    print("%-22s %-8s model %.2e (bound %.2e), inputs %.2e (bound %.0e), states %.2e (bound %.0e)"
          % ("roll-out", case, worst_m, bound, worst_u, inputs.INPUT_BOUND, worst_x, STATE_BOUND))
    assert worst_m <= bound
    assert worst_u <= inputs.INPUT_BOUND
    assert worst_x <= STATE_BOUND


def test_unfitting_lifted_output_shape_is_refused_before_the_handle_is_touched(torch_mod, KM):
    torch = torch_mod
    from koopmpc._ffi import KmpcError
    from koopmpc.synth import initial_states, offline_edmd, vdp_rk4

    L = N = 30
    B = 8
    cx = 4 * np.random.RandomState(L + N).rand(L, 2) - 2
    lift = lambda x: ko.rbf_lift(x, cx)
    model0 = offline_edmd(lift, plant=vdp_rk4)
    handles = [KM(n=2, L=L, N=N, batch=B, lift="rbf", centres=cx, output="lift", lb=-6.0, ub=6.0, lam=0.95, Rw=1.0) for _ in range(2)]
    X = initial_states(B, seed=11)
    for k in range(3):
        r = lift(inputs.moving_reference(k, N))
        us = []
        for m in handles:
            if k == 0:
                m.set_model(*model0)
            us.append(m.step(X, r).cpu().numpy().copy())
        assert np.array_equal(us[0], us[1])
        X = ko.plant_step("vdp", X, us[0])
    mpc, twin = handles
    r = lift(inputs.moving_reference(3, N))
    before = mpc.state_dict()["blob"].copy()
    Xd = torch.tensor(X, dtype=torch.float64, device="cuda:0").contiguous()
    calls = {"shared_step": lambda: mpc.shared_step(X, r), "shared_solve": lambda: mpc.shared_solve(torch.zeros(2 * L + 3, L + 1, dtype=torch.float64, device="cuda:0"), r),
             "shared_rollout": lambda: mpc.shared_rollout("vdp", Xd, r, 2, switch_step=-1)}
    for name, call in calls.items():
        with pytest.raises(KmpcError) as e:
            call()
        text = str(e.value)
        print("%s: %s" % (name, text))
        assert "(-3)" in text
        assert "y = psi" in text and "condensed QP of the shared model" in text and "LDS" in text and "252240" in text
        after = mpc.state_dict()["blob"]
        assert after.shape == before.shape and np.array_equal(after, before), name
    assert np.array_equal(Xd.cpu().numpy(), X)
    ua, ub = mpc.step(X, r).cpu().numpy(), twin.step(X, r).cpu().numpy()
    assert np.isfinite(ua).all() and np.array_equal(ua, ub)
    assert np.array_equal(mpc.Useq.cpu().numpy(), twin.Useq.cpu().numpy()) and np.array_equal(mpc.status.cpu().numpy(), twin.status.cpu().numpy())
    assert np.array_equal(mpc.state_dict()["blob"], twin.state_dict()["blob"])
