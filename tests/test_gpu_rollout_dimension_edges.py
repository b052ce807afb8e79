"""The fused roll-out at the edges of the dimension sets it accepts (csrc/rollout_plugin.hip rollout_plugin_dims: n = 2, L in 2..44,
N in 2..40, q in {1, 2, L}), every set a plug-in made when the handle is created -- and the two sets next to them that it refuses.
Runs on the MI355X box:  python -m pytest tests/test_gpu_rollout_dimension_edges.py -m gpu

The kernel picks its code from compile-time predicates on (L, N, q); every case sits next to one that no other fused test crosses.
Inputs, case table and the oracle's step are tests/test_rollout_dimension_edges_cpu.py's (which proves from the oracle alone that the
box is active in at least 1/4 of the steps, that all variables sit at bounds in at most 1/2, and how few QPs are numerically singular).
B = 32 (the library deals such a batch as workgroups of eight trajectories, of four for the largest sets), ONE kmpc_rollout(log=True)
launch of 5 steps from iteration 99 across the plant switch at 102.

  id       (L, N, q)     lift, y        straddles
  N2       (8, 2, 2)     MLP, C x       smallest horizon: a 2 x 2 tableau
  N3       (8, 3, 2)     MLP, C x       smallest odd horizon
  N15      (9, 15, 2)    MLP, C x       odd N (scalar loads of the H / tableau rows, padded row stride) and odd L below the 16 / 17 switch
  N17      (8, 17, 2)    MLP, C x       first block-form tableau product (row_dot<N, N > 16>); encoder called, not inline (N >= 16)
  N29      (12, 29, 2)   MLP, C x       last chain-dump horizon (v2_chain_dump N < 30), odd
  N31      (12, 31, 2)   MLP, C x       last horizon below the ownmask switch at 32, odd
  v2max    (30, 32, 2)   MLP, C x       the corner of the register-state form (L + 2 = 32, N = 32)
  L2q1     (2, 6, 1)     MLP, C x       smallest L, one output row
  L2q2     (2, 6, 2)     MLP, C x       q == L with y = C x: REFUSED, per-step launches (finding 1)
  L29q1    (29, 17, 1)   MLP, C x       q = 1, odd L, odd N, p = 30
  L31      (31, 12, 2)   MLP, C x       first set of the LDS step (L + 2 > 32), odd L
  L31N24   (31, 24, 2)   MLP, C x       last horizon with two LDS regions
  L31N25   (31, 25, 2)   MLP, C x       first horizon with one LDS region (ro_one_region N > 24), odd L (finding 2)
  N33      (30, 33, 2)   MLP, C x       leaves the register form through N
  L33      (33, 16, 2)   MLP, C x       odd L, LDS step, called encoder
  L44q1    (44, 12, 1)   MLP, C x       largest L, q = 1
  max      (44, 45, 2)   MLP, C x       (L + 1)^2 = N^2 = 2025 <= 2048: REFUSED, per-step launches (finding 3)
  max40    (44, 40, 2)   MLP, C x       the largest set that runs fused: the nearest to `max` on its side of N <= 40
  psi9     (9, 11, 9)    MLP, psi       the 8 x 8-grid step at odd L = N - 2
  psi16    (16, 25, 16)  MLP, psi       ... N > 24 at L > 8
  psi31    (31, 13, 31)  MLP, psi       ... L > 30
  rbf23    (23, 33, 2)   RBF, C x       below ro_rbf_eight (L >= 24 and N > 32)
  rbf24    (24, 33, 2)   RBF, C x       first eight-wave / 256-register RBF set

Every case asserts where the kernel comes from (rollout_is_fused(), plug-in status 1, rollout_variant() = 1 after the launch; the two
refused sets: not fused, status 2 with the reason printed, rollout_variant() = 0) and compares
  - every u_k of the launch with the first move of the oracle's minimiser: 1e-6; every x_{k+1} with the oracle's plant: 1e-9
    (per-trajectory loops, gain-form RLS, ko.condense, ko.qp_exact, regressing on the input the device applied and continuing from the
    device's state: tests/test_gpu_dpp_blocks.py);
  - [A B] and C after the last step (get_model): 1e-9 relative to max(1, max|.|);
  - a twin handle walking the loop with kmpc_step + kmpc_plant_step: its whole Useq with the oracle's minimiser at 1e-6 (the sharper check
    where u_0 sits at a bound), its U0 with the launch's U_log at 1e-9, its plant steps with the launch's X_log at 1e-9.
y = C x with the MLP lift: every status 0.  y = psi and RBF: status 1 (iteration cap) is tolerated as in tests/test_gpu_round6.py; such a
trajectory, a step whose cond(H) >= 1e9 or where qp_exact does not terminate, and a twin step with status 1 are LEFT OUT of the
comparisons with the minimiser and of U0 against U_log -- at most 1/16 of the 160 trajectory-steps (RBF: 1/8), asserted on what was
actually skipped.  The twin is led like the oracle (set_applied_input(U_log[k]), next state X_log[k]): where H is numerically singular
there is no unique minimiser, and a free-running RBF twin (lift kernel + step kernel, not the fused kernel) left the launch's trajectory
at exactly such steps -- |U0 - U_log| up to 2.0 on them, printed as the last column, while both agree with the oracle everywhere else.

Findings (all three fixed in the library with this module):
 1. L2q2: y = C x with q == L was accepted for the fused route, whose static instantiations take the output kind from Q_ == L_
    (csrc/step_body.h, csrc/rollout_kernel.hip).  Measured on a library without the guard: the launch tracked psi(x) -- u and Useq off by
    3.22, C never updated (16.5 relative) -- while [A B] and the plant agreed.  fused_dims_ok (csrc/api.hip) now refuses the fused route
    when (q == L) != (output is the lifted state), as the per-step launcher always did (csrc/step_kernel.hip).
 2. L31N25: one-wave one-region sets with odd L and L + q > 32 took the four-wave kernel's recursion (csrc/step_body.h, condense): no
    w-chain, f wrong -- u off by 4.0 (the opposite bound), launch and twin 2.1 apart.  They now take the one-wave static path, with
    8-byte vector reads for odd L.
 3. max: beyond N = 40 the one-wave step runs the LDS solver, whose N x N tableau has no region in the roll-out's LDS layouts: at
    (44, 45, 2) it ran over the neighbouring trajectories' regions and the status words (status came back as garbage).  Horizons above 40
    are now per-step launches (rollout_plugin_dims).

Measured on the MI355X (worst over the compared steps; left out = launch / twin of 160; U0 = twin U0 against U_log):
  id       u        x        [A B]    C        Useq     U0       left out  U0 on the steps left out
  N2       4.11e-12 2.22e-16 3.69e-13 7.22e-16 4.11e-12 1.46e-13 0 / 0     0.00e+00
  N3       5.97e-12 2.22e-16 3.41e-13 8.08e-16 5.97e-12 1.90e-13 0 / 0     0.00e+00
  N15      7.77e-12 2.22e-16 4.74e-13 1.08e-15 6.49e-11 0.00e+00 0 / 0     0.00e+00
  N17      6.17e-12 2.22e-16 3.45e-13 6.83e-16 8.14e-12 1.55e-15 0 / 0     0.00e+00
  N29      2.08e-11 2.22e-16 5.80e-13 1.99e-15 1.37e-10 1.28e-13 0 / 0     0.00e+00
  N31      5.08e-11 2.22e-16 5.80e-13 1.99e-15 1.53e-10 2.05e-14 0 / 0     0.00e+00
  v2max    2.71e-12 2.22e-16 2.19e-13 3.28e-15 1.96e-11 6.22e-14 1 / 1     0.00e+00
  L2q1     3.09e-11 2.22e-16 5.67e-13 3.32e-16 3.08e-11 2.68e-13 0 / 0     0.00e+00
  L2q2     1.03e-11 2.22e-16 4.24e-13 5.09e-16 1.84e-11 0.00e+00 0 / 0     0.00e+00   (per-step launches)
  L29q1    1.04e-11 2.22e-16 3.34e-13 2.80e-15 1.99e-11 7.55e-15 0 / 0     0.00e+00
  L31      2.30e-11 2.22e-16 2.21e-13 4.88e-15 2.30e-11 0.00e+00 0 / 0     0.00e+00
  L31N24   6.72e-12 2.22e-16 2.21e-13 4.88e-15 1.54e-11 0.00e+00 1 / 1     0.00e+00
  L31N25   8.17e-12 2.22e-16 2.01e-13 4.88e-15 1.73e-11 0.00e+00 1 / 1     0.00e+00
  N33      2.13e-12 2.22e-16 1.80e-13 3.59e-15 2.48e-11 0.00e+00 1 / 1     0.00e+00
  L33      5.34e-12 2.22e-16 1.14e-13 2.34e-15 6.15e-12 0.00e+00 0 / 0     0.00e+00
  L44q1    2.59e-12 2.22e-16 1.31e-13 4.00e-15 1.20e-11 0.00e+00 0 / 0     0.00e+00
  max      2.69e-11 2.22e-16 9.15e-14 4.16e-15 4.02e-11 0.00e+00 6 / 6     0.00e+00   (per-step launches)
  max40    2.34e-11 2.22e-16 8.61e-14 4.16e-15 3.16e-11 0.00e+00 3 / 3     0.00e+00
  psi9     5.28e-11 2.22e-16 4.07e-12 -        3.20e-10 0.00e+00 0 / 0     0.00e+00
  psi16    2.09e-09 2.22e-16 8.52e-13 -        3.56e-09 0.00e+00 0 / 0     0.00e+00
  psi31    6.44e-10 2.22e-16 1.36e-12 -        1.35e-09 0.00e+00 0 / 0     0.00e+00
  rbf23    1.58e-11 2.22e-16 1.29e-11 5.78e-13 3.83e-10 7.32e-13 12 / 12   1.43e+00
  rbf24    1.85e-11 2.22e-16 1.61e-11 6.34e-13 1.13e-10 2.64e-12 13 / 13   2.00e+00
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_rollout_dimension_edges_cpu as edges  # noqa: E402  (the case table, the inputs, the oracle's step)

from oracle import koopman_oracle as ko  # noqa: E402

pytestmark = pytest.mark.gpu

B, STEPS, STEP0, SWITCH = edges.B, edges.STEPS, edges.STEP0, edges.SWITCH
TOL_U, TOL_X, TOL_MODEL, TOL_TWIN = 1e-6, 1e-9, 1e-9, 1e-9
# cases the library serves with per-step launches, and the words its reason (kmpc_rollout_plugin_status, code 2) must hold
PER_STEP = {"L2q2": "q == L", "max": "N <= 40"}


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    return torch


def _rel(a, b):
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("case", list(edges.CASES))
def test_fused_rollout_at_a_dimension_edge_vs_oracle(torch_mod, case):
    torch = torch_mod
    from koopmpc import KoopmanMPC

    inp = edges.inputs_of(case)
    L, N, q = inp.L, inp.N, inp.q
    strict = inp.kind == "mlp"  # y = C x with the MLP lift: every status 0
    mpc, twin = KoopmanMPC(**inp.handle_kw()), KoopmanMPC(**inp.handle_kw())
    code, text = mpc.rollout_plugin_status()
    print("%s (%d, %d, %d): status %d, %s" % (case, L, N, q, code, text))
    if case in PER_STEP:
        assert not mpc.rollout_is_fused() and code == 2 and PER_STEP[case] in text, (code, text)
    else:
        assert mpc.rollout_is_fused() and code == 1, (code, text)
    for m in (mpc, twin):
        m.set_model(inp.A0, inp.B0, inp.C0)
    X0 = inp.X0
    Xd = torch.tensor(X0, dtype=torch.float64, device="cuda:0")
    Ul, Xl = mpc.rollout(inp.plant, Xd, inp.r, STEPS, step0=STEP0, switch_step=SWITCH, log=True)
    torch.cuda.synchronize()
    assert mpc.rollout_variant() == (0 if case in PER_STEP else 1)
    st = mpc.status.cpu().numpy()
    assert (st >= 0).all() and (st <= (0 if strict else 1)).all(), st
    # the twin: the same loop as per-step calls, led like the oracle -- it regresses on the input the launch applied and continues from
    # the launch's state (a step that is left out has no unique minimiser: a free-running twin may leave the launch's trajectory there)
    X2 = torch.tensor(X0, dtype=torch.float64, device="cuda:0")
    Useq2, st2, dU0 = np.zeros((STEPS, N, B)), np.zeros((STEPS, B), dtype=np.int64), np.zeros((STEPS, B))
    worst_x2 = 0.0
    for k in range(STEPS):
        u2 = twin.step(X2, inp.r).clone()
        Useq2[k], st2[k] = twin.Useq.cpu().numpy(), twin.status.cpu().numpy()
        dU0[k] = (u2 - Ul[k]).abs().cpu().numpy()
        twin.set_applied_input(Ul[k])
        X2 = twin.plant_step(inp.plant, X2, Ul[k].clone(), switched=inp.switched(k))
        worst_x2 = max(worst_x2, float((X2 - Xl[k]).abs().max()))
        X2 = Xl[k].clone()
    assert (st2 >= 0).all() and (st2 <= (0 if strict else 1)).all(), st2
    Ul, Xl = Ul.cpu().numpy(), Xl.cpu().numpy()
    Ad, Bd, Cd = [t.cpu().numpy() if t is not None else None for t in mpc.get_model()]
    worst_u = worst_x = worst_k = worst_c = worst_useq = worst_u0 = left_u0 = 0.0
    left_launch = left_twin = at_bound = 0
    for b in range(B):
        capped = st[b] != 0  # (tolerated for y = psi and RBF only: the whole trajectory is left out, but for its plant steps)
        ctl = inp.controller()
        x = X0[:, b].copy()
        for k in range(STEPS):
            psi, H, f, U = edges.oracle_qp(inp, ctl, x)
            if U is None or capped:
                left_launch += 1
                left_twin += 1
                left_u0 = max(left_u0, dU0[k, b])
            else:
                worst_u = max(worst_u, abs(Ul[k, b] - U[0]))
                at_bound += int(abs(U[0]) == inp.bound)
                if st2[k, b] != 0:
                    left_twin += 1
                    left_u0 = max(left_u0, dU0[k, b])
                else:
                    worst_useq = max(worst_useq, float(np.abs(Useq2[k, :, b] - U).max()))
                    worst_u0 = max(worst_u0, dU0[k, b])
            # both sides regress on the input that was applied and continue from the device's state
            ctl.prev = (psi, float(Ul[k, b]))
            xo = ko.plant_step(inp.plant, x, float(Ul[k, b]), switched=inp.switched(k))
            worst_x = max(worst_x, float(np.abs(Xl[k, :, b] - xo).max()))
            x = Xl[k, :, b].copy()
        if capped:
            continue
        Kd = np.concatenate([Ad[b].reshape(L, L), Bd[b].reshape(L, 1)], axis=1)
        worst_k = max(worst_k, _rel(Kd, ctl.gK))
        if Cd is not None:
            worst_c = max(worst_c, _rel(Cd[b], ctl.gC))
    total = B * STEPS
    print("%s (%d, %d, %d): u %.2e  x %.2e  [A B] %.2e  C %.2e  Useq %.2e  U0 vs U_log %.2e  twin x %.2e  left out %d / %d of %d  "
          "(u_0 at a bound in %d; U0 vs U_log on the steps left out %.2e)"
          % (case, L, N, q, worst_u, worst_x, worst_k, worst_c, worst_useq, worst_u0, worst_x2, left_launch, left_twin, total, at_bound, left_u0))
    cap = edges.LEFT_OUT_CAP[inp.kind] * total
    assert left_launch <= cap and left_twin <= cap
    assert worst_u < TOL_U and worst_x < TOL_X
    assert worst_k <= TOL_MODEL and worst_c <= TOL_MODEL
    assert worst_useq < TOL_U and worst_u0 < TOL_TWIN and worst_x2 < TOL_X
