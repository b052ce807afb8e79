"""The row products of the register-state step as single asm blocks (csrc/step_body.h row_dot / row_upd), at the edges of that code.
Runs on the MI355X box:  python -m pytest tests/test_gpu_dpp_blocks.py -m gpu

Every case is a fused roll-out (kmpc_rollout, one launch) of 4 steps on 32 trajectories -- two workgroups of the sixteen-wave kernels --
from the states of tests/test_gpu_parity.py::test_fused_rollout_vs_oracle (weights seed 5, offline EDMD model, initial_states seed 3,
iteration 97 on), against per-trajectory oracle loops (gain-form RLS, exact QP, the oracle's plant) that regress on the input the device
applied and continue from the device's state.  Compared: every u_k (1e-6) and x_{k+1} (1e-9), the bounds of that test, and [A B] and C
after the last step (1e-9 relative to max(1, max|.|): the bound tests/test_gpu_state_dims.py holds a sequence of updates to).

  (L, N, q)
  (8, 10, 2)    p = L + 1 = 9 <= 16: the vector stays in the lane's own register (no row exchange)
  (15, 12, 2)   p = 16: the last column of the first 16-lane row
  (16, 12, 2)   p = 17: the first column that is served from the second row
  (20, 20, 2)   the instantiation the benchmark runs
  (30, 12, 2)   p = 31: more columns than one asm statement has operands for -- the two-block form
  (20, 20, 2), lam = 0.98   the scaling of the rows between the products of the update
  (8, 10, 1)    one output row
"""
import numpy as np
import pytest

from oracle import koopman_oracle as ko

pytestmark = pytest.mark.gpu

B, STEPS, STEP0, SWITCH = 32, 4, 97, 102

CASES = [
    (8, 10, 2, 1.0),
    (15, 12, 2, 1.0),
    (16, 12, 2, 1.0),
    (20, 20, 2, 1.0),
    (30, 12, 2, 1.0),
    (20, 20, 2, 0.98),
    (8, 10, 1, 1.0),
]


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    return torch


@pytest.mark.parametrize("L,N,q,lam", CASES, ids=lambda v: str(v))
def test_fused_rollout_row_blocks_vs_oracle(torch_mod, L, N, q, lam):
    torch = torch_mod
    from koopmpc import KoopmanMPC
    from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

    w = random_mlp_weights(2, 100, 3, L, seed=5)
    kw = dict(lam=lam)
    if q != 2:
        kw.update(out_rows=q, out_row0=0)
    mpc = KoopmanMPC(n=2, L=L, N=N, batch=B, weights=w, **kw)
    assert mpc.rollout_is_fused()
    lift_fn = lambda x: ko.mlp_lift(w, x)
    A0, B0, C0 = offline_edmd(lambda X: mpc.Encoder(X), plant=duffing_rk4)
    mpc.set_model(A0, B0, C0)
    r = np.tile(np.array([[1.0], [0.0]])[:q], (1, N))
    X0 = initial_states(B, seed=3)
    Xd = torch.tensor(X0, dtype=torch.float64, device="cuda:0")
    Ul, Xl = mpc.rollout("duffing", Xd, r, STEPS, step0=STEP0, switch_step=SWITCH, log=True)
    assert int(mpc.status.max().item()) == 0
    Ul, Xl = Ul.cpu().numpy(), Xl.cpu().numpy()
    Ad, Bd, Cd = [t.cpu().numpy() for t in mpc.get_model()]
    worst_u = worst_x = worst_k = worst_c = 0.0
    for b in range(B):
        ctl = ko.OracleController(lift_fn, L, 2, N, -2.0, 2.0, A0, B0, C0, rls="gain")
        x = X0[:, b].copy()
        for k in range(STEPS):
            psi = lift_fn(x.reshape(2, 1)).reshape(-1)
            if ctl.prev is not None:
                ppsi, pu = ctl.prev
                ctl.gK, ctl.gP = ko.rls_update_gain(ctl.gK, ctl.gP, np.concatenate([ppsi, [pu]]), psi, lam)
                # (the forgetting factor discounts inv_K_G only, Koopman_update.m:270-274: bar_Q runs with lambda = 1)
                ctl.gC, ctl.gQ = ko.rls_update_gain(ctl.gC, ctl.gQ, ppsi, x)
                ctl.A, ctl.B, ctl.C = ctl.gK[:, :-1].copy(), ctl.gK[:, -1:].copy(), ctl.gC.copy()
            _, _, H, f, _ = ko.condense(ctl.A, ctl.B, ctl.C[:q], psi, r, N, ctl.Qw, ctl.Rw)
            U, _ = ko.qp_exact(H, f, -2.0, 2.0)
            worst_u = max(worst_u, abs(Ul[k, b] - U[0]))
            # both sides regress on the input that was applied and continue from the device's state
            ctl.prev = (psi, float(Ul[k, b]))
            xo = ko.plant_step("duffing", x, float(Ul[k, b]), switched=(STEP0 + k >= SWITCH))
            worst_x = max(worst_x, float(np.abs(Xl[k, :, b] - xo).max()))
            x = Xl[k, :, b].copy()
        Kd = np.concatenate([Ad[b].reshape(L, L), Bd[b].reshape(L, 1)], axis=1)
        worst_k = max(worst_k, float(np.abs(Kd - ctl.gK).max()) / max(1.0, float(np.abs(ctl.gK).max())))
        worst_c = max(worst_c, float(np.abs(Cd[b] - ctl.gC).max()) / max(1.0, float(np.abs(ctl.gC).max())))
    print("row blocks (L, N, q, lam) = (%d, %d, %d, %g): max |u - u_oracle| = %.2e, |x - x_oracle| = %.2e, [A B] %.2e, C %.2e (relative)"
          % (L, N, q, lam, worst_u, worst_x, worst_k, worst_c))
    assert worst_u < 1e-6 and worst_x < 1e-9
    assert worst_k <= 1e-9 and worst_c <= 1e-9
