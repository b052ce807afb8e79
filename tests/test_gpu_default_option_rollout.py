"""The default-option instantiation of the fused roll-out kernel (csrc/step_body.h RoOpt) against the generic one, and
the routing between the two.  Runs on the MI355X box:  python -m pytest tests/test_gpu_default_option_rollout.py -m gpu

Agreement.  A handle created with the default options and rolled out without a log runs the default-option kernel (rollout_variant() = 2);
under KMPC_ROLLOUT_GENERIC the same calls run the generic kernel (1).  The switch is read once per process, so each side is a fresh child
process; one child runs the four cases -- (20, 20, 2) with the MLP lift and (8, 30, 2) with the RBF lift, B = 16 (one full workgroup of
sixteen waves) and B = 40 (a last workgroup with eight dead waves) -- as 3 steps from the RLS reset (no update, the first update, the first
carried tableau and the first carried u_{k-1}; the plant switch falls on the third) and 2 more steps as a second launch (have_prev, u_{k-1}
and psi across the launch boundary).  A roll-out WITH a log is by definition a generic launch, so the inputs of the default-option kernel
are compared through what it leaves: X after each launch, the whole state of the handle (kmpc_state_export: inv_K_G, [A B], bar_Q, C,
psi(x_k), u_k), the exported model, status and iters -- all bit for bit.  The generic child also rolls a second handle out WITH the log and
its logged X must be the unlogged X bit for bit: the logged inputs are the inputs of these trajectories.

Routing.  One handle per non-default option at (20, 20, 2), B = 16, 3 steps: each reports variant 1 and matches the per-step route
(step + plant_step) to the bounds of tests/test_gpu_parity.py::test_rollout_equals_step_plus_plant_loop (1e-9 on inputs and states, 1e-9
relative on the model); the default handle without a log reports 2.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "koopman-online-updated-mpc_amd")

CASES = [("mlp", 20, 20, 16), ("mlp", 20, 20, 40), ("rbf", 8, 30, 16), ("rbf", 8, 30, 40)]

CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [%(root)r, %(pkg)r]
from koopmpc import KoopmanMPC
from koopmpc.synth import random_mlp_weights

def rand_model(rng, L, q, rho=0.95):
    A = rng.randn(L, L)
    A *= rho / np.abs(np.linalg.eigvals(A)).max()
    return A, rng.randn(L, 1) * 0.1, rng.randn(q, L) * 0.5

out = {}
for lift, L, N, B in %(cases)r:
    rng = np.random.RandomState(4)
    kw = dict(weights=random_mlp_weights(2, 100, 3, L, seed=3)) if lift == "mlp" else dict(lift="rbf", centres=4 * rng.rand(L, 2) - 2)
    A, Bm, Cm = rand_model(rng, L, 2)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = 4 * rng.rand(2, B) - 2
    tag = "%%s_%%d_" %% (lift, B)
    for logged in (False, True):
        m = KoopmanMPC(n=2, L=L, N=N, batch=B, **kw)
        m.lib.kmpc_set_rollout_workgroup(16)  # (small batches are spread as workgroups of eight otherwise)
        m.set_model(A, Bm, Cm)
        X = torch.tensor(X0, dtype=torch.float64, device="cuda:0")
        t = tag + ("log_" if logged else "")
        for li, (steps, step0) in enumerate(((3, 100), (2, 103))):
            res = m.rollout("duffing", X, r, steps, step0=step0, switch_step=102, log=logged)
            torch.cuda.synchronize()
            out[t + "variant%%d" %% li] = m.rollout_variant()
            out[t + "X%%d" %% li] = X.cpu().numpy()
            out[t + "status%%d" %% li] = m.status.cpu().numpy()
            out[t + "iters%%d" %% li] = m.iters.cpu().numpy()
            if logged:
                out[t + "Ulog%%d" %% li] = res[0].cpu().numpy()
                out[t + "Xlog%%d" %% li] = res[1].cpu().numpy()
            else:
                out[t + "state%%d" %% li] = m.state_dict()["blob"].copy()
        if not logged:
            for name, v in zip("ABC", m.get_model()):
                out[t + name] = v.cpu().numpy()
np.savez(%(out)r, **out)
"""


def _run_child(tmp, name, extra_env):
    out = os.path.join(str(tmp), name + ".npz")
    code = CHILD % dict(root=ROOT, pkg=PKG, cases=CASES, out=out)
    env = {k: v for k, v in os.environ.items() if k != "KMPC_ROLLOUT_GENERIC"}
    env.update(KMPC_DEBUG="1", **extra_env)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def both(torch_mod, tmp_path_factory):
    """The four cases once as they come and once under KMPC_ROLLOUT_GENERIC, a fresh process each."""
    tmp = tmp_path_factory.mktemp("default_option")
    return _run_child(tmp, "default", {}), _run_child(tmp, "generic", {"KMPC_ROLLOUT_GENERIC": "1"})


@pytest.mark.parametrize("lift,L,N,B", CASES, ids=lambda v: str(v))
def test_default_option_kernel_equals_generic_kernel(both, lift, L, N, B):
    d, g = both
    t = "%s_%d_" % (lift, B)
    for li in (0, 1):
        assert int(d[t + "variant%d" % li]) == 2 and int(g[t + "variant%d" % li]) == 1
        # (a logged roll-out is a generic launch in both processes)
        assert int(d[t + "log_variant%d" % li]) == 1 and int(g[t + "log_variant%d" % li]) == 1
        for key in ("X", "state", "status", "iters"):
            a, b = d[t + "%s%d" % (key, li)], g[t + "%s%d" % (key, li)]
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (key, li)
        # the logged inputs belong to these trajectories: the logged run's states are the unlogged run's, bit for bit
        assert g[t + "log_Xlog%d" % li][-1].tobytes() == g[t + "X%d" % li].tobytes()
        assert d[t + "log_Ulog%d" % li].tobytes() == g[t + "log_Ulog%d" % li].tobytes()
        assert np.isfinite(d[t + "X%d" % li]).all() and int(d[t + "iters%d" % li].min()) >= 1
    for name in "ABC":
        assert d[t + name].tobytes() == g[t + name].tobytes(), name
    # the launches did something: the model moved away from the one that was set, differently per trajectory
    assert float(np.abs(d[t + "A"][0] - d[t + "A"][1]).max()) > 0.0


ROUTES = ["lam", "delta_u", "terminal", "cold_start", "ref_per_traj", "log", "no_update", "default"]


@pytest.fixture(scope="module")
def sixteen(torch_mod):
    """Workgroups of sixteen trajectories also for a batch of 16 (the library spreads small batches as workgroups of eight)."""
    from koopmpc import _ffi

    lib = _ffi.load()
    lib.kmpc_set_rollout_workgroup(16)
    yield lib
    lib.kmpc_set_rollout_workgroup(0)


@pytest.mark.parametrize("route", ROUTES)
def test_routing_of_non_default_options(torch_mod, sixteen, route):
    torch = torch_mod
    from koopmpc import KoopmanMPC
    from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

    # (the states and the offline model of tests/test_gpu_dpp_blocks.py: every QP of these steps has a unique minimiser, status 0 -- with a
    #  random model the QPs right after the RLS reset are numerically singular and two routes may return different minimisers)
    L, N, B, steps = 20, 20, 16, 3
    rng = np.random.RandomState(4)
    kw = dict(weights=random_mlp_weights(2, 100, 3, L, seed=5))
    if route == "lam":
        kw.update(lam=0.98)
    elif route == "delta_u":
        kw.update(delta_u=True, lb=-0.5, ub=0.5, umin=-2.0, umax=2.0)
    elif route == "cold_start":
        kw.update(cold_start=True)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    if route == "ref_per_traj":
        r = np.tile(r[None], (B, 1, 1)) * (1.0 + 0.1 * rng.rand(B, 1, 1))
    ms = [KoopmanMPC(n=2, L=L, N=N, batch=B, **kw) for _ in range(2)]
    A, Bm, Cm = offline_edmd(lambda X: ms[0].Encoder(X), plant=duffing_rk4)
    for m in ms:
        m.set_model(A, Bm, Cm)
        if route == "terminal":
            m.set_terminal_weight(np.array([[150.0, 5.0], [5.0, 120.0]]))
        if route == "no_update":
            m.set_online_update(False)
    X0 = initial_states(B, seed=3)
    X1 = torch.tensor(X0, dtype=torch.float64, device="cuda:0")
    X2 = X1.clone()
    log = route == "log"
    res = ms[0].rollout("duffing", X1, r, steps, step0=100, switch_step=102, log=log)
    assert ms[0].rollout_is_fused()
    assert ms[0].rollout_variant() == (2 if route == "default" else 1), route
    assert int(ms[0].status.max().item()) == 0
    worst_u = worst_x = 0.0
    for i in range(steps):
        u = ms[1].step(X2, r).clone()
        assert int(ms[1].status.max().item()) == 0
        X2 = ms[1].plant_step("duffing", X2, u, switched=(100 + i >= 102))
        if log:
            worst_u = max(worst_u, float((u - res[0][i]).abs().max()))
            worst_x = max(worst_x, float((X2 - res[1][i]).abs().max()))
    worst_x = max(worst_x, float((X1 - X2).abs().max()))
    # the handles are in the same state: one more step agrees
    u1, u2 = ms[0].step(X1, r).clone(), ms[1].step(X2, r).clone()
    worst_u = max(worst_u, float((u1 - u2).abs().max()))
    assert int(ms[0].status.max().item()) == 0 and int(ms[1].status.max().item()) == 0
    A1, A2 = ms[0].get_model()[0], ms[1].get_model()[0]
    dA = float((A1 - A2).abs().max()) / max(1.0, float(A2.abs().max()))
    print("routing %s: variant %d, max |u - u_loop| = %.2e, |x - x_loop| = %.2e, A %.2e (relative)" % (route, ms[0].rollout_variant(), worst_u, worst_x, dA))
    assert worst_u < 1e-9 and worst_x < 1e-9
    assert dA <= 1e-9
