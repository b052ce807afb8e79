"""The default-option roll-out kernel of (20, 20, 2) hands the vector of every product of the condensed-QP recursion to the two 16-lane
rows of a half THROUGH LDS (csrc/step_body.h RoOpt::LG_CHAIN, lds_row_dot; DESIGN.md 4.1, profiles/lds_gather.txt): the next product reads
v0 / v1 back from where every lane stores its element of the step anyway, instead of exchanging registers (half_gather).  Only the route of
a value between lanes changes, so every operand of every multiply-add is what it was.
Runs on the MI355X box:  python -m pytest tests/test_gpu_lds_gather.py -m gpu

Every case is the default-option kernel (rollout_variant() = 2, the new route) against the generic kernel (1, the register exchange;
KMPC_ROLLOUT_GENERIC is read once per process, so each side is one fresh child process that runs all the scenarios) with np.array_equal
after every launch: X, the checkpoint (kmpc_state_export: the RLS state, psi(x_k), the warm start, u_k), get_model(), status and iters.
The bound is equality.

Scenarios, all on the set (20, 20, 2) with the MLP lift -- (8, 30, 2) has no dump area (its recursion's stores are masked) and its lift's
vectors fit one 16-lane row, so it keeps its code and is not here.
  steps      B in {16, 23, 40} (a full workgroup, a ragged last one, three workgroups) x launches of {1, 2, 5} steps, each twice in a
             row: the first step of a launch has no covariance update done ahead and reads x_warm from memory, the last one stores.
  fall-back  256 trajectories, 25 steps after a reset as launches of 5 (the recipe of tests/test_gpu_launch_boundary_state.py): solves
             take the qp_lds fall-back in the middle of a launch, and its vectors cover the dump area the recursion's reads come from.
  sets       the mixed case over 6 + 6 + 6 steps across the plant switch with a logged twin: first inputs leave and reach the box
             inside a launch, i.e. the solves behind the recursion sweep and rebuild their tableaux.
  layers2    two hidden layers (nhh = 1).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "koopman-online-updated-mpc_amd")
TESTS = os.path.join(ROOT, "tests")

# name -> (B, hidden layers, constructor options, script).  Script operations: ("roll", steps), ("reset",), ("probe", count): `count`
# logged one-step launches on a twin handle from the same start (the generic kernel in either process).
SCENARIOS = {}
for _B in (16, 23, 40):
    for _k in (1, 2, 5):
        SCENARIOS["steps-B%d-K%d" % (_B, _k)] = (_B, 3, dict(Rw=1.0), [("roll", _k), ("roll", _k)])
SCENARIOS["fallback"] = (256, 3, {}, [("reset",), ("probe", 25)] + [("roll", 5)] * 5)
SCENARIOS["sets"] = (32, 3, dict(Rw=1.0), [("probe", 18), ("roll", 6), ("roll", 6), ("roll", 6)])
SCENARIOS["layers2"] = (23, 2, dict(Rw=1.0), [("roll", 3), ("roll", 2)])
STEP0, SWITCH, L, N = 94, 102, 20, 20

CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
from koopmpc import KoopmanMPC, _ffi
from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

_ffi.load().kmpc_set_rollout_workgroup(16)  # (small batches are spread as workgroups of eight otherwise)
L, N = %(L)d, %(N)d
cache = {}

def make(B, layers, kw):
    m = KoopmanMPC(n=2, L=L, N=N, batch=B, weights=random_mlp_weights(2, 100, layers, L, seed=5), layers=layers, **kw)
    if layers not in cache:
        cache[layers] = offline_edmd(lambda X: m.Encoder(X), plant=duffing_rk4)
    m.set_model(*cache[layers])
    assert m.rollout_is_fused()
    return m

out = {}
r = np.tile(np.array([[1.0], [0.0]]), (1, N))
for name, (B, layers, kw, script) in %(scenarios)r.items():
    m = make(B, layers, kw)
    X = torch.tensor(initial_states(B, seed=3), dtype=torch.float64, device="cuda:0").contiguous()
    k, launch = %(step0)d, 0
    for op in script:
        if op[0] == "roll":
            m.rollout("duffing", X, r, op[1], step0=k, switch_step=%(switch)d)
            torch.cuda.synchronize()
            t = "%%s/%%d/" %% (name, launch)
            out[t + "variant"] = m.rollout_variant()
            out[t + "X"] = X.cpu().numpy()
            out[t + "status"] = m.status.cpu().numpy()
            out[t + "iters"] = m.iters.cpu().numpy()
            out[t + "state"] = m.state_dict()["blob"].copy()
            for nm, v in zip("ABC", m.get_model()):
                out[t + nm] = v.cpu().numpy()
            k += op[1]
            launch += 1
        elif op[0] == "reset":
            m.reset()
        elif op[0] == "probe":
            p = make(B, layers, kw)
            if ("reset",) in script:
                p.reset()
            Xp = X.clone()
            U, it, st = [], [], []
            for i in range(op[1]):
                res = p.rollout("duffing", Xp, r, 1, step0=k + i, switch_step=%(switch)d, log=True)
                torch.cuda.synchronize()
                assert p.rollout_variant() == 1
                U.append(res[0][0].cpu().numpy()); it.append(p.iters.cpu().numpy().copy()); st.append(p.status.cpu().numpy().copy())
            out[name + "/probe/U"] = np.array(U); out[name + "/probe/iters"] = np.array(it); out[name + "/probe/status"] = np.array(st)
            out[name + "/probe/box"] = np.array([p.cfg.lb, p.cfg.ub])
    out[name + "/launches"] = launch
np.savez(%(out)r, **out)
"""


def _run_child(tmp, name, extra_env):
    out = os.path.join(str(tmp), name + ".npz")
    code = CHILD % dict(root=ROOT, pkg=PKG, tests=TESTS, scenarios=SCENARIOS, step0=STEP0, switch=SWITCH, L=L, N=N, out=out)
    env = {k: v for k, v in os.environ.items() if k != "KMPC_ROLLOUT_GENERIC"}
    env.update(KMPC_DEBUG="1", **extra_env)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """Every scenario once as it comes (the new route) and once under KMPC_ROLLOUT_GENERIC (the register exchange), a fresh process each."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    tmp = tmp_path_factory.mktemp("lds_gather")
    return _run_child(tmp, "default", {}), _run_child(tmp, "generic", {"KMPC_ROLLOUT_GENERIC": "1"})


def _same(d, g, name):
    n = int(d[name + "/launches"])
    assert n == int(g[name + "/launches"]) and n > 0
    for li in range(n):
        t = "%s/%d/" % (name, li)
        assert int(d[t + "variant"]) == 2 and int(g[t + "variant"]) == 1, (t, int(d[t + "variant"]), int(g[t + "variant"]))
        for key in ("X", "state", "status", "iters", "A", "B", "C"):
            assert d[t + key].dtype == g[t + key].dtype and np.array_equal(d[t + key], g[t + key], equal_nan=True), (t, key)
            assert d[t + key].tobytes() == g[t + key].tobytes(), (t, key)  # (the sign of a zero included)
        assert np.isfinite(d[t + "X"]).all() and int(d[t + "iters"].min()) >= 1


@pytest.mark.parametrize("name", [n for n in SCENARIOS if n.startswith("steps")] + ["layers2"])
def test_lds_route_equals_register_exchange_after_every_launch(both, name):
    d, g = both
    _same(d, g, name)


def test_fall_back_in_the_middle_of_a_launch(both):
    d, g = both
    _same(d, g, "fallback")
    it = g["fallback/probe/iters"]  # (25, B): per-step iters of the generic kernel
    handed = it >= N
    steps_with = np.nonzero(handed.any(axis=1))[0]
    print("fall-back: %d solves of %d reached the hand-over (iters >= N), at steps %s" % (int(handed.sum()), it.size, steps_with.tolist()))
    # at least one of them not in the last step of a launch of 5: the recursion behind it reads the dump area the fall-back wrote over
    assert any(s % 5 != 4 for s in steps_with), steps_with


def test_set_changes_inside_a_launch(both):
    d, g = both
    _same(d, g, "sets")
    U, (lb, ub) = g["sets/probe/U"], g["sets/probe/box"]
    on = (U == lb) | (U == ub)
    change = on[1:] != on[:-1]
    inside = np.array([(i + 1) % 6 != 0 for i in range(change.shape[0])])
    count = int(change[inside].sum())
    print("sets: %d first inputs change sides between steps inside a launch" % count)
    assert count >= 8 and on.any() and (~on).any()
    assert int(g["sets/probe/status"].max()) == 0
