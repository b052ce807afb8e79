"""The launch-resident encoder operands of the default-option (20, 20, 2) roll-out kernel (csrc/rollout_kernel.hip ro_encoder_tiles' resident
mode): the biases of the hidden and the output layer and output tile 0 sit in an LDS area behind the x slots, filled once
per launch; output tile 1 keeps the global path.  Runs on the MI355X box:  python -m pytest tests/test_gpu_encoder_resident_operands.py -m gpu

The pattern is tests/test_gpu_launch_boundary_state.py's: one script runs in fresh child processes -- as it comes (the default-option kernel,
rollout_variant() = 2; the launcher plans the biases and output tile 0), with the plan cut down to the biases alone (KMPC_ROLLOUT_RESIDENT,
the launcher's measurement aid: what is not in the area stays on the global path), and under KMPC_ROLLOUT_GENERIC (the generic kernel, 1:
the arithmetic without an area) -- and X, the checkpoint, the exported model, status and iters are compared with np.array_equal after
every launch.  What the launcher planned is asserted too (rollout_resident(): the parts in the area and the LDS bytes of the launch --
145 664 B without an area, + 2 048 B with the biases, + 12 800 B with output tile 0), so a plan that silently dropped a part fails.

Scenarios, all on (20, 20, 2) with the MLP lift and the mixed box of tests/test_unlogged_rollout_cpu.py (Rw = 1, +-2):
  steps     B in {16, 23, 40} (one full workgroup, one with absent trajectory columns, more than one) x launches of {1, 2, 5} steps, each
            twice in a row: the second launch fills the area again.
  layers2   a handle with two hidden layers (layers=2): nhh = 1, one bias vector does not exist and Whp[1] aliases Whp[0].
  reload    new encoder weights loaded into the handle between two launches; the second launch equals the generic kernel's with the new
            weights, and differs from the second launch of the same script without the reload (the area is not a stale copy).
  routing   a logged roll-out and a float32-panel handle report variant 1 in every process.
  oracle    a 3-step launch at B = 16, then one more step: the lift that step stores (kmpc_get_prev_transition) is psi of the 3-step
            launch's final states; oracle.koopman_oracle.mlp_lift of those states with the same weights, within the bound
            tests/test_gpu_parity.py::test_mlp_lift_scaled_dims holds the MLP lift to (1e-12 * max(1, max |psi|)), rows 0-15 (output
            tile 0, from the area) and rows 16-19 (output tile 1, from global memory beside a resident bias) asserted separately.
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

# name -> (B, layers, script).  Script operations: ("roll", steps[, logged]), ("reload", seed), ("psi",): the stored lift of the last step
SCENARIOS = {}
for _B in (16, 23, 40):
    for _k in (1, 2, 5):
        SCENARIOS["steps-B%d-K%d" % (_B, _k)] = (_B, 3, [("roll", _k), ("roll", _k)])
SCENARIOS["layers2"] = (23, 2, [("roll", 3), ("roll", 2)])
SCENARIOS["reload"] = (23, 3, [("roll", 3), ("reload", 6), ("roll", 3)])
SCENARIOS["reload-not"] = (23, 3, [("roll", 3), ("roll", 3)])
SCENARIOS["routing-logged"] = (16, 3, [("roll", 2), ("roll", 2, True), ("roll", 2)])
SCENARIOS["oracle"] = (16, 3, [("roll", 3), ("roll", 1), ("psi",)])
STEP0, SWITCH = 94, 102

CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
from koopmpc import KoopmanMPC, _ffi
from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

_ffi.load().kmpc_set_rollout_workgroup(16)  # (small batches are spread as workgroups of eight otherwise)
L, N = 20, 20
cache = {}

def make(B, layers, **kw):
    w = random_mlp_weights(2, 100, layers, L, seed=5)
    m = KoopmanMPC(n=2, L=L, N=N, batch=B, weights=w, layers=layers, Rw=1.0, **kw)
    if layers not in cache:
        cache[layers] = offline_edmd(lambda X: m.Encoder(X), plant=duffing_rk4)
    m.set_model(*cache[layers])
    assert m.rollout_is_fused()
    return m

out = {}
r = np.tile(np.array([[1.0], [0.0]]), (1, N))
for name, (B, layers, script) in %(scenarios)r.items():
    m = make(B, layers)
    X = torch.tensor(initial_states(B, seed=3), dtype=torch.float64, device="cuda:0").contiguous()
    k, launch = %(step0)d, 0
    for op in script:
        if op[0] == "roll":
            logged = len(op) > 2 and op[2]
            out["%%s/%%d/X_in" %% (name, launch)] = X.cpu().numpy()
            m.rollout("duffing", X, r, op[1], step0=k, switch_step=%(switch)d, log=logged)
            torch.cuda.synchronize()
            t = "%%s/%%d/" %% (name, launch)
            out[t + "variant"] = m.rollout_variant()
            out[t + "resident"] = np.array(m.rollout_resident())
            out[t + "logged"] = int(logged)
            out[t + "X"] = X.cpu().numpy()
            out[t + "status"] = m.status.cpu().numpy()
            out[t + "iters"] = m.iters.cpu().numpy()
            out[t + "state"] = m.state_dict()["blob"].copy()
            for nm, v in zip("ABC", m.get_model()):
                out[t + nm] = v.cpu().numpy()
            k += op[1]
            launch += 1
        elif op[0] == "reload":
            m.set_encoder(random_mlp_weights(2, 100, layers, L, seed=op[1]))
        elif op[0] == "psi":
            psi_p = torch.empty(B, L, dtype=torch.float64, device="cuda:0")
            u_p = torch.empty(B, dtype=torch.float64, device="cuda:0")
            rc = m.lib.kmpc_get_prev_transition(m.h, m._p(psi_p), m._p(u_p), m._stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            out[name + "/psi"] = psi_p.cpu().numpy()
    out[name + "/launches"] = launch
# a float32-panel handle: the generic kernel behind float32 panels in every process
m = make(16, 3, dtype=torch.float32)
X = torch.tensor(initial_states(16, seed=3), dtype=torch.float32, device="cuda:0").contiguous()
m.rollout("duffing", X, r, 2, step0=%(step0)d, switch_step=%(switch)d)
torch.cuda.synchronize()
out["routing-f32/variant"] = m.rollout_variant()
out["routing-f32/resident"] = np.array(m.rollout_resident())
out["routing-f32/X"] = X.cpu().numpy()
out["routing-f32/status"] = m.status.cpu().numpy()
np.savez(%(out)r, **out)
"""

# process -> environment: the parts of the area KMPC_ROLLOUT_RESIDENT allows beside the biases are a mask, 2: output tile 0
PROCESSES = {"default": {}, "bias": {"KMPC_ROLLOUT_RESIDENT": "0"}, "generic": {"KMPC_ROLLOUT_GENERIC": "1"}}
# ... and what a launch of the default-option kernel must then report: (parts, LDS bytes).  18 208 doubles without an area (lift scratch
# 4 096, sixteen per-wave regions of 846, psi and the x slots 576), the biases 256, output tile 0 25 x 64
LDS0 = 18208 * 8
PLAN = {"default": (3, LDS0 + 256 * 8 + 1600 * 8), "bias": (1, LDS0 + 256 * 8), "generic": (0, LDS0)}


def _run_child(tmp, name, extra_env):
    out = os.path.join(str(tmp), name + ".npz")
    code = CHILD % dict(root=ROOT, pkg=PKG, tests=TESTS, scenarios=SCENARIOS, step0=STEP0, switch=SWITCH, out=out)
    env = {k: v for k, v in os.environ.items() if k not in ("KMPC_ROLLOUT_GENERIC", "KMPC_ROLLOUT_RESIDENT")}
    env.update(KMPC_DEBUG="1", **extra_env)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every scenario in each process of PROCESSES, a fresh process each."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    tmp = tmp_path_factory.mktemp("encoder_resident")
    return {name: _run_child(tmp, name, env) for name, env in PROCESSES.items()}


def _same(d, g, name, resident=True):
    """A resident process against the generic one (resident=False: the generic one against itself, for the variants it reports): every
    launch of the scenario, np.array_equal on everything a launch leaves."""
    n = int(d[name + "/launches"])
    assert n == int(g[name + "/launches"]) and n > 0
    for li in range(n):
        t = "%s/%d/" % (name, li)
        want = 2 if resident and not int(d[t + "logged"]) else 1
        assert int(d[t + "variant"]) == want and int(g[t + "variant"]) == 1, (t, int(d[t + "variant"]), int(g[t + "variant"]))
        assert tuple(g[t + "resident"]) == PLAN["generic"], (t, g[t + "resident"])
        if want == 1:
            assert tuple(d[t + "resident"]) == PLAN["generic"], (t, d[t + "resident"])
        for key in ("X", "state", "status", "iters", "A", "B", "C"):
            a, b = d[t + key], g[t + key]
            assert a.shape == b.shape and np.array_equal(a, b) and a.tobytes() == b.tobytes(), (t, key)
        assert np.isfinite(d[t + "X"]).all() and int(d[t + "iters"].min()) >= 1


RESIDENT = [p for p in PROCESSES if p != "generic"]


@pytest.mark.parametrize("proc", RESIDENT)
@pytest.mark.parametrize("name", [n for n in SCENARIOS if n.startswith("steps")] + ["layers2"])
def test_resident_kernel_equals_generic_kernel_after_every_launch(runs, proc, name):
    d = runs[proc]
    _same(d, runs["generic"], name)
    for li in range(int(d[name + "/launches"])):  # the plan the launcher made: the parts in the area and the LDS the launch asked for
        assert tuple(d["%s/%d/resident" % (name, li)]) == PLAN[proc], (proc, name, li, d["%s/%d/resident" % (name, li)])


@pytest.mark.parametrize("proc", RESIDENT)
def test_new_encoder_weights_between_two_launches(runs, proc):
    d, g = runs[proc], runs["generic"]
    _same(d, g, "reload")
    _same(d, g, "reload-not")
    assert np.array_equal(d["reload/0/X"], d["reload-not/0/X"])  # the same first launch ...
    dx = float(np.abs(d["reload/1/X"] - d["reload-not/1/X"]).max())
    print("%s: second launch with new weights against the old ones, max |x| difference %.3e" % (proc, dx))
    assert dx > 1e-6  # ... and a second one that depends on the weights: a stale area would give reload-not's


@pytest.mark.parametrize("proc", list(PROCESSES))
def test_routing_is_unchanged(runs, proc):
    d, g = runs[proc], runs["generic"]
    _same(d, g, "routing-logged", resident=proc != "generic")
    assert int(d["routing-logged/1/variant"]) == 1  # the logged launch: the generic kernel
    assert int(d["routing-logged/0/variant"]) == (1 if proc == "generic" else 2)
    assert int(d["routing-f32/variant"]) == 1 and int(d["routing-f32/resident"][0]) == 0
    assert np.array_equal(d["routing-f32/X"], g["routing-f32/X"]) and np.array_equal(d["routing-f32/status"], g["routing-f32/status"])
    assert np.isfinite(d["routing-f32/X"]).all()


@pytest.mark.parametrize("proc", list(PROCESSES))
def test_stored_lift_against_the_oracle(runs, proc):
    """So that "both kernels wrong alike" cannot pass: the psi the kernel stores against oracle.koopman_oracle.mlp_lift."""
    sys.path[:0] = [p for p in (ROOT, PKG) if p not in sys.path]
    from koopmpc.synth import random_mlp_weights
    from oracle import koopman_oracle as ko

    d = runs[proc]
    _same(d, runs["generic"], "oracle", resident=proc != "generic")
    w = random_mlp_weights(2, 100, 3, 20, seed=5)
    x3 = d["oracle/0/X"]  # the final states of the 3-step launch: what the next launch's only step lifts
    assert np.array_equal(x3, d["oracle/1/X_in"])
    want = ko.mlp_lift(w, x3)  # (L, B)
    got = d["oracle/psi"].T     # stored (B, L)
    assert got.shape == want.shape == (20, 16)
    bound = 1e-12 * max(1.0, float(np.abs(want).max()))  # tests/test_gpu_parity.py::test_mlp_lift_scaled_dims
    e0, e1 = float(np.abs(got[:16] - want[:16]).max()), float(np.abs(got[16:] - want[16:]).max())
    print("%s: |psi - oracle| rows 0-15 %.3e, rows 16-19 %.3e, bound %.3e" % (proc, e0, e1, bound))
    assert e0 <= bound, ("output tile 0 (rows 0-15)", e0, bound)
    assert e1 <= bound, ("output tile 1 (rows 16-19)", e1, bound)
