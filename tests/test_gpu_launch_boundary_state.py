"""The state a launch of the default-option roll-out kernel keeps to itself until its last steps (csrc/step_body.h RoOpt::LB):
psi_now is stored by the last two steps of a launch, the warm start travels from solve to solve in LDS and U0, u_store and the state are
stored by the last step.  Runs on the MI355X box:  python -m pytest tests/test_gpu_launch_boundary_state.py -m gpu

Every case is the default-option kernel (rollout_variant() = 2) against the generic kernel (1, KMPC_ROLLOUT_GENERIC: read once per process,
so each side is one fresh child process that runs all the scenarios) BIT FOR BIT after every launch: X, the checkpoint (kmpc_state_export:
the RLS state, psi(x_k), the warm start, u_k), get_model(), status and iters.

Scenarios.  Sets (20, 20, 2) with the MLP lift and (8, 30, 2) with the RBF lift, with the boxes and weights of
tests/test_unlogged_rollout_cpu.py's mixed cases (Rw = 1, +-2 and +-6: first inputs on the box and strictly inside it).
  steps      B in {16, 23, 40} (a full workgroup, one with dead waves, more than one) x launch lengths {1, 2, 3, 5} (first = last; the
             "last two" rule with two steps only; both ping-pong parities), each launch twice in a row: the second one starts from what
             the first one left.
  split      launches of 1 + 2 + 3 steps and one launch of 6 from the same start; the two ends agree within the 1e-9 that
             tests/test_gpu_unlogged_rollout.py gives routes that differ in what a solve starts from (a launch starts without a
             carried tableau).
  hand-overs roll-out -> step() x 2 -> roll-out;  roll-out -> checkpoint -> a fresh handle -> roll-out;  roll-out -> logged roll-out
             (generic in both processes) -> roll-out;  set_applied_input between two launches.
  interior   the interior cases (Qw = 1, Rw = 1, +-2; Rw = 1, +-20).
  active set the (20, 20, 2) mixed case over 6 + 6 + 6 steps across the plant switch, with a logged twin: first inputs must leave and
             reach the box from step to step inside a launch, so the parked minimiser is read after prediction rounds have written the
             solver's hand-over vector.
  fall-back  256 trajectories, 25 steps after a reset (P0 = 1e4, the default weights: the post-reset window of bench.py).  A logged twin
             run as 25 one-step launches gives per-step iters on the generic kernel; a solve that reached the hand-over to the active-set
             loop of qp_lds shows as iters >= N.  The unlogged handle runs the same 25 steps as launches of 5: hand-overs in the middle
             of a launch must leave the next step its warm start.

Measured on the card: all 38 cases bit for bit; split launches end within 1.5e-14 (cfg2) and 1.9e-13 (cfg3) of the single launch; 80 first
inputs change sides inside a launch in the active-set case; 151 of 6 400 solves reach the hand-over, at steps 0, 2, 3, 4, 5 and 9.
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

MIXED = {"cfg2": dict(Rw=1.0), "cfg3": dict(lb=-6.0, ub=6.0)}
INTERIOR = {"cfg2": dict(Qw=1.0, Rw=1.0), "cfg3": dict(lb=-20.0, ub=20.0, Rw=1.0)}
R3 = ("roll", 3)

# name -> (set, B, constructor options, script).  Script operations: ("roll", steps[, logged]), ("steps", count), ("clone",),
# ("applied",), ("reset",), ("probe", count): `count` logged one-step launches on the twin handle P.
SCENARIOS = {}
for _s in ("cfg2", "cfg3"):
    for _B in (16, 23, 40):
        for _k in (1, 2, 3, 5):
            SCENARIOS["steps-%s-B%d-K%d" % (_s, _B, _k)] = (_s, _B, MIXED[_s], [("roll", _k), ("roll", _k)])
    SCENARIOS["split-%s-123" % _s] = (_s, 23, MIXED[_s], [("roll", 1), ("roll", 2), ("roll", 3)])
    SCENARIOS["split-%s-6" % _s] = (_s, 23, MIXED[_s], [("roll", 6)])
    SCENARIOS["handover-%s-per_step_calls" % _s] = (_s, 16, MIXED[_s], [R3, ("steps", 2), R3])
    SCENARIOS["handover-%s-checkpoint" % _s] = (_s, 16, MIXED[_s], [R3, ("clone",), R3])
    SCENARIOS["handover-%s-logged_between" % _s] = (_s, 16, MIXED[_s], [R3, ("roll", 3, True), R3])
    SCENARIOS["handover-%s-applied_input" % _s] = (_s, 16, MIXED[_s], [R3, ("applied",), R3])
    SCENARIOS["interior-%s" % _s] = (_s, 23, INTERIOR[_s], [("roll", 5), ("roll", 2)])
SCENARIOS["active_set-cfg2"] = ("cfg2", 32, MIXED["cfg2"], [("probe", 18), ("roll", 6), ("roll", 6), ("roll", 6)])
SCENARIOS["fallback-cfg2"] = ("cfg2", 256, {}, [("reset",), ("probe", 25)] + [("roll", 5)] * 5)
STEP0 = {"cfg2": (94, 102), "cfg3": (0, 7)}

CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
from koopmpc import KoopmanMPC, _ffi
from koopmpc.synth import duffing_rk4, initial_states, offline_edmd
import test_unlogged_rollout_cpu as inputs

_ffi.load().kmpc_set_rollout_workgroup(16)  # (small batches are spread as workgroups of eight otherwise)
SETS = {"cfg2": (20, 20), "cfg3": (8, 30)}
cache = {}

def make(set_name, B, kw):
    L, N = SETS[set_name]
    if set_name == "cfg2":
        m = KoopmanMPC(n=2, L=L, N=N, batch=B, weights=inputs.cfg2_weights(), **kw)
        if "model" not in cache:
            cache["model"] = offline_edmd(lambda X: m.Encoder(X), plant=duffing_rk4)
        m.set_model(*cache["model"])
    else:
        if "off" not in cache:
            cache["off"] = inputs.cfg3_offline()
        cx, Xo, Yo, Uo = cache["off"]
        m = KoopmanMPC(n=2, L=L, N=N, batch=B, centres=cx, output="Cx", **dict(dict(lift="rbf"), **kw))
        m.offline_fit(Xo, Yo, Uo, init_rls=True)
    assert m.rollout_is_fused()
    return m

out = {}
for name, (set_name, B, kw, script) in %(scenarios)r.items():
    L, N = SETS[set_name]
    plant = "duffing" if set_name == "cfg2" else "vdp"
    step0, switch = %(step0)r[set_name]
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = initial_states(B, seed=3)
    hs = {"U": make(set_name, B, kw)}
    Xs = {"U": torch.tensor(X0, dtype=torch.float64, device="cuda:0").contiguous()}
    k, launch = step0, 0
    for op in script:
        if op[0] == "roll":
            logged = len(op) > 2 and op[2]
            for h in sorted(hs):
                m, X = hs[h], Xs[h]
                res = m.rollout(plant, X, r, op[1], step0=k, switch_step=switch, log=logged)
                torch.cuda.synchronize()
                t = "%%s/%%s.%%d/" %% (name, h, launch)
                out[t + "variant"] = m.rollout_variant()
                out[t + "logged"] = int(logged)
                out[t + "X"] = X.cpu().numpy()
                out[t + "status"] = m.status.cpu().numpy()
                out[t + "iters"] = m.iters.cpu().numpy()
                out[t + "state"] = m.state_dict()["blob"].copy()
                for nm, v in zip("ABC", m.get_model()):
                    out[t + nm] = v.cpu().numpy()
            k += op[1]
            launch += 1
        elif op[0] == "steps":
            for i in range(op[1]):
                for h in sorted(hs):
                    m = hs[h]
                    u = m.step(Xs[h], r).clone()
                    Xs[h] = m.plant_step(plant, Xs[h], u, switched=(switch >= 0 and k >= switch))
                k += 1
        elif op[0] == "clone":
            hs["U2"] = make(set_name, B, kw)
            hs["U2"].load_state_dict(hs["U"].state_dict())
            Xs["U2"] = Xs["U"].clone()
        elif op[0] == "applied":
            v = np.linspace(-0.9, 0.9, B) * min(abs(hs["U"].cfg.lb), abs(hs["U"].cfg.ub))
            for h in hs:
                hs[h].set_applied_input(v)
        elif op[0] == "reset":
            for h in hs:
                hs[h].reset()
        elif op[0] == "probe":
            # a twin from the same start, logged one-step launches (the generic kernel in either process): per-step inputs and iters
            p = make(set_name, B, kw)
            if ("reset",) in script:
                p.reset()
            Xp = Xs["U"].clone()
            U, it, st = [], [], []
            for i in range(op[1]):
                res = p.rollout(plant, Xp, r, 1, step0=k + i, switch_step=switch, log=True)
                torch.cuda.synchronize()
                assert p.rollout_variant() == 1
                U.append(res[0][0].cpu().numpy()); it.append(p.iters.cpu().numpy().copy()); st.append(p.status.cpu().numpy().copy())
            out[name + "/probe/U"] = np.array(U); out[name + "/probe/iters"] = np.array(it); out[name + "/probe/status"] = np.array(st)
            out[name + "/probe/box"] = np.array([p.cfg.lb, p.cfg.ub])
    out[name + "/launches"] = launch
    out[name + "/handles"] = np.array(sorted(h for h in hs))
np.savez(%(out)r, **out)
"""


def _run_child(tmp, name, extra_env):
    out = os.path.join(str(tmp), name + ".npz")
    code = CHILD % dict(root=ROOT, pkg=PKG, tests=TESTS, scenarios=SCENARIOS, step0=STEP0, out=out)
    env = {k: v for k, v in os.environ.items() if k != "KMPC_ROLLOUT_GENERIC"}
    env.update(KMPC_DEBUG="1", **extra_env)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """Every scenario once as it comes and once under KMPC_ROLLOUT_GENERIC, a fresh process each."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    tmp = tmp_path_factory.mktemp("launch_boundary")
    return _run_child(tmp, "default", {}), _run_child(tmp, "generic", {"KMPC_ROLLOUT_GENERIC": "1"})


def _same(d, g, name):
    """Default-option child against generic child: every launch of every unlogged-capable handle of the scenario, bit for bit."""
    n = int(d[name + "/launches"])
    assert n == int(g[name + "/launches"]) and n > 0
    for h in d[name + "/handles"]:
        for li in range(n):
            t = "%s/%s.%d/" % (name, h, li)
            if t + "variant" not in d:
                continue  # (a handle cloned later in the script)
            want = 1 if int(d[t + "logged"]) else 2
            assert int(d[t + "variant"]) == want and int(g[t + "variant"]) == 1, (t, int(d[t + "variant"]), int(g[t + "variant"]))
            for key in ("X", "state", "status", "iters", "A", "B", "C"):
                a, b = d[t + key], g[t + key]
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (t, key)
            assert np.isfinite(d[t + "X"]).all() and int(d[t + "iters"].min()) >= 1


@pytest.mark.parametrize("name", [n for n in SCENARIOS if n.split("-")[0] in ("steps", "handover", "interior")])
def test_default_option_kernel_equals_generic_kernel_after_every_launch(both, name):
    d, g = both
    _same(d, g, name)
    if name.startswith("handover") and "checkpoint" in name:
        assert "%s/U2.1/variant" % name in d  # the restored handle was rolled out


@pytest.mark.parametrize("set_name", ["cfg2", "cfg3"])
def test_split_launches(both, set_name):
    d, g = both
    a, b = "split-%s-123" % set_name, "split-%s-6" % set_name
    _same(d, g, a)
    _same(d, g, b)
    dx = float(np.abs(d[a + "/U.2/X"] - d[b + "/U.0/X"]).max())
    print("split %s: 1 + 2 + 3 steps against 6, max |x| difference %.2e" % (set_name, dx))
    assert dx < 1e-9


def test_active_set_changes_inside_a_launch(both):
    d, g = both
    name = "active_set-cfg2"
    _same(d, g, name)
    U, (lb, ub) = g[name + "/probe/U"], g[name + "/probe/box"]
    on = (U == lb) | (U == ub)
    # first inputs that leave or reach the box between two consecutive steps which are not the first step of a launch of 6
    change = on[1:] != on[:-1]
    inside = np.array([(i + 1) % 6 != 0 for i in range(change.shape[0])])
    count = int(change[inside].sum())
    print("active set: %d first inputs change sides between steps inside a launch (%d on the box, %d inside)" % (count, int(on.sum()), int((~on).sum())))
    assert count >= 8 and on.any() and (~on).any()
    assert int(g[name + "/probe/status"].max()) == 0


def test_fall_back_inside_a_launch(both):
    d, g = both
    name = "fallback-cfg2"
    _same(d, g, name)
    it = g[name + "/probe/iters"]  # (25, B): per-step iters of the generic kernel
    N = 20
    handed = it >= N
    steps_with = np.nonzero(handed.any(axis=1))[0]
    print("fall-back: %d solves of %d reached the hand-over (iters >= N), at steps %s; largest iters %d"
          % (int(handed.sum()), it.size, steps_with.tolist(), int(it.max())))
    # at least one of them not in the last step of a launch of 5: the step behind it reads the warm start the fall-back left
    assert any(s % 5 != 4 for s in steps_with), steps_with
