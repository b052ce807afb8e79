"""The fused roll-out WITHOUT a log -- what bench.py times and a user gets by default: the default-option kernel (rollout_variant() = 2,
csrc/step_body.h RoOpt) at (20, 20, 2) with the MLP lift and at (8, 30, 2) with the RBF lift -- held to the oracle, to
the logged generic kernel and to the per-step route, launch after launch and across hand-overs of the handle's state.
Runs on the MI355X box:  python -m pytest tests/test_gpu_unlogged_rollout.py -m gpu

The harness (Rig).  A case is a script of operations -- "roll out s steps", "set the applied input", "reset", ... -- applied alike to
    U   every roll-out unlogged; after each one rollout_variant() must be the value the script lists (2 or 1), so no case can pass by
        silently running the other kernel;
    G   the same calls with log=True: always the generic kernel (1).  tests/test_gpu_default_option_rollout.py establishes that a logged
        generic launch has the unlogged one's states bit for bit, so a difference between U and G belongs to the default-option kernel
        or to a hand-over into it;
    S   the per-step route, step + plant_step, with the roll-out's switch rule;
    Uq, Gq   as U and G, but nothing reads their state between the launches (a checkpoint makes a handle forget its carried QP tableaux,
        api.hip state_export): what launches hand to each other untouched.
After EVERY roll-out: U against G bit for bit -- X, status, iters, the state_dict() blob, get_model(); Uq against Gq bit for bit -- X,
status, iters (blob and model when the script ends); G against S -- logged inputs and states within 1e-9, A, B, C within 1e-9 relative,
status 0 on all three: the bounds of tests/test_gpu_parity.py::test_rollout_equals_step_plus_plant_loop.

Against the oracle (section 1): per-trajectory OracleController(rls="gain"), teacher-forced on G's logs as test_fused_rollout_vs_oracle
does -- inputs within 1e-6, states within 1e-9 -- with weights and boxes for which a large share of the first inputs is strictly inside
the box (tests/test_unlogged_rollout_cpu.py proves the shares from the oracle alone: 223 / 576 and 565 / 576 at (20, 20), 114 / 280 and
272 / 280 at (8, 30)), and G's final A, B, C against the oracle's: within 8 x the deviation between the oracle's own two RLS forms on
the same transitions (floor 1e-12, relative to max(1, |.|max)); measured on the oracle alone 1.4e-10, 1.4e-10, 2.4e-10 and 4.0e-10.
Measured on the card (cfg2 mixed, cfg2 interior, cfg3 mixed, cfg3 interior): inputs 1.3e-11, 4.7e-12, 5.7e-8, 1.2e-7; states 3.3e-16 at
most; model 3.0e-13, 1.1e-13, 5.0e-11, 5.0e-11 against bounds (from the teacher-forced transitions) of 1.6e-10, 1.9e-10, 3.8e-10, 3.6e-10.
Roll-out against the per-step route over all cases: inputs 1.8e-10, states 4.8e-12, model 7.0e-12 at most.

Teeth: with a library in which the first step of a launch takes u_{k-1} from the (empty) register instead of memory, 44 of the 46 cases of
sections 1 to 4 fail (the two that pass reset the estimator before every later launch: no update reads u_{k-1} there).

Every case uses B <= 64 and at most 18 steps.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import koopman_oracle as ko

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_unlogged_rollout_cpu as inputs  # noqa: E402  (the cases' inputs and the model bound)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "koopman-online-updated-mpc_amd")
TOL = 1e-9  # roll-out against step + plant_step: inputs, states; relative on the model


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


@pytest.fixture(scope="module")
def sixteen(torch_mod):
    """Workgroups of sixteen trajectories for every batch (the library spreads small batches as workgroups of eight otherwise)."""
    from koopmpc import _ffi

    lib = _ffi.load()
    lib.kmpc_set_rollout_workgroup(16)
    yield lib
    lib.kmpc_set_rollout_workgroup(0)


def _rel(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


_MODELS = {}


class Rig:
    """One script on the handles U, G, S (and Uq, Gq): see the module docstring."""

    def __init__(self, torch, KM, set_name, B, kw=None, plant=None, step0=100, switch=102, h=0.05, layers=3, hidden=100, abs_x0=False,
                 quiet=True, no_place=None, dtype=None, use_s=True):
        from koopmpc.synth import initial_states

        self.torch, self.KM, self.set, self.B = torch, KM, set_name, B
        self.L, self.N = inputs.SETS[set_name]
        self.dtype = dtype or torch.float64
        self.kw = dict(kw or {})
        self.layers, self.hidden = layers, hidden
        if set_name == "cfg2":
            from koopmpc.synth import random_mlp_weights

            self.weights = inputs.cfg2_weights() if (layers, hidden) == (3, 100) else random_mlp_weights(2, hidden, layers, self.L, seed=5)
            self.plant = plant or "duffing"
        else:
            self.cx, self.Xo, self.Yo, self.Uo = inputs.cfg3_offline()
            self.plant = plant or "vdp"
        self.k, self.switch, self.hs = step0, switch, h
        self.r = np.tile(np.array([[1.0], [0.0]]), (1, self.N))
        X0 = initial_states(B, seed=3)
        self.X0 = np.abs(X0) if abs_x0 else X0
        self.monkeypatch = no_place
        names = ["U", "G"] + (["S"] if use_s else []) + (["Uq", "Gq"] if quiet else []) + (["Un"] if no_place is not None else [])
        self.h, self.X, self.model0 = {}, {}, None
        for name in names:
            self.make(name)
        self.logs = []     # G's (U_log, X_log) of every launch
        self.variants = []

    # ------------------------------------------------------------------ handles
    def make(self, name):
        torch = self.torch
        if self.set == "cfg2":
            m = self.KM(n=2, L=self.L, N=self.N, batch=self.B, weights=self.weights, layers=self.layers, hidden=self.hidden,
                        dtype=self.dtype, **self.kw)
            key = (self.layers, self.hidden)
            if key not in _MODELS:
                from koopmpc.synth import duffing_rk4, offline_edmd

                enc = m if self.dtype == torch.float64 else self.KM(n=2, L=self.L, N=self.N, batch=1, weights=self.weights,
                                                                    layers=self.layers, hidden=self.hidden)
                _MODELS[key] = offline_edmd(lambda X: enc.Encoder(X), plant=duffing_rk4)
            self.model0 = _MODELS[key]
            m.set_model(*self.model0)
        else:
            m = self.KM(n=2, L=self.L, N=self.N, batch=self.B, centres=self.cx, output="Cx", dtype=self.dtype,
                        **dict(dict(lift="rbf"), **self.kw))
            # vanderpol_RBF.py never restarts its estimator: it continues from the offline samples (:434-438)
            model = [t.cpu().numpy() for t in m.offline_fit(self.Xo, self.Yo, self.Uo, init_rls=True)]
            self.model0 = self.model0 or model
        assert m.rollout_is_fused()
        self.h[name] = m
        self.X[name] = torch.tensor(self.X0, dtype=self.dtype, device="cuda:0").contiguous()
        return m

    def fused(self):
        return [n for n in self.h if n != "S"]

    def every(self, fn):
        for name, m in self.h.items():
            fn(m)

    def switched(self, gi):
        return self.switch >= 0 and gi >= self.switch

    # ------------------------------------------------------------------ the operations
    def roll(self, steps, variant, u_log=False, diag=False, raw=None, check_s=True):
        """One roll-out of `steps` steps on every handle; `variant` is what U must report.  u_log: U logs too; diag: U and G call
        rollout(diagnostics=True); raw: U hands only that panel ("U" or "X") to the C ABI."""
        torch = self.torch
        out = {}
        for name in self.fused():
            m, X = self.h[name], self.X[name]
            logged = name[0] == "G" or u_log or diag
            args = (self.plant, X, self.r, steps)
            kw = dict(step0=self.k, switch_step=self.switch, h=self.hs)
            if name == "Un":
                self.monkeypatch.setenv("KMPC_ROLLOUT_NO_PLACE", "1")
            try:
                if raw and name[0] == "U":
                    res = self._raw(m, X, steps, raw)
                elif diag:
                    res = m.rollout(*args, log=True, diagnostics=True, **kw)
                else:
                    res = m.rollout(*args, log=logged, **kw)
            finally:
                if name == "Un":
                    self.monkeypatch.delenv("KMPC_ROLLOUT_NO_PLACE", raising=False)
            torch.cuda.synchronize()
            want = 1 if name[0] == "G" else variant
            assert m.rollout_variant() == want, (name, m.rollout_variant(), want, len(self.variants))
            out[name] = dict(res=res, status=m.status.clone(), iters=m.iters.clone())
        self.variants.append(variant)
        Ul, Xl = out["G"]["res"][0], out["G"]["res"][1]
        self.logs.append((Ul.cpu().numpy(), Xl.cpu().numpy()))
        # U against G, and every other unlogged handle against U, bit for bit
        for a, b in (("U", "G"), ("Uq", "Gq"), ("Un", "U"), ("U2", "U")):
            if a not in self.h:
                continue
            assert torch.equal(self.X[a], self.X[b]), (a, b, "X", float((self.X[a] - self.X[b]).abs().max()))
            assert torch.equal(out[a]["status"], out[b]["status"]), (a, b, "status")
            assert torch.equal(out[a]["iters"], out[b]["iters"]), (a, b, "iters")
            if a != "Uq":
                self.same_state(a, b)
        if out["U"]["res"] is not None:  # a panel U was handed is G's
            for pa, pb in zip(out["U"]["res"][:2], out["G"]["res"][:2]):
                if pa is not None:
                    assert torch.equal(pa, pb)
            if diag:
                for key in ("Psi", "dA", "dB", "dC"):
                    assert torch.equal(out["U"]["res"][2][key], out["G"]["res"][2][key]), key
        assert int(out["U"]["status"].max().item()) == 0 and int(out["G"]["status"].max().item()) == 0
        # G against the per-step route
        if "S" in self.h and check_s:
            m, worst_u, worst_x = self.h["S"], 0.0, 0.0
            for i in range(steps):
                u = m.step(self.X["S"], self.r).clone()
                assert int(m.status.max().item()) == 0, ("S", i)
                self.X["S"] = m.plant_step(self.plant, self.X["S"], u, h=self.hs, switched=self.switched(self.k + i))
                worst_u = max(worst_u, float((u - Ul[i]).abs().max()))
                worst_x = max(worst_x, float((self.X["S"] - Xl[i]).abs().max()))
            worst_x = max(worst_x, float((self.X["S"] - self.X["G"]).abs().max()))
            dm = max(_rel(a, b) for a, b in zip(self.h["G"].get_model(), m.get_model()))
            print("launch %d (%d steps from %d, variant %d): roll-out vs step loop u %.2e x %.2e model %.2e"
                  % (len(self.variants), steps, self.k, variant, worst_u, worst_x, dm))
            assert worst_u < TOL and worst_x < TOL and dm <= TOL
        self.k += steps
        return out

    def _raw(self, m, X, steps, panel):
        """kmpc_rollout through the C ABI with only one of the two log panels."""
        torch = self.torch
        rr, per = m._ref(self.r)
        Ul = torch.full((steps, self.B), float("nan"), dtype=m.dtype, device=m.device) if panel == "U" else None
        Xl = torch.full((steps, 2, self.B), float("nan"), dtype=m.dtype, device=m.device) if panel == "X" else None
        m._chk(m.lib.kmpc_rollout(m.h, m._plant_id(self.plant), m._p(X), m._p(rr), per, int(steps), int(self.k), int(self.switch), float(self.hs),
                                  m._p(Ul) if Ul is not None else None, m._p(Xl) if Xl is not None else None, m._p(m.status), m._p(m.iters),
                                  m._stream()), "kmpc_rollout")
        torch.cuda.synchronize()
        return Ul, Xl

    def same_state(self, a, b):
        sa, sb = self.h[a].state_dict()["blob"], self.h[b].state_dict()["blob"]
        assert sa.shape == sb.shape and sa.tobytes() == sb.tobytes(), (a, b, "state")
        for name, ta, tb in zip("ABC", self.h[a].get_model(), self.h[b].get_model()):
            assert self.torch.equal(ta, tb), (a, b, name)

    def roll0(self):
        """rollout(steps=0) only prepares the handle: it is no launch and leaves rollout_variant() alone."""
        for name in self.fused():
            m = self.h[name]
            before = m.rollout_variant()
            X = self.X[name].clone()
            res = m.rollout(self.plant, self.X[name], self.r, 0, step0=self.k, switch_step=self.switch, h=self.hs, log=name[0] == "G")
            assert res is None or (res[0].shape[0] == 0 and res[1].shape[0] == 0)
            assert m.rollout_variant() == before and self.torch.equal(self.X[name], X)

    def steps(self, count):
        """Per-step calls on every handle (kmpc_step is no roll-out: rollout_variant() keeps the last roll-out's value)."""
        torch = self.torch
        for i in range(count):
            us = {}
            for name, m in self.h.items():
                before = m.rollout_variant()
                us[name] = m.step(self.X[name], self.r).clone()
                assert m.rollout_variant() == before
                assert int(m.status.max().item()) == 0
                self.X[name] = m.plant_step(self.plant, self.X[name], us[name], h=self.hs, switched=self.switched(self.k))
            for name in self.fused():
                if name != "U":
                    assert torch.equal(us[name], us["U"]) and torch.equal(self.X[name], self.X["U"]), name
            if "S" in self.h:
                assert float((us["S"] - us["U"]).abs().max()) < TOL and float((self.X["S"] - self.X["U"]).abs().max()) < TOL
            self.k += 1

    def clone(self):
        """U's checkpoint into a fresh handle U2, which is rolled out unlogged beside U from here on."""
        m = self.make("U2")
        m.load_state_dict(self.h["U"].state_dict())
        self.X["U2"] = self.X["U"].clone()

    def set_ref(self, per_trajectory):
        r = np.tile(np.array([[1.0], [0.0]]), (1, self.N))
        self.r = np.tile(r[None], (self.B, 1, 1)) * (1.0 + 0.1 * np.random.RandomState(4).rand(self.B, 1, 1)) if per_trajectory else r

    def finish(self):
        if "Uq" in self.h:
            self.same_state("Uq", "Gq")

    def run(self, script):
        for op in script:
            getattr(self, op[0])(*op[1:]) if isinstance(op, tuple) else op(self)
        self.finish()
        return self


def _launches(lengths, variant=2):
    return [("roll", s, variant) for s in lengths]


# ---------------------------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("case", sorted(inputs.CASES))
def test_unlogged_rollout_vs_oracle(torch_mod, KM, sixteen, monkeypatch, case):
    """Section 1: the four cases of tests/test_unlogged_rollout_cpu.py.  The second and third launch of the cfg2 cases (B = 32, six steps
    each) run with the placement table; the cfg2 mixed case drives a fourth unlogged handle under KMPC_ROLLOUT_NO_PLACE (read per launch)
    that must equal U bit for bit."""
    c = inputs.CASES[case]
    L, N = inputs.SETS[c["set"]]
    rig = Rig(torch_mod, KM, c["set"], c["B"], kw=dict(c["kw"], lb=c["lb"], ub=c["ub"]), plant=c["plant"], step0=c["step0"], switch=c["switch"],
              no_place=monkeypatch if case == "cfg2_mixed" else None)
    rig.run(_launches(c["launches"]))
    Ul = np.concatenate([u for u, _ in rig.logs])
    Xl = np.concatenate([x for _, x in rig.logs])
    steps = sum(c["launches"])
    assert Ul.shape == (steps, c["B"])
    A0, B0, C0 = [np.asarray(t, dtype=np.float64) for t in rig.model0]
    start = None
    if c["set"] == "cfg2":
        lift_fn = lambda x: ko.mlp_lift(rig.weights, x)
    else:
        lift_fn = lambda x: ko.rbf_lift(x, rig.cx)
        start = inputs.storage_start(lift_fn, rig.Xo, rig.Yo, rig.Uo)
    r = rig.r
    Ag, Bg, Cg = [t.cpu().numpy() for t in rig.h["G"].get_model()]
    worst_u = worst_x = worst_m = dev = 0.0
    interior = 0
    for b in range(c["B"]):
        ctl = inputs.make_controller(case, lift_fn, L, N, A0, B0, C0, start)
        st = inputs.make_reference_rls(L, start)
        x = rig.X0[:, b].copy()
        for k in range(steps):
            prev = ctl.prev
            uo, _, psi = ctl.step(x, r)
            if prev is not None:
                ko.rls_update_reference(st, prev[0], prev[1], psi, x)
            worst_u = max(worst_u, abs(Ul[k, b] - uo))
            interior += int(c["lb"] < uo < c["ub"])
            # both sides regress on the input that was applied and continue from the GPU's state
            ctl.prev = (ctl.prev[0], float(Ul[k, b]))
            xo = ko.plant_step(c["plant"], x, float(Ul[k, b]), switched=(c["step0"] + k >= c["switch"]))
            worst_x = max(worst_x, float(np.abs(Xl[k, :, b] - xo).max()))
            x = Xl[k, :, b].copy()
        dev = max(dev, inputs.model_deviation(ctl, st))
        worst_m = max(worst_m, inputs.rel(Ag[b], ctl.A), inputs.rel(Bg[b], ctl.B), inputs.rel(Cg[b], ctl.C))
    bound = inputs.model_bound(dev)
    print("%s: max |u - u_oracle| = %.2e, |x - x_oracle| = %.2e; model vs oracle %.2e (bound %.2e); %d / %d oracle inputs interior"
          % (case, worst_u, worst_x, worst_m, bound, interior, steps * c["B"]))
    assert interior >= c["interior"] * steps * c["B"]
    assert bound < inputs.MODEL_BOUND_MAX
    assert worst_u < 1e-6 and worst_x < 1e-9
    assert worst_m <= bound


# ---------------------------------------------------------------------------------------------------------------- 2. shapes, launch lengths
BASE = {"cfg2": dict(kw=dict(Rw=1.0)), "cfg3": dict(kw=dict(lb=-6.0, ub=6.0))}  # the inputs of the two mixed cases
STEP0 = {"cfg2": dict(step0=98, switch=102), "cfg3": dict(step0=0, switch=7)}


def _rig(torch_mod, KM, set_name, B, kw=None, **more):
    return Rig(torch_mod, KM, set_name, B, kw=dict(BASE[set_name]["kw"], **(kw or {})), **dict(STEP0[set_name], **more))


@pytest.mark.parametrize("B", [1, 7, 17, 23, 64])
@pytest.mark.parametrize("set_name", ["cfg2", "cfg3"])
def test_batches_and_launch_lengths(torch_mod, KM, sixteen, set_name, B):
    """Section 2.  B = 1: only wave 0 is live while the encoder's tile waves work for dead trajectories; 7: only waves with an encoder
    tile; 17, 23: a second workgroup with one and seven live waves; 64: four full workgroups.  Launches of 1, 1, 2, 5 and 3 steps in a
    row: a one-step launch never uses the carried u, the five-step one arms the placement of the last launch at B = 64."""
    _rig(torch_mod, KM, set_name, B).run(_launches((1, 1, 2, 5, 3)))


def test_two_hidden_layers(torch_mod, KM, sixteen):
    """(20, 20, 2) with layers=2: nhh = 1, the tile-less waves meet another number of barriers.  Against the twins only (cond(H) reaches
    5e7 on these inputs: no oracle)."""
    _rig(torch_mod, KM, "cfg2", 32, layers=2).run(_launches((1, 5, 3)))


# ---------------------------------------------------------------------------------------------------------------- 3. launch arguments
ARGUMENTS = {
    "box": ("cfg2", dict(kw=dict(lb=-1.0, ub=1.0))),
    "box_asymmetric": ("cfg2", dict(kw=dict(lb=-1.5, ub=0.5))),
    "weights": ("cfg2", dict(kw=dict(Qw=10.0, Rw=0.5))),
    "rls_scales": ("cfg2", dict(kw=dict(P0=1e3, barQ0=10.0))),
    "vdp": ("cfg2", dict(plant="vdp")),
    "tank": ("cfg2", dict(plant="tank", abs_x0=True)),
    "duffing_matlab": ("cfg2", dict(plant="duffing_matlab")),
    "vdp_matlab": ("cfg2", dict(plant="vdp_matlab")),
    "h": ("cfg2", dict(h=0.02)),
    "switch_negative": ("cfg2", dict(step0=100, switch=-1)),
    "switch_before_step0": ("cfg2", dict(step0=100, switch=99)),
    "switch_at_step0": ("cfg2", dict(step0=100, switch=100)),
    "switch_first_step_of_a_launch": ("cfg2", dict(step0=100, switch=103)),
    "switch_last_step_of_a_launch": ("cfg2", dict(step0=100, switch=105)),
    "rbf_matlab": ("cfg3", dict(kw=dict(lift="rbf_matlab"))),
    "rbf_eps": ("cfg3", dict(kw=dict(rbf_eps=1e-2))),
    "cfg3_box_asymmetric": ("cfg3", dict(kw=dict(lb=-4.0, ub=1.0))),
    "cfg3_duffing_h": ("cfg3", dict(plant="duffing", h=0.02)),
}


@pytest.mark.parametrize("name", list(ARGUMENTS))
def test_arguments_that_stay_launch_arguments(torch_mod, KM, sixteen, name):
    """Section 3: box, weights, RLS scales, plant kind and Runge-Kutta form, step size, the switch, the RBF form and eps are arguments of
    the default-option kernel too (variant 2); one it froze or mis-read shows against the per-step route.  Two launches of 3 steps."""
    set_name, more = ARGUMENTS[name]
    more = dict(more)
    _rig(torch_mod, KM, set_name, 23, kw=more.pop("kw", None), **more).run(_launches((3, 3)))


# ---------------------------------------------------------------------------------------------------------------- 4. hand-overs
def _applied(rig):
    v = np.linspace(-0.9, 0.9, rig.B) * min(abs(rig.h["U"].cfg.lb), abs(rig.h["U"].cfg.ub))  # inside the box, one value per trajectory
    rig.every(lambda m: m.set_applied_input(v))


def _another_model(rig):
    from koopmpc.synth import duffing_rk4, offline_edmd

    model = offline_edmd(lambda X: rig.h["S"].Encoder(X), plant=duffing_rk4, n_steps=60, n_traj=80, seed=7)
    assert inputs.rel(model[0], rig.model0[0]) > 1e-3
    rig.every(lambda m: m.set_model(*model))


def _offline_fit(rig):
    from koopmpc.synth import offline_data

    rig.every(lambda m: m.offline_fit(*offline_data(), ridge=1e-8, init_rls=True))


PN = np.array([[150.0, 5.0], [5.0, 120.0]])
R3 = ("roll", 3, 2)
HANDOVERS = {
    "applied_input": [R3, _applied, R3],
    "per_step_calls": [R3, ("steps", 2), R3],
    "reset_and_state_init": [R3, lambda rig: rig.every(lambda m: m.reset()), R3, lambda rig: rig.every(lambda m: m.state_init(P0=1e5, barQ0=1e5)), R3],
    "checkpoint": [R3, ("clone",), R3],
    "update_off_and_on": [R3, lambda rig: rig.every(lambda m: m.set_online_update(False)), ("roll", 3, 1),
                          lambda rig: rig.every(lambda m: m.set_online_update(True)), R3],
    "terminal_weight": [R3, lambda rig: rig.every(lambda m: m.set_terminal_weight(PN)), ("roll", 3, 1),
                        lambda rig: rig.every(lambda m: m.set_terminal_weight(None)), R3],
    "no_steps": [R3, ("roll0",), R3],
    "reference_per_trajectory": [R3, ("set_ref", True), ("roll", 3, 1), ("set_ref", False), R3],
    "set_model": [R3, _another_model, R3],
    "offline_fit": [R3, _offline_fit, R3],
    "alternating_log": [("roll", 3, 1, True), R3, ("roll", 3, 1, True), R3],
}
CFG3_HANDOVERS = ["applied_input", "per_step_calls", "reset_and_state_init"]


@pytest.mark.parametrize("set_name,name", [("cfg2", n) for n in HANDOVERS] + [("cfg3", n) for n in CFG3_HANDOVERS])
def test_handovers_between_launches(torch_mod, KM, sixteen, set_name, name):
    """Section 4: the state of a default-option handle changed between launches of 3 steps, B = 16 -- where a value carried in registers
    instead of re-read from memory would go wrong.  The first step after set_applied_input must regress on the given input."""
    _rig(torch_mod, KM, set_name, 16).run(HANDOVERS[name])


# ---------------------------------------------------------------------------------------------------------------- 5. the predicate
def _per_trajectory_terminal(rig):
    rig.every(lambda m: m.terminal_from_dare(per_trajectory=True))


def _diagnostics(on):
    return lambda rig: [rig.h[n].set_rollout_diagnostics(on) for n in rig.fused()]


PREDICATE = {
    # name: (constructor options, script)
    "c_skip_first": (dict(kw=dict(c_skip_first=True)), [("roll", 3, 1), ("roll", 3, 1)]),
    "qp_max_iter_plus_one": (dict(kw=dict(qp_max_iter=8 * 20 + 41)), [("roll", 3, 1), ("roll", 3, 1)]),
    "qp_max_iter_explicit_default": (dict(kw=dict(qp_max_iter=8 * 20 + 40)), [R3, R3]),
    "terminal_per_trajectory": (dict(), [R3, _per_trajectory_terminal, ("roll", 3, 1)]),
    "terminal_refresh": (dict(), [R3, lambda rig: rig.every(lambda m: m.set_terminal_refresh(every=2)), ("roll", 3, 1)]),
    # armed diagnostics: plain kmpc_rollout without a log passes no diagnostic logs (2); rollout(diagnostics=True) is the DIAG object (1)
    "diagnostics": (dict(), [_diagnostics(True), R3, ("roll", 3, 1, False, True), R3, _diagnostics(False), R3]),
    "c_abi_only_u_log": (dict(), [R3, ("roll", 3, 1, False, False, "U"), R3]),
    "c_abi_only_x_log": (dict(), [R3, ("roll", 3, 1, False, False, "X"), R3]),
    "hidden_64": (dict(hidden=64), [("roll", 3, 1), ("roll", 3, 1)]),
    "per_step_calls_keep_the_variant": (dict(), [("roll", 3, 1, True), ("steps", 1), R3, ("steps", 1), ("roll", 3, 1, True)]),
}


@pytest.mark.parametrize("name", list(PREDICATE))
def test_the_rest_of_the_predicate(torch_mod, KM, sixteen, name):
    """Section 5: options of DESIGN.md 4.1's list that tests/test_gpu_default_option_rollout.py::test_routing_of_non_default_options
    leaves out.  (20, 20, 2), B = 16, launches of 3 steps; a predicate that lost a line would run the default-option kernel (2) where
    1 is listed and compute the default behaviour, which shows against S."""
    opts, script = PREDICATE[name]
    opts = dict(opts)
    _rig(torch_mod, KM, "cfg2", 16, kw=opts.pop("kw", None), **opts).run(script)


@pytest.mark.parametrize("wg", [8, 4])
def test_other_workgroup_sizes_are_generic(torch_mod, KM, sixteen, wg):
    """kmpc_set_rollout_workgroup(8) and (4) at (20, 20, 2): the default-option kernel is built for sixteen waves only."""
    try:
        assert sixteen.kmpc_set_rollout_workgroup(wg) == 0
        _rig(torch_mod, KM, "cfg2", 16).run([("roll", 3, 1), ("roll", 3, 1)])
    finally:
        sixteen.kmpc_set_rollout_workgroup(16)


def test_float32_handle_is_never_the_default_option_kernel(torch_mod, KM, sixteen):
    """A float32 handle at (20, 20, 2) (float32 panels around the float64 roll-out): variant 1 with and without a log, the unlogged
    launches bit for bit the logged ones.  (The float32 panels round X to 6e-8 relative at every step: the per-step comparison to 1e-9 is
    not this format's; tests/test_gpu_float32.py holds the float32 routes to the float32 oracle.)"""
    _rig(torch_mod, KM, "cfg2", 16, dtype=torch_mod.float32, use_s=False).run([("roll", 3, 1), ("roll", 3, 1)])


CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import test_gpu_unlogged_rollout as t
from koopmpc import KoopmanMPC, _ffi
_ffi.load().kmpc_set_rollout_workgroup(16)
rig = t._rig(torch, KoopmanMPC, "cfg2", 16, quiet=False, use_s=False)
m, X = rig.h["U"], rig.X["U"]
m.rollout(rig.plant, X, rig.r, 6, step0=rig.k, switch_step=rig.switch)
torch.cuda.synchronize()
A, B, C = m.get_model()
np.savez(%(out)r, variant=m.rollout_variant(), status=m.status.cpu().numpy(), X=X.cpu().numpy(), A=A.cpu().numpy(), B=B.cpu().numpy(), C=C.cpu().numpy())
"""


def test_qp_predict_off_is_generic(torch_mod, KM, sixteen, tmp_path):
    """KMPC_QP_PREDICT=0 (read once per process: one child): the cfg2 mixed inputs for 6 steps at B = 16 run the generic kernel, and
    leave the states and the model of this process's default run (variant 2) to 1e-9."""
    out = str(tmp_path / "predict0.npz")
    code = CHILD % dict(root=ROOT, pkg=PKG, tests=os.path.join(ROOT, "tests"), out=out)
    env = dict(os.environ, KMPC_DEBUG="1", KMPC_QP_PREDICT="0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    d = np.load(out)
    assert int(d["variant"]) == 1 and int(d["status"].max()) == 0
    rig = _rig(torch_mod, KM, "cfg2", 16, quiet=False, use_s=False)
    rig.run([("roll", 6, 2)])
    X = rig.X["U"].cpu().numpy()
    worst_x = float(np.abs(d["X"] - X).max())
    worst_m = max(inputs.rel(d[k], t.cpu().numpy()) for k, t in zip("ABC", rig.h["U"].get_model()))
    print("KMPC_QP_PREDICT=0 against the default run: x %.2e model %.2e" % (worst_x, worst_m))
    assert worst_x < TOL and worst_m <= TOL
