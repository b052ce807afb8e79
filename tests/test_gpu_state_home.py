"""Where a handle's state is valid (csrc/state_home.h: StateHome, Progress) as seen through the public entry points.
Runs on the MI355X box:  python -m pytest tests/test_gpu_state_home.py -m gpu

The per-trajectory state has a dense form and, on handles with a fused roll-out, a fast form that the roll-out advances: the wave
image of a float64 handle, the float64 core of a float32 handle.  Every case here uses the smallest dimension set whose
register-state fused roll-out is built in for both float64 and float32 panels, (L, N, q) = (8, 10, 2), with an MLP lift of two hidden
layers of 16, B = 32 and the Duffing plant, once as KMPC_F64 and once as KMPC_F32; kmpc_rollout_plugin_status is 0 (no plug-in).
All comparisons are bitwise (torch.equal): nothing here depends on a tolerance.

The edges of the Home diagram and the case that walks each:
  Dense -> Fast, take fast (converts)      the first roll-out of every case here (the handle comes from kmpc_set_model or an import)
  Fast  -> Both, dense read (converts)     test_read_only_calls_leave_the_rollout_untouched: get_model / condense after a roll-out
  Both  -> Fast, take fast (no conversion) the same case: the next roll-out of handle A; float32: the core is NOT pushed again, which
                                           would round its float64 state and part from handle B
  Both  -> Dense, drop fast                test_exporter_and_importer_continue_alike[*f32*]: export / pack of the whole batch on a
                                           float32 handle; at (20, 20, 2) also test_gpu_round5.py::test_f32_handle_mixes_rollouts_and_per_step_calls
                                           (checkpoint) and test_gpu_state_rows.py::test_whole_handle_round_trip_reproduces_the_blob[mlp32]
  Both  -> Both, export on float64         test_exporter_and_importer_continue_alike[*f64*] (the image stays valid: no conversion)
  any   -> Dense, dense overwritten        the importers of test_exporter_and_importer_continue_alike: a fresh handle (Dense) and a
                                           handle that has rolled out (Fast); test_gpu_state_blob_layout.py holds the bytes
  Dense / Both -> Fast by steps = 0        test_rollout_without_steps_changes_nothing_observable
  Both  -> Dense, dense write              test_reset_after_a_read_restarts_like_a_reset_after_a_rollout (handle A)
  Fast  -> Dense, dense write (converts)   the same case (handle B); float32, kmpc_step after a roll-out:
                                           test_gpu_round5.py::test_f32_handle_mixes_rollouts_and_per_step_calls; float64, rows into a
                                           handle that is rolling: test_gpu_state_rows.py::test_scatter_into_a_running_handle[mlp64]
The estimator's progress on the device route (Progress::advance): test_estimator_status_follows_the_progress_rule.

launch_state_to_image / launch_image_to_state (csrc/aux_kernels.hip, state_image_kernel) move elements without arithmetic and the
float32 <-> float64 casts of float32-representable values are exact, so the steps = 0 case asserts bitwise equality for both dtypes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, N, B, HID = 8, 10, 32, 16
DTYPES = ["f64", "f32"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    return torch


class Setup:
    """weights, offline model, reference and initial states, computed once; handles of either dtype"""

    def __init__(self, torch):
        from koopmpc import KoopmanMPC
        from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

        self.torch, self.KM = torch, KoopmanMPC
        self.w = random_mlp_weights(2, HID, 2, L, seed=7)
        probe = self.make("f64", model=False)
        self.model = offline_edmd(lambda X: np.asarray(probe.Encoder(X), dtype=np.float64), plant=duffing_rk4)
        self.r = np.tile(np.array([[1.0], [0.0]]), (1, N))
        self.X0 = initial_states(B, seed=3)

    def tdt(self, dt):
        return self.torch.float64 if dt == "f64" else self.torch.float32

    def make(self, dt, model=True):
        m = self.KM(n=2, L=L, N=N, batch=B, weights=self.w, hidden=HID, layers=2, dtype=self.tdt(dt), device="cuda:0")
        if model:
            m.set_model(*self.model)
            assert m.rollout_is_fused() and m.rollout_plugin_status()[0] == 0, m.rollout_plugin_status()
        return m

    def states(self, dt):
        return self.torch.tensor(self.X0, dtype=self.tdt(dt), device="cuda:0").contiguous()

    def roll(self, m, X, steps, step0):
        Ul, Xl = m.rollout("duffing", X, self.r, steps, step0=step0, log=True)
        assert bool(self.torch.isfinite(Ul).all()) and bool(self.torch.isfinite(Xl).all())
        return Ul, Xl


@pytest.fixture(scope="module")
def su(torch_mod):
    return Setup(torch_mod)


def _same(torch, a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dt", DTYPES)
def test_read_only_calls_leave_the_rollout_untouched(su, dt):
    """Handle A runs roll-outs of 3, 4 and 3 steps with get_model, condense, estimator_status and state_bytes between them, handle B
    only the roll-outs: U_log, X_log and the final get_model are bitwise equal.  The reads bring A to Both; neither dtype converts
    back before the next roll-out (a float32 handle that pushed its rounded blocks to the core would part from B)."""
    torch = su.torch
    A, Bh = su.make(dt), su.make(dt)
    Xa, Xb = su.states(dt), su.states(dt)
    step0 = 0
    for steps in (3, 4, 3):
        la = su.roll(A, Xa, steps, step0)
        lb = su.roll(Bh, Xb, steps, step0)
        assert _same(torch, la, lb) and torch.equal(Xa, Xb), (dt, step0)
        step0 += steps
        A.get_model()
        H, f = A.condense(A.Encoder(Xa), su.r)
        assert bool(torch.isfinite(H).all()) and bool(torch.isfinite(f).all())
        assert A.estimator_status()[:2] == Bh.estimator_status()[:2]
        assert A.lib.kmpc_state_bytes(A.h) == Bh.lib.kmpc_state_bytes(Bh.h) > 80
    assert _same(torch, A.get_model(), Bh.get_model())


@pytest.mark.parametrize("how", ["blob", "rows"])
@pytest.mark.parametrize("dt", DTYPES)
def test_exporter_and_importer_continue_alike(su, dt, how):
    """A roll-out of 3 steps, then the state leaves the handle -- kmpc_state_export, or kmpc_state_pack of the whole batch -- and the
    same handle rolls 4 more steps; a fresh handle, and one that has already rolled out on other states, take the state in
    (kmpc_state_import / kmpc_state_unpack) and roll the same 4 steps: bitwise equal logs.  On float32 the exporter continues from its
    rounded float32 blocks as the importers do (drop_fast), not from its core's float64 state."""
    torch = su.torch
    src = su.make(dt)
    X = su.states(dt)
    su.roll(src, X, 3, 0)
    fresh, used = su.make(dt), su.make(dt)
    Xu = torch.flip(su.states(dt), dims=[1]).contiguous()
    su.roll(used, Xu, 3, 0)
    if how == "blob":
        blob = src.state_to()
        for m in (fresh, used):
            m.state_from(blob)
    else:
        rows = src.pack_state()
        for m in (fresh, used):
            m.unpack_state(rows)
    assert fresh.estimator_status()[:2] == used.estimator_status()[:2] == src.estimator_status()[:2] == (True, False)
    logs = []
    for m in (src, fresh, used):
        Xm = X.clone()
        logs.append(su.roll(m, Xm, 4, 3) + (Xm,) + tuple(m.get_model()))
    assert _same(torch, logs[0], logs[1]), (dt, how, "fresh importer")
    assert _same(torch, logs[0], logs[2]), (dt, how, "importer that had rolled out")


@pytest.mark.parametrize("dt", DTYPES)
def test_rollout_without_steps_changes_nothing_observable(su, dt):
    """kmpc_rollout with steps = 0 only prepares the fast form: get_model before and after it is bitwise equal -- from Both (after a
    roll-out and the first get_model) and from Dense (after an import, where the call converts), and the roll-out behind it equals the
    roll-out of a handle that was not prepared."""
    torch = su.torch
    m, twin = su.make(dt), su.make(dt)
    X, Xt = su.states(dt), su.states(dt)
    su.roll(m, X, 3, 0)
    su.roll(twin, Xt, 3, 0)
    before = m.get_model()
    st = m.estimator_status()
    assert m.rollout("duffing", X, su.r, 0) is None
    assert m.estimator_status() == st and torch.equal(X, Xt)
    assert _same(torch, before, m.get_model())
    blob = m.state_to()
    for h in (m, twin):
        h.state_from(blob)  # Dense on both
    before = m.get_model()
    m.rollout("duffing", X, su.r, 0)
    assert _same(torch, before, m.get_model())
    m.rollout("duffing", X, su.r, 0)
    assert _same(torch, su.roll(m, X, 3, 3), su.roll(twin, Xt, 3, 3)) and torch.equal(X, Xt)


@pytest.mark.parametrize("dt", DTYPES)
def test_reset_after_a_read_restarts_like_a_reset_after_a_rollout(su, dt):
    """kmpc_reset writes the dense blocks: from Both (handle A, after get_model) and from Fast (handle B) it leaves the same state,
    and the next roll-out starts from it, not from the fast form the reset left behind."""
    torch = su.torch
    A, Bh = su.make(dt), su.make(dt)
    Xa, Xb = su.states(dt), su.states(dt)
    su.roll(A, Xa, 3, 0)
    su.roll(Bh, Xb, 3, 0)
    kept = A.get_model()
    A.reset()
    Bh.reset()
    assert A.estimator_status()[:2] == Bh.estimator_status()[:2] == (False, True)
    assert _same(torch, kept, A.get_model())  # (a reset restarts the estimator and keeps the model)
    assert _same(torch, su.roll(A, Xa, 3, 3), su.roll(Bh, Xb, 3, 3)) and _same(torch, A.get_model(), Bh.get_model())


def _rule(state, steps, update_on):
    """the progress rule, one step at a time: a step updates if a previous transition exists and the update is on; an update ends
    the restart; every step leaves a transition behind -> (have_prev, rls_fresh)"""
    have_prev, fresh = state
    for _ in range(steps):
        if have_prev and update_on:
            fresh = False
        have_prev = True
    return have_prev, fresh


@pytest.mark.parametrize("dt", DTYPES)
def test_estimator_status_follows_the_progress_rule(su, dt):
    """kmpc_estimator_status (bit 0 have_prev, bit 1 rls_fresh and the update is on) after a reset, a 1-step roll-out, another one,
    a 1-step roll-out with the update switched off and then on, and a 5-step roll-out from a reset: the bits the rule gives."""
    m = su.make(dt)
    X = su.states(dt)

    def bits(state, update_on=True):
        return state[0], state[1] and update_on

    state = (False, True)
    m.reset()
    assert m.estimator_status()[:2] == bits(state) == (False, True)
    for k in range(2):
        su.roll(m, X, 1, k)
        state = _rule(state, 1, True)
        assert m.estimator_status()[:2] == bits(state), (dt, k)
    assert state == (True, False)
    # the update switched off and on around one step, from a restart: the step with the update off leaves the restart pending
    m.reset()
    state = (False, True)
    su.roll(m, X, 1, 2)
    state = _rule(state, 1, True)
    assert m.estimator_status()[:2] == bits(state) == (True, True)
    m.set_online_update(False)
    assert m.estimator_status()[:2] == bits(state, False) == (True, False)
    su.roll(m, X, 1, 3)
    state = _rule(state, 1, False)
    assert m.estimator_status()[:2] == bits(state, False)
    m.set_online_update(True)
    assert m.estimator_status()[:2] == bits(state) == (True, True)
    su.roll(m, X, 1, 4)
    state = _rule(state, 1, True)
    assert m.estimator_status()[:2] == bits(state) == (True, False)
    m.reset()
    su.roll(m, X, 5, 5)
    assert m.estimator_status()[:2] == bits(_rule((False, True), 5, True)) == (True, False)
