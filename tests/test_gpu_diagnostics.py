"""Diagnostics of the closed loop from inside the roll-out (kmpc_set_rollout_diagnostics / kmpc_rollout_diag): the lifted state every
step controlled from (logXLOClift, duffing.py:850) and the spectral norms of the change the online update made to A, B and C
(A_error, B_error, C_error, duffing.py:985-990), as the reference writes them into DuffingPlotrealtime.mat (duffing.py:1015).

Every case holds the logged series against per-trajectory gain-form oracles (ko.rls_update_gain) that follow the device's logged
X and U: the expected entry is np.linalg.norm(model after - model before, 2) of the oracle's models.

Tolerance of the norm checks (fixed by reasoning, not by what the device gives): |logged - |Delta_oracle|_2| <= tol * |model before|_2,
tol = 10 * max(cpu figure, 1e-8) where
  cpu figure  the worst |norm(Delta, 2) - rank-one formula| / |model|_2 when the set's own transitions are replayed through
              ko.rls_update_gain on the host (what the quantity itself is uncertain by; printed per case),
  1e-8        the relative model deviation tests/test_gpu_round4.py accepts between a fused launch and per-step calls for the
              BASELINE sets (`dm < 1e-8`): the logged value inherits the device-against-oracle deviation of the model,
  10          the summation order of the half-wave sums;
tol < 1e-6 is asserted, every entry of every compared trajectory is asserted, small norms get the same absolute bound as large ones.
The measured ratios are printed and recorded in profiles/diag_parity.txt.

Runs on the MI355X box:  python -m pytest tests -m gpu
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import koopman_oracle as ko

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "koopman-online-updated-mpc_amd")
G = os.path.join(ROOT, "tests", "golden")
MODEL_TOL = 1e-8  # (tests/test_gpu_round4.py: fused launch against per-step calls, model, relative)


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


def _t(torch, a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype or torch.float64, device="cuda:0")


def _bench_controller(name, B):
    """A BASELINE configuration exactly as bench.py builds it (Loop): controller, initial states, reference, oracle-side set-up."""
    import torch

    import bench

    c = bench.CONFIGS[name]
    w = bench.workload_inputs(name, c["L"], c["N"])
    loop = bench.Loop(name, w, B, torch.float64, torch.device("cuda", 0), 0)
    return c, w, loop


def _oracle_series(lift_fn, L, model0, x0, Xl_b, Ul_b, P0=1e4, barQ0=100.0, init=None, update=True):
    """One trajectory's expected series from a gain-form oracle that follows the device's logged states and inputs.  Returns
    Psi (steps, L); exp (steps, 3): |A_new - A_old|_2, |B..|, |C..| of the update step k executes (0 at a step without one);
    scale (steps, 3): |model before that update|_2; form (steps, 3): the rank-one formula on the oracle's own quantities;
    fresh (steps,): the update is the first after a restart (the model in use was not the estimator's)."""
    steps = len(Ul_b)
    A, Bm, C = [np.array(m, dtype=np.float64) for m in model0]
    Bm = Bm.reshape(L, 1)
    if init is None:
        K, P, Cg, Q = np.zeros((L, L + 1)), P0 * np.eye(L + 1), np.zeros((2, L)), barQ0 * np.eye(L)
    else:
        K, P, Cg, Q = [np.array(m) for m in init]
    Psi, exp, scale, form = np.zeros((steps, L)), np.zeros((steps, 3)), np.ones((steps, 3)), np.zeros((steps, 3))
    fresh = np.zeros(steps, dtype=bool)
    x, prev, first = np.array(x0, dtype=np.float64), None, init is None
    for k in range(steps):
        psi = lift_fn(x.reshape(2, 1)).reshape(-1)
        Psi[k] = psi
        if prev is not None and update:
            ppsi, pu = prev
            z = np.concatenate([ppsi, [pu]])
            g = P @ z / (1.0 + z @ P @ z)
            e = psi - K @ z
            h = Q @ ppsi / (1.0 + ppsi @ Q @ ppsi)
            ec = x - Cg @ ppsi
            form[k] = [np.linalg.norm(e) * np.linalg.norm(g[:L]), np.linalg.norm(e) * abs(g[L]), np.linalg.norm(ec) * np.linalg.norm(h)]
            K, P = ko.rls_update_gain(K, P, z, psi)
            Cg, Q = ko.rls_update_gain(Cg, Q, ppsi, x)
            An, Bn, Cn = K[:, :-1].copy(), K[:, -1:].copy(), Cg.copy()
            exp[k] = [np.linalg.norm(An - A, 2), np.linalg.norm(Bn - Bm, 2), np.linalg.norm(Cn - C, 2)]
            scale[k] = [np.linalg.norm(A, 2), np.linalg.norm(Bm, 2), np.linalg.norm(C, 2)]
            fresh[k] = first
            first = False
            A, Bm, C = An, Bn, Cn
        prev = (psi, float(Ul_b[k]))
        x = np.array(Xl_b[k], dtype=np.float64)
    return Psi, exp, scale, form, fresh


def _check(name, lift_fn, L, model0, X0, Ul, Xl, diag, trajs, psi_tol=1e-12, **okw):
    """Every logged entry of the trajectories `trajs` against the oracle; returns (worst device ratio, cpu figure, tol, the oracle's
    expected series (steps, len(trajs), 3), their scales)."""
    Ul, Xl = Ul.cpu().numpy(), Xl.cpu().numpy()
    Psi, dA, dB, dC = [diag[k].cpu().numpy() for k in ("Psi", "dA", "dB", "dC")]
    logged = np.stack([dA, dB, dC], axis=2)  # (steps, B, 3)
    assert not np.isnan(logged).any() and not np.isnan(Psi).any()
    series = [_oracle_series(lift_fn, L, model0, X0[:, b], Xl[:, :, b], Ul[:, b], **okw) for b in trajs]
    cpu_fig = max(float((np.abs(e - f) / s)[~fr].max()) if (~fr).any() else 0.0 for _, e, s, f, fr in series)
    tol = 10.0 * max(cpu_fig, MODEL_TOL)
    assert tol < 1e-6, (cpu_fig, tol)
    worst = worst_psi = 0.0
    for b, (P_, e, s, f, fr) in zip(trajs, series):
        worst_psi = max(worst_psi, float(np.abs(Psi[:, :, b] - P_).max()))
        worst = max(worst, float((np.abs(logged[:, b, :] - e) / s).max()))
    print("%s: %d trajectories x %d steps: worst |logged - |Delta_oracle|_2| / |model|_2 = %.3e (cpu figure %.3e, tol %.1e); |Psi - oracle lift| %.2e"
          % (name, len(trajs), Ul.shape[0], worst, cpu_fig, tol, worst_psi))
    for b, (P_, e, s, f, fr) in zip(trajs, series):
        assert np.abs(Psi[:, :, b] - P_).max() <= psi_tol, (b, float(np.abs(Psi[:, :, b] - P_).max()))
        bad = np.abs(logged[:, b, :] - e) > tol * s  # every entry, the same absolute bound for small norms as for large ones
        assert not bad.any(), (b, np.argwhere(bad)[:5], logged[:, b, :][bad][:5], e[bad][:5])
        assert (logged[0, b, :] == 0.0).all(), "step 0 of a handle without a previous transition runs no update"
    return worst, cpu_fig, tol, np.stack([e for _, e, _, _, _ in series], axis=1), np.stack([s for _, _, s, _, _ in series], axis=1)


def _same_as_plain(torch, m_diag, m_plain, plant, X0, r, steps, step0, sw, Ud, Xd, Xend):
    """Bit for bit: U_log, X_log, the final X, status and state_dict() of the diagnostics run equal a plain rollout(log=True)."""
    Xp = _t(torch, X0)
    Up, Xlp = m_plain.rollout(plant, Xp, r, steps, step0=step0, switch_step=sw, log=True)
    assert torch.equal(Ud, Up) and torch.equal(Xd, Xlp) and torch.equal(Xend, Xp)
    assert torch.equal(m_diag.status, m_plain.status)
    assert np.array_equal(m_diag.state_dict()["blob"], m_plain.state_dict()["blob"])


def _golden():
    g = np.load(os.path.join(G, "duffing_loop.npz"))
    w = ko.load_mlp_weights(np.load(os.path.join(G, "weights_duffing.npz")))
    return g, w


def _main_case(torch, KM, B=64, steps=131):
    from koopmpc.synth import initial_states

    g, w = _golden()
    model0 = (g["A0"], g["B0"], g["C0"])
    ms = [KM(n=2, L=8, N=10, batch=B, weights=w) for _ in range(2)]
    for m in ms:
        m.set_model(*model0)
    X0 = initial_states(B, seed=3)
    r = g["loop_r"][0]
    return g, w, model0, ms, X0, r


# ------------------------------------------------------------------ cases 6 and 9: the reference's own set, fused
def test_main_case_reference_set_fused(torch_mod, KM):
    """L = 8, N = 10, the reference's encoder weights and offline model, B = 64, 131 steps from iteration 0, switch at 102: the DIAG
    plug-in is loaded (setter returns 0), Psi against ko.mlp_lift of the logged states within 1e-12 (the bound of
    test_mlp_lift_real_weights), dA, dB, dC of EVERY step of EVERY trajectory against the oracle's models; the first-update entry
    (step 1: the estimator restarts, the model in use was the offline one) comes from the wrapper, the 0.0 at step 0 is checked;
    and the run equals a plain rollout(log=True) bit for bit."""
    torch = torch_mod
    g, w, model0, ms, X0, r = _main_case(torch, KM)
    B, steps, sw = 64, 131, 102
    assert ms[0].set_rollout_diagnostics(True) == 0
    code, text = ms[0].rollout_plugin_status()
    assert code == 0 and "built-in" in text and "kmpc_rollout_diag: plug-in" in text and "_f64_diag_" in text, (code, text)
    assert ms[0].estimator_status() == (False, True, 1e4, 100.0)
    Xd = _t(torch, X0)
    Ul, Xl, diag = ms[0].rollout("duffing", Xd, r, steps, step0=0, switch_step=sw, log=True, diagnostics=True)
    assert int(ms[0].status.max().item()) == 0
    assert tuple(diag["Psi"].shape) == (steps, 8, B) and tuple(diag["dA"].shape) == (steps, B)
    lift_fn = lambda x: ko.mlp_lift(w, x)
    _check("reference set (8, 10), fused", lift_fn, 8, model0, X0, Ul, Xl, diag, range(B))
    for k in ("dA", "dB", "dC"):
        assert float(diag[k][0].abs().max()) == 0.0
        assert float(diag[k][1].min()) > 1e-3  # (the restart: offline model -> y g', a change of the model's own size)
    _same_as_plain(torch, ms[0], ms[1], "duffing", X0, r, steps, 0, sw, Ul, Xl, Xd)


# ------------------------------------------------------------------ cases 7, 8 and 9: cfg2 and cfg3 as bench.py builds them
@pytest.mark.parametrize("name,B,steps,step0", [("cfg2", 4096, 40, 80), ("cfg3", 1024, 40, 80)])
def test_bench_sets_fused(torch_mod, name, B, steps, step0):
    """BASELINE cfg2 (20, 20, MLP, B = 4096: the estimator restarts) and cfg3's set (8, 30, RBF: the estimator continues from the
    offline samples, no first-update case), built as bench.py builds them, 40 steps across the plant switch: the same norm checks on
    24 trajectories, and the run equals a plain rollout(log=True) bit for bit."""
    torch = torch_mod
    c, w, l1 = _bench_controller(name, B)
    _, _, l2 = _bench_controller(name, B)
    assert l1.m.rollout_is_fused() and l1.m.set_rollout_diagnostics(True) == 0
    X0 = l1.X.cpu().numpy().copy()
    L, N = c["L"], c["N"]
    Xo, Yo, Uo = w["data"]
    rbf = c.get("lift") == "rbf"
    lift_fn = (lambda x: ko.rbf_lift(x, w["centres"])) if rbf else (lambda x: ko.mlp_lift(w["weights"], x))
    PX, PY = lift_fn(Xo), lift_fn(Yo)
    Z = np.concatenate([PX, Uo[None, :]], 0)
    ridge = 1e-9 if rbf else 0.0  # (the model the device fitted: kmpc_offline_fit = Gram form of duffing.py:152-177)
    Gm = Z @ Z.T + ridge * np.eye(L + 1)
    K0 = (PY @ Z.T) @ np.linalg.inv(Gm)
    Qm = np.linalg.inv(PX @ PX.T + ridge * np.eye(L))
    model0 = (K0[:, :L], K0[:, L:], (Xo @ PX.T) @ Qm)
    init = (K0, np.linalg.inv(Gm), model0[2], Qm) if rbf else None  # (vanderpol_RBF.py:434-438: continues from the offline samples)
    Ul, Xl, diag = l1.m.rollout(c["plant"], l1.X, l1.r, steps, step0=step0, switch_step=102, log=True, diagnostics=True)
    assert int(l1.m.status.max().item()) == 0
    trajs = sorted(np.random.RandomState(17).choice(B, 24, replace=False))
    # (Psi: 1e-12 of the lift's scale for the encoder, 1e-11 for the thin-plate lift, whose log differs from NumPy's in the last bits)
    _check("%s (%d, %d), fused, B = %d" % (name, L, N, B), lift_fn, L, model0, X0, Ul, Xl, diag, trajs,
           psi_tol=(1e-11 if rbf else 1e-12) * max(1.0, float(np.abs(PX).max())), P0=c["P0"], barQ0=c["barQ0"], init=init)
    _same_as_plain(torch, l1.m, l2.m, c["plant"], X0, l2.r, steps, step0, 102, Ul, Xl, l1.X)


# ------------------------------------------------------------------ case 10: the second implementation (rls_diag_kernel, per-step route)
def test_per_step_route_against_oracle_and_fused(torch_mod, KM):
    """The per-step route: a batched kernel in front of each step's update computes the three norms from the dense state blocks
    (csrc/aux_kernels.hip rls_diag_kernel), an independent implementation.  In a process with KMPC_NO_FUSED_ROLLOUT the main case runs
    on it (setter returns 1): the same checks against the oracle, and its series against the fused variant's of this process."""
    torch = torch_mod
    g, w, model0, ms, X0, r = _main_case(torch, KM)
    steps, sw, B = 131, 102, 64
    Xd = _t(torch, X0)
    Uf, Xf, df = ms[0].rollout("duffing", Xd, r, steps, step0=0, switch_step=sw, log=True, diagnostics=True)
    out = os.path.join(str(os.environ.get("TMPDIR", "/tmp")), "kmpc_diag_per_step_%d.npz" % os.getpid())
    code = (
        "import sys, numpy as np, torch\n"
        "sys.path[:0] = [%r, %r]\n"
        "from koopmpc import KoopmanMPC\n"
        "from koopmpc.synth import initial_states\n"
        "from oracle import koopman_oracle as ko\n"
        "g = np.load(%r); w = ko.load_mlp_weights(np.load(%r))\n"
        "m = KoopmanMPC(n=2, L=8, N=10, batch=64, weights=w)\n"
        "m.set_model(g['A0'], g['B0'], g['C0'])\n"
        "assert not m.rollout_is_fused()\n"
        "route = m.set_rollout_diagnostics(True)\n"
        "X = torch.tensor(initial_states(64, seed=3), dtype=torch.float64, device='cuda:0')\n"
        "U, Xl, d = m.rollout('duffing', X, g['loop_r'][0], 131, step0=0, switch_step=102, log=True, diagnostics=True)\n"
        "np.savez(%r, route=route, U=U.cpu().numpy(), X=Xl.cpu().numpy(), **{k: v.cpu().numpy() for k, v in d.items()})\n"
    ) % (ROOT, PKG, os.path.join(G, "duffing_loop.npz"), os.path.join(G, "weights_duffing.npz"), out)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KMPC_DEBUG="1", KMPC_NO_FUSED_ROLLOUT="1"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    d = np.load(out)
    os.remove(out)
    assert int(d["route"]) == 1
    lift_fn = lambda x: ko.mlp_lift(w, x)
    dd = {k: _t(torch, d[k]) for k in ("Psi", "dA", "dB", "dC")}
    _, _, tol_p, exp_p, sc_p = _check("reference set (8, 10), per-step route", lift_fn, 8, model0, X0, _t(torch, d["U"]), _t(torch, d["X"]), dd, range(B))
    _, _, tol_f, exp_f, sc_f = _check("reference set (8, 10), fused, this process", lift_fn, 8, model0, X0, Uf, Xf, df, range(B))
    # fused against per-step, entry by entry.  The two runs are two closed loops (they agree to the encoder's summation order at every
    # step, and the plant amplifies that over 131 steps), each within tol of the oracle that follows ITS logged states; so the series
    # may differ by what the two oracles differ by, plus both tolerances -- the triangle inequality, nothing wider
    for i, k in enumerate(("dA", "dB", "dC")):
        diff = np.abs(df[k].cpu().numpy() - d[k])
        bound = tol_f * sc_f[:, :, i] + tol_p * sc_p[:, :, i] + np.abs(exp_f[:, :, i] - exp_p[:, :, i])
        print("fused vs per-step %s: max |difference| %.3e, of which the two oracles differ by up to %.3e; first 10 steps %.3e"
              % (k, float(diff.max()), float(np.abs(exp_f[:, :, i] - exp_p[:, :, i]).max()), float(diff[:10].max())))
        assert (diff <= bound).all(), k
        # ... and over the first ten steps, before the plant has amplified anything, the two implementations are held against each
        # other directly: both tolerances, no allowance for the oracles
        assert (diff[:10] <= tol_f * sc_f[:10, :, i] + tol_p * sc_p[:10, :, i]).all(), (k, float(diff[:10].max()))


@pytest.mark.parametrize("L,N,output", [(36, 24, "Cx"), (12, 12, "lift"), (64, 50, "Cx")])
def test_per_step_route_of_sets_without_a_register_state_step(torch_mod, KM, L, N, output):
    """An LDS-step set (L + 2 > 32), a y = psi set and the four-wave set of cfg5 (L = 64: p = 65 elements, the two-register path of
    rls_diag_kernel): kmpc_set_rollout_diagnostics returns 1, kmpc_rollout_diag runs per-step launches
    with rls_diag_kernel; the same checks against the oracle (dC = 0.0 for y = psi, where C is not used)."""
    torch = torch_mod
    from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

    B, steps, step0, sw = 10, 8, 99, 102
    w = random_mlp_weights(2, 100, 3, L, seed=5)
    bnd = 6.0 if output == "lift" else 2.0
    m = KM(n=2, L=L, N=N, batch=B, weights=w, layers=3, output=output, lb=-bnd, ub=bnd)
    lift_fn = lambda x: ko.mlp_lift(w, x)
    A0, B0, C0 = offline_edmd(lambda X: m.Encoder(X), plant=duffing_rk4)
    m.set_model(A0, B0, C0)
    assert m.set_rollout_diagnostics(True) == 1
    assert "kmpc_rollout_diag: per-step launches" in m.rollout_plugin_status()[1]
    r = np.tile(lift_fn(np.array([[1.0], [0.0]])), (1, N)) if output == "lift" else np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = initial_states(B, seed=3)
    Xd = _t(torch, X0)
    Ul, Xl, diag = m.rollout("duffing", Xd, r, steps, step0=step0, switch_step=sw, log=True, diagnostics=True)
    if output == "lift":
        assert float(diag["dC"].abs().max()) == 0.0
        diag = dict(diag)
    Ulc, Xlc = Ul.cpu().numpy(), Xl.cpu().numpy()
    Psi, dA, dB = [diag[k].cpu().numpy() for k in ("Psi", "dA", "dB")]
    worst = 0.0
    series = [_oracle_series(lift_fn, L, (A0, B0, C0 if C0 is not None else np.zeros((2, L))), X0[:, b], Xlc[:, :, b], Ulc[:, b]) for b in range(B)]
    cpu_fig = max(float((np.abs(e - f) / s)[~fr][:, :2].max()) for _, e, s, f, fr in series)
    tol = 10.0 * max(cpu_fig, MODEL_TOL)
    assert tol < 1e-6
    ncol = 2 if output == "lift" else 3
    logged = np.stack([dA, dB, diag["dC"].cpu().numpy()], axis=2)
    for b, (P_, e, s, f, fr) in enumerate(series):
        assert np.abs(Psi[:, :, b] - P_).max() <= 1e-12
        dev = np.abs(logged[:, b, :ncol] - e[:, :ncol]) / s[:, :ncol]
        worst = max(worst, float(dev.max()))
    print("(%d, %d, %s) per-step route: worst ratio %.3e (cpu figure %.3e, tol %.1e)" % (L, N, output, worst, cpu_fig, tol))
    for b, (P_, e, s, f, fr) in enumerate(series):
        assert (np.abs(logged[:, b, :ncol] - e[:, :ncol]) <= tol * s[:, :ncol]).all(), b


# ------------------------------------------------------------------ case 11: the raw C ABI
def test_raw_c_abi(torch_mod, KM):
    """kmpc_rollout_diag itself: -3 on an unarmed handle; NaN (all three logs) at the first update after a restart and nowhere else;
    0.0 everywhere with the online update off; the setter refuses lambda = 0.98 and a float32 handle with a message; with the terminal
    refresh armed as well the combined variant runs and its inputs equal those of the refresh-only run."""
    torch = torch_mod
    g, w, model0, ms, X0, r = _main_case(torch, KM)
    B, steps = 64, 12
    m = ms[0]
    lib = m.lib

    def raw(mm, X, n_steps, step0=0):
        rr, per = mm._ref(r)
        kw = dict(dtype=torch.float64, device="cuda:0")
        U, Xl, Psi = torch.empty(n_steps, B, **kw), torch.empty(n_steps, 2, B, **kw), torch.empty(n_steps, 8, B, **kw)
        d = [torch.full((n_steps, B), -7.0, **kw) for _ in range(3)]
        rc = lib.kmpc_rollout_diag(mm.h, 0, mm._p(X), mm._p(rr), per, n_steps, step0, 102, 0.05, mm._p(U), mm._p(Xl), mm._p(Psi),
                                   mm._p(d[0]), mm._p(d[1]), mm._p(d[2]), mm._p(mm.status), mm._p(mm.iters), mm._stream())
        torch.cuda.synchronize()
        return rc, U, Xl, Psi, d

    X = _t(torch, X0)
    rc, *_ = raw(m, X, steps)
    assert rc == -3 and b"kmpc_set_rollout_diagnostics" in lib.kmpc_last_error(m.h)
    assert torch.equal(X, _t(torch, X0))
    assert lib.kmpc_set_rollout_diagnostics(m.h, 1) == 0
    rc, U, Xl, Psi, d = raw(m, X, steps)
    assert rc == 0
    for t in d:
        t = t.cpu().numpy()
        assert (t[0] == 0.0).all() and np.isnan(t[1]).all() and not np.isnan(t[2:]).any() and (t[2:] > 0.0).all()
    # a second call continues the estimator: an update in its first step, no NaN anywhere
    rc, U2, Xl2, Psi2, d2 = raw(m, X, 5, step0=steps)
    assert rc == 0 and all(not np.isnan(t.cpu().numpy()).any() and float(t.min()) > 0.0 for t in d2)
    # the online update off: the model does not move
    m.set_online_update(False)
    rc, _, _, _, d3 = raw(m, X, 4, step0=steps + 5)
    assert rc == 0 and all(float(t.abs().max()) == 0.0 for t in d3)
    m.set_online_update(True)
    assert lib.kmpc_set_rollout_diagnostics(m.h, 0) == 0
    assert raw(m, X, 2)[0] == -3
    # what is unsupported says so
    m98 = KM(n=2, L=8, N=10, batch=B, weights=w, lam=0.98)
    assert lib.kmpc_set_rollout_diagnostics(m98.h, 1) < 0 and b"lambda" in lib.kmpc_last_error(m98.h)
    m32 = KM(n=2, L=8, N=10, batch=B, weights=w, dtype=torch.float32)
    assert lib.kmpc_set_rollout_diagnostics(m32.h, 1) < 0 and b"float64 handles only" in lib.kmpc_last_error(m32.h)
    with pytest.raises(Exception):
        m32.set_rollout_diagnostics(True)
    # terminal refresh + diagnostics: the variant that has both
    mt, md = [KM(n=2, L=8, N=10, batch=B, weights=w) for _ in range(2)]
    for mm in (mt, md):
        mm.set_model(*model0)
        mm.set_terminal_refresh(every=1)
    assert lib.kmpc_set_rollout_diagnostics(md.h, 1) == 0
    code, text = md.rollout_plugin_status()
    assert code == 1 and "_f64_term_diag_" in text, (code, text)
    Xt, Xdg = _t(torch, X0), _t(torch, X0)
    Ut, _ = mt.rollout("duffing", Xt, r, steps, log=True)
    rc, Ud, _, _, dd = raw(md, Xdg, steps)
    assert rc == 0 and torch.equal(Ut, Ud) and torch.equal(Xt, Xdg)
    assert np.isnan(dd[0][1].cpu().numpy()).all() and float(dd[0][2:].min()) > 0.0
    # the refresh switched off again on the armed handle: kmpc_rollout_diag stays fused, on the variant without the refresh
    for mm in (mt, md):
        mm.set_terminal_refresh(every=0)
    code, text = md.rollout_plugin_status()
    assert "kmpc_rollout_diag: plug-in" in text and "_f64_diag_" in text and "_term_diag_" not in text.split("kmpc_rollout_diag")[1], (code, text)
    Ut2, _ = mt.rollout("duffing", Xt, r, 6, step0=steps, log=True)
    rc, Ud2, _, _, dd2 = raw(md, Xdg, 6, step0=steps)
    assert rc == 0 and torch.equal(Ut2, Ud2) and torch.equal(Xt, Xdg) and not np.isnan(dd2[0].cpu().numpy()).any()
    # a handle that runs the shared-model loop is refused
    msh = KM(n=2, L=8, N=10, batch=B, weights=w)
    msh.set_model(*model0)
    Xs = _t(torch, X0)
    for _ in range(2):
        Xs = msh.plant_step("duffing", Xs, msh.shared_step(Xs, r).clone())
    assert lib.kmpc_set_rollout_diagnostics(msh.h, 1) < 0 and b"shared-model" in lib.kmpc_last_error(msh.h)


# ------------------------------------------------------------------ arming order, refused calls
def test_diagnostics_armed_before_the_terminal_refresh(torch_mod, KM):
    """kmpc_set_rollout_diagnostics FIRST, kmpc_set_terminal_refresh after it (test_raw_c_abi arms in the other order): the refresh setter
    loads the variant that has both, the status text names it, and the diagnostics roll-out (6 steps from iteration 99, switch at 102)
    equals a plain roll-out on a twin that only has the refresh, bit for bit; so does a second window after the diagnostics were
    switched off and on again."""
    torch = torch_mod
    g, w, model0, (md, mt), X0, r = _main_case(torch, KM)
    assert md.set_rollout_diagnostics(True) == 0
    for mm in (md, mt):
        mm.set_terminal_refresh(every=1)
    code, text = md.rollout_plugin_status()
    assert code == 1 and "_f64_term_diag_" in text.split("kmpc_rollout_diag")[1], (code, text)
    Xd, Xt = _t(torch, X0), _t(torch, X0)
    for window, step0 in enumerate((99, 105)):
        if window == 1:
            assert md.set_rollout_diagnostics(False) == 0 and md.set_rollout_diagnostics(True) == 0
        Ud, Xld, dg = md.rollout("duffing", Xd, r, 6, step0=step0, switch_step=102, log=True, diagnostics=True)
        Ut, Xlt = mt.rollout("duffing", Xt, r, 6, step0=step0, switch_step=102, log=True)
        assert torch.equal(Ud, Ut) and torch.equal(Xld, Xlt) and torch.equal(Xd, Xt) and torch.equal(md.status, mt.status), window
        assert not any(bool(torch.isnan(v).any()) for v in dg.values())


def test_a_refused_call_leaves_nothing_behind(torch_mod, KM):
    """Calls the argument checks refuse before any launch (kmpc_rollout_diag with X = NULL, then with steps = -1; kmpc_shared_solve_plant
    with X = NULL; each returns -3) leave no trace in the handle: the plain rollout(log=True), the step() calls and the state_dict()
    that follow equal those of an untouched twin bit for bit."""
    torch = torch_mod
    g, w, model0, (m, twin), X0, r = _main_case(torch, KM)
    B, steps, lib = 64, 6, m.lib
    assert m.set_rollout_diagnostics(True) == 0
    rr, per = m._ref(r)
    kw = dict(dtype=torch.float64, device="cuda:0")
    X = _t(torch, X0)
    U, Xl, Psi = torch.empty(steps, B, **kw), torch.empty(steps, 2, B, **kw), torch.empty(steps, 8, B, **kw)
    d = [torch.empty(steps, B, **kw) for _ in range(3)]

    def refused_diag(Xp, n_steps):
        return lib.kmpc_rollout_diag(m.h, 0, Xp, m._p(rr), per, n_steps, 99, 102, 0.05, m._p(U), m._p(Xl), m._p(Psi), m._p(d[0]), m._p(d[1]),
                                     m._p(d[2]), m._p(m.status), m._p(m.iters), m._stream())

    def same_step():
        u, ut = m.step(X, r), twin.step(Xt, r)
        assert torch.equal(u, ut) and torch.equal(m.Useq, twin.Useq) and torch.equal(m.status, twin.status)
        assert np.array_equal(m.state_dict()["blob"], twin.state_dict()["blob"])

    assert refused_diag(None, steps) == -3
    assert refused_diag(m._p(X), -1) == -3
    Xt = _t(torch, X0)
    Um, Xlm = m.rollout("duffing", X, r, steps, step0=99, switch_step=102, log=True)
    Ut, Xlt = twin.rollout("duffing", Xt, r, steps, step0=99, switch_step=102, log=True)
    assert torch.equal(Um, Ut) and torch.equal(Xlm, Xlt) and torch.equal(X, Xt) and torch.equal(m.status, twin.status)
    same_step()
    delta = torch.zeros(int(lib.kmpc_gram_elems(m.h)), **kw)
    assert lib.kmpc_shared_solve_plant(m.h, m._p(delta), m._p(rr), m._p(m.U0), m._p(m.Useq), m._p(m.status), m._p(m.iters), 0, None, 0, 0.05,
                                       m._stream()) == -3
    same_step()


# ------------------------------------------------------------------ consecutive calls: the wrapper leaves the handle alone
@pytest.mark.parametrize("route", ["fused", "fused+term3", "per-step"])
def test_consecutive_diagnostics_calls_equal_consecutive_plain_calls(torch_mod, KM, route):
    """A running loop calls the roll-out window after window.  Three consecutive rollout(log=True, diagnostics=True) calls (1, 20 and
    20 steps: the first leaves a previous transition behind, so the first update after the restart is step 0 of the SECOND call)
    against three consecutive rollout(log=True) calls on a twin: U_log, X_log, X, status of every call and state_dict() at the end
    are equal bit for bit -- on the fused route, on the fused route with a terminal refresh every third step (the refresh schedule
    runs through the calls), and on the per-step route (the four-wave set (64, 50), whose step carries its QP tableau from call to
    call).  Steps 0 to 2 of the series -- no update, the first update as step 0 of the second call, the first rank-one update -- equal,
    to 1e-9 of their size, those of ONE 41-step call on a third handle, where the first update is step 1 of the call.  (Only those:
    a launch boundary changes the controls in their last bits, the plant and the refreshed terminal blocks amplify that, and from
    then on the one-call run is another closed loop; the later entries are held by the equality with the plain calls above and by
    the oracle cases.  The figure over all 41 steps is printed.)"""
    torch = torch_mod
    from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

    if route == "per-step":
        L, N, B = 64, 50, 8
        w = random_mlp_weights(2, 100, 3, L, seed=5)
        ms = [KM(n=2, L=L, N=N, batch=B, weights=w) for _ in range(3)]
        model0 = offline_edmd(lambda X: ms[0].Encoder(X), plant=duffing_rk4)
        r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    else:
        g, w = _golden()
        L, N, B = 8, 10, 64
        ms = [KM(n=2, L=L, N=N, batch=B, weights=w) for _ in range(3)]
        model0 = (g["A0"], g["B0"], g["C0"])
        r = g["loop_r"][0]
    for m in ms:
        m.set_model(*model0)
        if route == "fused+term3":
            m.set_terminal_refresh(every=3)
    want = 1 if route == "per-step" else 0
    assert ms[0].set_rollout_diagnostics(True) == want and ms[2].set_rollout_diagnostics(True) == want
    assert ms[1].rollout_is_fused() == (route != "per-step")
    X0 = initial_states(B, seed=3)
    Xd, Xp, Xo = _t(torch, X0), _t(torch, X0), _t(torch, X0)
    parts, step0 = [], 90
    for cnt in (1, 20, 20):
        Ud, Xld, dg = ms[0].rollout("duffing", Xd, r, cnt, step0=step0, switch_step=102, log=True, diagnostics=True)
        Up, Xlp = ms[1].rollout("duffing", Xp, r, cnt, step0=step0, switch_step=102, log=True)
        assert torch.equal(Ud, Up) and torch.equal(Xld, Xlp) and torch.equal(Xd, Xp) and torch.equal(ms[0].status, ms[1].status), (route, step0)
        assert not any(bool(torch.isnan(v).any()) for v in dg.values())
        parts.append(dg)
        step0 += cnt
    assert ms[0].estimator_status()[:2] == (True, False)
    assert np.array_equal(ms[0].state_dict()["blob"], ms[1].state_dict()["blob"])
    _, _, one = ms[2].rollout("duffing", Xo, r, 41, step0=90, switch_step=102, log=True, diagnostics=True)
    for k in ("dA", "dB", "dC"):
        cat = torch.cat([p_[k] for p_ in parts])
        assert float(cat[0].abs().max()) == 0.0 and float(cat[1].min()) > 0.0
        rel = (cat - one[k]).abs() / one[k].abs().clamp(min=1e-3)
        dev = float(rel[:3].max())
        print("%s, %s: three calls against one call: max relative difference %.2e over steps 0-2, %.2e over all 41" % (route, k, dev, float(rel.max())))
        assert dev < 1e-9, (route, k, dev)


# ------------------------------------------------------------------ case 12: the script
def test_duffing_script_writes_the_reference_result_file(torch_mod, tmp_path):
    """python -m koopmpc.scripts.duffing --mat: one fused roll-out with the diagnostics logs, written with the reference's keys."""
    import scipy.io as sio

    out = tmp_path / "DuffingPlotrealtime.mat"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get("PYTHONPATH", "")]))
    p = subprocess.run([sys.executable, "-m", "koopmpc.scripts.duffing", "--weights", os.path.join(G, "weights_duffing.npz"), "--model",
                        os.path.join(G, "duffing_loop.npz"), "--batch", "64", "--steps", "40", "--mat", str(out)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    d = sio.loadmat(str(out))
    for k in ("logXloc", "logUloc", "logXLOClift", "A_error", "B_error", "C_error", "T_EX", "tspan"):
        assert k in d, k
    assert d["logXloc"].shape == (2, 40) and d["logUloc"].shape == (1, 40) and d["logXLOClift"].shape == (8, 40)
    for k in ("A_error", "B_error", "C_error", "T_EX"):
        assert d[k].shape == (1, 39) and not np.isnan(d[k]).any()
    assert np.allclose(d["T_EX"].ravel(), 0.05 * np.arange(39))
