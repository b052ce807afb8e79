"""Round-6 parity tests of the HIP path (through the C ABI).

  the configurations bench.py times, held against the oracle AT THE SIZE THEY ARE TIMED AT:
     cfg4  8192 trajectories, kmpc_shared_rollout, pooled model + delta-u QPs                 Tank_System.m:170-291, Koopman_update.m:94-101
     cfg5  32768 trajectories, four-wave step kernel, the plant switch inside                  duffing.py:823-1012, 991-992
     cfg2 / cfg3  a fused launch whose 20 steps contain the plant switch (step 102)            duffing.py:991-992
  advisor findings of round 5 (float32 handle: terminal weight through a checkpoint, a workgroup of four, non-resetting
  profile reads; the handle's own stream marks)

Runs on the MI355X box:  python -m pytest tests -m gpu
"""
import os

import numpy as np
import pytest

from oracle import koopman_oracle as ko

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


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


# ------------------------------------------------------------------ cfg4 at 8192 trajectories
def test_cfg4_full_size_shared_rollout_vs_oracle(torch_mod):
    """BASELINE cfg4 at the size bench.py times it (8192 trajectories per GPU, controller built by bench.Loop), through
    kmpc_shared_rollout -- lift + Gram sums -> [all-reduce] -> pooled model -> interior / box QPs -> tank plant, 34 steps from the reset,
    the tank's parameter switch (Tank_System.m:193-196) at step 20 inside.  The loop is taken one native step at a time so that the pooled
    model of every step can be exported (kmpc_shared_get_model).  Against the oracle:
      (1) the pooled model itself at FULL size: SharedEdmd (Koopman_update.m:94-101) fed with the oracle's lift of all 8192 states and
          the inputs the device applied -- [A B] and C of every step within 1e-6 of their scale (the Gram block's condition number is
          ~1e10 here; the small-batch tests hold 1e-7);
      (2) 20 randomly chosen trajectories x every step: the delta-u QP of OracleDeltaUController (Tank_System.m:110-113, 182-188,
          265-268) on the exported pooled model, exact minimiser: |u - u_oracle| <= 1e-6 (the north star's tolerance)."""
    torch = torch_mod
    import bench

    B = bench.CONFIGS["cfg4"]["B"]
    c, w, loop = _bench_controller("cfg4", B)
    assert loop.native and loop.comm is None
    L, N = c["L"], c["N"]
    lift_fn = lambda x: ko.mlp_lift(w["weights"], x)
    r = w["ref"]
    steps, sw = 34, 20
    A, Bm, C = [t.cpu().numpy() for t in loop.m.shared_model()]  # (the offline fit: the model until transitions exist)
    sh = ko.SharedEdmd(L, 2, P0=1e4, barQ0=1e4)
    rng = np.random.RandomState(4)
    pick = np.sort(rng.choice(B, 20, replace=False))
    uabs = np.zeros(B)
    prev = None
    worst_u = worst_m = 0.0
    compared = skipped = 0
    for k in range(steps):
        X = loop.X.cpu().numpy().copy()
        Ul, Xl = loop.m.shared_rollout("tank", loop.X, loop.r, 1, step0=k, switch_step=sw, comm=None, log=True)
        u = Ul[0].cpu().numpy()
        st = loop.m.status.cpu().numpy()
        assert (st <= 1).all(), k
        Ag, Bg, Cg = [t.cpu().numpy() for t in loop.m.shared_model()]
        Psi = lift_fn(X)
        if prev is not None:
            sh.add(*ko.SharedEdmd.gram(prev[0], prev[1], Psi, X))
            A, Bm, C = sh.model()
            scale = max(np.abs(A).max(), np.abs(Bm).max())
            worst_m = max(worst_m, np.abs(Ag - A).max() / scale, np.abs(Bg - Bm).max() / scale, np.abs(Cg - C).max() / max(1e-3, np.abs(C).max()))
        ctl = ko.OracleDeltaUController(lift_fn, L, 2, N, Ag, Bg, Cg)
        for b in pick:
            ctl.u = float(uabs[b])
            At, Bt, Co, xt = ctl.qp(Psi[:, b])
            _, _, H, f, _ = ko.condense(At, Bt, Co, xt, r, N, ctl.Qw, ctl.Rw)
            lbv = np.full(N, ctl.lb); ubv = np.full(N, ctl.ub)
            lbv[0] = max(ctl.lb, ctl.umin - uabs[b]); ubv[0] = min(ctl.ub, ctl.umax - uabs[b])
            if st[b] != 0 or not np.linalg.cond(H) < 1e12:  # (a pooled model of the very first steps can make H numerically singular)
                skipped += 1
                continue
            dU, _ = ko.qp_exact(H, f, lbv, ubv)
            worst_u = max(worst_u, abs(uabs[b] + float(dU[0]) - u[b]))
            compared += 1
        # the plant the kernel advanced, for the sampled trajectories
        for b in pick:
            xo = ko.tank_step(X[:, b], float(u[b]), switched=(k >= sw))
            assert np.abs(Xl[0, :, b].cpu().numpy() - xo).max() < 1e-9, (k, b)
        uabs = u.copy()
        prev = (Psi, u.copy())
    print("cfg4, B = %d, %d native steps: pooled model vs SharedEdmd at full size %.2e; %d QPs of 20 trajectories vs the oracle "
          "(%d skipped): max |u - u_oracle| %.2e" % (B, steps, worst_m, compared, skipped, worst_u))
    assert compared >= 20 * 30
    assert worst_m < 1e-6 and worst_u < 1e-6


# ------------------------------------------------------------------ cfg5 at 32768 trajectories
def test_cfg5_full_size_rollout_vs_oracle(torch_mod):
    """BASELINE cfg5 at the size bench.py times it (32768 trajectories per GPU: 7 GB of per-trajectory state), bench.Loop's
    controller, kmpc_rollout over 116 steps from the RLS reset with the Duffing parameter switch where the reference has it
    (duffing.py:991-992: from step 102 on) -- one lift launch + one four-wave step_kernel launch per step, tableaux carried in global
    memory.  8 randomly chosen trajectories against per-trajectory oracle controllers (gain-form RLS, exact QP, duffing.py:847-984)
    over ALL steps: |u - u_oracle| <= 1e-6, states 1e-9; every QP of the batch solved (status 0).
    (A switch a few steps after the reset -- tried first -- is not a test of anything: with fewer transitions than regressors the
    estimator interpolates, the switched plant then gives models with spectral radius >> 1 and H = O(1e24) is not a QP in float64.)"""
    torch = torch_mod
    import bench

    B = bench.CONFIGS["cfg5"]["B"]
    c, w, loop = _bench_controller("cfg5", B)
    L, N = c["L"], c["N"]
    lift_fn = lambda x: ko.mlp_lift(w["weights"], x)
    r = w["ref"]
    A0, B0, C0 = [t.cpu().numpy() for t in loop.m.shared_model()]  # the device's offline fit (every trajectory's start, duffing.py:811-813)
    X0 = loop.X.cpu().numpy().copy()
    steps, sw = 116, 102
    Ul, Xl = loop.m.rollout(c["plant"], loop.X, loop.r, steps, step0=0, switch_step=sw, log=True)
    nbad = int((loop.m.status != 0).sum().item())
    assert nbad == 0, "%d of %d trajectories left a QP with status != 0" % (nbad, B)
    assert bool(torch.isfinite(loop.X).all())
    Ul, Xl = Ul.cpu().numpy(), Xl.cpu().numpy()
    rng = np.random.RandomState(5)
    worst_u = worst_x = worst_u_sw = 0.0
    for b in rng.choice(B, 8, replace=False):
        ctl = ko.OracleController(lift_fn, L, 2, N, c["lb"], c["ub"], A0, B0, C0, P0=c["P0"], barQ0=c["barQ0"], rls="gain")
        x = X0[:, b].copy()
        for k in range(steps):
            uo, _, _ = ctl.step(x, r)
            worst_u = max(worst_u, abs(Ul[k, b] - uo))
            if k >= sw:
                worst_u_sw = max(worst_u_sw, abs(Ul[k, b] - uo))
            ctl.prev = (ctl.prev[0], float(Ul[k, b]))  # (both sides regress on the applied input and continue from the device's state)
            xo = ko.plant_step(c["plant"], x, float(Ul[k, b]), switched=(k >= sw))
            worst_x = max(worst_x, float(np.abs(Xl[k, :, b] - xo).max()))
            x = Xl[k, :, b].copy()
    print("cfg5, B = %d, %d steps from the reset, switch at %d: 8 trajectories vs per-trajectory oracles: max |u - u_oracle| %.2e "
          "(after the switch %.2e), |x - x_oracle| %.2e" % (B, steps, sw, worst_u, worst_u_sw, worst_x))
    assert worst_u < 1e-6 and worst_x < 1e-9


# ------------------------------------------------------------------ the plant switch inside a fused launch at full size
@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
def test_fused_launch_with_the_switch_inside_full_size(torch_mod, name):
    """bench.py's `switch_window` leg as a test: BASELINE cfg2 (4096 trajectories, (20, 20, 2)) / cfg3 (16384, (8, 30, 2)), bench.Loop's
    controllers, 95 closed-loop steps from the RLS reset as one launch, then ONE fused K = 20 launch over steps 95..114 -- the plant's
    parameters switch at step 102 (duffing.py:991-992) INSIDE it, while tableaux are carried and the covariance half of the update
    runs a step ahead.  32 randomly chosen trajectories against per-trajectory oracle controllers from the reset on (all 115 steps,
    gain-form RLS, exact QP): inputs within 1e-6 (north star), states within 1e-9."""
    torch = torch_mod
    import bench

    B = bench.CONFIGS[name]["B"]
    c, w, l1 = _bench_controller(name, B)
    assert l1.m.rollout_is_fused()
    X0 = l1.X.cpu().numpy().copy()
    pre, K = bench.SWITCH_WINDOW_START, 20
    assert pre < 102 <= pre + K - 1
    Up, Xp = l1.m.rollout(c["plant"], l1.X, l1.r, pre, step0=0, log=True)
    assert int(l1.m.status.max().item()) == 0
    Ul, Xl = l1.m.rollout(c["plant"], l1.X, l1.r, K, step0=pre, log=True)
    assert int(l1.m.status.max().item()) == 0
    L, N = c["L"], c["N"]
    Xo, Yo, Uo = w["data"]
    rbf = c.get("lift") == "rbf"
    lift_fn = (lambda x: ko.rbf_lift(x, w["centres"])) if rbf else (lambda x: ko.mlp_lift(w["weights"], x))
    PX, PY = lift_fn(Xo), lift_fn(Yo)
    Z = np.concatenate([PX, Uo[None, :]], 0)
    ridge = 1e-9 if rbf else 0.0  # (the model the device fitted: kmpc_offline_fit = Gram form of duffing.py:152-177)
    Gm = Z @ Z.T + ridge * np.eye(L + 1)
    K0 = (PY @ Z.T) @ np.linalg.inv(Gm)
    A0, B0 = K0[:, :L], K0[:, L:]
    C0 = (Xo @ PX.T) @ np.linalg.inv(PX @ PX.T + ridge * np.eye(L))
    Uall = np.concatenate([Up.cpu().numpy(), Ul.cpu().numpy()])
    Xall = np.concatenate([Xp.cpu().numpy(), Xl.cpu().numpy()])
    rng = np.random.RandomState(17)
    worst_u = worst_x = worst_u_win = 0.0
    r = w["ref"]
    for b in rng.choice(B, 32, replace=False):
        ctl = ko.OracleController(lift_fn, L, 2, N, c["lb"], c["ub"], A0, B0, C0, P0=c["P0"], barQ0=c["barQ0"], rls="gain")
        if rbf:  # (vanderpol_RBF.py:434-438: the estimator continues from the offline samples)
            ctl.gP = np.linalg.inv(Gm); ctl.gK = (PY @ Z.T) @ ctl.gP
            ctl.gQ = np.linalg.inv(PX @ PX.T + ridge * np.eye(L)); ctl.gC = (Xo @ PX.T) @ ctl.gQ
        x = X0[:, b].copy()
        for k in range(pre + K):
            uo, _, _ = ctl.step(x, r)
            worst_u = max(worst_u, abs(Uall[k, b] - uo))
            if k >= pre:
                worst_u_win = max(worst_u_win, abs(Uall[k, b] - uo))
            ctl.prev = (ctl.prev[0], float(Uall[k, b]))
            xo = ko.plant_step(c["plant"], x, float(Uall[k, b]), switched=(k >= 102))
            worst_x = max(worst_x, float(np.abs(Xall[k, :, b] - xo).max()))
            x = Xall[k, :, b].copy()
    print("%s, B = %d: fused launch over steps %d..%d (switch at 102 inside), 32 trajectories vs oracles from the reset: "
          "max |u - u_oracle| %.2e (in the window %.2e), |x - x_oracle| %.2e" % (name, B, pre, pre + K - 1, worst_u, worst_u_win, worst_x))
    assert worst_u < 1e-6 and worst_x < 1e-9


# ------------------------------------------------------------------ advisor findings of round 5
def _cfg2_f32(KM, torch, B, seed=101):
    from koopmpc.synth import initial_states, offline_data, random_mlp_weights

    L, N = 20, 20
    w = random_mlp_weights(2, 100, 3, L, seed=2024)
    Xo, Yo, Uo = offline_data()
    PX, PY = ko.mlp_lift(w, Xo), ko.mlp_lift(w, Yo)
    Z = np.concatenate([PX, Uo[None, :]], 0)
    K0 = PY @ np.linalg.pinv(Z)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    model = (f32(K0[:, :L]), f32(K0[:, L:]), f32(Xo @ np.linalg.pinv(PX)))
    X0 = f32(initial_states(B, seed=seed))
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))

    def make():
        m = KM(n=2, L=L, N=N, batch=B, weights=w, dtype=torch.float32, device="cuda:0")
        m.set_model(*model)
        return m
    return w, X0, r, make


def test_f32_handle_terminal_weight_travels_through_a_checkpoint(torch_mod, KM):
    """ADVICE r5 (api.hip state_import): a KMPC_F32 handle runs its fused roll-outs on a float64 core, and the core only learns about a
    terminal weight through set_terminal_weight.  (1) A checkpoint of a float32 handle WITH a terminal block, loaded into a fresh
    float32 handle, gives the same next launch bit for bit -- and not the launch of a handle without the block (the block is in
    effect).  (2) The reverse: a checkpoint WITHOUT a block loaded over a handle that holds one drops it."""
    torch = torch_mod
    B = 128
    w, X0, r, make = _cfg2_f32(KM, torch, B)
    PN = np.array([[400.0, 30.0], [30.0, 250.0]])
    ma, mplain = make(), make()
    ma.set_terminal_weight(PN)
    assert ma.rollout_is_fused()
    Xa = torch.tensor(X0, dtype=torch.float32, device="cuda:0").contiguous()
    Xp = Xa.clone()
    ma.rollout("duffing", Xa, r, 6)
    mplain.rollout("duffing", Xp, r, 6)
    assert not torch.equal(Xa, Xp)  # the terminal block changes the closed loop
    sd = ma.state_dict()
    mb = make()
    mb.load_state_dict(sd)
    Xb = Xa.clone()
    Ua, _ = ma.rollout("duffing", Xa, r, 5, step0=6, log=True)
    Ub, _ = mb.rollout("duffing", Xb, r, 5, step0=6, log=True)
    assert torch.equal(Ua, Ub) and torch.equal(Xa, Xb)
    # the per-step route of the restored handle uses the same block (float32 kernels on both)
    ua, ub = ma.step(Xa, r).clone(), mb.step(Xb, r).clone()
    assert torch.equal(ua, ub)
    # (2) a blob without a block over a handle with one
    sdp = mplain.state_dict()
    mc = make()
    mc.set_terminal_weight(PN)
    mc.load_state_dict(sdp)
    Xc, Xq = Xp.clone(), Xp.clone()
    Uc, _ = mc.rollout("duffing", Xc, r, 5, step0=6, log=True)
    Uq, _ = mplain.rollout("duffing", Xq, r, 5, step0=6, log=True)
    assert torch.equal(Uc, Uq) and torch.equal(Xc, Xq)


def test_f32_rollout_with_a_workgroup_of_four_requested(torch_mod, KM):
    """ADVICE r5 (rollout_kernel.hip io32 launcher): kmpc_set_rollout_workgroup(4) is a public setting; the float32-panel roll-out only
    has workgroups of sixteen and eight trajectories.  A KMPC_F32 handle must still run (eight serve the request) and give the result
    of the default workgroup bit for bit -- a trajectory's arithmetic does not depend on the workgroup it sits in."""
    torch = torch_mod
    from koopmpc import _ffi

    lib = _ffi.load()
    B = 72
    w, X0, r, make = _cfg2_f32(KM, torch, B, seed=3)
    m16, m4 = make(), make()
    X16 = torch.tensor(X0, dtype=torch.float32, device="cuda:0").contiguous()
    X4 = X16.clone()
    U16, _ = m16.rollout("duffing", X16, r, 9, log=True)
    try:
        assert lib.kmpc_set_rollout_workgroup(4) == 0
        assert m4.rollout_is_fused()
        U4, _ = m4.rollout("duffing", X4, r, 9, log=True)
        torch.cuda.synchronize()
    finally:
        lib.kmpc_set_rollout_workgroup(0)
    assert int(m4.status.max().item()) == 0
    assert torch.equal(U16, U4) and torch.equal(X16, X4)


def test_profile_read_without_reset_keeps_both_halves_of_a_f32_handle(torch_mod, KM):
    """ADVICE r5 (api.hip profile_read): on a float32 handle the fused launches are recorded by the float64 core and the per-step
    launches by the handle itself; a NON-resetting read must leave both records in place and count both."""
    torch = torch_mod
    B = 64
    w, X0, r, make = _cfg2_f32(KM, torch, B, seed=8)
    m = make()
    X = torch.tensor(X0, dtype=torch.float32, device="cuda:0").contiguous()
    m.profile(True)
    m.rollout("duffing", X, r, 7)
    for _ in range(3):
        m.step(X, r)
    p1 = m.profile_read(reset=False)
    p2 = m.profile_read(reset=False)
    assert p1["count"] == 10 and p2["count"] == 10, (p1, p2)
    assert p1["step_ms"] > 0 and abs(p1["step_ms"] - p2["step_ms"]) < 1e-9
    p3 = m.profile_read(reset=True)
    assert p3["count"] == 10
    p4 = m.profile_read(reset=True)
    assert p4["count"] == 0 and p4["step_ms"] == 0.0
    m.profile(False)


def test_handle_waits_for_every_stream_it_was_used_on(torch_mod, KM):
    """ADVICE r5 (api.hip sync_own): the entry points that work on the null stream (kmpc_set_model, checkpoints) wait for the handle's
    own outstanding work through events recorded behind every stream-ordered call -- one per distinct stream.  A roll-out on stream A
    followed by a call on stream B, then a checkpoint: the blob must be the state AFTER the roll-out (the raw `last stream` of round 5
    covered B only), also when stream A's Python object has been dropped in between."""
    torch = torch_mod
    from koopmpc.synth import random_mlp_weights

    L, N, B = 20, 20, 2048
    w = random_mlp_weights(2, 100, 3, L, seed=6)
    rng = np.random.RandomState(2)
    A, Bm, Cm = rng.randn(L, L) * 0.1, rng.randn(L, 1) * 0.1, rng.randn(2, L) * 0.1
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = 4 * rng.rand(2, B) - 2

    def run(two_streams):
        m = KM(n=2, L=L, N=N, batch=B, weights=w)
        m.set_model(A, Bm, Cm)
        X = _t(torch, X0)
        torch.cuda.synchronize()
        sa = torch.cuda.Stream()
        with torch.cuda.stream(sa):
            m.rollout("duffing", X, r, 60)  # (tens of milliseconds of work on stream A)
        if two_streams:
            sb = torch.cuda.Stream()
            with torch.cuda.stream(sb):
                m.Encoder(X0[:, :4])  # an unrelated, short call on stream B
            del sb
        del sa
        blob = m.state_dict()["blob"].copy()  # kmpc_state_export: null stream + the handle's marks
        torch.cuda.synchronize()
        return blob, m.state_dict()["blob"].copy()

    for two in (False, True):
        early, late = run(two)
        assert np.array_equal(early, late), "checkpoint taken before the roll-out on the other stream had finished (two_streams=%s)" % two


# ------------------------------------------------------------------ the fused roll-out for ANY dimension set (roll-out plug-ins)
_PLUGIN_SETS = [
    # L,  N, output, out_rows, lift, layers, B,   steps, bound   (none of them has an instantiation inside libkoopmpc.so)
    (12, 16, "Cx", 0, "mlp", 3, 40, 12, 2.0),      # register-state step, two output rows
    (16, 24, "Cx", 1, "mlp", 2, 33, 10, 2.0),      # ... one output row (out_rows = 1), two hidden layers
    (28, 32, "Cx", 0, "mlp", 3, 20, 8, 2.0),       # ... its largest horizon, L + 2 = 30 state rows in the lanes
    (6, 12, "Cx", 0, "rbf", 0, 50, 12, 2.0),       # RBF lift: every wave lifts its own state
    (14, 20, "Cx", 0, "rbf", 0, 300, 8, 2.0),
    (12, 12, "lift", 0, "mlp", 3, 24, 10, 6.0),    # y = psi (vanderpol.py:456-459): the 8 x 8-grid step of step_body.h
    (36, 24, "Cx", 0, "mlp", 3, 10, 6, 2.0),       # y = C x beyond the register-state form (L + 2 > 32): the LDS step
    (26, 34, "Cx", 0, "rbf", 0, 24, 6, 2.0),       # RBF, long horizon, L >= 24: eight waves per workgroup with 256 registers (ro_rbf_eight)
]


@pytest.mark.parametrize("L,N,output,out_rows,lift,layers,B,steps,bnd", _PLUGIN_SETS)
def test_fused_rollout_of_dimension_sets_without_a_builtin_instantiation(torch_mod, KM, L, N, output, out_rows, lift, layers, B, steps, bnd):
    """the fused roll-out is a property of the library, not of nine (L, N, q) triples.  The reference's dimensions
    are constants edited in its scripts (duffing.py:66, 632-633); a controller of a set libkoopmpc.so has no instantiation for gets
    its kernel as a plug-in when it is created (kernel cache, else hipcc on csrc/rollout_jit.hip).  Every set: kmpc_rollout is ONE
    launch (rollout_is_fused, status code 1 = plug-in), closed loop across the plant switch against per-trajectory oracle controllers
    (gain-form RLS, exact QP; duffing.py:847-984): inputs within 1e-6, states within 1e-9.  The MLP sets restart their estimator
    (duffing.py:927-930), the RBF sets continue from the offline samples as vanderpol_RBF.py:434-438 does.  A QP whose Hessian is
    numerically singular (cond(H) > 1e9: the first steps after a restart at L = 28, N = 32) has no minimiser to hold 1e-6 against:
    those steps are counted, not compared -- the device's per-step launches are the second witness there (1e-9)."""
    torch = torch_mod
    from koopmpc.synth import duffing_rk4, initial_states, offline_data, offline_edmd, random_mlp_weights, vdp_rk4

    rng = np.random.RandomState(L * N)
    kw = dict(output=output, lb=-bnd, ub=bnd)
    if out_rows:
        kw.update(out_rows=out_rows, out_row0=0)
    rbf = lift == "rbf"
    plant = "vdp" if rbf else "duffing"
    if not rbf:
        w = random_mlp_weights(2, 100, layers, L, seed=5)
        make = lambda: KM(n=2, L=L, N=N, batch=B, weights=w, layers=layers, **kw)
        lift_fn = lambda x: ko.mlp_lift(w, x)
    else:
        Xo, Yo, Uo = offline_data(plant=vdp_rk4)
        cx = Xo[:, np.random.RandomState(0).choice(Xo.shape[1], L, replace=False)].T.copy()  # centres as bench.py's cfg3 takes them
        make = lambda: KM(n=2, L=L, N=N, batch=B, lift="rbf", centres=cx, **kw)
        lift_fn = lambda x: ko.rbf_lift(x, cx)
    mpc, mstep = make(), make()
    code, text = mpc.rollout_plugin_status()
    print("(%d, %d, %s): %s" % (L, N, output, text))
    assert code == 1 and mpc.rollout_is_fused(), (code, text)
    if rbf:
        A0, B0, C0 = [t.cpu().numpy() for t in mpc.offline_fit(Xo, Yo, Uo, init_rls=True)]
        mstep.offline_fit(Xo, Yo, Uo, init_rls=True)
        PX, PY = lift_fn(Xo), lift_fn(Yo)
        Z = np.concatenate([PX, Uo[None, :]], 0)
    else:
        A0, B0, C0 = offline_edmd(lambda X: mpc.Encoder(X), plant=duffing_rk4)
        mpc.set_model(A0, B0, C0); mstep.set_model(A0, B0, C0)
    q = L if output == "lift" else (out_rows or 2)
    if output == "lift":
        r = np.tile(lift_fn(np.array([[1.0], [0.0]])), (1, N))   # vanderpol.py:668-675
    else:
        r = np.tile(np.array([[1.0], [0.0]])[:q], (1, N))
    X0 = initial_states(B, seed=3)
    Xd = _t(torch, X0)
    step0, sw = 99, 102
    Ul, Xl = mpc.rollout(plant, Xd, r, steps, step0=step0, switch_step=sw, log=True)
    st = mpc.status.cpu().numpy()
    assert (st <= (1 if output == "lift" else 0)).all()
    # second witness: the same loop as per-step launches on the device (kmpc_step of an MLP set is a one-step launch of the same plug-in;
    # of an RBF set the lift kernel + the step kernel)
    X2 = _t(torch, X0)
    for k in range(steps):
        u2 = mstep.step(X2, r).clone()
        assert float((u2 - Ul[k]).abs().max()) < 1e-9, k
        X2 = mstep.plant_step(plant, X2, u2, switched=(step0 + k >= sw))
    Ul, Xl = Ul.cpu().numpy(), Xl.cpu().numpy()
    worst_u = worst_x = 0.0
    compared = singular = 0
    for b in range(min(B, 24)):
        if st[b] != 0:
            continue
        ctl = ko.OracleController(lift_fn, L, 2, N, -bnd, bnd, A0, B0, C0, output=output, rls="gain")
        if rbf:  # gain-form state of the least-squares fit over the offline samples
            ctl.gP = np.linalg.inv(Z @ Z.T); ctl.gK = (PY @ Z.T) @ ctl.gP
            ctl.gQ = np.linalg.inv(PX @ PX.T); ctl.gC = (Xo @ PX.T) @ ctl.gQ
        x = X0[:, b].copy()
        for k in range(steps):
            psi = lift_fn(x.reshape(2, 1)).reshape(-1)
            if ctl.prev is not None:
                ppsi, pu = ctl.prev
                ctl.gK, ctl.gP = ko.rls_update_gain(ctl.gK, ctl.gP, np.concatenate([ppsi, [pu]]), psi)
                ctl.gC, ctl.gQ = ko.rls_update_gain(ctl.gC, ctl.gQ, ppsi, x)
                ctl.A, ctl.B, ctl.C = ctl.gK[:, :-1].copy(), ctl.gK[:, -1:].copy(), ctl.gC.copy()
            Co = None if output == "lift" else ctl.C[:q]
            _, _, H, f, _ = ko.condense(ctl.A, ctl.B, Co, psi, r, N, ctl.Qw, ctl.Rw)
            if np.linalg.cond(H) < 1e9:
                U, _ = ko.qp_exact(H, f, -bnd, bnd)
                worst_u = max(worst_u, abs(Ul[k, b] - U[0]))
                compared += 1
            else:
                singular += 1
            ctl.prev = (psi, float(Ul[k, b]))  # (both sides regress on the applied input and continue from the device's state)
            xo = ko.plant_step(plant, x, float(Ul[k, b]), switched=(step0 + k >= sw))
            worst_x = max(worst_x, float(np.abs(Xl[k, :, b] - xo).max()))
            x = Xl[k, :, b].copy()
    print("   plug-in roll-out (%d, %d, q = %d, %s) vs oracle: %d QPs compared (%d numerically singular): max |u - u_oracle| %.2e, |x - x_oracle| %.2e"
          % (L, N, q, lift, compared, singular, worst_u, worst_x))
    assert compared >= singular and compared > 0
    # (26 thin-plate centres in the plane: the regressors are nearly dependent, cond(inv_K_G) ~ 1e12 -- the estimators of the two sides agree
    #  to 1e-9 of their scale and the minimisers to 2e-5; the device's own per-step launches above hold the fused launch to 1e-9)
    tol_u = 1e-4 if (rbf and L >= 24) else 1e-6
    assert worst_u < tol_u and worst_x < 1e-9


def test_matlab_twin_dimension_set_runs_fused(torch_mod, KM):
    """The reference's own MATLAB controller runs L = 10, N = 10, liftFun = [x; Encoder(x)] - [0; Encoder(0)] (Koopman_update.m:67, 70,
    113) -- not one of the built-in triples; round 5 served it with per-step launches.  KoopmanMPC(L=10, N=10, lift_offset="x_psi0") now
    reports a fused roll-out (plug-in; __graft_entry__.build() pre-builds it into the tree's kernel cache), 30 closed-loop steps as ONE
    launch with the reference encoder's weights match per-trajectory oracle controllers that lift the same way (u 1e-6), and the
    per-step route (kmpc_step = one-step launches of the same kernel) gives the same loop."""
    torch = torch_mod
    w = ko.load_mlp_weights(np.load(os.path.join(G, "weights_duffing.npz")))
    L, N, B, steps = 10, 10, 64, 30
    rng = np.random.RandomState(11)
    A = rng.randn(L, L) * 0.2 / np.sqrt(L)
    Bm, Cm = rng.randn(L, 1) * 0.3, rng.randn(2, L) * 0.3
    m = KM(n=2, L=L, N=N, batch=B, weights=w, lift_offset="x_psi0")
    code, text = m.rollout_plugin_status()
    print(text)
    assert code == 1 and m.rollout_is_fused()
    m.set_model(A, Bm, Cm)
    m2 = KM(n=2, L=L, N=N, batch=B, weights=w, lift_offset="x_psi0")
    m2.set_model(A, Bm, Cm)
    lift = lambda x: ko.mlp_lift_offset(w, x, "x_psi0")
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = 4 * rng.rand(2, B) - 2
    X = _t(torch, X0)
    Ul, Xl = m.rollout("duffing", X, r, steps, step0=90, switch_step=102, log=True)
    assert int(m.status.max().item()) == 0
    X2 = _t(torch, X0)
    for k in range(steps):
        u = m2.step(X2, r).clone()
        assert float((u - Ul[k]).abs().max()) < 1e-9, k
        X2 = m2.plant_step("duffing", X2, u, switched=(90 + k >= 102))
    Ul, Xl = Ul.cpu().numpy(), Xl.cpu().numpy()
    worst = 0.0
    for b in range(16):
        ctl = ko.OracleController(lift, L, 2, N, -2.0, 2.0, A, Bm, Cm, rls="gain")
        x = X0[:, b].copy()
        for k in range(steps):
            uo, _, _ = ctl.step(x, r)
            worst = max(worst, abs(Ul[k, b] - uo))
            ctl.prev = (ctl.prev[0], float(Ul[k, b]))
            x = Xl[k, :, b].copy()
    print("MATLAB-twin set (10, 10, 2), [x; psi(x)] - [0; psi(0)] lift, 30 fused steps vs oracle: max |u - u_oracle| %.2e" % worst)
    assert worst < 1e-6


def test_plugin_is_compiled_on_the_box_when_the_cache_is_empty_and_f32_panels_get_theirs(torch_mod, KM, tmp_path, monkeypatch):
    """The hipcc route itself, on the GPU box: with an empty kernel cache ($KMPC_KERNEL_CACHE -> a fresh directory; the dimension set is
    one no other test uses, so the process table does not hold it either) kmpc_create compiles csrc/rollout_jit.hip, reports the
    seconds it took, and the launch works; a KMPC_F32 controller of the set gets the float32-panel variant and equals the float64
    launch rounded once (row g2's statement, for a plug-in set)."""
    torch = torch_mod
    from koopmpc.synth import initial_states, random_mlp_weights

    monkeypatch.setenv("KMPC_KERNEL_CACHE", str(tmp_path))
    L, N, B = 18, 14, 48
    w = random_mlp_weights(2, 100, 3, L, seed=12)
    rng = np.random.RandomState(3)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    A, Bm, Cm = f32(rng.randn(L, L) * 0.2 / np.sqrt(L)), f32(rng.randn(L, 1) * 0.3), f32(rng.randn(2, L) * 0.3)
    m64 = KM(n=2, L=L, N=N, batch=B, weights=w)
    code, text = m64.rollout_plugin_status()
    print(text)
    assert code == 1 and "compiled with hipcc" in text and str(tmp_path) in text, text
    m32 = KM(n=2, L=L, N=N, batch=B, weights=w, dtype=torch.float32)
    code32, text32 = m32.rollout_plugin_status()
    print(text32)
    assert code32 == 1 and "_f32_" in text32 and m32.rollout_is_fused()
    for m in (m64, m32):
        m.set_model(A, Bm, Cm)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = f32(initial_states(B, seed=4))
    X64 = torch.tensor(X0, dtype=torch.float64, device="cuda:0").contiguous()
    X32 = torch.tensor(X0, dtype=torch.float32, device="cuda:0").contiguous()
    U64, _ = m64.rollout("duffing", X64, r, 12, log=True)
    U32, _ = m32.rollout("duffing", X32, r, 12, log=True)
    assert int(m64.status.max().item()) == 0 and int(m32.status.max().item()) == 0
    assert torch.equal(U32, U64.float()) and torch.equal(X32, X64.float())
    # a second controller of the set finds the plug-in in the process table: no second compile
    m64b = KM(n=2, L=L, N=N, batch=B, weights=w)
    assert m64b.rollout_plugin_status() == (code, text)


def test_plugin_handle_keeps_its_workgroup_and_a_launch_never_compiles(torch_mod, KM, tmp_path, monkeypatch):
    """A plug-in handle launches the object it loaded when it was created: kmpc_set_rollout_workgroup afterwards neither compiles
    anything at the launch (the kernel cache is unchanged) nor changes the result -- U and X equal those of a handle run at the default
    workgroup bit for bit (a trajectory's arithmetic does not depend on its workgroup)."""
    import re

    torch = torch_mod
    from koopmpc import _ffi
    from koopmpc.synth import initial_states, random_mlp_weights

    lib = _ffi.load()
    monkeypatch.setenv("KMPC_KERNEL_CACHE", str(tmp_path))
    L, N, B, steps = 12, 9, 40, 7
    w = random_mlp_weights(2, 100, 3, L, seed=21)
    rng = np.random.RandomState(5)
    A, Bm, Cm = rng.randn(L, L) * 0.2 / np.sqrt(L), rng.randn(L, 1) * 0.3, rng.randn(2, L) * 0.3
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = initial_states(B, seed=6)
    m0, m1 = KM(n=2, L=L, N=N, batch=B, weights=w), KM(n=2, L=L, N=N, batch=B, weights=w)
    code, text = m1.rollout_plugin_status()
    print(text)
    assert code == 1 and m1.rollout_is_fused(), text
    nw = int(re.search(r"_nw(\d+)_", text).group(1))
    for m in (m0, m1):
        m.set_model(A, Bm, Cm)
    X_0, X_1 = _t(torch, X0), _t(torch, X0)
    U0, Xl0 = m0.rollout("duffing", X_0, r, steps, log=True)
    torch.cuda.synchronize()
    listing = sorted(os.listdir(tmp_path))
    try:
        assert lib.kmpc_set_rollout_workgroup(8 if nw == 4 else 4) == 0
        assert m1.rollout_is_fused()
        U1, Xl1 = m1.rollout("duffing", X_1, r, steps, log=True)
        torch.cuda.synchronize()
    finally:
        lib.kmpc_set_rollout_workgroup(0)
    assert sorted(os.listdir(tmp_path)) == listing
    assert int(m0.status.max().item()) == 0 and int(m1.status.max().item()) == 0
    assert torch.equal(U0, U1) and torch.equal(Xl0, Xl1) and torch.equal(X_0, X_1)


# ------------------------------------------------------------------ per-step terminal refresh inside the roll-out
@pytest.mark.parametrize("L,N,B,lift,lift_offset,every", [(8, 10, 48, "mlp", None, 1), (10, 10, 40, "mlp", "x_psi0", 1), (8, 10, 30, "rbf", None, 1),
                                                          (20, 20, 24, "mlp", None, 3)])
def test_terminal_refresh_inside_the_rollout(torch_mod, KM, L, N, B, lift, lift_offset, every):
    """VERDICT r5 item 6.  The MATLAB controller recomputes its terminal ingredients with the updated model at EVERY iteration
    (Koopman_update.m:215 K = -dlqr(A, B, ...), :381 Q_bar(end) = C*P*C'; P from the Riccati iteration as stand-in for its LMI,
    duffing.py:583-613).  kmpc_set_terminal_refresh(every): 30 closed-loop steps as ONE launch -- RLS update, then the Riccati iteration
    on the trajectory's fresh [A B] inside the kernel, then the condensed QP with Co P Co' as terminal block -- against an oracle loop
    that calls solve_dare + terminal_block with the updated model at each refresh step (u <= 1e-6, x <= 1e-9), and against the same
    loop taken step by step (kmpc_step; for the RBF set that is the per-step route: RLS launch, dare_kernel, QP launch: 1e-9).  (20, 20) is a built-in dimension set: the
    refreshing kernel is a plug-in there too; every = 3 holds the block between refreshes."""
    torch = torch_mod
    from koopmpc.synth import offline_data, random_mlp_weights, vdp_rk4

    rng = np.random.RandomState(100 * L + N)
    rbf = lift == "rbf"
    plant = "vdp" if rbf else "duffing"
    if lift == "mlp":
        w = ko.load_mlp_weights(np.load(os.path.join(G, "weights_duffing.npz"))) if L in (8, 10) else random_mlp_weights(2, 100, 3, L, seed=5)
        make = lambda: KM(n=2, L=L, N=N, batch=B, weights=w, lift_offset=lift_offset)
        lift_fn = (lambda x: ko.mlp_lift_offset(w, x, lift_offset)) if lift_offset else (lambda x: ko.mlp_lift(w, x))
    else:
        # (as vanderpol_RBF.py: centres from the data, the estimator continues from the offline samples, :434-438)
        Xo, Yo, Uo = offline_data(plant=vdp_rk4)
        cx = Xo[:, np.random.RandomState(0).choice(Xo.shape[1], L, replace=False)].T.copy()
        make = lambda: KM(n=2, L=L, N=N, batch=B, lift="rbf", centres=cx)
        lift_fn = lambda x: ko.rbf_lift(x, cx)
    Qd, Rd = 10.0 * np.eye(L), 0.01
    m, ms = make(), make()
    if rbf:
        A, Bm, Cm = [t_.cpu().numpy() for t_ in m.offline_fit(Xo, Yo, Uo, init_rls=True)]
        ms.offline_fit(Xo, Yo, Uo, init_rls=True)
        PX, PY = lift_fn(Xo), lift_fn(Yo)
        Z = np.concatenate([PX, Uo[None, :]], 0)
    else:
        A = rng.randn(L, L) * 0.5 / np.sqrt(L)
        Bm, Cm = rng.randn(L, 1) * 0.3, rng.randn(2, L) * 0.3
    for c in (m, ms):
        if not rbf:
            c.set_model(A, Bm, Cm)
        c.set_terminal_refresh(every, Qd, Rd)
    code, text = m.rollout_plugin_status()
    print(text)
    assert code == 1 and "_term_" in text and m.rollout_is_fused()
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = 4 * rng.rand(2, B) - 2
    steps = 30
    X = _t(torch, X0)
    Ul, Xl = m.rollout(plant, X, r, steps, step0=95, switch_step=102, log=True)
    assert int(m.status.max().item()) == 0
    # the same loop step by step on a second handle (kmpc_step: one-step launches of the refreshing kernel for the MLP sets, the per-step
    # route -- RLS launch, dare_kernel, QP launch -- for the RBF set)
    X2 = _t(torch, X0)
    worst_step = 0.0
    for k in range(steps):
        u2 = ms.step(X2, r).clone()
        worst_step = max(worst_step, float((u2 - Ul[k]).abs().max()))
        X2 = ms.plant_step(plant, X2, u2, switched=(95 + k >= 102))
    Ul, Xl = Ul.cpu().numpy(), Xl.cpu().numpy()
    worst_u = worst_x = 0.0
    for b in range(min(B, 16)):
        ctl = ko.OracleController(lift_fn, L, 2, N, -2.0, 2.0, A, Bm, Cm, rls="gain")
        if rbf:  # gain-form state of the least-squares fit over the offline samples
            ctl.gP = np.linalg.inv(Z @ Z.T); ctl.gK = (PY @ Z.T) @ ctl.gP
            ctl.gQ = np.linalg.inv(PX @ PX.T); ctl.gC = (Xo @ PX.T) @ ctl.gQ
        PN = None
        x = X0[:, b].copy()
        for k in range(steps):
            psi = lift_fn(x.reshape(2, 1)).reshape(-1)
            if ctl.prev is not None:
                ppsi, pu = ctl.prev
                ctl.gK, ctl.gP = ko.rls_update_gain(ctl.gK, ctl.gP, np.concatenate([ppsi, [pu]]), psi)
                ctl.gC, ctl.gQ = ko.rls_update_gain(ctl.gC, ctl.gQ, ppsi, x)
                ctl.A, ctl.B, ctl.C = ctl.gK[:, :-1].copy(), ctl.gK[:, -1:].copy(), ctl.gC.copy()
            if k % every == 0:  # K = -dlqr(A, B, ...) / P with the UPDATED model; Q_bar(end) = C*P*C'   (Koopman_update.m:215, 381)
                P, _ = ko.solve_dare(ctl.A, ctl.B, Qd, Rd)
                PN = ko.terminal_block(ctl.C, P)
            _, _, H, f, _ = ko.condense(ctl.A, ctl.B, ctl.C, psi, r, N, ctl.Qw, ctl.Rw, PN=PN)
            U, _ = ko.qp_exact(H, f, -2.0, 2.0)
            worst_u = max(worst_u, abs(Ul[k, b] - U[0]))
            ctl.prev = (psi, float(Ul[k, b]))
            xo = ko.plant_step(plant, x, float(Ul[k, b]), switched=(95 + k >= 102))
            worst_x = max(worst_x, float(np.abs(Xl[k, :, b] - xo).max()))
            x = Xl[k, :, b].copy()
    print("terminal refresh every %d step(s) inside ONE launch, (%d, %d, %s): vs oracle loop with solve_dare + terminal_block max |u - u_oracle| %.2e, "
          "|x - x_oracle| %.2e; vs the per-step route %.2e" % (every, L, N, lift, worst_u, worst_x, worst_step))
    # (the RBF set's second route is another kernel -- LDS step instead of the register-state step, another order of summation -- on an
    #  estimator whose covariance has condition ~1e10: 3e-9 measured)
    assert worst_u < 1e-6 and worst_x < 1e-9 and worst_step < (1e-7 if rbf else 1e-9)
    # the blocks the launch left are those kmpc_terminal_from_dare computes for the same (final) models -- when the last step refreshed
    if (steps - 1) % every == 0:
        PNk, itk = m.terminal_from_dare(Qd, Rd, per_trajectory=True)
        PNo = []
        Af, Bf, Cf = [t.cpu().numpy() for t in m.get_model()]
        for b in range(4):
            P, _ = ko.solve_dare(Af[b], Bf[b], Qd, Rd)
            PNo.append(ko.terminal_block(Cf[b], P))
        assert np.abs(PNk[:4] - np.array(PNo)).max() <= 1e-8 * max(1.0, np.abs(np.array(PNo)).max())


# ------------------------------------------------------------------ the placement pass: O(B) radix sort instead of all pairs
@pytest.mark.parametrize("B", [16, 4096, 16384, 65536, 262144])
def test_rank_by_work_is_a_stable_descending_sort(torch_mod, B):
    """the rank pass behind a fused launch compared every pair of trajectories (O(B^2): 62 us at 16 384, switched
    off beyond).  Round 6: a stable radix sort by one workgroup, O(B), for up to 2^20 trajectories.  kmpc_rank_by_work on random work
    counters (many ties, values beyond the 12-bit key range, negatives) against NumPy: read back through the card deal, the
    trajectories appear in the order of a STABLE sort by descending (clipped) work -- ties by index, so the table is a function of the
    counters alone."""
    torch = torch_mod
    import ctypes as C

    from koopmpc import _ffi

    lib = _ffi.load()
    rng = np.random.RandomState(B)
    w = rng.randint(-3, 60, size=B).astype(np.int32)
    w[rng.rand(B) < 0.02] = 10 ** 6            # beyond the key range: clipped to 4095
    wd = torch.tensor(w, device="cuda:0")
    perm = torch.full((3 * B,), -1, dtype=torch.int32, device="cuda:0")
    rc = lib.kmpc_rank_by_work(C.c_void_p(wd.data_ptr()), B, C.c_void_p(perm.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    tab = perm[:B].cpu().numpy().reshape(B // 16, 16)   # [workgroup g][wave p] -> trajectory
    G = B // 16
    order = np.empty(B, dtype=np.int64)
    for p in range(16):
        col = tab[:, p] if p % 2 == 0 else tab[::-1, p]
        order[p * G:(p + 1) * G] = col
    key = np.clip(w, 0, 4095)
    want = np.argsort(-key.astype(np.int64), kind="stable")
    assert np.array_equal(order, want)


def test_round6_entry_points_refuse_bad_arguments(torch_mod, KM):
    """The entry points added in round 6 answer bad arguments with an error code (never a launch): the placement pass with a batch that is
    no multiple of 16 / above 2^20 / null buffers, the terminal refresh with a negative period, no Q, no iterations or on a float32
    handle, the plug-in pre-build with dimensions outside the single-wave kernels, and the status query with a tiny text buffer."""
    torch = torch_mod
    import ctypes as C

    from koopmpc import _ffi

    lib = _ffi.load()
    w = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    perm = torch.zeros(3 * 64, dtype=torch.int32, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.kmpc_rank_by_work(C.c_void_p(w.data_ptr()), 24, C.c_void_p(perm.data_ptr()), s) != 0
    assert lib.kmpc_rank_by_work(C.c_void_p(w.data_ptr()), 0, C.c_void_p(perm.data_ptr()), s) != 0
    assert lib.kmpc_rank_by_work(C.c_void_p(w.data_ptr()), (1 << 20) + 16, C.c_void_p(perm.data_ptr()), s) != 0
    assert lib.kmpc_rank_by_work(None, 64, C.c_void_p(perm.data_ptr()), s) != 0
    assert lib.kmpc_rank_by_work(C.c_void_p(w.data_ptr()), 64, None, s) != 0
    torch.cuda.synchronize()

    from koopmpc.synth import random_mlp_weights

    wts = random_mlp_weights(2, 16, 2, 8, seed=3)
    m = KM(n=2, L=8, N=10, batch=16, weights=wts, hidden=16, layers=2)
    Q = np.ascontiguousarray(10.0 * np.eye(8))
    qp = Q.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.kmpc_set_terminal_refresh(m.h, -1, qp, 0.01, 500, 0.01) != 0
    assert lib.kmpc_set_terminal_refresh(m.h, 1, None, 0.01, 500, 0.01) != 0
    assert lib.kmpc_set_terminal_refresh(m.h, 1, qp, 0.01, 0, 0.01) != 0
    assert lib.kmpc_set_terminal_refresh(m.h, 0, None, 0.01, 0, 0.01) == 0      # switching it off needs nothing
    with pytest.raises(ValueError):
        m.set_terminal_refresh(every=1, Q=np.eye(7))
    m32 = KM(n=2, L=8, N=10, batch=16, weights=wts, hidden=16, layers=2, dtype=torch.float32)
    assert lib.kmpc_set_terminal_refresh(m32.h, 1, qp, 0.01, 500, 0.01) != 0

    buf = C.create_string_buffer(256)
    for bad in [(3, 8, 10, 0, 0, 16, 64, 1), (2, 0, 10, 0, 0, 16, 64, 1), (2, 8, 0, 0, 0, 16, 64, 1), (2, 8, 10, 0, 0, 0, 64, 1),
                (2, 8, 10, 0, 0, 200, 64, 1), (2, 8, 10, 0, 0, 16, 0, 1), (2, 8, 10, 0, 0, 16, 64, 7)]:
        assert lib.kmpc_rollout_plugin_prebuild(*bad, buf, 256) == -3, bad
    assert lib.kmpc_rollout_plugin_prebuild(2, 80, 10, 0, 0, 16, 64, 1, buf, 256) == 2   # (81^2 > 2048: no single-wave kernel, not an error)
    tiny = C.create_string_buffer(4)
    code = lib.kmpc_rollout_plugin_status(m.h, tiny, 4)
    assert code in (0, 1, 2, -1) and len(tiny.value) <= 3
    assert lib.kmpc_rollout_plugin_status(None, buf, 256) == -100
