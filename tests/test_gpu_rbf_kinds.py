"""rbf.m's Gaussian, inverse-quadric, inverse-multiquadric and polyharmonic dictionaries (KMPC_LIFT_RBF_GAUSS .. KMPC_LIFT_RBF_POLYHARMONIC)
on every route that serves the thin plates.  Runs on the MI355X box:  python -m pytest tests/test_gpu_rbf_kinds.py -m gpu -s

The statement of the four formulas is `rbf_m` below: rbf.m:10-44 of the reference transcribed line by line into NumPy (the product does
not import the oracle and oracle/ does not take new code).  The closed-loop machinery is the oracle's, used as
tests/test_gpu_round6.py::test_fused_rollout_of_dimension_sets_without_a_builtin_instantiation uses it, with `rbf_m` as the lift.

Bounds
  lift, float64   1e-12 * max(1, max|psi|): each formula is about ten correctly rounded operations, the Gaussian's argument amplifies
                  one ulp by at most eps^2 r2 < 50
  lift, float32   tests/test_gpu_float32.py's CAP_LIFT = 1e-4 of the same scale, against the float64 transcription
  r = 0           X ends with the centres themselves: gauss, invquad, invmultquad give exactly 1.0 there, polyharmonic exactly 0.0
  closed loop     fused launch vs kmpc_step / kmpc_plant_step 1e-9; vs per-trajectory oracle controllers u 1e-6, x 1e-9; no step may
                  be left out as numerically singular (cond(H) < 1e9) and a third of the compared u_0 lies strictly inside the box
"""
import ctypes

import numpy as np
import pytest

from oracle import koopman_oracle as ko

pytestmark = pytest.mark.gpu

CAP_LIFT = 1e-4  # (tests/test_gpu_float32.py)


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


def rbf_m(X, C, type, eps=None, k=None):
    """rbf.m:10-44.  X (n, N), C (n, K) -> (K, N)."""
    type = type.lower()                                                # :11
    if eps is None:                                                    # :12-14
        eps = 1
    if k is None:                                                      # :15-17
        k = 1
    Cbig = C                                                           # :19
    Y = np.zeros((C.shape[1], X.shape[1]))                             # :20
    for i in range(Cbig.shape[1]):                                     # :21
        C = Cbig[:, i:i + 1]                                           # :22
        C = np.tile(C, (1, X.shape[1]))                                # :23
        r_squared = np.sum((X - C) ** 2, axis=0)                       # :24
        with np.errstate(divide="ignore", invalid="ignore"):
            if type == "thinplate":                                    # :26
                y = r_squared * np.log(np.sqrt(r_squared))             # :27
                y[np.isnan(y)] = 0                                     # :29
            elif type == "gauss":                                      # :30
                y = np.exp(-eps ** 2 * r_squared)                      # :31
            elif type == "invquad":                                    # :32
                y = 1 / (1 + eps ** 2 * r_squared)                     # :33
            elif type == "invmultquad":                                # :34
                y = 1 / np.sqrt((1 + eps ** 2 * r_squared))            # :36
            elif type == "polyharmonic":                               # :37
                y = r_squared ** (k / 2) * np.log(np.sqrt(r_squared))  # :38
                y[np.isnan(y)] = 0                                     # :39
            else:
                raise ValueError("RBF type not recognize")             # :41
        Y[i, :] = y                                                    # :43
    return Y


# (rbf.m type, eps, k): what the issue's cases name
_KINDS = [("gauss", e, 1) for e in (1.0, 0.5)] + [("invquad", e, 1) for e in (1.0, 0.5)] + [("invmultquad", e, 1) for e in (1.0, 0.5)] + \
         [("polyharmonic", 1.0, k) for k in (1, 2, 3, 4, 8)]


def _kid(c):
    return "%s-%s" % (c[0], ("k%d" % c[2]) if c[0] == "polyharmonic" else ("eps%g" % c[1]))


def _make(KM, type, eps, k, **kw):
    if type == "polyharmonic":
        return KM(lift="rbf_polyharmonic", rbf_k=k, **kw)
    return KM(lift="rbf_" + type, rbf_eps=eps, **kw)


# ------------------------------------------------------------------ 1. lift parity
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("n,L", [(2, 8), (1, 33), (4, 4), (3, 5)])
@pytest.mark.parametrize("kind", _KINDS, ids=_kid)
def test_lift_parity(torch_mod, KM, kind, n, L, f32):
    torch = torch_mod
    type, eps, k = kind
    rng = np.random.RandomState(100 * n + L)
    cx = 4 * rng.rand(L, n) - 2
    X = np.concatenate([4 * rng.rand(n, 17) - 2, cx.T], axis=1)  # the centres themselves: r = 0 exactly at [j, 17 + j]
    ref = rbf_m(X, cx.T, type, eps, k)
    dt = torch.float32 if f32 else torch.float64
    m = _make(KM, type, eps, k, n=n, L=L, N=4, batch=X.shape[1], centres=cx, dtype=dt)
    psi = m.rbf(_t(torch, X, dt)).double().cpu().numpy()
    assert psi.shape == ref.shape
    scale = max(1.0, float(np.abs(ref).max()))
    dev = float(np.abs(psi - ref).max()) / scale
    print("   lift %s (n = %d, L = %d, %s): max |psi - rbf.m| / max(1, |psi|) = %.2e (scale %.3g)" % (_kid(kind), n, L, "f32" if f32 else "f64", dev, scale))
    at_centres = psi[np.arange(L), 17 + np.arange(L)]
    assert np.array_equal(at_centres, np.full(L, 0.0 if type == "polyharmonic" else 1.0)), at_centres
    assert dev <= (CAP_LIFT if f32 else 1e-12), dev


# ------------------------------------------------------------------ 2., 3. fused roll-out against the per-step route and the oracle
def _closed_loop(torch, KM, L, N, B, steps, kind, expect_code, bnd=20.0):
    from koopmpc.synth import initial_states, offline_data, vdp_rk4

    type, eps, k = kind
    Xo, Yo, Uo = offline_data(plant=vdp_rk4)
    cx = Xo[:, np.random.RandomState(0).choice(Xo.shape[1], L, replace=False)].T.copy()  # (the centres of _PLUGIN_SETS' RBF rows)
    make = lambda: _make(KM, type, eps, k, n=2, L=L, N=N, batch=B, centres=cx, output="Cx", lb=-bnd, ub=bnd)
    lift_fn = lambda x: rbf_m(x, cx.T, type, eps, k)
    mpc, mstep = make(), make()
    code, text = mpc.rollout_plugin_status()
    print("(%d, %d) %s: %s" % (L, N, _kid(kind), text))
    assert code == expect_code and mpc.rollout_is_fused(), (code, text)
    A0, B0, C0 = [t.cpu().numpy() for t in mpc.offline_fit(Xo, Yo, Uo, init_rls=True)]
    mstep.offline_fit(Xo, Yo, Uo, init_rls=True)
    PX, PY = lift_fn(Xo), lift_fn(Yo)
    Z = np.concatenate([PX, Uo[None, :]], 0)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = initial_states(B, seed=3)
    Xd = _t(torch, X0)
    step0, sw = 99, 102
    Ul, Xl = mpc.rollout("vdp", Xd, r, steps, step0=step0, switch_step=sw, log=True)
    st = mpc.status.cpu().numpy()
    assert (st == 0).all(), st
    X2 = _t(torch, X0)
    worst_route = 0.0
    for j in range(steps):
        u2 = mstep.step(X2, r).clone()
        worst_route = max(worst_route, float((u2 - Ul[j]).abs().max()))
        X2 = mstep.plant_step("vdp", X2, u2, switched=(step0 + j >= sw))
    Ul, Xl = Ul.cpu().numpy(), Xl.cpu().numpy()
    worst_u = worst_x = 0.0
    compared = singular = interior = 0
    for b in range(min(B, 24)):
        ctl = ko.OracleController(lift_fn, L, 2, N, -bnd, bnd, A0, B0, C0, output="Cx", rls="gain")
        ctl.gP = np.linalg.inv(Z @ Z.T); ctl.gK = (PY @ Z.T) @ ctl.gP  # gain-form state of the least-squares fit over the offline samples
        ctl.gQ = np.linalg.inv(PX @ PX.T); ctl.gC = (Xo @ PX.T) @ ctl.gQ
        x = X0[:, b].copy()
        for j in range(steps):
            psi = lift_fn(x.reshape(2, 1)).reshape(-1)
            if ctl.prev is not None:
                ppsi, pu = ctl.prev
                ctl.gK, ctl.gP = ko.rls_update_gain(ctl.gK, ctl.gP, np.concatenate([ppsi, [pu]]), psi)
                ctl.gC, ctl.gQ = ko.rls_update_gain(ctl.gC, ctl.gQ, ppsi, x)
                ctl.A, ctl.B, ctl.C = ctl.gK[:, :-1].copy(), ctl.gK[:, -1:].copy(), ctl.gC.copy()
            _, _, H, f, _ = ko.condense(ctl.A, ctl.B, ctl.C[:2], psi, r, N, ctl.Qw, ctl.Rw)
            if np.linalg.cond(H) < 1e9:
                U, _ = ko.qp_exact(H, f, -bnd, bnd)
                worst_u = max(worst_u, abs(Ul[j, b] - U[0]))
                compared += 1
                interior += int(-bnd < U[0] < bnd)
            else:
                singular += 1
            ctl.prev = (psi, float(Ul[j, b]))  # (both sides regress on the applied input and continue from the device's state)
            xo = ko.plant_step("vdp", x, float(Ul[j, b]), switched=(step0 + j >= sw))
            worst_x = max(worst_x, float(np.abs(Xl[j, :, b] - xo).max()))
            x = Xl[j, :, b].copy()
    print("   roll-out (%d, %d) %s: fused vs per-step %.2e; vs oracle over %d QPs (%d singular, %d interior): max |u - u_oracle| %.2e, |x - x_oracle| %.2e"
          % (L, N, _kid(kind), worst_route, compared, singular, interior, worst_u, worst_x))
    assert worst_route < 1e-9
    assert singular == 0 and compared > 0
    assert 3 * interior >= compared, (interior, compared)
    assert worst_u < 1e-6 and worst_x < 1e-9


@pytest.mark.parametrize("kind", [("gauss", 1.0, 1), ("invquad", 1.0, 1), ("invmultquad", 1.0, 1), ("polyharmonic", 1.0, 3)], ids=_kid)
def test_fused_rollout_plugin_set(torch_mod, KM, kind):
    """(L, N) = (6, 12): no instantiation inside the library; ONE plug-in object (..._ksm2_...) serves the four kinds, which of them is a
    launch argument."""
    _closed_loop(torch_mod, KM, 6, 12, 50, 12, kind, expect_code=1)


def test_fused_rollout_builtin_set(torch_mod, KM):
    """(8, 30): the set of BASELINE cfg3's instantiation inside the library, B = 33 leaves a tail wave.  The library's own instantiation is
    the thin plates' and stays what it was; the other kinds of this set run on a plug-in object too (status 1), as its refreshing and
    diagnostics variants do."""
    _closed_loop(torch_mod, KM, 8, 30, 33, 8, ("gauss", 1.0, 1), expect_code=1)


# ------------------------------------------------------------------ float32 handles: the float64 fused roll-out behind float32 panels
@pytest.mark.parametrize("kind", [("polyharmonic", 1.0, 2), ("gauss", 1.0, 1)], ids=_kid)
def test_f32_handle_fused_rollout(torch_mod, KM, kind):
    """A KMPC_F32 handle of a new kind at cfg3's set runs the float64 roll-out of its core behind float32 panels, on the float32-panel
    object of rbf.m's kinds (..._ksm2_f32_...); kind, width and k must reach the core.  The set-up and the stated tolerance are those of
    tests/test_gpu_round5.py::test_f32_io_rbf_rollout (the same dimensions with the thin plate): both handles start from the same
    host-computed estimator state, 15 closed-loop steps, every solve optimal, states within 1e-3 of the float64 handle and inputs within
    0.25 % of the box -- that test states its 1e-2 as 0.25 % of its box +-2; the box here is +-20 (with +-2 nearly every input of these
    dictionaries is saturated and the comparison is empty), so 0.1.  Measured: polyharmonic k = 2 |du| 3.8e-3, |dx| 1.1e-4, 789 of 960
    inputs inside the box; gauss |du| 1.3e-2, |dx| 3.3e-4, 592 of 960 inside.  Polyharmonic k = 2 is r2 log(sqrt(r2)), the thin plate of
    that test; with the default k = 1 in the core the loops would part by the size of the box."""
    torch = torch_mod
    from koopmpc.synth import initial_states, offline_data, vdp_rk4

    type, eps, k = kind
    f32x = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    L, N, B, bnd = 8, 30, 64, 20.0
    Xo, Yo, Uo = [f32x(a) for a in offline_data(plant=vdp_rk4)]
    cx = Xo[:, np.random.RandomState(0).choice(Xo.shape[1], L, replace=False)].T.copy()
    PX, PY = rbf_m(Xo, cx.T, type, eps, k), rbf_m(Yo, cx.T, type, eps, k)
    Z = np.concatenate([PX, Uo[None, :]], 0)
    P = np.linalg.inv(Z @ Z.T + 1e-9 * np.eye(L + 1)); KA = PY @ Z.T
    bQ = np.linalg.inv(PX @ PX.T + 1e-9 * np.eye(L)); bX = Xo @ PX.T
    ms = []
    for dt in (torch.float32, torch.float64):
        m = _make(KM, type, eps, k, n=2, L=L, N=N, batch=B, centres=cx, P0=1e5, barQ0=1e5, lb=-bnd, ub=bnd, dtype=dt)
        m.set_model((KA @ P)[:, :L], (KA @ P)[:, L], bX @ bQ)
        m.state_init(K_A=KA, inv_K_G=P, bar_X=bX, bar_Q=bQ)
        ms.append(m)
    m32, m64 = ms
    code, text = m32.rollout_plugin_status()
    print("float32 handle %s: %s" % (_kid(kind), text))
    assert m32.rollout_is_fused() and code == 1 and "ksm2_f32" in text, (code, text)
    X0 = f32x(initial_states(B, seed=3))
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X32, X64 = _t(torch, X0, torch.float32), _t(torch, X0)
    U32, _ = m32.rollout("vdp", X32, r, 15, log=True)
    U64, _ = m64.rollout("vdp", X64, r, 15, log=True)
    assert int(m32.status.max().item()) == 0 and int(m64.status.max().item()) == 0 and bool(torch.isfinite(X32).all())
    du, dx = float((U32.double() - U64).abs().max()), float((X32.double() - X64).abs().max())
    inside = int((U64.abs() < bnd).sum().item())
    print("   %s behind float32 panels, 15 steps: max |du| %.2e |dx| %.2e, %d of %d inputs inside the box" % (_kid(kind), du, dx, inside, U64.numel()))
    assert 3 * inside >= U64.numel()
    assert du < 0.0025 * (2 * bnd) and dx < 1e-3


# ------------------------------------------------------------------ 4. the stand-alone lift and the fused roll-out run the same machine code
def test_fused_lift_is_the_stand_alone_lift_bit_for_bit(torch_mod, KM):
    torch = torch_mod
    from koopmpc.synth import initial_states, offline_data, vdp_rk4

    L, N, B, steps = 8, 10, 40, 6
    Xo, Yo, Uo = offline_data(plant=vdp_rk4)
    cx = Xo[:, np.random.RandomState(0).choice(Xo.shape[1], L, replace=False)].T.copy()
    make = lambda: KM(n=2, L=L, N=N, batch=B, lift="rbf_invmultquad", centres=cx, lb=-20.0, ub=20.0)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = initial_states(B, seed=3)
    mpc = make()
    mpc.offline_fit(Xo, Yo, Uo, init_rls=True)
    assert mpc.set_rollout_diagnostics(True) == 0 and mpc.rollout_is_fused()  # (the diagnostics variant of the fused kernel)
    Xd = _t(torch, X0)
    Ul, Xl, diag = mpc.rollout("vdp", Xd, r, steps, step0=99, switch_step=102, log=True, diagnostics=True)
    assert int(mpc.status.max().item()) == 0
    for j in range(steps):
        Xj = _t(torch, X0) if j == 0 else Xl[j - 1].contiguous()
        assert np.array_equal(diag["Psi"][j].cpu().numpy(), mpc.rbf(Xj).cpu().numpy()), j
    # With the per-step terminal refresh armed: the TERM variant of the kernel against its per-step route.  The two routes are two orders of
    # the same arithmetic, so their inputs differ by about cond(H) * 2^-53 * |u|.  Measured at this set (invmultquad, box +-20): unarmed
    # cond(H) 1.3e2 -> 1.3e-11; armed with the refresh's default weights (Q = 10 I, R = 0.01) the terminal block is 1e7, cond(H) 8.8e8 ->
    # 3.6e-7 (the thin plate "rbf_matlab" at the same set: 1.4e8 -> 1.3e-7); Q = I: 9.1e7 -> 3.7e-8; 0.1 I: 1.1e7 -> 9.8e-9; 1e-3 I with
    # R = 1: 6.5e5 -> 5.4e-10.  1e-9 is therefore held where cond(H) is at most a few 1e5: Q = 1e-4 I, R = 1 (measured: cond(H) 2.5e2 ->
    # 7.8e-12).  The refresh is not idle there: the armed inputs differ from the unarmed launch's by more than 1 (measured 1.7).
    Qd, Rd = 1e-4 * np.eye(L), 1.0
    arm, armstep = make(), make()
    for m in (arm, armstep):
        m.offline_fit(Xo, Yo, Uo, init_rls=True)
        m.set_terminal_refresh(every=1, Q=Qd, R=Rd)
    code, text = arm.rollout_plugin_status()
    assert arm.rollout_is_fused() and code == 1 and "_term" in text, (code, text)
    Xa = _t(torch, X0)
    Ua, _ = arm.rollout("vdp", Xa, r, steps, step0=99, switch_step=102, log=True)
    assert int(arm.status.max().item()) == 0
    X2, worst, cond = _t(torch, X0), 0.0, 0.0
    for j in range(steps):
        u2 = armstep.step(X2, r).clone()
        worst = max(worst, float((u2 - Ua[j]).abs().max()))
        H = armstep.condense(armstep.rbf(X2), r)[0].cpu().numpy()
        cond = max(cond, max(float(np.linalg.cond(H[b])) for b in range(0, B, 8)))
        X2 = armstep.plant_step("vdp", X2, u2, switched=(99 + j >= 102))
    moved = float((Ua - Ul).abs().max())
    print("   armed refresh (8, 10) invmultquad, Q = 1e-4 I, R = 1: fused vs per-step %.2e, cond(H) <= %.2e, |U_armed - U_unarmed| %.2e" % (worst, cond, moved))
    assert moved > 1.0
    assert worst < 1e-9


# ------------------------------------------------------------------ 5. refusals
def test_refusals(torch_mod, KM):
    from koopmpc import _ffi
    from koopmpc import api as kapi

    lib = _ffi.load()
    cx = np.array([[0.0, 1.0], [1.0, 0.0], [0.5, 0.5]])
    gauss = KM(n=2, L=3, N=4, batch=1, lift="rbf_gauss", centres=cx, rbf_k=2)  # (k is read by the polyharmonic only, as in rbf.m: ignored here)
    mlp = KM(n=2, L=3, N=4, batch=1, lift="mlp", hidden=8, layers=2)
    poly = KM(n=2, L=3, N=4, batch=1, lift="rbf_polyharmonic", centres=cx)
    assert lib.kmpc_set_rbf_order(gauss.h, 2) == -3 and lib.kmpc_last_error(gauss.h)
    assert lib.kmpc_set_rbf_order(mlp.h, 2) == -3 and lib.kmpc_last_error(mlp.h)
    assert lib.kmpc_set_rbf_order(poly.h, 0) == -3 and lib.kmpc_last_error(poly.h)
    assert lib.kmpc_set_rbf_order(poly.h, 9) == -3
    assert lib.kmpc_set_rbf_order(poly.h, 8) == 0 and lib.kmpc_set_rbf_order(poly.h, 1) == 0

    def create(**change):
        cfg = _ffi.KmpcConfig()
        ctypes.memmove(ctypes.byref(cfg), ctypes.byref(gauss.cfg), ctypes.sizeof(cfg))
        for name, v in change.items():
            setattr(cfg, name, v)
        h = ctypes.c_void_p()
        rc = lib.kmpc_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc == 0:
            lib.kmpc_destroy(h)
        return rc, (lib.kmpc_last_error(None) or b"").decode()

    assert create()[0] == 0
    rc, text = create(lift_kind=7)
    assert rc != 0 and "lift_kind" in text, (rc, text)
    rc, text = create(lift_kind=_ffi.KMPC_LIFT_RBF_GAUSS, rbf_eps=float("nan"))
    assert rc != 0 and "rbf_eps" in text, (rc, text)
    with pytest.raises(ValueError, match="RBF type not recognize"):
        kapi.rbf(np.zeros((2, 1)), cx, type="bogus")
