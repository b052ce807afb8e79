"""The state dimensions n = 1, 3 and 4 that kmpc_create accepts (every other GPU file builds its controllers with n = 2),
with the row ranges out_row0 / out_rows of y = C x that n > 2 makes possible: q = 3, q = 4, and q < n from any row.
Runs on the MI355X box:  python -m pytest tests/test_gpu_state_dims.py -m gpu

Every comparison is against the NumPy oracle (oracle/koopman_oracle.py, n-general) with the tolerances of
tests/test_gpu_parity.py (fp64):
  lift          1e-12 relative
  RLS           1e-10 relative for one step vs rls_update_gain; 1e-9 relative to max(1, |K|) for a carried sequence
                (the bound of test_rls_random_batches)
  H, f          1e-10 relative
  QP            1e-8 absolute on U vs qp_exact
  closed loop   1e-6 on u_k vs the oracle controller on the same states
  shared model  1e-6 on u_k, 1e-7 on the model (test_shared_model_closed_loop_vs_oracle)
fp32: lift 2e-5.

There is no plant with n != 2 on the device (the plant entry points refuse, last group): closed loops advance the linear
plant x+ = A_d x + b_d u on the host.

GRID lists (n, L, N, threads, out_rows, out_row0, output) so that every arm of launch_step (csrc/step_kernel.hip) is entered
with n != 2; the RLS, condense / QP and closed-loop groups all run over it.
"""
import ctypes

import numpy as np
import pytest

from oracle import koopman_oracle as ko

pytestmark = pytest.mark.gpu


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


# ------------------------------------------------------------------ the case grid
def _grid():
    g = []
    # static q = 2 instantiations entered with n = 3, 4: rows 0..1 and rows n-2..n-1 of C x
    for L, N in ((20, 20), (8, 10), (8, 30), (20, 30)):
        for n in (3, 4):
            for row0 in (0, n - 2):
                g.append((n, L, N, 64, 2, row0, "Cx"))
    # static q = 1 (and q = 2 at (32, 40)): the last row of C x; n = 1 runs as q = 1; n = 4, L = 32 at 64 threads is the
    # 128-of-128 prefetch of C;  (10, 20) with q = 2 has no instantiation (generic kernel)
    for L, N in ((10, 20), (32, 40)):
        g.append((1, L, N, 64, 0, 0, "Cx"))
        g.append((3, L, N, 64, 1, 2, "Cx"))
        g.append((4, L, N, 64, 1, 3, "Cx"))
        g.append((4, L, N, 64, 2, 2, "Cx"))
        g.append((4, L, N, 64, 2, 0, "Cx"))
    # static four-wave kernel
    g.append((4, 64, 50, 256, 2, 2, "Cx"))
    g.append((4, 64, 50, 256, 2, 0, "Cx"))
    # q = n rows of C x (out_rows = 0): generic kernel; odd L with n = 1, 3 makes n L odd
    for L, N in ((20, 20), (9, 11), (33, 12)):
        for n in (1, 3, 4):
            g.append((n, L, N, 64, 0, 0, "Cx"))
    g.append((4, 4, 6, 64, 0, 0, "Cx"))      # L == n: q == L with KMPC_OUT_CX
    g.append((3, 48, 50, 256, 0, 0, "Cx"))   # generic four-wave arm, q = 3
    g.append((3, 48, 20, 64, 0, 0, "Cx"))    # n L = 144 > 2 * 64 on one wave (create accepts 64 threads at L = 48)
    g.append((3, 8, 30, 64, 0, 0, "lift"))   # y = psi: C unused, x and the lift carry n
    return g


GRID = _grid()


def _gid(c):
    n, L, N, th, rows, row0, out = c
    return "n%d-L%d-N%d-t%d-rows%d-row0_%d-%s" % (n, L, N, th, rows, row0, out)


def _q(c):
    n, L, N, th, rows, row0, out = c
    return L if out == "lift" else (rows if rows else n)


def _tag(c):
    """(n, L, N, q, row0) for the assertion messages"""
    return (c[0], c[1], c[2], _q(c), c[5])


def _seed(c):
    n, L, N, th, rows, row0, out = c
    return 1000 * n + 37 * L + 11 * N + 5 * rows + 3 * row0 + (th == 256) + 2 * (out == "lift")


def _rand_model(rng, L, n, rho=0.95):
    A = rng.randn(L, L)
    A *= rho / np.abs(np.linalg.eigvals(A)).max()
    return A, rng.randn(L, 1) * 0.1, rng.randn(n, L) * 0.5


def _rows(c, Cm):
    """the output map of the case: rows out_row0 .. out_row0 + q - 1 of C (None: y = psi)"""
    if c[6] == "lift":
        return None
    return Cm[c[5]:c[5] + _q(c)]


def _host_plant(n, seed):
    """x+ = A_d x + b_d u with A_d = 0.95 orth(n), b_d = 0.3 randn(n)"""
    rng = np.random.RandomState(seed)
    Qo, _ = np.linalg.qr(rng.randn(n, n))
    return 0.95 * Qo, 0.3 * rng.randn(n)


def _lift_of(c, seed, hidden=100, layers=3):
    """(constructor arguments, oracle lift) of a case: the MLP encoder, thin-plate RBFs where L == n"""
    n, L = c[0], c[1]
    if L == n:
        cx = 4 * np.random.RandomState(seed).rand(L, n) - 2
        return dict(lift="rbf", centres=cx), (lambda x: ko.rbf_lift(x, cx))
    from koopmpc.synth import random_mlp_weights

    w = random_mlp_weights(n, hidden, layers, L, seed=seed)
    return dict(weights=w, hidden=hidden, layers=layers), (lambda x: ko.mlp_lift(w, x))


def _edmd(lift_fn, Ad, bd, n, seed, M=2000):
    """the one-off fit of duffing.py:152-177 on samples of the host plant: K = PHIY pinv([PHIX; U]), C = X pinv(PHIX)"""
    rng = np.random.RandomState(seed)
    X = 4 * rng.rand(n, M) - 2
    U = 4 * rng.rand(1, M) - 2
    Y = Ad @ X + bd[:, None] * U
    PX, PY = lift_fn(X), lift_fn(Y)
    K = PY @ np.linalg.pinv(np.concatenate([PX, U], 0))
    Cm = X @ np.linalg.pinv(PX)
    return K[:, :-1].copy(), K[:, -1:].copy(), Cm


def _make(KM, c, B, lift_kw, **kw):
    n, L, N, th, rows, row0, out = c
    return KM(n=n, L=L, N=N, batch=B, threads=th, out_rows=rows, out_row0=row0, output=out, **lift_kw, **kw)


# ------------------------------------------------------------------ 1. lift
@pytest.mark.parametrize("L,hidden,layers", [(20, 100, 3), (5, 37, 2), (64, 128, 3)])
@pytest.mark.parametrize("n", [1, 3, 4])
def test_mlp_lift_state_dims(torch_mod, KM, n, L, hidden, layers):
    from koopmpc.synth import random_mlp_weights

    w = random_mlp_weights(n, hidden, layers, L, seed=11 + n)
    mpc = KM(n=n, L=L, N=10, batch=2, weights=w, hidden=hidden, layers=layers)
    rng = np.random.RandomState(n)
    for B in (1, 17, 4099):
        X = 4 * rng.rand(n, B) - 2
        psi = mpc.Encoder(X)
        want = ko.mlp_lift(w, X)
        assert psi.shape == (L, B), (n, L, hidden, layers, B)
        err = np.abs(psi - want).max()
        assert err <= 1e-12 * max(1.0, np.abs(want).max()), (n, L, hidden, layers, B, err)


@pytest.mark.parametrize("form,kind", [("python", "rbf"), ("matlab", "rbf_matlab")])
@pytest.mark.parametrize("n,L", [(1, 8), (3, 8), (4, 8), (3, 21), (4, 4), (1, 33)])
def test_rbf_lift_state_dims(torch_mod, KM, n, L, form, kind):
    """both RBF forms with centres (L, n); the last L columns of X ARE the centres (r = 0 exactly)"""
    rng = np.random.RandomState(10 * n + L)
    cx = 4 * rng.rand(L, n) - 2
    mpc = KM(n=n, L=L, N=10, batch=2, lift=kind, centres=cx)
    X = np.concatenate([4 * rng.rand(n, 530) - 2, cx.T], axis=1)
    psi = mpc.Encoder(X)
    want = ko.rbf_lift(X, cx, form=form)
    assert psi.shape == want.shape == (L, 530 + L)
    err = np.abs(psi - want).max()
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), (n, L, form, err)
    if form == "matlab":  # rbf.m:24-29: r2 log(sqrt(r2)) is NaN at r = 0 and NaN -> 0
        assert np.all(np.diag(psi[:, 530:]) == 0.0), (n, L)


@pytest.mark.parametrize("form", ["psi0", "x_psi0"])
@pytest.mark.parametrize("n,hidden,layers,Lenc", [(1, 100, 3, 8), (4, 100, 3, 8), (1, 126, 2, 20), (4, 120, 3, 20)])
def test_lift_offsets_state_dims(torch_mod, KM, n, hidden, layers, Lenc, form):
    """psi(x) - psi(0) and [x; psi(x)] - [0; psi(0)]; the second form carries x through 2n more hidden units: the rows with
    hidden + 2n = 128 exactly (126 + 2, 120 + 8) fill the widest encoder the library has"""
    from koopmpc.synth import random_mlp_weights

    w = random_mlp_weights(n, hidden, layers, Lenc, seed=3 + n)
    L = Lenc + (n if form == "x_psi0" else 0)
    mpc = KM(n=n, L=L, N=10, batch=2, weights=w, hidden=hidden, layers=layers, lift_offset=form)
    rng = np.random.RandomState(7 * n + hidden)
    for B in (1, 300):
        X = 4 * rng.rand(n, B) - 2
        X[:, 0] = 0.0
        psi = mpc.Encoder(X)
        want = ko.mlp_lift_offset(w, X, form)
        scale = max(1.0, np.abs(want).max())
        assert psi.shape == want.shape == (L, B)
        err = np.abs(psi - want).max()
        assert err <= 1e-12 * scale, (n, hidden, layers, form, B, err)
        assert np.abs(psi[:, 0]).max() <= 1e-13 * scale  # psi(0) = 0
        if form == "x_psi0":
            assert np.array_equal(psi[:n], X), (n, hidden)  # relu(x) - relu(-x) is x, bit for bit


@pytest.mark.parametrize("n,hidden", [(1, 127), (4, 121)])
def test_lift_offset_wider_than_the_encoder_is_refused(torch_mod, KM, n, hidden):
    from koopmpc._ffi import KmpcError

    with pytest.raises(KmpcError, match="hidden \\+ 2 n"):  # hidden + 2n = 129
        KM(n=n, L=8 + n, N=10, batch=2, hidden=hidden, layers=3, lift_offset="x_psi0")
    KM(n=n, L=8 + n, N=10, batch=2, hidden=hidden, layers=3, lift_offset="psi0")  # (no extra units: accepted)


def test_mlp_lift_fp32_three_states(torch_mod, KM):
    from koopmpc.synth import random_mlp_weights

    w = random_mlp_weights(3, 100, 3, 20, seed=11)
    mpc = KM(n=3, L=20, N=10, batch=2, weights=w, dtype=torch_mod.float32)
    X = 4 * np.random.RandomState(1).rand(3, 777) - 2
    psi = mpc.Encoder(X)
    want = ko.mlp_lift(w, X)
    assert np.abs(psi - want).max() <= 2e-5 * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------ 2. RLS
def _rls_sequence(KM, c, B, steps, lam):
    """`steps` successive Koopman_update calls on random (psi, u, psi+, x+), x+ of n rows; A, B, C of every trajectory against
    rls_update_gain carried along on the host.  The first update is also held to the one-step bound 1e-10."""
    n, L = c[0], c[1]
    rng = np.random.RandomState(_seed(c) + steps)
    lift_kw, _ = _lift_of(c, 1)
    mpc = _make(KM, c, B, lift_kw, lam=lam)
    Ks = [np.zeros((L, L + 1)) for _ in range(B)]
    Ps = [1e4 * np.eye(L + 1) for _ in range(B)]
    Cs = [np.zeros((n, L)) for _ in range(B)]
    Qs = [100.0 * np.eye(L) for _ in range(B)]
    for step in range(steps):
        xl, yl = rng.randn(L, B), rng.randn(L, B)
        u, xn = rng.randn(B), rng.randn(n, B)
        A_, B_, C_ = mpc.Koopman_update(xl, u, yl, xn)
        A_, B_ = A_.cpu().numpy(), B_.cpu().numpy()
        C_ = C_.cpu().numpy() if C_ is not None else None
        assert (C_ is None) == (c[6] == "lift")
        bound = 1e-10 if step == 0 else 1e-9
        for b in range(B):
            Ks[b], Ps[b] = ko.rls_update_gain(Ks[b], Ps[b], np.concatenate([xl[:, b], [u[b]]]), yl[:, b], lam)
            # (the forgetting factor discounts inv_K_G only, Koopman_update.m:270-274: bar_Q runs with lambda = 1)
            Cs[b], Qs[b] = ko.rls_update_gain(Cs[b], Qs[b], xl[:, b], xn[:, b])
            Kb = np.concatenate([A_[b], B_[b]], axis=1)
            err = np.abs(Kb - Ks[b]).max()
            assert err <= bound * max(1.0, np.abs(Ks[b]).max()), (_tag(c), lam, step, b, err)
            if C_ is not None:
                assert C_[b].shape == (n, L)
                err = np.abs(C_[b] - Cs[b]).max()
                assert err <= bound * max(1.0, np.abs(Cs[b]).max()), (_tag(c), lam, step, b, err)


@pytest.mark.parametrize("case", GRID, ids=_gid)
def test_rls_ten_updates(torch_mod, KM, case):
    _rls_sequence(KM, case, 33, 10, 1.0)


@pytest.mark.parametrize("case", [(1, 9, 11, 64, 0, 0, "Cx"), (3, 20, 20, 64, 2, 1, "Cx"), (4, 32, 40, 64, 1, 3, "Cx")], ids=_gid)
def test_rls_with_forgetting(torch_mod, KM, case):
    _rls_sequence(KM, case, 33, 10, 0.95)


# ------------------------------------------------------------------ 3. condense + QP
QP_QW, QP_RW = 1.0, 0.05  # (weights that keep cond(H) small: the 1e-8 on U is then a statement about the solver, see _check_qp)


def _qp_case(KM, c, B=7, **kw):
    n, L = c[0], c[1]
    q = _q(c)
    rng = np.random.RandomState(_seed(c) + 1)
    lift_kw, _ = _lift_of(c, 1)
    mpc = _make(KM, c, B, lift_kw, Qw=QP_QW, Rw=QP_RW, **kw)
    A, Bm, Cm = _rand_model(rng, L, n)
    mpc.set_model(A, Bm, None if c[6] == "lift" else Cm)
    psi = rng.randn(L, B)
    return mpc, rng, A, Bm, Cm, psi, q


def _check_qp(c, U, st, Hs, fs, lb=-2.0, ub=2.0):
    """U (N, B) from the device against the exact minimiser of the oracle's own (H, f); cond(H) is bounded by the choice of
    the weights (asserted: a property of the input), so that 1e-8 is far above what rounding in H, f can move the minimiser"""
    assert (st == 0).all(), (_tag(c), st)
    for b in range(len(Hs)):
        cond = np.linalg.cond(Hs[b])
        assert cond < 1e5, (_tag(c), b, cond)
        Ux, _ = ko.qp_exact(Hs[b], fs[b], lb, ub)
        err = np.abs(U[:, b] - Ux).max()
        assert err <= 1e-8, (_tag(c), b, err)


@pytest.mark.parametrize("case", GRID, ids=_gid)
def test_condense_and_qp(torch_mod, KM, case):
    c = case
    N = c[2]
    mpc, rng, A, Bm, Cm, psi, q = _qp_case(KM, c)
    B = psi.shape[1]
    r = 2.0 * rng.randn(q, N)
    H, f = [t.cpu().numpy() for t in mpc.condense(psi, r)]
    Hs, fs = [], []
    for b in range(B):
        _, _, Ho, fo, _ = ko.condense(A, Bm, _rows(c, Cm), psi[:, b], r, N, QP_QW, QP_RW)
        Hs.append(Ho); fs.append(fo)
        eH, ef = np.abs(H[b] - Ho).max(), np.abs(f[b] - fo).max()
        assert eH <= 1e-10 * np.abs(Ho).max(), (_tag(c), b, eH)
        assert ef <= 1e-10 * max(1.0, np.abs(fo).max()), (_tag(c), b, ef)
        assert np.array_equal(H[b], H[b].T), (_tag(c), b)
    U, st, _ = mpc.qp_solve(H, f)
    _check_qp(c, U.cpu().numpy(), st.cpu().numpy(), Hs, fs)
    U2, st2, _ = mpc.mpc_solve(psi, r)  # the same through the wrapper
    _check_qp(c, U2.cpu().numpy(), st2.cpu().numpy(), Hs, fs)


@pytest.mark.parametrize("case", [(3, 20, 20, 64, 2, 1, "Cx"), (4, 9, 11, 64, 0, 0, "Cx"), (4, 64, 50, 256, 2, 2, "Cx")], ids=_gid)
def test_condense_and_qp_with_a_reference_per_trajectory(torch_mod, KM, case):
    c = case
    N = c[2]
    mpc, rng, A, Bm, Cm, psi, q = _qp_case(KM, c)
    B = psi.shape[1]
    r = 2.0 * rng.randn(B, q, N)
    H, f = [t.cpu().numpy() for t in mpc.condense(psi, r)]
    Hs, fs = [], []
    for b in range(B):
        _, _, Ho, fo, _ = ko.condense(A, Bm, _rows(c, Cm), psi[:, b], r[b], N, QP_QW, QP_RW)
        Hs.append(Ho); fs.append(fo)
        assert np.abs(H[b] - Ho).max() <= 1e-10 * np.abs(Ho).max(), (_tag(c), b)
        assert np.abs(f[b] - fo).max() <= 1e-10 * max(1.0, np.abs(fo).max()), (_tag(c), b)
    U, st, _ = mpc.mpc_solve(psi, r)
    _check_qp(c, U.cpu().numpy(), st.cpu().numpy(), Hs, fs)


@pytest.mark.parametrize("case", [(3, 20, 20, 64, 0, 0, "Cx"), (4, 33, 12, 64, 3, 1, "Cx"), (3, 48, 50, 256, 0, 0, "Cx")], ids=_gid)
def test_condense_with_a_three_by_three_terminal_block(torch_mod, KM, case):
    """Q_bar(end) = P_N (Koopman_update.m:381) with a symmetric positive definite (3, 3) block: q = 3 needs n >= 3"""
    c = case
    N = c[2]
    mpc, rng, A, Bm, Cm, psi, q = _qp_case(KM, c)
    assert q == 3
    B = psi.shape[1]
    G = rng.randn(q, q)
    PN = 3.0 * (G @ G.T / q + 0.1 * np.eye(q))
    mpc.set_terminal_weight(PN)
    r = 2.0 * rng.randn(q, N)
    H, f = [t.cpu().numpy() for t in mpc.condense(psi, r)]
    Hs, fs = [], []
    for b in range(B):
        _, _, Ho, fo, _ = ko.condense(A, Bm, _rows(c, Cm), psi[:, b], r, N, QP_QW, QP_RW, PN=PN)
        _, _, Hplain, _, _ = ko.condense(A, Bm, _rows(c, Cm), psi[:, b], r, N, QP_QW, QP_RW)
        assert np.abs(Ho - Hplain).max() > 1e-3 * np.abs(Ho).max()  # the terminal block matters here
        Hs.append(Ho); fs.append(fo)
        assert np.abs(H[b] - Ho).max() <= 1e-10 * np.abs(Ho).max(), (_tag(c), b)
        assert np.abs(f[b] - fo).max() <= 1e-10 * max(1.0, np.abs(fo).max()), (_tag(c), b)
    U, st, _ = mpc.qp_solve(H, f)
    _check_qp(c, U.cpu().numpy(), st.cpu().numpy(), Hs, fs)
    mpc.set_terminal_weight(None)
    H0, _ = [t.cpu().numpy() for t in mpc.condense(psi, r)]
    _, _, Hplain, _, _ = ko.condense(A, Bm, _rows(c, Cm), psi[:, 0], r, N, QP_QW, QP_RW)
    assert np.abs(H0[0] - Hplain).max() <= 1e-10 * np.abs(Hplain).max(), _tag(c)


# ------------------------------------------------------------------ 4. closed loop
CL_B, CL_STEPS = 19, 12
# two weight settings per case: the reference's (duffing.py:580), which saturate most moves of these loops, and a soft
# one whose moves stay inside the box
CL_SETTINGS = [dict(Qw=100.0, Rw=1e-4), dict(Qw=1.0, Rw=0.5)]
# The online update restarts from K_A = 0 (duffing.py:927-930).  With the reference's P0 = 1e4 the model of the first steps of
# these synthetic loops is often unstable (spectral radius up to 2.5), and over N = 30 .. 50 steps cond(H) then reaches 1e16 .. 1e25
# (measured on the oracle alone): no float64 minimiser exists to hold 1e-6 against.  P0 = barQ0 = 1 keeps the estimate regularised;
# the oracle's cond(H) stays below 1e8 on every QP of the grid (asserted per QP, as a property of the input: a relative rounding
# error of 2.2e-16 in H, f moves the minimiser by at most about cond(H) * 2.2e-16 * |U| = 4e-8).
CL_RLS = dict(P0=1.0, barQ0=1.0)
CL_COND = 1e8


def _closed_loop_inputs(c, setting):
    """everything a closed loop of case c needs that does not involve the device"""
    n, N = c[0], c[2]
    q = _q(c)
    s = _seed(c)
    Ad, bd = _host_plant(n, s)
    lift_kw, lift_fn = _lift_of(c, s % 89 + 1)
    A0, B0, C0 = _edmd(lift_fn, Ad, bd, n, s + 1)
    rng = np.random.RandomState(s + 2 + setting)
    X0 = 4 * rng.rand(n, CL_B) - 2
    amp = 1.0 if setting == 0 else 0.3
    if c[6] == "lift":  # track the lift of a target state (vanderpol.py:668-675)
        r = np.stack([np.tile(lift_fn(amp * rng.randn(n, 1)), (1, N)) for _ in range(CL_B)])
    else:
        r = np.stack([np.tile(amp * rng.randn(q, 1), (1, N)) for _ in range(CL_B)])
    return Ad, bd, lift_kw, lift_fn, A0, B0, C0, X0, r


class _RowController(ko.OracleController):
    """OracleController (gain form, exact QP) whose output map is rows out_row0 .. out_row0 + q - 1 of the adapted C; all n rows
    of x still feed the update of C.  The out_row0 / out_rows slice, and nothing else, on top of the oracle's own step."""

    def __init__(self, *a, rows=None, **kw):
        super().__init__(*a, rls="gain", **kw)
        self.rows = rows

    def step(self, x, r):
        psi = self.lift(np.reshape(x, (-1, 1))).reshape(-1)
        if self.prev is not None:
            ppsi, pu = self.prev
            self.gK, self.gP = ko.rls_update_gain(self.gK, self.gP, np.concatenate([ppsi, [pu]]), psi)
            self.gC, self.gQ = ko.rls_update_gain(self.gC, self.gQ, ppsi, np.reshape(x, -1))
            self.A, self.B, self.C = self.gK[:, :-1].copy(), self.gK[:, -1:].copy(), self.gC.copy()
        Co = None if self.output == "lift" else self.C[self.rows[0]:self.rows[0] + self.rows[1]]
        _, _, H, f, _ = ko.condense(self.A, self.B, Co, psi, r, self.N, self.Qw, self.Rw)
        U, _ = ko.qp_exact(H, f, self.lb, self.ub)
        self.condH = np.linalg.cond(H)
        self.prev = (psi, float(U[0]))
        return float(U[0]), U, psi


def _oracle_controllers(c, lift_fn, A0, B0, C0, w):
    n, L, N = c[0], c[1], c[2]
    return [_RowController(lift_fn, L, n, N, -2.0, 2.0, A0, B0, C0, Qw=w["Qw"], Rw=w["Rw"], output=c[6], rows=(c[5], _q(c)), **CL_RLS)
            for _ in range(CL_B)]


@pytest.mark.parametrize("case", GRID, ids=_gid)
def test_closed_loop_vs_oracle(torch_mod, KM, case):
    """12 steps of kmpc_step for 19 trajectories against one oracle controller per trajectory that sees the device's states and
    applied inputs, under both weight settings: |u - u_oracle| <= 1e-6 at every step of every trajectory, status 0 everywhere.
    From the oracle's first moves alone (pooled over the two settings): at least a quarter strictly inside the box, at least a
    tenth on it, and both bounds met."""
    c = case
    inside = at_lb = at_ub = total = 0
    for si, w in enumerate(CL_SETTINGS):
        Ad, bd, lift_kw, lift_fn, A0, B0, C0, X0, r = _closed_loop_inputs(c, si)
        mpc = _make(KM, c, CL_B, lift_kw, **w, **CL_RLS)
        mpc.set_model(A0, B0, None if c[6] == "lift" else C0)
        ctls = _oracle_controllers(c, lift_fn, A0, B0, C0, w)
        X = X0.copy()
        for k in range(CL_STEPS):
            u = mpc.step(X, r).cpu().numpy().copy()
            st = mpc.status.cpu().numpy()
            assert (st == 0).all(), (_tag(c), si, k, st)
            for b in range(CL_B):
                uo, _, _ = ctls[b].step(X[:, b], r[b])
                assert ctls[b].condH < CL_COND, (_tag(c), si, k, b, ctls[b].condH)
                err = abs(u[b] - uo)
                assert err <= 1e-6, (_tag(c), si, k, b, err, u[b], uo)
                inside += int(-2.0 < uo < 2.0); at_lb += int(uo == -2.0); at_ub += int(uo == 2.0); total += 1
                ctls[b].prev = (ctls[b].prev[0], float(u[b]))  # both sides regress on the input that was applied
            X = Ad @ X + bd[:, None] * u[None, :]
    assert total == 2 * CL_STEPS * CL_B
    assert inside >= 0.25 * total, (_tag(c), inside, total)
    assert at_lb + at_ub >= 0.10 * total, (_tag(c), at_lb, at_ub, total)
    assert at_lb > 0 and at_ub > 0, (_tag(c), at_lb, at_ub)


# ------------------------------------------------------------------ 5. shared model
@pytest.mark.parametrize("n", [1, 3, 4])
def test_shared_model_closed_loop_state_dims(torch_mod, KM, n):
    """Gram -> model -> shared condense -> per-trajectory QP at (20, 20) with q = n rows, against SharedEdmd + condense +
    qp_exact: the model to 1e-7, the controls to 1e-6 (test_shared_model_closed_loop_vs_oracle at n = 2)"""
    L, N, B = 20, 20, 37
    c = (n, L, N, 0, 0, 0, "Cx")
    Ad, bd = _host_plant(n, 50 + n)
    lift_kw, lift_fn = _lift_of(c, 7)
    A0, B0, C0 = _edmd(lift_fn, Ad, bd, n, 60 + n)
    mpc = KM(n=n, L=L, N=N, batch=B, Qw=1.0, Rw=0.5, **lift_kw)
    mpc.set_model(A0, B0, C0)
    rng = np.random.RandomState(70 + n)
    r = np.tile(0.5 * rng.randn(n, 1), (1, N))
    sh = ko.SharedEdmd(L, n)
    A, Bm, Cm = A0, B0, C0
    X = 4 * rng.rand(n, B) - 2
    prev = None
    for k in range(6):
        u = mpc.shared_step(X, r).cpu().numpy().copy()
        assert int(mpc.status.max().item()) == 0, (n, k)
        Psi = lift_fn(X)
        if prev is not None:
            sh.add(*ko.SharedEdmd.gram(prev[0], prev[1], Psi, X))
            A, Bm, Cm = sh.model()
            Ag, Bg, Cg = [t.cpu().numpy() for t in mpc.shared_model()]
            assert Cg.shape == (n, L)
            scale = max(np.abs(A).max(), np.abs(Bm).max())
            em = max(np.abs(Ag - A).max() / scale, np.abs(Bg - Bm).max() / scale, np.abs(Cg - Cm).max() / max(1e-3, np.abs(Cm).max()))
            assert em < 1e-7, (n, L, N, n, 0, k, em)
        Useq = mpc.Useq.cpu().numpy()
        _, _, H, _, _ = ko.condense(A, Bm, Cm, Psi[:, 0], r, N, 1.0, 0.5)
        for b in range(B):
            _, _, _, f, _ = ko.condense(A, Bm, Cm, Psi[:, b], r, N, 1.0, 0.5)
            Uo, _ = ko.qp_exact(H, f, -2.0, 2.0)
            err = max(np.abs(Useq[:, b] - Uo).max(), abs(u[b] - Uo[0]))
            assert err < 1e-6, (n, L, N, n, 0, k, b, err)
        prev = (Psi, u)
        X = Ad @ X + bd[:, None] * u[None, :]


@pytest.mark.parametrize("n", [1, 3, 4])
def test_shared_model_delta_u_state_dims(torch_mod, KM, n):
    """the increment form (Tank_System.m:110-113, 182-192) on a shared model at cfg4's sizes (32, 40), output = the last row of
    C x (out_rows = 1, out_row0 = n - 1): SharedEdmd for the model, the delta-u condense and exact QP of
    OracleDeltaUController per trajectory"""
    L, N, B = 32, 40, 37
    c = (n, L, N, 0, 1, n - 1, "Cx")
    Ad, bd = _host_plant(n, 80 + n)
    lift_kw, lift_fn = _lift_of(c, 9, layers=2)
    A0, B0, C0 = _edmd(lift_fn, Ad, bd, n, 90 + n)
    Qw, Rw = 1.0, 0.5
    mpc = KM(n=n, L=L, N=N, batch=B, lb=-0.5, ub=0.5, umin=-8.0, umax=8.0, Qw=Qw, Rw=Rw, delta_u=True, out_row0=n - 1, out_rows=1,
             **lift_kw)
    mpc.set_model(A0, B0, C0)
    rng = np.random.RandomState(100 + n)
    r = np.full((1, N), 0.5 * rng.randn())
    sh = ko.SharedEdmd(L, n)
    A, Bm, Cm = A0, B0, C0
    X = 4 * rng.rand(n, B) - 2
    uabs = np.zeros(B)
    prev = None
    for k in range(6):
        u = mpc.shared_step(X, r).cpu().numpy().copy()
        dU = mpc.Useq.cpu().numpy()
        assert int(mpc.status.max().item()) == 0, (n, k)
        Psi = lift_fn(X)
        if prev is not None:
            sh.add(*ko.SharedEdmd.gram(prev[0], prev[1], Psi, X))
            A, Bm, Cm = sh.model()
            Ag, Bg, Cg = [t.cpu().numpy() for t in mpc.shared_model()]
            scale = max(np.abs(A).max(), np.abs(Bm).max())
            em = max(np.abs(Ag - A).max() / scale, np.abs(Bg - Bm).max() / scale, np.abs(Cg - Cm).max() / max(1e-3, np.abs(Cm).max()))
            assert em < 1e-7, (n, L, N, 1, n - 1, k, em)
        ctl = ko.OracleDeltaUController(lift_fn, L, n, N, A, Bm, Cm, cy0=n - 1, q=1, Qw=Qw, Rw=Rw)
        for b in range(B):
            ctl.u = float(uabs[b])
            At, Bt, Co, xt = ctl.qp(Psi[:, b])
            _, _, H, f, _ = ko.condense(At, Bt, Co, xt, r, N, Qw, Rw)
            lbv = np.full(N, -0.5); ubv = np.full(N, 0.5)
            lbv[0] = max(-0.5, -8.0 - uabs[b]); ubv[0] = min(0.5, 8.0 - uabs[b])
            dUo, _ = ko.qp_exact(H, f, lbv, ubv)
            err = max(np.abs(dU[:, b] - dUo).max(), abs(u[b] - (uabs[b] + dUo[0])))
            assert err < 1e-6, (n, L, N, 1, n - 1, k, b, err)
        uabs = u
        prev = (Psi, u)
        X = Ad @ X + bd[:, None] * u[None, :]


def test_gram_accumulate_and_offline_fit_three_states(torch_mod, KM):
    """kmpc_gram_accumulate (R = p + L + n rows) against the NumPy Gram sums, kmpc_offline_fit against pinv, at n = 3"""
    torch = torch_mod
    n, L, B = 3, 20, 130
    c = (n, L, 10, 0, 0, 0, "Cx")
    lift_kw, lift_fn = _lift_of(c, 2)
    mpc = KM(n=n, L=L, N=10, batch=B, **lift_kw)
    mpc.set_model(np.zeros((L, L)), np.zeros(L), np.zeros((n, L)))
    rng = np.random.RandomState(4)
    r = np.zeros((n, 10))
    p = L + 1
    delta = torch.zeros(p + L + n, p, dtype=torch.float64, device="cuda:0")
    gram = lambda X: mpc._chk(mpc.lib.kmpc_gram_accumulate(mpc.h, ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(delta.data_ptr()),
                                                           mpc._stream()), "kmpc_gram_accumulate")
    X0 = 4 * rng.rand(n, B) - 2
    gram(_t(torch, X0))
    assert float(delta.abs().max()) == 0.0  # no transition yet
    u0 = mpc.shared_solve(delta, r).cpu().numpy().copy()
    X1 = 4 * rng.rand(n, B) - 2
    gram(_t(torch, X1))
    G, YZ, XZ = ko.SharedEdmd.gram(lift_fn(X0), u0, lift_fn(X1), X1)
    want = np.concatenate([G, YZ, XZ], axis=0)
    got = delta.cpu().numpy()
    assert got.shape == want.shape == (p + L + n, p)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # offline fit on samples of the host plant
    Ad, bd = _host_plant(n, 5)
    M = 5000
    X = 4 * rng.rand(n, M) - 2
    U = 4 * rng.rand(M) - 2
    Y = Ad @ X + bd[:, None] * U[None, :]
    A, Bm, Cm = [t.cpu().numpy() for t in mpc.offline_fit(X, Y, U)]
    PX, PY = lift_fn(X), lift_fn(Y)
    Z = np.concatenate([PX, U[None, :]], 0)
    K = PY @ np.linalg.pinv(Z)
    Cn = X @ np.linalg.pinv(PX)
    scale = np.abs(K).max()
    # the Gram form squares the condition number of the regressor matrix: agreement ~ cond^2 * eps (test_offline_fit_on_device_matches_pinv)
    cond = np.linalg.cond(Z)
    tol = max(1e-9, 50 * cond ** 2 * 2.2e-16)
    assert Cm.shape == (n, L)
    assert np.abs(A - K[:, :L]).max() <= tol * scale and np.abs(Bm - K[:, L:]).max() <= tol * scale, cond
    assert np.abs(Cm - Cn).max() <= tol * max(1.0, np.abs(Cn).max()), cond
    A2, _, C2 = [t.cpu().numpy() for t in mpc.get_model()]
    assert np.array_equal(A2[0], A) and np.array_equal(A2[B - 1], A) and np.array_equal(C2[B - 1], Cm)  # handed to every trajectory


# ------------------------------------------------------------------ 6. state
@pytest.mark.parametrize("case", [(1, 9, 11, 64, 0, 0, "Cx"), (3, 9, 11, 64, 0, 0, "Cx"), (3, 20, 20, 64, 2, 1, "Cx"),
                                  (4, 32, 40, 64, 1, 3, "Cx"), (4, 64, 50, 256, 2, 2, "Cx")], ids=_gid)
def test_checkpoint_roundtrip_state_dims(torch_mod, KM, case):
    """state_dict -> fresh handle -> load_state_dict -> the next steps bit for bit ((1, 9) and (3, 9): n L odd)"""
    c = case
    n, N = c[0], c[2]
    B = 16
    Ad, bd = _host_plant(n, 3)
    lift_kw, lift_fn = _lift_of(c, 3)
    A0, B0, C0 = _edmd(lift_fn, Ad, bd, n, 4)
    rng = np.random.RandomState(9)
    r = np.tile(0.5 * rng.randn(_q(c), 1), (1, N))
    m1 = _make(KM, c, B, lift_kw, Qw=1.0, Rw=0.5)
    m1.set_model(A0, B0, C0)
    X = 4 * rng.rand(n, B) - 2
    for k in range(3):
        u = m1.step(X, r).cpu().numpy()
        X = Ad @ X + bd[:, None] * u[None, :]
    sd = m1.state_dict()
    m2 = _make(KM, c, B, lift_kw, Qw=1.0, Rw=0.5)
    m2.load_state_dict(sd)
    for k in range(3):
        u1 = m1.step(X, r).cpu().numpy().copy()
        u2 = m2.step(X, r).cpu().numpy().copy()
        assert np.array_equal(u1, u2), (_tag(c), k)
        assert np.array_equal(m1.Useq.cpu().numpy(), m2.Useq.cpu().numpy()), (_tag(c), k)
        X = Ad @ X + bd[:, None] * u1[None, :]
    for a, b in zip(m1.get_model(), m2.get_model()):
        assert torch_mod.equal(a, b), _tag(c)


def test_checkpoint_of_another_state_dimension_is_refused(torch_mod, KM):
    from koopmpc._ffi import KmpcError

    L, N, B = 20, 20, 4
    cx3, cx4 = np.zeros((L, 3)), np.zeros((L, 4))
    m3 = KM(n=3, L=L, N=N, batch=B, lift="rbf", centres=cx3)
    sd = m3.state_dict()
    with pytest.raises(KmpcError, match="does not match"):
        KM(n=4, L=L, N=N, batch=B, lift="rbf", centres=cx4).load_state_dict(sd)
    KM(n=3, L=L, N=N, batch=B, lift="rbf", centres=cx3).load_state_dict(sd)


def test_state_init_from_three_state_accumulators(torch_mod, KM):
    """kmpc_state_init_from with n x L accumulators: the model is K_A inv_K_G, C = bar_X bar_Q for every trajectory, and the
    next update continues from them as rls_update_gain does"""
    n, L, B = 3, 9, 5
    p = L + 1
    rng = np.random.RandomState(12)
    Z = rng.randn(p, 60)
    P = np.linalg.inv(Z @ Z.T + np.eye(p))
    K_A = rng.randn(L, 60) @ Z.T
    Qb = np.linalg.inv(Z[:L] @ Z[:L].T + np.eye(L))
    bar_X = rng.randn(n, 60) @ Z[:L].T
    mpc = KM(n=n, L=L, N=11, batch=B, lift="rbf", centres=rng.rand(L, n))
    mpc.state_init(K_A=K_A, inv_K_G=P, bar_X=bar_X, bar_Q=Qb)
    K0, C0 = K_A @ P, bar_X @ Qb
    A, Bm, Cm = [t.cpu().numpy() for t in mpc.get_model()]
    for b in range(B):
        assert np.abs(np.concatenate([A[b], Bm[b]], 1) - K0).max() <= 1e-10 * max(1.0, np.abs(K0).max()), b
        assert Cm[b].shape == (n, L) and np.abs(Cm[b] - C0).max() <= 1e-10 * max(1.0, np.abs(C0).max()), b
    xl, yl, u, xn = rng.randn(L, B), rng.randn(L, B), rng.randn(B), rng.randn(n, B)
    A, Bm, Cm = [t.cpu().numpy() for t in mpc.Koopman_update(xl, u, yl, xn)]
    for b in range(B):
        K1, _ = ko.rls_update_gain(K0, P, np.concatenate([xl[:, b], [u[b]]]), yl[:, b])
        C1, _ = ko.rls_update_gain(C0, Qb, xl[:, b], xn[:, b])
        assert np.abs(np.concatenate([A[b], Bm[b]], 1) - K1).max() <= 1e-10 * max(1.0, np.abs(K1).max()), b
        assert np.abs(Cm[b] - C1).max() <= 1e-10 * max(1.0, np.abs(C1).max()), b


# ------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("n", [1, 3, 4])
def test_plant_entry_points_refuse_and_leave_the_handle_alone(torch_mod, KM, n):
    """no plant has n != 2 states: plant_step, rollout, shared_rollout, shared_solve_plant and generate_and_fit say so, no fused
    roll-out exists, and after every refusal the handle steps exactly like a twin that was never asked"""
    torch = torch_mod
    from koopmpc import _ffi
    from koopmpc._ffi import KmpcError

    L, N, B = 8, 10, 6
    c = (n, L, N, 0, 0, 0, "Cx")
    Ad, bd = _host_plant(n, 21)
    lift_kw, lift_fn = _lift_of(c, 5)
    A0, B0, C0 = _edmd(lift_fn, Ad, bd, n, 22)
    rng = np.random.RandomState(23)
    r = np.tile(0.5 * rng.randn(n, 1), (1, N))
    m, twin = [KM(n=n, L=L, N=N, batch=B, Qw=1.0, Rw=0.5, **lift_kw) for _ in range(2)]
    m.set_model(A0, B0, C0); twin.set_model(A0, B0, C0)
    assert not m.rollout_is_fused() and m.lib.kmpc_rollout_is_fused(m.h) == 0
    X = 4 * rng.rand(n, B) - 2
    Xd = _t(torch, X)
    delta = torch.zeros(L + 1 + L + n, L + 1, dtype=torch.float64, device="cuda:0")
    asks = [
        lambda: m.plant_step("duffing", Xd, np.zeros(B)),
        lambda: m.rollout("duffing", Xd, r, 3),
        lambda: m.shared_rollout("tank", Xd, r, 3),
        lambda: m.shared_solve(delta, r, plant="vdp", X=Xd),
        lambda: m.generate_and_fit("duffing", X, np.zeros((4, B))),
    ]
    for i, ask in enumerate(asks):
        with pytest.raises(KmpcError, match="two-state"):
            ask()
        assert np.array_equal(Xd.cpu().numpy(), X), (n, i)  # the states were not touched
        u1 = m.step(X, r).cpu().numpy().copy()
        u2 = twin.step(X, r).cpu().numpy().copy()
        assert int(m.status.max().item()) == 0
        assert np.array_equal(u1, u2), (n, i)
        X = Ad @ X + bd[:, None] * u1[None, :]
        Xd = _t(torch, X)
    buf = ctypes.create_string_buffer(256)
    assert m.lib.kmpc_rollout_plugin_prebuild(n, L, N, 0, _ffi.KMPC_LIFT_MLP, 100, B, _ffi.KMPC_F64, buf, len(buf)) == -3


def test_create_refuses_state_dimensions_and_row_ranges_outside_the_advertised_ones(torch_mod, KM):
    from koopmpc._ffi import KmpcError

    for n in (0, 5):
        with pytest.raises(KmpcError, match="n must be in 1..4"):
            KM(n=n, L=8, N=10, batch=2)
    for n, row0, rows in ((3, 2, 2), (4, 3, 2), (1, 0, 2), (3, 3, 1), (4, 1, 4), (3, -1, 1)):
        with pytest.raises(KmpcError, match="out_row0/out_rows"):
            KM(n=n, L=8, N=10, batch=2, out_row0=row0, out_rows=rows)
    KM(n=4, L=8, N=10, batch=2, out_row0=1, out_rows=3)
