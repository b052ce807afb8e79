"""Parity of the HIP path (through the C ABI) against the CPU oracle and the reference goldens.
Runs on the MI355X box:  python -m pytest tests -m gpu

Tolerances (fp64 path; the reference computes in fp64, duffing.py:48):
  lift          1e-12 relative   (same arithmetic, different summation order)
  RLS one step  1e-10 relative   vs the oracle's gain form;  vs the reference's K_A*inv_K_G form
                                 1e-9 * inv_K_G0 relative -- that form's own re-association floor (see
                                 test_oracle_golden.test_gain_form_equals_reference_form_...)
  H, f          1e-10 relative
  QP            1e-8 absolute on U (|U| <= 6) vs the exact minimiser
  closed loop   1e-6 on u_k vs the oracle controller on the same states (north-star tolerance)
fp32 path: stated per test (lift 2e-5; the QP/RLS chain cannot meet 1e-6 in fp32).
State dimensions n = 1, 3, 4 and the row ranges out_row0 / out_rows of C x (q = 3, 4, q < n): tests/test_gpu_state_dims.py, same bounds.
"""
import os

import numpy as np
import pytest

from oracle import koopman_oracle as ko

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    return np.load(os.path.join(G, name))


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


# ------------------------------------------------------------------ lift
@pytest.mark.parametrize("wfile,gfile,L,layers", [
    ("weights_duffing.npz", "duffing_loop.npz", 8, 3),
    ("weights_vdp.npz", "vanderpol_loop.npz", 8, 3),
    ("weights_tank.npz", None, 10, 2),
])
def test_mlp_lift_real_weights(torch_mod, KM, wfile, gfile, L, layers):
    w = ko.load_mlp_weights(_load(wfile))
    mpc = KM(n=2, L=L, N=10, batch=4, weights=w, layers=layers)
    rng = np.random.RandomState(5)
    for B in (1, 15, 16, 17, 64, 1000):
        X = 4 * rng.rand(2, B) - 2
        psi = mpc.Encoder(X)
        want = ko.mlp_lift(w, X)
        assert psi.shape == (L, B)
        assert np.abs(psi - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    if gfile:
        g = _load(gfile)
        psi = mpc.Encoder(g["lift_X"].T)
        assert np.abs(psi.T - g["lift_Psi"]).max() < 1e-12  # the reference's own outputs
    # reference shapes: (n,) -> (L,)
    assert mpc.Encoder(np.array([0.0, 0.0])).shape == (L,)


@pytest.mark.parametrize("L,hidden,layers", [(20, 100, 3), (32, 100, 2), (64, 100, 3), (20, 128, 3), (5, 37, 2)])
def test_mlp_lift_scaled_dims(torch_mod, KM, L, hidden, layers):
    from koopmpc.synth import random_mlp_weights

    w = random_mlp_weights(2, hidden, layers, L, seed=11)
    mpc = KM(n=2, L=L, N=10, batch=2, weights=w, hidden=hidden, layers=layers)
    X = 4 * np.random.RandomState(1).rand(2, 4099) - 2
    psi = mpc.Encoder(X)
    want = ko.mlp_lift(w, X)
    assert np.abs(psi - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_mlp_lift_fp32(torch_mod, KM):
    torch = torch_mod
    from koopmpc.synth import random_mlp_weights

    w = random_mlp_weights(2, 100, 3, 20, seed=11)
    mpc = KM(n=2, L=20, N=10, batch=2, weights=w, dtype=torch.float32)
    X = 4 * np.random.RandomState(1).rand(2, 777) - 2
    psi = mpc.Encoder(X)
    want = ko.mlp_lift(w, X)
    assert np.abs(psi - want).max() <= 2e-5 * max(1.0, np.abs(want).max())


def test_rbf_lift(torch_mod, KM):
    g = _load("vanderpol_rbf_loop.npz")
    mpc = KM(n=2, L=8, N=10, batch=2, lift="rbf", centres=g["cx"])
    psi = mpc.Encoder(g["lift_X"].T)
    assert np.abs(psi.T - g["lift_Psi"]).max() <= 1e-12 * np.abs(g["lift_Psi"]).max()
    assert mpc.rbf(np.array([0.3, -0.2])).shape == (8, 1)  # vanderpol_RBF.py:23 returns a column
    m2 = KM(n=2, L=8, N=10, batch=2, lift="rbf_matlab", centres=g["cx"])
    X = np.concatenate([g["lift_X"].T, g["cx"][:2].T], axis=1)  # includes r = 0 exactly
    assert np.abs(m2.Encoder(X) - ko.rbf_lift(X, g["cx"], form="matlab")).max() < 1e-12


# ------------------------------------------------------------------ RLS
@pytest.mark.parametrize("gfile,P0,Q0,boundK,boundC", [("duffing_loop.npz", 1e4, 100.0, 1e-7, 1.1e-10),
                                                        ("vanderpol_loop.npz", 1e5, 1e5, 8.5e-5, 1.5e-5)])
def test_rls_replay_of_reference_loop(torch_mod, KM, gfile, P0, Q0, boundK, boundC):
    g = _load(gfile)
    B = 3
    mpc = KM(n=2, L=8, N=10, batch=B, weights=ko.load_mlp_weights(_load("weights_duffing.npz")), P0=P0, barQ0=Q0)
    K, P = np.zeros((8, 9)), P0 * np.eye(9)
    Cg, Qg = np.zeros((2, 8)), Q0 * np.eye(8)
    floorK, floorC = 0.0, 0.0
    for k in range(len(g["loop_i"])):
        xl, u, yl, xn = g["loop_xlift"][k], g["loop_u_loc"][k].ravel(), g["loop_ylift"][k], g["loop_x_loc"][k]
        A_, B_, C_ = mpc.Koopman_update(np.tile(xl, (1, B)), np.tile(u, B), np.tile(yl, (1, B)), np.tile(xn, (1, B)))
        K, P = ko.rls_update_gain(K, P, np.concatenate([xl.ravel(), u]), yl.ravel())
        Cg, Qg = ko.rls_update_gain(Cg, Qg, xl.ravel(), xn.ravel())
        A_, B_, C_ = A_.cpu().numpy(), B_.cpu().numpy(), C_.cpu().numpy()
        for b in range(B):
            Kb = np.concatenate([A_[b], B_[b]], axis=1)
            # same estimator, same form: only summation order differs (error scales with the init magnitude)
            assert np.abs(Kb - K).max() <= 1e-13 * max(P0, Q0) * np.abs(K).max(), k
            assert np.abs(C_[b] - Cg).max() <= 1e-13 * max(P0, Q0) * max(1e-3, np.abs(Cg).max()), k
            # against the reference's own numbers: inside its re-association floor (grows with P0)
            floorK = max(floorK, np.abs(Kb - g["loop_K_ext"][k]).max() / np.abs(K).max())
            floorC = max(floorC, np.abs(C_[b] - g["loop_C_prev"][k]).max() / max(1e-3, np.abs(Cg).max()))
        assert np.array_equal(A_[0], A_[1]) and np.array_equal(A_[0], A_[2])  # batch-invariant, bitwise
    print("%s: HIP (gain form) vs the reference's logged K_ext %.1e, C %.1e (relative)" % (gfile, floorK, floorC))
    # the reference's K_A*inv_K_G evaluation is itself only reproducible to ~1e-9*inv_K_G0 .. 1e-8*inv_K_G0: the bounds are twice
    # what this (bitwise reproducible) path measures against the logs -- 5.0e-8 / 5.1e-11 (duffing), 4.1e-5 / 7.1e-6 (vanderpol)
    assert floorK <= boundK and floorC <= boundC


@pytest.mark.parametrize("L,B,threads", [(20, 130, 64), (32, 33, 64), (64, 9, 256), (20, 5, 256)])
def test_rls_random_batches(torch_mod, KM, L, B, threads):
    rng = np.random.RandomState(L + B)
    mpc = KM(n=2, L=L, N=10, batch=B, lift="rbf", centres=rng.rand(L, 2), threads=threads)
    Ks = [np.zeros((L, L + 1)) for _ in range(B)]
    Ps = [1e4 * np.eye(L + 1) for _ in range(B)]
    Cs = [np.zeros((2, L)) for _ in range(B)]
    Qs = [100.0 * np.eye(L) for _ in range(B)]
    for step in range(4):
        xl, yl = rng.randn(L, B), rng.randn(L, B)
        u, xn = rng.randn(B), rng.randn(2, B)
        A_, B_, C_ = [t.cpu().numpy() for t in mpc.Koopman_update(xl, u, yl, xn)]
        for b in range(B):
            Ks[b], Ps[b] = ko.rls_update_gain(Ks[b], Ps[b], np.concatenate([xl[:, b], [u[b]]]), yl[:, b])
            Cs[b], Qs[b] = ko.rls_update_gain(Cs[b], Qs[b], xl[:, b], xn[:, b])
            Kb = np.concatenate([A_[b], B_[b]], axis=1)
            assert np.abs(Kb - Ks[b]).max() <= 1e-9 * max(1.0, np.abs(Ks[b]).max()), (step, b)
            assert np.abs(C_[b] - Cs[b]).max() <= 1e-9 * max(1.0, np.abs(Cs[b]).max()), (step, b)


# ------------------------------------------------------------------ condense
def _rand_model(rng, L, q, rho=0.95):
    A = rng.randn(L, L)
    A *= rho / np.abs(np.linalg.eigvals(A)).max()
    return A, rng.randn(L, 1) * 0.1, rng.randn(q, L) * 0.5


@pytest.mark.parametrize("L,N,output,threads", [(8, 10, "Cx", 64), (20, 20, "Cx", 64), (32, 40, "Cx", 64), (64, 50, "Cx", 256), (8, 30, "lift", 64), (20, 20, "lift", 256)])
def test_condense_matches_oracle(torch_mod, KM, L, N, output, threads):
    rng = np.random.RandomState(N)
    B = 5
    q = L if output == "lift" else 2
    mpc = KM(n=2, L=L, N=N, batch=B, lift="rbf", centres=rng.rand(L, 2), output=output, threads=threads)
    A, Bm, Cm = _rand_model(rng, L, 2)
    mpc.set_model(A, Bm, Cm)
    psi = rng.randn(L, B)
    r_shared = rng.randn(q, N)
    H, f = [t.cpu().numpy() for t in mpc.condense(psi, r_shared)]
    for b in range(B):
        _, _, Ho, fo, _ = ko.condense(A, Bm, None if output == "lift" else Cm, psi[:, b], r_shared, N)
        assert np.abs(H[b] - Ho).max() <= 1e-10 * np.abs(Ho).max()
        assert np.abs(f[b] - fo).max() <= 1e-10 * max(1.0, np.abs(fo).max())
        assert np.array_equal(H[b], H[b].T)
    r_per = rng.randn(B, q, N)
    H2, f2 = [t.cpu().numpy() for t in mpc.condense(psi, r_per)]
    for b in range(B):
        _, _, Ho, fo, _ = ko.condense(A, Bm, None if output == "lift" else Cm, psi[:, b], r_per[b], N)
        assert np.abs(f2[b] - fo).max() <= 1e-10 * max(1.0, np.abs(fo).max())


def test_state_init_from_reference_accumulators(torch_mod, KM):
    """kmpc_state_init_from: the reference's own accumulators after 60 loop iterations (K_A, inv_K_G, bar_X, bar_Q of
    the golden Duffing loop) become the state of every trajectory; the model is K_A inv_K_G / bar_X bar_Q, and the
    next update with the loop's next transition gives the model the reference had one iteration later (to the
    K_A inv_K_G re-association floor of this loop, 5e-8).  kmpc_state_init restarts with other scales."""
    g = _load("duffing_loop.npz")
    w = ko.load_mlp_weights(_load("weights_duffing.npz"))
    k = 60
    B = 3
    mpc = KM(n=2, L=8, N=10, batch=B, weights=w)
    mpc.state_init(K_A=g["loop_K_A"][k], inv_K_G=g["loop_inv_K_G"][k], bar_X=g["loop_bar_X"][k], bar_Q=g["loop_bar_Q"][k])
    A, Bm, Cm = [t.cpu().numpy() for t in mpc.get_model()]
    Kext = g["loop_K_A"][k] @ g["loop_inv_K_G"][k]
    for b in range(B):
        # (the product cancels: entries of inv_K_G reach 1e4 -- summation order shows at 1e-12)
        assert np.abs(A[b] - Kext[:, :8]).max() <= 1e-10 * np.abs(Kext).max()
        assert np.abs(Bm[b][:, 0] - Kext[:, 8]).max() <= 1e-10 * np.abs(Kext).max()
        assert np.abs(Cm[b] - g["loop_bar_X"][k] @ g["loop_bar_Q"][k]).max() <= 1e-10
    tile = lambda v: np.tile(np.reshape(v, (-1, 1)), (1, B))
    A, Bm, Cm = [t.cpu().numpy() for t in mpc.Koopman_update(tile(g["loop_xlift"][k + 1]), np.full(B, float(np.ravel(g["loop_u_loc"][k + 1])[0])),
                                                              tile(g["loop_ylift"][k + 1]), tile(g["loop_x_loc"][k + 1]))]
    ref = g["loop_K_ext"][k + 1]
    assert np.abs(A[1] - ref[:, :8]).max() <= 5e-7 * np.abs(ref).max()
    assert np.abs(Bm[1][:, 0] - ref[:, 8]).max() <= 5e-7 * np.abs(ref).max()
    Cref = g["loop_bar_X"][k + 1] @ g["loop_bar_Q"][k + 1]  # C = bar_X bar_Q after the update (duffing.py:953)
    assert np.abs(Cm[1] - Cref).max() <= 5e-7 * max(1.0, np.abs(Cref).max())
    # scales-only restart: the first update afterwards starts from K_A = 0, P = 1e5 I like vanderpol.py:875
    mpc.state_init(P0=1e5, barQ0=1e5)
    z = np.concatenate([g["loop_xlift"][k + 1].ravel(), np.ravel(g["loop_u_loc"][k + 1])[:1]])
    A, Bm, Cm = [t.cpu().numpy() for t in mpc.Koopman_update(tile(g["loop_xlift"][k + 1]), np.full(B, z[-1]), tile(g["loop_ylift"][k + 1]),
                                                              tile(g["loop_x_loc"][k + 1]))]
    K1 = np.outer(g["loop_ylift"][k + 1].ravel(), z) * (1e5 / (1.0 + 1e5 * (z @ z)))  # = y z' (P0 I - P0^2 z z' / (1 + P0 z'z))
    assert np.abs(np.concatenate([A[0], Bm[0]], 1) - K1).max() <= 1e-9 * max(1.0, np.abs(K1).max())


def test_solve_dare_and_dlqr_match_reference_vectors(torch_mod):
    """kmpc_solve_dare (batched Riccati iteration on the device) against the values the reference's own solve_DARE /
    dlqr computed (tests/golden/dare.npz) and against the oracle's iteration counts.  Converged cases: P within 1e-9
    relative; the two cases the reference leaves unconverged after 500 iterations (the offline L = 8 model with
    Q = 10 I and with Q_Lift) are compared after the same 500 iterations, where rounding has been amplified: 1e-6."""
    torch = torch_mod
    from koopmpc import dlqr, solve_DARE

    g = _load("dare.npz")
    for k in range(int(g["n"])):
        A, B, Q, R = g["A%d" % k], g["B%d" % k], g["Q%d" % k], float(g["R%d" % k])
        P, it = solve_DARE(A, B, Q, R, return_iters=True)
        Po, ito = ko.solve_dare(A, B, Q, R)
        tol = 1e-6 if ito == 500 else 1e-9
        assert int(it.item()) == ito, (k, int(it.item()), ito)
        assert np.abs(P.cpu().numpy() - g["P%d" % k]).max() <= tol * np.abs(g["P%d" % k]).max(), k
        K = dlqr(A, B, Q, R).cpu().numpy()
        assert K.shape == (1, A.shape[0])
        assert np.abs(K - g["K%d" % k]).max() <= tol * max(1.0, np.abs(g["K%d" % k]).max()), k
    # a batch of models in one call (one workgroup each), L = 20
    rng = np.random.RandomState(2)
    nb, L = 70, 20
    As = rng.randn(nb, L, L)
    for m in range(nb):
        As[m] *= (0.5 + 0.45 * rng.rand()) / np.abs(np.linalg.eigvals(As[m])).max()
    Bs = rng.randn(nb, L)
    Q = np.diag(1.0 + rng.rand(L))
    P, it = solve_DARE(As, Bs, Q, 0.3, eps=1e-9, return_iters=True)
    K = dlqr(As, Bs, Q, 0.3, eps=1e-9).cpu().numpy()
    P = P.cpu().numpy()
    for m in range(nb):
        Po, ito = ko.solve_dare(As[m], Bs[m], Q, 0.3, eps=1e-9)
        assert abs(int(it[m].item()) - ito) <= 1, m  # (the stop test sits at 1e-9: rounding may move it by one)
        assert np.abs(P[m] - Po).max() <= 1e-8 * np.abs(Po).max(), m
        assert np.abs(K[m] - ko.dlqr(As[m], Bs[m], Q, 0.3, eps=1e-9)).max() <= 1e-8 * max(1.0, np.abs(K[m]).max()), m
    assert solve_DARE(np.zeros((0, L, L)), np.zeros((0, L)), Q, 0.3).shape == (0, L, L)  # empty batch


def test_dare_edge_sizes_and_errors(torch_mod, KM):
    """L = 64 (the largest lift: 98 KB of LDS per model), L = 1, a float32 handle (refused: the reference's Riccati
    iteration is float64), bad arguments."""
    torch = torch_mod
    from koopmpc import _ffi, dlqr, solve_DARE

    rng = np.random.RandomState(64)
    for L in (64, 1):
        A = rng.randn(L, L)
        A *= 0.8 / max(1e-12, np.abs(np.linalg.eigvals(A)).max())
        B = rng.randn(L, 1)
        Q = np.eye(L)
        P, it = solve_DARE(A, B, Q, 0.5, eps=1e-10, return_iters=True)
        Po, ito = ko.solve_dare(A, B, Q, 0.5, eps=1e-10)
        assert abs(int(it.item()) - ito) <= 1
        assert np.abs(P.cpu().numpy() - Po).max() <= 1e-8 * np.abs(Po).max()
        assert np.abs(dlqr(A, B, Q, 0.5, eps=1e-10).cpu().numpy() - ko.dlqr(A, B, Q, 0.5, eps=1e-10)).max() <= 1e-8 * max(1.0, np.abs(Po).max())
    m32 = KM(n=2, L=8, N=10, batch=2, lift="rbf", centres=rng.rand(8, 2), dtype=torch.float32)
    with pytest.raises(RuntimeError):
        m32.terminal_from_dare(np.eye(8), 0.01)
    lib = _ffi.load()
    assert lib.kmpc_solve_dare(None, None, None, 0.1, 10, 0.01, 1, 8, None, None, None, None) == -3
    with pytest.raises(ValueError):
        solve_DARE(np.eye(3), np.ones(3), np.eye(4), 1.0)


def test_state_init_from_with_lifted_output(torch_mod, KM):
    """kmpc_state_init_from for y = psi (no C): bar_X0 may be NULL; K = K_A0 P0 becomes every trajectory's model."""
    rng = np.random.RandomState(12)
    L, B = 8, 4
    mpc = KM(n=2, L=L, N=10, batch=B, lift="rbf", centres=rng.rand(L, 2), output="lift", lb=-6.0, ub=6.0)
    G = rng.randn(L + 1, L + 1)
    P0 = np.linalg.inv(G @ G.T + np.eye(L + 1))
    KA = rng.randn(L, L + 1)
    mpc.state_init(K_A=KA, inv_K_G=P0, bar_X=None, bar_Q=np.eye(L))
    A, Bm, Cm = mpc.get_model()
    K = KA @ P0
    assert Cm is None
    assert np.abs(A.cpu().numpy()[B - 1] - K[:, :L]).max() <= 1e-12 * np.abs(K).max()
    assert np.abs(Bm.cpu().numpy()[0][:, 0] - K[:, L]).max() <= 1e-12 * np.abs(K).max()
    with pytest.raises(RuntimeError):
        mpc.state_init(P0=-1.0)


@pytest.mark.parametrize("L,N,output", [(20, 20, "Cx"), (8, 10, "lift")])
def test_terminal_from_dare(torch_mod, KM, L, N, output):
    """kmpc_terminal_from_dare: P_N = Co solve_DARE(A, B, Q, R) Co' (Koopman_update.m:381 with the LQR stand-in) from
    the shared model, then per trajectory from online-updated models; the condensed QP carries the block(s) and the
    closed loop solves with them."""
    torch = torch_mod
    rng = np.random.RandomState(L)
    B = 6
    q = L if output == "lift" else 2
    mpc = KM(n=2, L=L, N=N, batch=B, lift="rbf", centres=rng.rand(L, 2), output=output)
    A, Bm, Cm = _rand_model(rng, L, 2)
    mpc.set_model(A, Bm, Cm)
    Q = 10.0 * np.eye(L)
    PN, it = mpc.terminal_from_dare(Q, 0.01)
    Po, ito = ko.solve_dare(A, Bm, Q, 0.01)
    Co = np.eye(L) if output == "lift" else Cm
    PNo = ko.terminal_block(Co, Po)
    assert it == ito
    assert np.abs(PN - PNo).max() <= 1e-9 * np.abs(PNo).max()
    psi = rng.randn(L, B)
    r = rng.randn(q, N)
    H, f = [t.cpu().numpy() for t in mpc.condense(psi, r)]
    for b in range(B):
        _, _, Ho, fo, _ = ko.condense(A, Bm, None if output == "lift" else Cm, psi[:, b], r, N, PN=PNo)
        assert np.abs(H[b] - Ho).max() <= 1e-9 * np.abs(Ho).max()
        assert np.abs(f[b] - fo).max() <= 1e-9 * max(1.0, np.abs(fo).max())
    # per trajectory: a few online updates make the models differ, every trajectory gets its own block
    for k in range(3):  # (contractive data: the fitted models are stable, the Riccati iteration converges)
        mpc.Koopman_update(rng.randn(L, B), rng.randn(B), 0.3 * rng.randn(L, B), rng.randn(2, B))
    PNb, itb = mpc.terminal_from_dare(Q, 0.01, per_trajectory=True)
    Ab, Bb, Cb = [t.cpu().numpy() if t is not None else None for t in mpc.get_model()]
    H, f = [t.cpu().numpy() for t in mpc.condense(psi, r)]
    for b in range(B):
        Pb, itob = ko.solve_dare(Ab[b], Bb[b], Q, 0.01)
        Cob = np.eye(L) if output == "lift" else Cb[b]
        PNob = ko.terminal_block(Cob, Pb)
        tol = 1e-6 if itob == 500 else 1e-9
        assert abs(int(itb[b]) - itob) <= (0 if itob == 500 else 1), (b, itb[b], itob)
        assert np.abs(PNb[b] - PNob).max() <= tol * max(1.0, np.abs(PNob).max()), b
        _, _, Ho, fo, _ = ko.condense(Ab[b], Bb[b], None if output == "lift" else Cb[b], psi[:, b], r, N, PN=PNb[b])
        assert np.abs(H[b] - Ho).max() <= 1e-9 * np.abs(Ho).max(), b
        assert np.abs(f[b] - fo).max() <= 1e-9 * max(1.0, np.abs(fo).max()), b
    U, st, _ = mpc.qp_solve(H, f)
    assert int(st.max().item()) <= 1
    mpc.set_terminal_weight(None)  # back to Qw I
    H0, _ = [t.cpu().numpy() for t in mpc.condense(psi, r)]
    _, _, Hplain, _, _ = ko.condense(Ab[0], Bb[0], None if output == "lift" else Cb[0], psi[:, 0], r, N)
    assert np.abs(H0[0] - Hplain).max() <= 1e-10 * np.abs(Hplain).max()


@pytest.mark.parametrize("L,N,output,threads", [(20, 20, "Cx", 64), (8, 30, "lift", 64), (64, 50, "Cx", 256)])
def test_condense_with_terminal_weight(torch_mod, KM, L, N, output, threads):
    """Q_bar(end-n+1:end, end-n+1:end) = C*P*C' (Koopman_update.m:381): a q x q terminal block instead of Qw*I;
    per-trajectory condense, then the same through the shared-model condense + solve."""
    rng = np.random.RandomState(L + N)
    B = 4
    q = L if output == "lift" else 2
    mpc = KM(n=2, L=L, N=N, batch=B, lift="rbf", centres=rng.rand(L, 2), output=output, threads=threads)
    A, Bm, Cm = _rand_model(rng, L, 2)
    mpc.set_model(A, Bm, Cm)
    G = rng.randn(q, q)
    PN = 300.0 * (G @ G.T / q + 0.1 * np.eye(q))
    mpc.set_terminal_weight(PN)
    psi = rng.randn(L, B)
    r = rng.randn(q, N)
    H, f = [t.cpu().numpy() for t in mpc.condense(psi, r)]
    worst = 0.0
    for b in range(B):
        _, _, Ho, fo, _ = ko.condense(A, Bm, None if output == "lift" else Cm, psi[:, b], r, N, PN=PN)
        _, _, Hplain, _, _ = ko.condense(A, Bm, None if output == "lift" else Cm, psi[:, b], r, N)
        assert np.abs(Ho - Hplain).max() > 1e-3 * np.abs(Ho).max()  # the terminal block matters here
        assert np.abs(H[b] - Ho).max() <= 1e-10 * np.abs(Ho).max()
        assert np.abs(f[b] - fo).max() <= 1e-10 * max(1.0, np.abs(fo).max())
    # end to end: the solve on these problems
    U, st, _ = mpc.qp_solve(H, f)
    assert int(st.max().item()) == 0
    for b in range(B):
        _, _, Ho, fo, _ = ko.condense(A, Bm, None if output == "lift" else Cm, psi[:, b], r, N, PN=PN)
        Uo, _ = ko.qp_exact(Ho, fo, -2.0, 2.0)
        worst = max(worst, np.abs(U.cpu().numpy()[:, b] - Uo).max())
    assert worst < 1e-6, worst
    mpc.set_terminal_weight(None)
    H0, _ = [t.cpu().numpy() for t in mpc.condense(psi, r)]
    _, _, Hplain, _, _ = ko.condense(A, Bm, None if output == "lift" else Cm, psi[:, 0], r, N)
    assert np.abs(H0[0] - Hplain).max() <= 1e-10 * np.abs(Hplain).max()


def test_shared_mode_with_terminal_weight(torch_mod, KM):
    from koopmpc.synth import initial_states, offline_edmd, random_mlp_weights

    L, N, B = 20, 20, 16
    w = random_mlp_weights(2, 100, 3, L, seed=7)
    mpc = KM(n=2, L=L, N=N, batch=B, weights=w)
    A0, B0, C0 = offline_edmd(lambda X: mpc.Encoder(X))
    mpc.set_model(A0, B0, C0)
    PN = np.array([[900.0, 120.0], [120.0, 400.0]])
    mpc.set_terminal_weight(PN)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X = initial_states(B, seed=3)
    mpc.shared_step(X, r)  # first step: the offline model, no samples yet
    assert int(mpc.status.max().item()) == 0
    Useq = mpc.Useq.cpu().numpy()
    Psi = ko.mlp_lift(w, X)
    for b in range(B):
        _, _, H, f, _ = ko.condense(A0, B0, C0, Psi[:, b], r, N, PN=PN)
        Uo, _ = ko.qp_exact(H, f, -2.0, 2.0)
        assert np.abs(Useq[:, b] - Uo).max() < 1e-6, b


def test_condense_is_the_reference_cost_on_golden_models(torch_mod, KM):
    g = _load("duffing_loop.npz")
    mpc = KM(n=2, L=8, N=10, batch=1, lift="rbf", centres=np.zeros((8, 2)))
    for row, J in zip(g["cost_in"], g["cost_out"]):
        k = int(row[0])
        mpc.set_model(g["loop_Ap"][k], g["loop_Bp"][k], g["loop_Cp"][k])
        H, f = [t.cpu().numpy()[0] for t in mpc.condense(g["loop_xlift"][k], g["loop_r"][k])]
        _, _, _, _, c = ko.condense(g["loop_Ap"][k], g["loop_Bp"][k], g["loop_Cp"][k], g["loop_xlift"][k], g["loop_r"][k], 10)
        u = row[1:]
        assert abs(u @ H @ u + f @ u + c - J) <= 1e-10 * abs(J)  # J = reference costFunction value


# ------------------------------------------------------------------ QP
def test_qp_on_reference_loop_problems(torch_mod, KM):
    for gfile, lifted, bnd in (("duffing_loop.npz", False, 2.0), ("vanderpol_loop.npz", True, 6.0)):
        g = _load(gfile)
        Hs, fs, cs = [], [], []
        for k in range(len(g["loop_i"])):
            _, _, H, f, c = ko.condense(g["loop_Ap"][k], g["loop_Bp"][k], None if lifted else g["loop_Cp"][k],
                                        g["loop_xlift"][k], g["loop_r"][k], 10)
            Hs.append(H); fs.append(f); cs.append(c)
        mpc = KM(n=2, L=8, N=10, batch=1, lift="rbf", centres=np.zeros((8, 2)), lb=-bnd, ub=bnd)
        U, st, it = mpc.qp_solve(np.stack(Hs), np.stack(fs))
        U, st, it = U.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
        assert (st == 0).all()
        for k in range(len(Hs)):
            Ux, _ = ko.qp_exact(Hs[k], fs[k], -bnd, bnd)
            assert np.abs(U[:, k] - Ux).max() <= 1e-8, k
            J = U[:, k] @ Hs[k] @ U[:, k] + fs[k] @ U[:, k] + cs[k]
            assert J <= g["loop_J"][k] * (1 + 1e-12) + 1e-12  # never worse than the reference's solver
            assert abs(U[0, k] - g["loop_Useq"][k][0]) < 5e-3  # and close to what it returned


@pytest.mark.parametrize("L,N,q,rho,threads", [(20, 20, 2, 1.0, 64), (20, 20, 2, 1.15, 64), (32, 40, 1, 1.0, 64), (64, 50, 2, 1.0, 256), (8, 30, 8, 1.05, 64)])
def test_qp_random_mpc_problems(torch_mod, KM, L, N, q, rho, threads):
    rng = np.random.RandomState(N + L)
    Hs, fs = [], []
    for _ in range(96):
        A, Bm, Cm = _rand_model(rng, L, q, rho)
        _, _, H, f, _ = ko.condense(A, Bm, Cm, rng.randn(L), np.tile(rng.randn(q, 1), (1, N)), N)
        Hs.append(H); fs.append(f)
    mpc = KM(n=2, L=8, N=N, batch=1, lift="rbf", centres=np.zeros((8, 2)), threads=threads)
    U, st, it = mpc.qp_solve(np.stack(Hs), np.stack(fs))
    U, st = U.cpu().numpy(), st.cpu().numpy()
    assert (st == 0).all()
    nsat = 0
    for k in range(len(Hs)):
        kkt = ko.kkt_residual(Hs[k], fs[k], -2, 2, U[:, k])
        assert kkt <= 1e-7 * max(1.0, np.abs(fs[k]).max()), (k, kkt)
        assert np.all(np.abs(U[:, k]) <= 2.0)
        if np.linalg.cond(Hs[k]) < 1e7:
            Ux, _ = ko.qp_exact(Hs[k], fs[k], -2, 2)
            assert np.abs(U[:, k] - Ux).max() <= 1e-7, k
        nsat += int(np.sum(np.abs(U[:, k]) == 2.0))
    assert nsat > 0  # the set contains saturated solutions


def test_qp_instances_where_projected_newton_crawls(torch_mod, KM):
    """QPs recorded from a closed loop (L = 8, N = 30, cond(H) ~ 2e6, 27-28 of 30 inputs saturated) on which
    plain projected Newton needs hundreds of tiny Armijo steps: the active-set safeguard must finish them
    (status 0) at the exact minimiser, on the register solver (static N = 30) and on the LDS solver."""
    d = _load("qp_hard_instances.npz")
    H, f = d["H"], d["f"]
    for threads in (0, 256):
        mpc = KM(n=2, L=8, N=30, batch=1, lift="rbf", centres=np.zeros((8, 2)), threads=threads)
        U, st, it = mpc.qp_solve(H, f)
        U, st, it = U.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
        assert (st == 0).all(), (threads, st, it)
        for k in range(len(H)):
            Uo, _ = ko.qp_exact(H[k], f[k], -2.0, 2.0)
            assert np.abs(U[:, k] - Uo).max() <= 1e-7, (threads, k)
        assert it.max() < 8 * 30 + 40  # finished well before the cap


def test_qp_edge_cases_and_status(torch_mod, KM):
    mpc = KM(n=2, L=8, N=2, batch=1, lift="rbf", centres=np.zeros((8, 2)))
    H = np.array([[2.0, 0.5], [0.5, 1.0]])
    Hs = np.stack([H, H, H, H])
    fs = np.array([[-100.0, -100.0], [100.0, 100.0], [0.0, 0.0], [np.nan, 1.0]])
    U, st, it = mpc.qp_solve(Hs, fs)
    U, st = U.cpu().numpy(), st.cpu().numpy()
    assert np.allclose(U[:, 0], [2, 2]) and np.allclose(U[:, 1], [-2, -2]) and np.allclose(U[:, 2], [0, 0])
    assert list(st[:3]) == [0, 0, 0] and st[3] == 2  # non-finite data is reported, not thrown
    m1 = KM(n=2, L=8, N=1, batch=1, lift="rbf", centres=np.zeros((8, 2)))
    U, st, _ = m1.qp_solve(np.array([[[3.0]]]), np.array([[-6.0]]))
    assert abs(U.cpu().numpy()[0, 0] - 1.0) < 1e-12
    # iteration cap -> status 1
    rng = np.random.RandomState(0)
    A, Bm, Cm = _rand_model(rng, 20, 2, 1.1)
    _, _, Hh, fh, _ = ko.condense(A, Bm, Cm, rng.randn(20), np.ones((2, 20)), 20)
    mcap = KM(n=2, L=8, N=20, batch=1, lift="rbf", centres=np.zeros((8, 2)), qp_max_iter=1)
    _, st, it = mcap.qp_solve(Hh[None], fh[None])
    Ux, its = ko.qp_exact(Hh, fh, -2, 2)
    if np.any(np.abs(Ux) == 2.0):
        assert st.cpu().numpy()[0] == 1 and it.cpu().numpy()[0] == 1


# ------------------------------------------------------------------ the fused step
@pytest.mark.parametrize("gfile,wfile,output,bnd,P0,Q0", [
    ("duffing_loop.npz", "weights_duffing.npz", "Cx", 2.0, 1e4, 100.0),
    ("vanderpol_loop.npz", "weights_vdp.npz", "lift", 6.0, 1e5, 1e5),
])
def test_closed_loop_step_on_reference_states(torch_mod, KM, gfile, wfile, output, bnd, P0, Q0):
    """kmpc_step fed the reference loop's own states (x_k of duffing.py / vanderpol.py).
    (1) vs the oracle controller with the same estimator in gain form: u_k and the whole sequence to 1e-7
        (north-star bar is 1e-6);
    (2) vs the oracle controller that evaluates the RLS exactly as the reference writes it (K_A inv_K_G):
        1e-6 on u_k for the Duffing loop; the Van der Pol loop initialises inv_K_G = 1e5 I, where that
        form's own re-association noise is ~2e-6 in [A B] and reaches ~3e-5 in free inputs
        (test_oracle_golden.test_reference_form_reassociation_floor) -> 1e-4 there;
    (3) vs the u_k the reference logged: within its L-BFGS-B error (5e-3)."""
    g = _load(gfile)
    w = ko.load_mlp_weights(_load(wfile))
    B = 4
    mpc = KM(n=2, L=8, N=10, batch=B, weights=w, output=output, lb=-bnd, ub=bnd, P0=P0, barQ0=Q0)
    mpc.set_model(g["A0"], g["B0"], g["C0"])
    mk = lambda form: ko.OracleController(lambda x: ko.mlp_lift(w, x), 8, 2, 10, -bnd, bnd, g["A0"], g["B0"], g["C0"],
                                          P0=P0, barQ0=Q0, output=output, rls=form)
    cg, cr = mk("gain"), mk("reference")
    x = np.array([-2.0, -2.0])
    w_gain, w_gain_seq, w_ref, w_ref_seq, w_log = 0.0, 0.0, 0.0, 0.0, 0.0
    for k in range(len(g["loop_i"])):
        r = g["loop_r"][k]
        u = mpc.step(np.tile(x[:, None], (1, B)), r).cpu().numpy()
        Useq = mpc.Useq.cpu().numpy()[:, 0]
        assert (mpc.status.cpu().numpy() == 0).all()
        assert np.all(u == u[0])
        ug, Ug, psi = cg.step(x, r)
        ur, Ur, _ = cr.step(x, r)
        w_gain = max(w_gain, abs(u[0] - ug)); w_gain_seq = max(w_gain_seq, np.abs(Useq - Ug).max())
        w_ref = max(w_ref, abs(u[0] - ur)); w_ref_seq = max(w_ref_seq, np.abs(Useq - Ur).max())
        w_log = max(w_log, abs(u[0] - g["logUloc"][0, k]))
        # follow the reference's trajectory exactly: its own u_k and x_{k+1}
        uk = float(g["logUloc"][0, k])
        cg.prev = (psi, uk)
        cr.prev = (psi, uk)
        _set_uprev(mpc, mpc.state_dict(), uk)
        x = g["logXloc"][:, k]
    print("closed loop %s: vs gain-form oracle u0 %.2e seq %.2e | vs reference-form u0 %.2e seq %.2e | vs logged u %.2e"
          % (gfile, w_gain, w_gain_seq, w_ref, w_ref_seq, w_log))
    assert w_gain < 1e-7 and w_gain_seq < 1e-7
    ref_tol = 1e-6 if P0 <= 1e4 else 1e-4
    assert w_ref < ref_tol and w_ref_seq < 20 * ref_tol
    assert w_log < 5e-3


@pytest.mark.parametrize("plant,lift,L,N,output,layers,B,threads,bnd", [
    ("duffing", "mlp", 20, 20, "Cx", 3, 6, 0, 2.0),     # BASELINE cfg1/cfg2 dimensions (static kernel)
    ("vdp", "rbf", 8, 30, "lift", 3, 6, 0, 6.0),        # cfg3: Van der Pol tracking in the lifted space, RBF lift
    ("duffing", "mlp", 32, 40, "Cx", 2, 4, 0, 2.0),     # cfg4-like sizes, two hidden layers, generic 64-thread path
    ("duffing", "mlp", 64, 50, "Cx", 3, 3, 256, 2.0),   # cfg5 dimensions, four waves per trajectory
    ("duffing", "mlp", 20, 20, "Cx", 3, 5, 256, 2.0),   # same problem on the generic 256-thread path
])
def test_closed_loop_vs_oracle_scaled_dims(torch_mod, KM, plant, lift, L, N, output, layers, B, threads, bnd):
    """kmpc_step vs the oracle controller (same estimator, gain form; exact QP) at the BASELINE dimensions with
    synthetic weights: distinct trajectories, closed loop through the oracle's plant, u_k within 1e-6."""
    from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights, vdp_rk4

    rng = np.random.RandomState(L * N)
    if lift == "mlp":
        w = random_mlp_weights(2, 100, layers, L, seed=5)
        mpc = KM(n=2, L=L, N=N, batch=B, weights=w, layers=layers, output=output, lb=-bnd, ub=bnd, threads=threads)
        lift_fn = lambda x: ko.mlp_lift(w, x)
    else:
        cx = 4 * rng.rand(L, 2) - 2
        mpc = KM(n=2, L=L, N=N, batch=B, lift="rbf", centres=cx, output=output, lb=-bnd, ub=bnd, threads=threads)
        lift_fn = lambda x: ko.rbf_lift(x, cx)
    A0, B0, C0 = offline_edmd(lambda X: mpc.Encoder(X), plant=duffing_rk4 if plant == "duffing" else vdp_rk4)
    mpc.set_model(A0, B0, C0)
    if output == "lift":
        r = np.tile(lift_fn(np.array([[1.0], [0.0]])), (1, N))   # vanderpol.py:668-675
    else:
        r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    ctls = [ko.OracleController(lift_fn, L, 2, N, -bnd, bnd, A0, B0, C0, output=output, rls="gain") for _ in range(B)]
    X = initial_states(B, seed=3)
    worst = 0.0
    for k in range(10):
        u = mpc.step(X, r).cpu().numpy()
        Useq = mpc.Useq.cpu().numpy()
        assert (mpc.status.cpu().numpy() == 0).all(), k
        for b in range(B):
            uo, Uo, _ = ctls[b].step(X[:, b], r)
            worst = max(worst, abs(u[b] - uo), np.abs(Useq[:, b] - Uo).max())
            ctls[b].prev = (ctls[b].prev[0], float(u[b]))  # both sides regress on the input that was applied
            X[:, b] = ko.plant_step(plant, X[:, b], float(u[b]))
    print("scaled dims %s L=%d N=%d threads=%d: max |U_gpu - U_oracle| = %.2e" % (plant, L, N, threads, worst))
    assert worst < 1e-6


# ------------------------------------------------------------------ shared-model mode
@pytest.mark.parametrize("L,B", [(20, 1), (20, 130), (32, 257), (64, 70), (8, 4096)])
def test_gram_kernel_mfma(torch_mod, KM, L, B):
    """K7: Gram sums on v_mfma_f64_16x16x4_f64 vs NumPy, ragged batches, two consecutive steps."""
    rng = np.random.RandomState(L + B)
    mpc = KM(n=2, L=L, N=10, batch=B, lift="rbf", centres=4 * rng.rand(L, 2) - 2)
    mpc.set_model(np.zeros((L, L)), np.zeros(L), np.zeros((2, L)))
    r = np.zeros((2, 10))
    X0 = 4 * rng.rand(2, B) - 2
    d0 = mpc.shared_local_gram(X0).cpu().numpy()
    assert np.all(d0 == 0.0)  # no transition yet
    u0 = mpc.shared_solve(mpc._delta, r).cpu().numpy().copy()
    X1 = 4 * rng.rand(2, B) - 2
    d1 = mpc.shared_local_gram(X1).cpu().numpy()
    cx = mpc_centres = None
    psi0 = mpc.Encoder(X0)
    psi1 = mpc.Encoder(X1)
    G, YZ, XZ = ko.SharedEdmd.gram(psi0, u0, psi1, X1)
    want = np.concatenate([G, YZ, XZ], axis=0)
    assert d1.shape == want.shape
    assert np.abs(d1 - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


# (48, 50: the widest interior-kernel tiling; 40, 20 and 40, 12: short horizons on the widest model kernel, N q < 4 ceil(65 / 4) --
#  the K padding of the last Gamma row used to be zeroed into the reference and the model, round-3 advisor finding)
@pytest.mark.parametrize("L,N,B,layers", [(20, 20, 37, 3), (32, 40, 12, 2), (8, 10, 1, 3), (48, 50, 9, 2), (40, 20, 9, 2), (40, 12, 5, 2)])
def test_shared_model_closed_loop_vs_oracle(torch_mod, KM, L, N, B, layers):
    """Shared-model step (Gram -> model -> shared condense -> per-trajectory QP) vs the NumPy oracle
    (SharedEdmd + condense + qp_exact) in closed loop; the model to 1e-7, the controls to 1e-6."""
    from koopmpc.synth import initial_states, offline_edmd, random_mlp_weights

    w = random_mlp_weights(2, 100, layers, L, seed=7)
    mpc = KM(n=2, L=L, N=N, batch=B, weights=w, layers=layers)
    lift = lambda x: ko.mlp_lift(w, x)
    A0, B0, C0 = offline_edmd(lambda X: mpc.Encoder(X))
    mpc.set_model(A0, B0, C0)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    sh = ko.SharedEdmd(L, 2)
    A, Bm, C = A0, B0, C0
    X = initial_states(B, seed=11)
    prev = None
    worst_u, worst_m = 0.0, 0.0
    for k in range(8):
        u = mpc.shared_step(X, r).cpu().numpy()
        assert int(mpc.status.max().item()) == 0
        Psi = lift(X)
        if prev is not None:
            sh.add(*ko.SharedEdmd.gram(prev[0], prev[1], Psi, X))
            A, Bm, C = sh.model()
            Ag, Bg, Cg = [t.cpu().numpy() for t in mpc.shared_model()]
            scale = max(np.abs(A).max(), np.abs(Bm).max())
            worst_m = max(worst_m, np.abs(Ag - A).max() / scale, np.abs(Bg - Bm).max() / scale,
                          np.abs(Cg - C).max() / max(1e-3, np.abs(C).max()))
        _, _, H, _, _ = ko.condense(A, Bm, C, Psi[:, 0], r, N)
        Useq = mpc.Useq.cpu().numpy()
        for b in range(B):
            _, _, _, f, _ = ko.condense(A, Bm, C, Psi[:, b], r, N)
            Uo, _ = ko.qp_exact(H, f, -2.0, 2.0)
            worst_u = max(worst_u, np.abs(Useq[:, b] - Uo).max())
        prev = (Psi, u.copy())
        X = ko.plant_step("duffing", X, u)
    print("shared mode L=%d N=%d B=%d: model %.2e, controls %.2e" % (L, N, B, worst_m, worst_u))
    assert worst_m < 1e-7 and worst_u < 1e-6


@pytest.mark.parametrize("L,N,B", [(10, 20, 24), (32, 40, 12), (10, 15, 16), (10, 12, 8)])  # (q = 1 with N q < 20: see above)
def test_shared_model_delta_u_tank_vs_oracle(torch_mod, KM, L, N, B):
    """BASELINE cfg4 as specified: cascaded tanks, ONE model for the batch from pooled Gram sums (the all-reduced
    block), the MPC in the delta-u form on the augmented model [A B; 0 1], [B; 1], [Cy C 0] (Tank_System.m:110-113,
    265-268, 290) with the first-move box (:182-188), output = second tank level.  Against the oracle: SharedEdmd for
    the model, the delta-u condense / exact QP of OracleDeltaUController per trajectory.  L = 32, N = 40 are cfg4's sizes."""
    torch = torch_mod
    from koopmpc.synth import random_mlp_weights

    rng = np.random.RandomState(L + N)
    w = ko.load_mlp_weights(_load("weights_tank.npz")) if L == 10 else random_mlp_weights(2, 100, 2, L, seed=9)
    lift_fn = lambda x: ko.mlp_lift(w, x)
    mpc = KM(n=2, L=L, N=N, batch=B, weights=w, layers=2, lb=-0.5, ub=0.5, umin=-8.0, umax=8.0, Qw=10.0, Rw=1e-3, P0=1e4,
             barQ0=1e4, delta_u=True, out_row0=1, out_rows=1)
    Ub = 10 * rng.rand(100, 100) - 5
    xc = np.maximum(4 * rng.rand(2, 100) - 2, 0.0)
    Xs, Ys, Us = [], [], []
    for i in range(100):
        xn = ko.tank_step(xc, Ub[i])
        Xs.append(xc); Ys.append(xn); Us.append(Ub[i][None, :]); xc = xn
    Xd, Yd, Ud = np.concatenate(Xs, 1), np.concatenate(Ys, 1), np.concatenate(Us, 1)
    V = np.concatenate([lift_fn(Xd), Ud], 0)
    M = np.concatenate([lift_fn(Yd), Xd], 0) @ V.T @ np.linalg.pinv(V @ V.T)
    A, Bm, C = M[:L, :L], M[:L, L:], M[L:, :L]
    mpc.set_model(A, Bm, C)
    r = np.ones((1, N))
    sh = ko.SharedEdmd(L, 2, P0=1e4, barQ0=1e4)
    X = np.abs(rng.rand(2, B))
    uabs = np.zeros(B)
    prev = None
    worst_u, worst_m, compared = 0.0, 0.0, 0
    for k in range(7):
        u = mpc.shared_step(X, r).cpu().numpy()
        dU = mpc.Useq.cpu().numpy()
        st = mpc.status.cpu().numpy()
        assert (st <= 1).all(), k
        Psi = lift_fn(X)
        if prev is not None:
            sh.add(*ko.SharedEdmd.gram(prev[0], prev[1], Psi, X))
            A, Bm, C = sh.model()
            Ag, Bg, Cg = [t.cpu().numpy() for t in mpc.shared_model()]
            scale = max(np.abs(A).max(), np.abs(Bm).max())
            worst_m = max(worst_m, np.abs(Ag - A).max() / scale, np.abs(Bg - Bm).max() / scale)
        ctl = ko.OracleDeltaUController(lift_fn, L, 2, N, A, Bm, C)
        for b in range(B):
            ctl.u = float(uabs[b])
            At, Bt, Co, xt = ctl.qp(Psi[:, b])
            _, _, H, f, _ = ko.condense(At, Bt, Co, xt, r, N, 10.0, 1e-3)
            lbv = np.full(N, -0.5); ubv = np.full(N, 0.5)
            lbv[0] = max(-0.5, -8.0 - uabs[b]); ubv[0] = min(0.5, 8.0 - uabs[b])
            if np.linalg.cond(H) < 1e10 and st[b] == 0:
                dUo, _ = ko.qp_exact(H, f, lbv, ubv)
                worst_u = max(worst_u, np.abs(dU[:, b] - dUo).max(), abs(u[b] - (uabs[b] + dUo[0])))
                compared += 1
        uabs = u.copy()
        prev = (Psi, u.copy())
        X = ko.tank_step(X, u, switched=(k > 3))
    print("shared delta-u tank L=%d N=%d: model %.2e, increments %.2e (%d QPs compared)" % (L, N, worst_m, worst_u, compared))
    assert compared >= 3 * B
    assert worst_m < 1e-6 and worst_u < 1e-6
    assert np.all(np.abs(u) <= 8.0) and np.all(np.abs(dU) <= 0.5 + 1e-12)


def test_allreduce_gram_with_a_one_rank_communicator(torch_mod, KM):
    """kmpc_allreduce_gram (the native entry point of the path's only collective): a one-rank RCCL communicator made
    with the RCCL that is loaded in this process; the sum over one rank leaves the block unchanged, bad arguments are
    refused.  (Two ranks sum their blocks: covered with gloo on the host and by the two-shard test below.)"""
    import ctypes as C
    import glob

    torch = torch_mod
    from koopmpc import _ffi

    lib = _ffi.load()
    cands = glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so*")) + ["librccl.so", "librccl.so.1"]
    rccl = None
    for c in cands:
        try:
            rccl = C.CDLL(c, mode=C.RTLD_GLOBAL)
            break
        except OSError:
            continue
    if rccl is None:
        pytest.skip("no RCCL library found")

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]

    uid = UniqueId()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    try:
        mpc = KM(n=2, L=8, N=10, batch=4, lift="rbf", centres=np.random.RandomState(0).rand(8, 2))
        ne = int(lib.kmpc_gram_elems(mpc.h))
        d = torch.arange(ne, dtype=torch.float64, device="cuda:0") * 0.5 - 3.0
        want = d.clone()
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.kmpc_allreduce_gram(mpc.h, C.c_void_p(d.data_ptr()), comm, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(d, want)
        assert lib.kmpc_allreduce_gram(mpc.h, None, comm, s) == -3
        assert lib.kmpc_allreduce_gram(mpc.h, C.c_void_p(d.data_ptr()), None, s) == -3
    finally:
        rccl.ncclCommDestroy.argtypes = [C.c_void_p]
        rccl.ncclCommDestroy(comm)


def test_shared_model_two_shards_equal_one_batch(torch_mod, KM):
    """The batch split over two handles (two 'ranks' on one GPU) with the Gram sums added by hand -- the job
    ncclAllReduce does between the two stages -- gives the same shared model and controls as one handle."""
    torch = torch_mod
    from koopmpc.synth import initial_states, offline_edmd, random_mlp_weights

    L, N, B = 20, 20, 96
    w = random_mlp_weights(2, 100, 3, L, seed=7)
    full = KM(n=2, L=L, N=N, batch=B, weights=w)
    h0 = KM(n=2, L=L, N=N, batch=40, weights=w)
    h1 = KM(n=2, L=L, N=N, batch=B - 40, weights=w)
    A0, B0, C0 = offline_edmd(lambda X: full.Encoder(X))
    for m in (full, h0, h1):
        m.set_model(A0, B0, C0)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X = torch.tensor(initial_states(B, seed=5), dtype=torch.float64, device="cuda:0")
    for k in range(6):
        uf = full.shared_step(X, r).clone()
        d = h0.shared_local_gram(X[:, :40].contiguous()) + h1.shared_local_gram(X[:, 40:].contiguous())  # "all-reduce"
        u0 = h0.shared_solve(d, r).clone()
        u1 = h1.shared_solve(d, r).clone()
        us = torch.cat([u0, u1])
        # (the Gram sums of the shards are added in another order than the full batch's: the models agree to 1e-10 relative, below,
        #  and the condensed QP -- Gamma_k = Co A^k up to k = N -- amplifies that to ~1e-9 in u)
        assert float((uf - us).abs().max()) < 5e-9
        Af, Bf, Cf = full.shared_model()
        As, Bs, Cs = h1.shared_model()
        assert float((Af - As).abs().max()) <= 1e-10 * float(Af.abs().max())
        X = full.plant_step("duffing", X.clone(), uf)


def test_offline_fit_on_device_matches_pinv(torch_mod, KM):
    """a10: the reference's one-off EDMD fit (duffing.py:152-177, pinv) done on the device in Gram form."""
    from koopmpc.synth import offline_data, offline_edmd, random_mlp_weights

    for L, wfile in ((8, "weights_duffing.npz"), (20, None)):
        w = ko.load_mlp_weights(_load(wfile)) if wfile else random_mlp_weights(2, 100, 3, L, seed=2)
        mpc = KM(n=2, L=L, N=10, batch=3, weights=w)
        X, Y, U = offline_data()
        A, Bm, C = [t.cpu().numpy() for t in mpc.offline_fit(X, Y, U)]
        PX, PY = ko.mlp_lift(w, X), ko.mlp_lift(w, Y)
        K = PY @ np.linalg.pinv(np.concatenate([PX, U[None, :]], 0))
        Cn = X @ np.linalg.pinv(PX)
        scale = np.abs(K).max()
        # the Gram form squares the condition number of the regressor matrix: agreement ~ cond^2 * eps
        cond = np.linalg.cond(np.concatenate([PX, U[None, :]], 0))
        tol = max(1e-9, 50 * cond ** 2 * 2.2e-16)
        assert np.abs(A - K[:, :L]).max() <= tol * scale and np.abs(Bm - K[:, L:]).max() <= tol * scale, (L, cond)
        assert np.abs(C - Cn).max() <= tol * max(1.0, np.abs(Cn).max())
        A2, B2, C2 = [t.cpu().numpy() for t in mpc.get_model()]
        assert np.array_equal(A2[0], A) and np.array_equal(A2[2], A)  # handed to every trajectory
        if wfile:  # the reference's own offline model (seed 101) from the golden file
            g = _load("duffing_loop.npz")
            assert np.abs(A - g["A0"]).max() <= tol * scale and np.abs(C - g["C0"]).max() <= tol * np.abs(g["C0"]).max()


def test_rls_continues_from_offline_gram(torch_mod, KM):
    """MATLAB twin semantics (Koopman_update.m:258-278): the online RLS starts from K_A = Ylift V',
    inv_K_G = pinv(V V') of the OFFLINE data, so after k online samples the model is the least-squares fit of
    offline + online data together (checked against the oracle's Gram-form fit of the pooled data)."""
    from koopmpc.synth import offline_data, random_mlp_weights

    L, B = 8, 3
    w = ko.load_mlp_weights(_load("weights_duffing.npz"))
    mpc = KM(n=2, L=L, N=10, batch=B, weights=w)
    X, Y, U = offline_data()
    mpc.offline_fit(X, Y, U, init_rls=True)
    PX, PY = ko.mlp_lift(w, X), ko.mlp_lift(w, Y)
    sh = ko.SharedEdmd(L, 2, P0=1e300, barQ0=1e300)  # no ridge: pinv of full-rank Grams
    G, YZ, _ = ko.SharedEdmd.gram(PX, U, PY, Y)
    sh.add(G, YZ, X @ np.concatenate([PX, U[None, :]], 0).T)  # C pairs X with PHIX (duffing.py:177)
    rng = np.random.RandomState(1)
    x = 4 * rng.rand(2, B) - 2
    for k in range(5):
        u = 4 * rng.rand(B) - 2
        xn = ko.plant_step("duffing", x, u)
        psi, psin = ko.mlp_lift(w, x), ko.mlp_lift(w, xn)
        A_, B_, C_ = [t.cpu().numpy() for t in mpc.Koopman_update(psi, u, psin, xn)]
        for b in range(B):  # every trajectory refines its own copy with its own samples
            shb = ko.SharedEdmd(L, 2, P0=1e300, barQ0=1e300)
            shb.G, shb.YZ, shb.XZ = sh.G.copy(), sh.YZ.copy(), sh.XZ.copy()
            if k == 0:
                hist = [[] for _ in range(B)] if b == 0 else hist
            hist[b].append((psi[:, b:b + 1], u[b:b + 1], psin[:, b:b + 1], xn[:, b:b + 1]))
            for (p0, u0, p1, x1) in hist[b]:
                shb.add(*ko.SharedEdmd.gram(p0, u0, p1, x1))
            Ao, Bo, Co = shb.model()
            scale = max(np.abs(Ao).max(), np.abs(Bo).max())
            assert np.abs(A_[b] - Ao).max() <= 1e-6 * scale and np.abs(B_[b] - Bo).max() <= 1e-6 * scale, (k, b)
            assert np.abs(C_[b] - Co).max() <= 1e-6 * max(1.0, np.abs(Co).max()), (k, b)
        x = xn


# ------------------------------------------------------------------ Tank_System.m: delta-u form
@pytest.mark.parametrize("lift,threads,N", [("rbf_matlab", 0, 20), ("mlp", 0, 20), ("rbf_matlab", 256, 20), ("rbf_matlab", 0, 18)])
def test_tank_delta_u_closed_loop(torch_mod, KM, lift, threads, N):
    """Cascaded tanks (Tank_System.m): thin-plate RBF lift with Nrbf = 10 random centres (:61-68) or the
    2-100-100-10 tank encoder (Encoder_Tank.m, Weights/Tank_New.mat), delta-u MPC N = 20, Q = 10, R = 1e-3,
    |du| <= 0.5, u in [-8, 8], output = second tank level, parameter switch after step 100; vs the oracle."""
    torch = torch_mod
    rng = np.random.RandomState(55)
    L, B = 10, 5
    kw = dict(n=2, L=L, N=N, batch=B, lb=-0.5, ub=0.5, umin=-8.0, umax=8.0, Qw=10.0, Rw=1e-3, P0=1e4, barQ0=1e4,
              delta_u=True, out_row0=1, out_rows=1, c_skip_first=True, threads=threads)
    if lift == "mlp":
        w = ko.load_mlp_weights(_load("weights_tank.npz"))
        mpc = KM(weights=w, layers=2, **kw)
        lift_fn = lambda x: ko.mlp_lift(w, x)
    else:
        cx = rng.rand(L, 2)
        mpc = KM(lift="rbf_matlab", centres=cx, **kw)
        lift_fn = lambda x: ko.rbf_lift(x, cx, form="matlab")
    # offline data as Tank_System.m:29-49, fit as :87-100
    Ub = 10 * rng.rand(100, 100) - 5
    xc = np.maximum(4 * rng.rand(2, 100) - 2, 0.0)
    Xs, Ys, Us = [], [], []
    for i in range(100):
        xn = ko.tank_step(xc, Ub[i])
        Xs.append(xc); Ys.append(xn); Us.append(Ub[i][None, :]); xc = xn
    Xd, Yd, Ud = np.concatenate(Xs, 1), np.concatenate(Ys, 1), np.concatenate(Us, 1)
    V = np.concatenate([lift_fn(Xd), Ud], 0)
    M = np.concatenate([lift_fn(Yd), Xd], 0) @ V.T @ np.linalg.pinv(V @ V.T)
    A0, B0, C0 = M[:L, :L], M[:L, L:], M[L:, :L]
    mpc.set_model(A0, B0, C0)
    r = np.ones((1, N))
    ctls = [ko.OracleDeltaUController(lift_fn, L, 2, N, A0, B0, C0) for _ in range(B)]
    X = np.abs(rng.rand(2, B))
    X[:, 0] = 0.0  # Tank_System.m:124 starts at the origin
    worst, ncap = 0.0, 0
    for k in range(14):
        u = mpc.step(X, r).cpu().numpy()
        dU = mpc.Useq.cpu().numpy()
        # the few-sample tank models right after the parameter switch can be numerically singular
        # (cond(H) ~ 1e19 observed): the iteration cap (status 1) is then allowed, the answer is still checked
        st = mpc.status.cpu().numpy()
        assert (st <= 1).all(), k
        ncap += int((st == 1).sum())
        for b in range(B):
            uo, dUo, psi_b = ctls[b].step(X[:, b], r)
            At, Bt, Co, xt = ctls[b].qp(psi_b)
            # (xt already carries the updated u; H does not depend on it)
            Hc = ko.condense(At, Bt, Co, xt, r, N, 10.0, 1e-3)[2]
            if np.linalg.cond(Hc) < 1e12:  # a singular H has no unique minimiser to compare with
                worst = max(worst, abs(u[b] - uo), np.abs(dU[:, b] - dUo).max())
            ctls[b].u = float(u[b]); ctls[b].prev = (ctls[b].prev[0], float(u[b]))
        Xg = mpc.plant_step("tank", torch.tensor(X, dtype=torch.float64, device="cuda:0"), u, switched=(k > 6)).cpu().numpy()
        Xo = ko.tank_step(X, u, switched=(k > 6))
        assert np.abs(Xg - Xo).max() < 1e-13
        X = Xo
    assert np.all(np.abs(u) <= 8.0) and np.all(np.abs(dU) <= 0.5 + 1e-12)
    print("tank delta-u (%s, threads %d, N %d): max |u_gpu - u_oracle| = %.2e" % (lift, threads, N, worst))
    assert worst < 1e-6 and ncap <= 1


@pytest.mark.parametrize("L,N,output,lift,threads,tol", [
    (20, 20, "Cx", "mlp", 0, 1e-9), (20, 20, "Cx", "mlp", 256, 1e-9),
    (8, 30, "Cx", "mlp", 0, 1e-6),  # long horizon, cond(H) up to ~2e6 in this loop: the north-star tolerance
])
def test_warm_start_is_the_same_minimiser_with_less_work(torch_mod, KM, L, N, output, lift, threads, tol):
    """The reference starts every solve at zeros (its pastRes_loc is never updated, duffing.py:634-635, 859);
    kmpc_step starts at the previous minimiser by default, cold_start=1 at clip(0) like the reference.  The QP is
    strictly convex, so both give the same minimiser (to the KKT tolerance) -- only the number of Newton solves
    differs."""
    torch = torch_mod
    from koopmpc.synth import duffing_rk4, initial_states, offline_data, random_mlp_weights, vdp_rk4

    B = 512
    rng = np.random.RandomState(5)
    kw = dict(weights=random_mlp_weights(2, 100, 3, L, seed=4)) if lift == "mlp" else dict(lift="rbf", centres=4 * rng.rand(L, 2) - 2)
    bnd = 2.0 if output == "Cx" else 6.0
    plant = "duffing" if output == "Cx" else "vdp"
    ms = [KM(n=2, L=L, N=N, batch=B, output=output, lb=-bnd, ub=bnd, threads=threads, cold_start=c, **kw) for c in (False, True)]
    Xo, Yo, Uo = offline_data(plant=vdp_rk4 if plant == "vdp" else duffing_rk4)
    for m in ms:
        m.offline_fit(Xo, Yo, Uo, ridge=1e-8)
    if output == "Cx":
        r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    else:  # the lifted reference point, vanderpol.py:756-763
        lift_fn = ms[0].Encoder if lift == "mlp" else ms[0].rbf
        lr = lift_fn(np.array([[1.0], [0.0]]))
        r = np.tile(np.reshape(lr.cpu().numpy() if hasattr(lr, "cpu") else np.asarray(lr), (L, 1)), (1, N))
    X0 = _t(torch, initial_states(B, seed=9))
    Xs = [X0.clone(), X0.clone()]
    worst = 0.0
    for k in range(25):
        us = [m.step(X, r).clone() for m, X in zip(ms, Xs)]
        sts = [int(m.status.max().item()) for m in ms]
        assert sts == [0, 0], (k, sts, [int((m.status != 0).sum()) for m in ms], [int(m.iters.max()) for m in ms])
        worst = max(worst, float((ms[0].Useq - ms[1].Useq).abs().max()))
        # both controllers follow the cold-start trajectory so that the comparison stays solve-by-solve
        Xn = ms[1].plant_step(plant, Xs[1].clone(), us[1])
        Xs = [Xn.clone(), Xn.clone()]
        _copy_uprev(ms[0], ms[1])
    its = [float(m.iters.double().mean()) for m in ms]
    print("warm vs cold start L=%d N=%d: max |dU| %.2e, last-step mean Newton solves warm %.2f cold %.2f" % (L, N, worst, its[0], its[1]))
    assert worst < tol
    assert its[0] <= its[1]


def _copy_uprev(dst, src):
    """u_{k} of `src` into `dst`, so that both see the same transition."""
    dst.set_applied_input(src.U0)


def _set_uprev(mpc, sd, uk):
    """Replace the stored u_{k} of every trajectory (the input that was applied on the followed trajectory)."""
    mpc.set_applied_input(uk)


@pytest.mark.parametrize("lift", ["rbf", "mlp"])
def test_step_matches_separate_ops(torch_mod, KM, lift):
    """kmpc_step equals lift -> rls_update -> condense -> qp_solve called one by one.  RBF lift: kmpc_step is the lift
    kernel + the step kernel, bitwise the same.  MLP lift with a fused instantiation: kmpc_step is ONE launch of the
    roll-out kernel (single step, no plant), whose in-kernel encoder sums the K dimension in another order than the
    stand-alone lift kernel: equal to 1e-9."""
    torch = torch_mod
    from koopmpc.synth import random_mlp_weights

    rng = np.random.RandomState(8)
    L, N, B = 20, 20, 37
    kw = dict(weights=random_mlp_weights(2, 100, 3, L, seed=3)) if lift == "mlp" else dict(lift="rbf", centres=4 * rng.rand(L, 2) - 2)
    A, Bm, Cm = _rand_model(rng, L, 2)
    m1 = KM(n=2, L=L, N=N, batch=B, cold_start=True, **kw)  # kmpc_qp_solve is stateless: it starts at clip(0)
    m2 = KM(n=2, L=L, N=N, batch=B, **kw)
    m1.set_model(A, Bm, Cm); m2.set_model(A, Bm, Cm)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X = _t(torch, 4 * rng.rand(2, B) - 2)
    psi_prev, u_prev = None, None
    same = (lambda a, b: torch.equal(a, b)) if lift == "rbf" else (lambda a, b: float((a - b).abs().max()) < 1e-9)
    for k in range(5):
        u1 = m1.step(X, r).clone()
        psi = m2.Encoder(X)
        if psi_prev is not None:
            m2.Koopman_update(psi_prev, u_prev, psi, X)
        U2, st, it = m2.mpc_solve(psi, r)
        assert same(u1, U2[0]), k
        assert same(m1.Useq, U2), k
        # (status 0, except that a QP of the random model right after the RLS reset may be numerically singular: then it is
        #  flagged on BOTH routes -- a few trajectories of this batch at most: one until round 6, three since the RBF observable
        #  is the shared function kmpc_rbf_psi2, whose sums round differently in the last bit; every flagged one is examined below)
        assert torch.equal(m1.status, st) and int(st.max().item()) <= 1 and int((st != 0).sum().item()) <= 3
        # ... and a flagged solve is not a free pass: either the QP the device condensed is numerically singular / indefinite
        # (smallest eigenvalue of H below 1e-13 of the largest: no solver has a minimiser to converge to), or the returned point
        # is held against the exact minimiser (cost within 1e-9 relative, box respected) -- a convergence regression on a
        # well-posed QP cannot hide behind "both routes run the same code"
        for bb in np.nonzero(st.cpu().numpy())[0]:
            Hh, fh = m2.condense(psi, r)
            Hb, fb = Hh[bb].cpu().numpy(), fh[bb].cpu().numpy()
            ev = np.linalg.eigvalsh(0.5 * (Hb + Hb.T))
            if ev.min() > 1e-13 * ev.max():
                Ue, _ = ko.qp_exact(Hb, fb, -2.0, 2.0)
                Ug = U2[:, bb].cpu().numpy()
                Jf = lambda v: float(v @ Hb @ v + fb @ v)
                assert np.all(np.abs(Ug) <= 2.0 + 1e-12)
                assert Jf(Ug) - Jf(Ue) <= 1e-9 * max(1.0, abs(Jf(Ue))), (k, int(bb), Jf(Ug), Jf(Ue))
        psi_prev, u_prev = psi, U2[0].clone()
        X = m1.plant_step("duffing", X.clone(), u1, switched=(k > 2))


@pytest.mark.parametrize("lift,L,N,output,B,steps", [
    ("mlp", 20, 20, "Cx", 50, 9),     # fused roll-out kernel, ragged last workgroup (50 = 3 x 16 + 2)
    ("mlp", 20, 20, "Cx", 16, 1),     # a single step: the RLS flags must come out like kmpc_step's
    ("mlp", 8, 10, "Cx", 33, 12),     # the reference's own dimensions
    ("mlp", 8, 10, "lift", 33, 12),   # vanderpol.py's dimensions, y = psi (round 4: register-state step for q = L)
    ("rbf", 8, 30, "lift", 40, 8),    # RBF lift inside the roll-out kernel (cfg3 dimensions)
    ("mlp", 32, 40, "Cx", 20, 5),     # cfg4 sizes: 29 KB of LDS per trajectory, four trajectories per workgroup
    ("mlp", 8, 30, "Cx", 24, 6),      # cfg3 sizes with the MLP lift: 19 KB of LDS per trajectory, 8 per CU
    ("mlp", 20, 30, "Cx", 21, 6),     # cfg3 horizon with the 20-dim lift
    ("tank", 10, 20, "Cx", 24, 8),    # Tank_System.m: delta-u form, one output row, two hidden layers, tank plant
    ("mlp64", 20, 20, "Cx", 18, 6),   # 64 hidden units: the run-time-width variant of the in-kernel encoder
    ("mlp128", 8, 10, "Cx", 9, 6),    # 128 hidden units (H_p = 128, eight M tiles)
    ("mlp", 20, 20, "Cx", 4096, 3),   # the bench's batch: 16 trajectories per workgroup (smaller batches use 8)
])
def test_rollout_equals_step_plus_plant_loop(torch_mod, KM, lift, L, N, output, B, steps):
    """kmpc_rollout is the Python loop of step + plant_step, including the plant-parameter switch
    (duffing.py:991-992), the logs and the status / iteration accumulation.  Where a fused instantiation exists
    the roll-out is ONE kernel (16 trajectories per workgroup, lift computed inside); its encoder sums the K
    dimension in a different order than the stand-alone lift kernel, so the comparison is to 1e-9, not bitwise.
    Two roll-out calls in a row continue each other (state flags, psi ping-pong)."""
    torch = torch_mod
    from koopmpc.synth import random_mlp_weights

    rng = np.random.RandomState(4)
    plant = "duffing"
    if lift == "mlp":
        kw = dict(weights=random_mlp_weights(2, 100, 3, L, seed=3))
    elif lift in ("mlp64", "mlp128"):
        hid = int(lift[3:])
        kw = dict(weights=random_mlp_weights(2, hid, 3, L, seed=3), hidden=hid)
    elif lift == "tank":
        plant = "tank"
        kw = dict(weights=ko.load_mlp_weights(_load("weights_tank.npz")), layers=2, lb=-0.5, ub=0.5, umin=-8.0, umax=8.0,
                  Qw=10.0, Rw=1e-3, P0=1e4, barQ0=1e4, delta_u=True, out_row0=1, out_rows=1, c_skip_first=True)
    else:
        kw = dict(lift="rbf", centres=4 * rng.rand(L, 2) - 2)
    A, Bm, Cm = _rand_model(rng, L, 2)
    q = L if output == "lift" else (1 if lift == "tank" else 2)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N)) if q == 2 else (np.ones((1, N)) if q == 1 else np.tile(rng.randn(q, 1), (1, N)))
    m1 = KM(n=2, L=L, N=N, batch=B, output=output, **kw)
    m2 = KM(n=2, L=L, N=N, batch=B, output=output, **kw)
    m1.set_model(A, Bm, Cm); m2.set_model(A, Bm, Cm)
    X0 = np.abs(rng.rand(2, B)) if lift == "tank" else 4 * rng.rand(2, B) - 2
    X1, X2 = _t(torch, X0), _t(torch, X0)
    s1 = steps // 2
    Ul, Xl = m1.rollout(plant, X1, r, s1, step0=98, switch_step=102, log=True) if s1 else (None, None)
    it1 = m1.iters.clone() if s1 else 0
    st1 = m1.status.clone() if s1 else 0
    Ul2, Xl2 = m1.rollout(plant, X1, r, steps - s1, step0=98 + s1, switch_step=102, log=True)
    its1 = it1 + m1.iters
    st1 = torch.maximum(st1, m1.status) if s1 else m1.status.clone()
    Ul = torch.cat([Ul, Ul2]) if s1 else Ul2
    Xl = torch.cat([Xl, Xl2]) if s1 else Xl2
    its = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    st2 = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    for i in range(steps):
        u = m2.step(X2, r).clone()
        its += m2.iters
        st2 = torch.maximum(st2, m2.status)
        assert float((u - Ul[i]).abs().max()) < 1e-9, i
        X2 = m2.plant_step(plant, X2, u, switched=(98 + i >= 102))
        assert float((X2 - Xl[i]).abs().max()) < 1e-9, i
    assert float((X1 - X2).abs().max()) < 1e-9
    assert torch.equal(st1, st2)  # (the random model of the lifted-output case has a few degenerate QPs: status 1 on both sides)
    if lift == "mlp" and B < 4096:
        # status 0 everywhere, except that ONE trajectory of the random model may meet a numerically singular QP right after the
        # RLS reset (cond(H) = 9e13 at (L, N) = (20, 20), step 5, tools/dbg/status_debug.py: the stateless solve of the same H, f
        # reports it too) -- it is flagged (status 1) on both sides, never silently wrong
        assert int(st1.max().item()) <= 1 and int((st1 != 0).sum().item()) <= 1
    assert int((its1 - its)[st2 == 0].abs().max()) <= 2  # refinement solves may differ by rounding
    # the handles are in the same state: one more step agrees
    u1, u2 = m1.step(X1, r).clone(), m2.step(X2, r).clone()
    assert float((u1 - u2).abs().max()) < 1e-9
    A1, B1, C1 = m1.get_model()
    A2, B2, C2 = m2.get_model()
    assert float((A1 - A2).abs().max()) <= 1e-9 * max(1.0, float(A2.abs().max()))


@pytest.mark.parametrize("L,N,B,steps", [(20, 20, 19, 14), (8, 10, 33, 20), (20, 30, 9, 8), (32, 40, 6, 6)])
def test_fused_rollout_vs_oracle(torch_mod, KM, L, N, B, steps):
    """The dominant kernel of the bench against the oracle directly: kmpc_rollout (one fused launch: encoder on
    MFMA inside, RLS, condense, QP, RK4 plant, parameter switch) vs per-trajectory oracle controllers (gain-form RLS,
    exact QP) driving the oracle's plant.  Inputs and states of every step within 1e-6 (north-star tolerance);
    observed ~1e-9."""
    torch = torch_mod
    from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

    w = random_mlp_weights(2, 100, 3, L, seed=5)
    mpc = KM(n=2, L=L, N=N, batch=B, weights=w)
    assert mpc.rollout_is_fused()
    lift_fn = lambda x: ko.mlp_lift(w, x)
    A0, B0, C0 = offline_edmd(lambda X: mpc.Encoder(X), plant=duffing_rk4)
    mpc.set_model(A0, B0, C0)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = initial_states(B, seed=3)
    Xd = _t(torch, X0)
    step0, sw = 97, 102
    Ul, Xl = mpc.rollout("duffing", Xd, r, steps, step0=step0, switch_step=sw, log=True)
    assert int(mpc.status.max().item()) == 0
    Ul, Xl = Ul.cpu().numpy(), Xl.cpu().numpy()
    worst_u, worst_x = 0.0, 0.0
    for b in range(B):
        ctl = ko.OracleController(lift_fn, L, 2, N, -2.0, 2.0, A0, B0, C0, rls="gain")
        x = X0[:, b].copy()
        for k in range(steps):
            uo, _, _ = ctl.step(x, r)
            worst_u = max(worst_u, abs(Ul[k, b] - uo))
            # both sides regress on the input that was applied and continue from the GPU's state
            ctl.prev = (ctl.prev[0], float(Ul[k, b]))
            xo = ko.plant_step("duffing", x, float(Ul[k, b]), switched=(step0 + k >= sw))
            worst_x = max(worst_x, float(np.abs(Xl[k, :, b] - xo).max()))
            x = Xl[k, :, b].copy()
    print("fused roll-out vs oracle L=%d N=%d: max |u - u_oracle| = %.2e, max |x - x_oracle| = %.2e" % (L, N, worst_u, worst_x))
    assert worst_u < 1e-6 and worst_x < 1e-9


@pytest.mark.parametrize("wg", [4, 8, 16])
def test_fused_rollout_workgroup_sizes(torch_mod, KM, wg):
    """kmpc_set_rollout_workgroup: 4 trajectories per workgroup (encoder on v_mfma_f64_4x4x4_4b_f64, four workgroups
    per CU), 8 or 16 (v_mfma_f64_16x16x4_f64).  Every choice is the same closed loop as the per-step path, and the
    lifted state the kernel leaves behind is the stand-alone encoder's."""
    torch = torch_mod
    from koopmpc import _ffi
    from koopmpc.synth import random_mlp_weights

    lib = _ffi.load()
    assert lib.kmpc_set_rollout_workgroup(5) == -1
    rng = np.random.RandomState(40 + wg)
    L, N, B, steps = 20, 20, 37, 7
    w = random_mlp_weights(2, 100, 3, L, seed=6)
    A, Bm, Cm = _rand_model(rng, L, 2)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = 4 * rng.rand(2, B) - 2
    m1, m2 = KM(n=2, L=L, N=N, batch=B, weights=w), KM(n=2, L=L, N=N, batch=B, weights=w)
    m1.set_model(A, Bm, Cm); m2.set_model(A, Bm, Cm)
    X1, X2 = _t(torch, X0), _t(torch, X0)
    try:
        assert lib.kmpc_set_rollout_workgroup(wg) == 0
        assert m1.rollout_is_fused()
        Ul, Xl = m1.rollout("duffing", X1, r, steps, step0=99, switch_step=102, log=True)
        torch.cuda.synchronize()
    finally:
        lib.kmpc_set_rollout_workgroup(0)
    assert int(m1.status.max().item()) == 0
    for i in range(steps):
        u = m2.step(X2, r).clone()
        assert float((u - Ul[i]).abs().max()) < 1e-9, (wg, i)
        X2 = m2.plant_step("duffing", X2, u, switched=(99 + i >= 102))
        assert float((X2 - Xl[i]).abs().max()) < 1e-9, (wg, i)
    A1, B1, C1 = m1.get_model()
    A2, B2, C2 = m2.get_model()
    assert float((A1 - A2).abs().max()) <= 1e-9 * max(1.0, float(A2.abs().max()))
    assert float((C1 - C2).abs().max()) <= 1e-9 * max(1.0, float(C2.abs().max()))


@pytest.mark.parametrize("B,per_traj,cold,term", [(1, False, False, False), (5, True, False, False), (21, False, True, False),
                                                  (12, True, False, True)])
def test_fused_rollout_options(torch_mod, KM, B, per_traj, cold, term):
    """Options of the step inside the fused roll-out kernel: batches smaller than a workgroup (idle waves still take
    part in the lift and its barriers), a reference per trajectory, cold starts, the terminal weight -- each against
    the per-step path, then a checkpoint taken between two roll-outs continues identically on a second handle."""
    torch = torch_mod
    from koopmpc.synth import random_mlp_weights

    rng = np.random.RandomState(B)
    L, N = 20, 20
    w = random_mlp_weights(2, 100, 3, L, seed=3)
    A, Bm, Cm = _rand_model(rng, L, 2)
    ms = [KM(n=2, L=L, N=N, batch=B, weights=w, cold_start=cold) for _ in range(3)]
    for m in ms:
        m.set_model(A, Bm, Cm)
        if term:
            m.set_terminal_weight(np.array([[700.0, 90.0], [90.0, 300.0]]))
    assert ms[0].rollout_is_fused()
    r = rng.randn(B, 2, N) if per_traj else np.tile(np.array([[1.0], [0.0]]), (1, N))
    X0 = 4 * rng.rand(2, B) - 2
    X = [_t(torch, X0) for _ in range(3)]
    ms[0].rollout("duffing", X[0], r, 4, step0=0)
    for k in range(4):
        X[1] = ms[1].plant_step("duffing", X[1], ms[1].step(X[1], r).clone())
    assert float((X[0] - X[1]).abs().max()) < 1e-9
    ms[2].load_state_dict(ms[0].state_dict())   # checkpoint after the first roll-out ...
    X[2] = X[0].clone()
    ms[0].rollout("duffing", X[0], r, 3, step0=4)
    ms[2].rollout("duffing", X[2], r, 3, step0=4)  # ... continues bit for bit on another handle
    assert torch.equal(X[0], X[2])
    for k in range(3):
        X[1] = ms[1].plant_step("duffing", X[1], ms[1].step(X[1], r).clone())
    assert float((X[0] - X[1]).abs().max()) < 1e-9


def test_checkpoint_roundtrip(torch_mod, KM):
    torch = torch_mod
    from koopmpc.synth import random_mlp_weights

    rng = np.random.RandomState(9)
    L, N, B = 20, 20, 16
    w = random_mlp_weights(2, 100, 3, L, seed=3)
    A, Bm, Cm = _rand_model(rng, L, 2)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    m1 = KM(n=2, L=L, N=N, batch=B, weights=w)
    m1.set_model(A, Bm, Cm)
    X = _t(torch, 4 * rng.rand(2, B) - 2)
    for k in range(3):
        u = m1.step(X, r)
        X = m1.plant_step("duffing", X.clone(), u)
    sd = m1.state_dict()
    m2 = KM(n=2, L=L, N=N, batch=B, weights=w)
    m2.load_state_dict(sd)
    for k in range(3):
        u1 = m1.step(X, r).clone()
        u2 = m2.step(X, r).clone()
        assert torch.equal(u1, u2)
        X = m1.plant_step("duffing", X.clone(), u1)
    with pytest.raises(Exception):
        KM(n=2, L=L, N=N, batch=B + 1, weights=w).load_state_dict(sd)


def test_plant_kernels(torch_mod, KM):
    torch = torch_mod
    mpc = KM(n=2, L=8, N=10, batch=1, lift="rbf", centres=np.zeros((8, 2)))
    rng = np.random.RandomState(2)
    X = 4 * rng.rand(2, 1000) - 2
    U = 4 * rng.rand(1000) - 2
    for kind in ("duffing", "vdp"):
        for sw in (False, True):
            got = mpc.plant_step(kind, _t(torch, X), U, 0.05, sw).cpu().numpy()
            want = ko.plant_step(kind, X, U, 0.05, sw)
            assert np.abs(got - want).max() < 1e-13


def test_edge_sizes(torch_mod, KM):
    """Empty batches are no-ops, the maximum dimensions (L = 64, N = 64) run, a batch of one works."""
    torch = torch_mod
    from koopmpc.synth import random_mlp_weights

    w = random_mlp_weights(2, 100, 3, 8, seed=1)
    mpc = KM(n=2, L=8, N=10, batch=1, weights=w)
    e = torch.empty(2, 0, dtype=torch.float64, device="cuda:0")
    assert tuple(mpc.Encoder(e).shape) == (8, 0)           # B = 0 lift: nothing launched, nothing written
    U, st, it = mpc.qp_solve(torch.empty(0, 10, 10, dtype=torch.float64, device="cuda:0"),
                             torch.empty(0, 10, dtype=torch.float64, device="cuda:0"))
    assert tuple(U.shape) == (10, 0)
    u = mpc.step(np.array([[0.5], [-0.5]]), np.tile(np.array([[1.0], [0.0]]), (1, 10)))  # batch of one, zero model
    assert tuple(u.shape) == (1,) and float(u.abs().max()) == 0.0 and int(mpc.status[0]) == 0
    w64 = random_mlp_weights(2, 128, 3, 64, seed=2)
    big = KM(n=2, L=64, N=64, batch=2, weights=w64, hidden=128)
    rng = np.random.RandomState(0)
    A, Bm, Cm = _rand_model(rng, 64, 2)
    big.set_model(A, Bm, Cm)
    r = np.tile(np.array([[1.0], [0.0]]), (1, 64))
    X = 4 * rng.rand(2, 2) - 2
    for k in range(3):
        ub = big.step(X, r).cpu().numpy()
        assert (big.status.cpu().numpy() == 0).all() and np.all(np.abs(big.Useq.cpu().numpy()) <= 2.0)
        psi = ko.mlp_lift(w64, X)
        Ak, Bk, Ck = [t.cpu().numpy() for t in big.get_model()]
        for b in range(2):
            _, _, H, f, _ = ko.condense(Ak[b], Bk[b], Ck[b], psi[:, b], r, 64)
            kk = ko.kkt_residual(H, f, -2, 2, big.Useq.cpu().numpy()[:, b])
            assert kk <= 1e-6 * max(1.0, np.abs(f).max())
        X = ko.plant_step("duffing", X, ub)


def test_errors_are_loud(torch_mod, KM):
    from koopmpc._ffi import KmpcError

    with pytest.raises(KmpcError):
        KM(n=2, L=200, N=10, batch=1)
    mpc = KM(n=2, L=8, N=10, batch=2)
    with pytest.raises(KmpcError):
        mpc.Encoder(np.zeros((2, 2)))  # encoder layers never set
    with pytest.raises(KmpcError):
        mpc.set_encoder([(np.zeros((50, 2)), np.zeros(50))])  # wrong shape


# ------------------------------------------------------------------ full-size property checks (cfg2)
def test_cfg2_full_size_properties(torch_mod, KM):
    """BASELINE cfg2 (Duffing, L=20, N=20, B=4096): size-independent properties of a closed-loop run:
    status 0 everywhere, box respected, returned U satisfies the KKT conditions of the condensed QP
    that kmpc_condense exports for the same model, P stays symmetric, trajectories are independent
    (a sub-batch run alone gives bitwise the same controls)."""
    torch = torch_mod
    from koopmpc.synth import initial_states, offline_edmd, random_mlp_weights

    L, N, B = 20, 20, 4096
    w = random_mlp_weights(2, 100, 3, L)
    mpc = KM(n=2, L=L, N=N, batch=B, weights=w)
    A0, B0, C0 = offline_edmd(lambda X: mpc.Encoder(X))
    mpc.set_model(A0, B0, C0)
    sub = KM(n=2, L=L, N=N, batch=64, weights=w)
    sub.set_model(A0, B0, C0)
    r = np.tile(np.array([[1.0], [0.0]]), (1, N))
    X = _t(torch, initial_states(B))
    Xs = X[:, 1000:1064].clone().contiguous()
    for k in range(12):
        u = mpc.step(X, r)
        us = sub.step(Xs, r)
        assert int(mpc.status.max().item()) == 0, k
        assert torch.equal(u[1000:1064], us)
        assert float(mpc.Useq.abs().max().item()) <= 2.0
        # KKT of the exported QP at the returned U
        psi = mpc.Encoder(X)
        H, f = mpc.condense(psi, r)
        U = mpc.Useq.t().contiguous()  # (B,N)
        g = 2 * torch.einsum("bij,bj->bi", H, U) + f
        res = (U - torch.clamp(U - g, -2.0, 2.0)).abs()
        scale = 2 * torch.einsum("bij,bj->bi", H.abs(), U.abs()) + f.abs()
        assert bool((res <= 1e-7 * torch.clamp(scale, min=1.0)).all()), k
        X = mpc.plant_step("duffing", X.clone(), u)
        Xs = sub.plant_step("duffing", Xs.clone(), us)
    A_, B_, C_ = mpc.get_model()
    assert bool(torch.isfinite(A_).all()) and bool(torch.isfinite(C_).all())


@pytest.mark.parametrize("script,args", [
    ("duffing", ["--weights", "weights_duffing.npz", "--batch", "5", "--steps", "30"]),
    ("vanderpol", ["--weights", "weights_vdp.npz", "--batch", "1", "--steps", "30"]),
    ("vanderpol_RBF", ["--batch", "6", "--steps", "25", "--horizon", "30"]),
    ("vanderpol_RBF", ["--plant", "duffing", "--batch", "6", "--steps", "25", "--switch-step", "12"]),  # (duffing_RBF.py: :40, 118, 342, 506)
    ("tank", ["--weights", "weights_tank.npz", "--batch", "4", "--steps", "30"]),
    ("tank", ["--batch", "8", "--steps", "12", "--shared", "--Nlift", "32", "--horizon", "40"]),
])
def test_reference_loop_scripts_run(torch_mod, tmp_path, monkeypatch, script, args):
    """koopmpc/scripts/*.py are the reference's experiment loops (duffing.py, vanderpol.py, vanderpol_RBF.py,
    Tank_System.m) on this library: each one runs, logs finite inputs inside its box and leaves finite states."""
    import importlib
    import sys

    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    argv = [a if not a.endswith(".npz") else os.path.join(gdir, a) for a in args]
    out = str(tmp_path / "log.npz")
    monkeypatch.setattr(sys, "argv", [script] + argv + ["--out", out])
    mod = importlib.import_module("koopmpc.scripts." + script)
    mod.main()
    log = np.load(out)
    U = log["logUloc"]
    bound = {"duffing": 2.0, "vanderpol": 6.0, "vanderpol_RBF": 2.0, "tank": 8.0}[script]
    assert np.isfinite(U).all() and np.abs(U).max() <= bound + 1e-9
    if "logXloc" in log.files:
        assert np.isfinite(log["logXloc"]).all()
