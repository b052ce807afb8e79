"""The float32 kernel instantiations (KMPC_F32 handles) against the float64 oracle.

A float32 handle runs separately compiled kernels and, in places, code a float64 handle never takes.  Every case here has one shape:
the inputs are built on the host and rounded ONCE to float32 (``_f32``: np.float32(...).astype(np.float64)), exactly those values go
to a KMPC_F32 handle and to oracle/koopman_oracle.py, and the results are compared.  The hand-over is exact; what is left is the
kernel's own float32 arithmetic.

Tolerances are measured, not chosen.  For every compared quantity the oracle's formula is evaluated a second time in NumPy float32
on the same inputs (the ``*32`` functions below: every operand cast, every ``eye`` / ``zeros`` created as float32).  Its deviation
from the float64 oracle, relative to the quantity's largest magnitude, is the error float32 arithmetic makes on the problem in the
reference's own order of operations.  The kernel sums in another order, on MFMA, in FMA form: its bound is 8 x that deviation and
never less than 16 float32 ulps (16 * 2^-24 = 9.5e-7) of the scale.  The deviation comes from the oracle alone, at test time.  The
derived bound may not exceed a cap -- 1e-4 lifts / condense / cost / plant steps, 1e-3 models (RLS, offline fit, pooled model) and
the relative KKT residual, 5e-3 closed-loop u_k -- and ``test_float32_oracle_deviations_stay_under_their_caps`` (no GPU) asserts
that for every case: inputs too ill-conditioned for float32 to mean anything fail there, on the CPU.  The only exact comparisons
are: tile-loop columns against a B = 16 launch, the x rows of the x_psi0 lift, r = 0 of the RBF lifts, U0 == U[0], box feasibility.

Kernel edges and the cases that execute them (lift_kernel.hip: lift_mlp_kernel<float, ..>, lift_rbf_kernel<float>; step_body.h):
  KSp < KS clamp of the fragment loads            test_mlp_lift[2-37-2-5] (KSp = 10 of KS = 28), [2-100-2-10] (25 of 28), [3-113-2-16] (29 of 32)
  Mma<float>::row accumulator map                 every test_mlp_lift / test_mlp_lift_offset case (hidden and output layers)
  second tile-loop iteration, NHH == 1 barrier    test_mlp_lift[..layers 2..] at B = 16400 (1025 tiles, grid 1024: block 0 walks tile 1024)
  second tile-loop iteration, NHH == 2            test_mlp_lift[1-128-3-64], [4-112-3-33] at B = 16400
  partial / single-row output tiles, Hp = 112     [2-37-2-5] (5 of 16 rows), [4-112-3-33] (tile 2 holds row 32 only; Hp = 112 exactly)
  first width padded to 128                       [3-113-2-16]; hidden + 2n = 128 in test_mlp_lift_offset[4-120-*]
  generic RBF branch at n = 2 (float has no       test_rbf_lift[*-2-8]; the RBF-lifted kmpc_step cases
    bit-for-bit n == 2 branch)
  float step_body, register-state set             test_step_kernels[reg-*]   (8, 10, y = Cx)
  float step_body, y = psi on the 8 x 8 grid      test_step_kernels[psi-*], test_closed_loop_steps[psi]   (8, 30, y = psi)
  float step_body, L = 32 with delta-u            test_step_kernels[du32-*], test_closed_loop_steps[du32]   (32, 40, Cx row 1)
  float step_body, four waves                     test_step_kernels[w4-*]   (64, 50)
  None of these handles compiles a plug-in: the lift handles and the psi set use y = psi, du32 is delta-u (neither has float32
  panels around the fused roll-out), (8, 10, 2) is a built-in float32-panel set, (64, 50) is a four-wave set without a fused roll-out;
  every test asserts kmpc_rollout_plugin_status in (0, 2).

Every float32 entry point exercised here is offered for KMPC_F32 (kmpc_mpc_solve, kmpc_condense_cost, kmpc_plant_step,
kmpc_offline_fit, the shared-model stage): none refuses, so there is no refusal to test beyond the float64-only features whose
refusals tests/test_gpu_parity.py, test_gpu_round6.py and test_gpu_diagnostics.py already hold.

Measured deviations of the float32 oracle (relative; the bound is 8 x, floor 9.5e-7), from the CPU companion (`pytest -s`):
  quantity                                       deviation  (B = 5)    cap
  mlp_lift (2, 37, 2, 5)                         2.03e-07              1e-04
  mlp_lift (2, 100, 2, 10)                       3.70e-07              1e-04
  mlp_lift (1, 128, 3, 64)                       6.18e-07              1e-04
  mlp_lift (4, 112, 3, 33)                       3.79e-07              1e-04
  mlp_lift (3, 113, 2, 16)                       3.02e-07              1e-04
  mlp_lift_offset psi0 (4, 120)                  3.27e-07              1e-04
  mlp_lift_offset x_psi0 (4, 120)                1.87e-07              1e-04
  mlp_lift_offset psi0 (1, 37)                   2.17e-07              1e-04
  mlp_lift_offset x_psi0 (1, 37)                 1.54e-07              1e-04
  rbf_lift python (2, 8)                         2.29e-07              1e-04
  rbf_lift matlab (2, 8)                         1.17e-07              1e-04
  rbf_lift python (1, 33)                        1.46e-07              1e-04
  rbf_lift matlab (1, 33)                        1.23e-07              1e-04
  rbf_lift python (4, 4)                         1.81e-07              1e-04
  rbf_lift matlab (4, 4)                         1.67e-07              1e-04
  reg: [A B] after 3 updates                     1.35e-07   1.35e-07   1e-03
  reg: C after 3 updates                         1.16e-07   1.32e-07   1e-03
  reg: H                                         1.25e-07   1.25e-07   1e-04
  reg: f                                         1.03e-07   9.74e-08   1e-04
  reg: cost constant                             5.68e-08   7.27e-08   1e-04
  reg: box QP, cond(H) = 1e3                     3.39e-06   2.52e-06   1e-03
  psi: [A B] after 3 updates                     1.56e-07   1.23e-07   1e-03
  psi: H                                         3.43e-07   3.43e-07   1e-04
  psi: f                                         9.88e-08   1.41e-07   1e-04
  psi: cost constant                             1.11e-07   2.90e-09   1e-04
  psi: box QP, cond(H) = 1e3                     2.40e-06   1.70e-06   1e-03
  du32: [A B] after 3 updates                    1.67e-07   2.20e-07   1e-03
  du32: C after 3 updates                        1.51e-07   1.08e-07   1e-03
  du32: H                                        3.46e-07   3.46e-07   1e-04
  du32: f                                        2.47e-07   2.85e-07   1e-04
  du32: cost constant                            1.25e-07   4.35e-08   1e-04
  du32: box QP, cond(H) = 1e3                    7.89e-07   7.89e-07   1e-03
  w4: [A B] after 3 updates                      2.07e-07   1.36e-07   1e-03
  w4: C after 3 updates                          1.71e-07   1.54e-07   1e-03
  w4: H                                          1.67e-07   1.67e-07   1e-04
  w4: f                                          2.47e-07   2.24e-07   1e-04
  w4: cost constant                              9.05e-08   7.08e-08   1e-04
  w4: box QP, cond(H) = 1e3                      3.24e-06   1.85e-06   1e-03
  psi: u_k over 3 closed-loop steps              7.70e-06              5e-03
  du32: u_k over 3 closed-loop steps             2.29e-06              5e-03
  plant_step duffing                             4.05e-08              1e-04
  plant_step duffing, switched                   4.56e-08              1e-04
  plant_step duffing_matlab                      3.08e-08              1e-04
  plant_step duffing_matlab, switched            1.87e-08              1e-04
  plant_step vdp                                 2.90e-08              1e-04
  plant_step vdp, switched                       3.83e-08              1e-04
  plant_step vdp_matlab                          7.66e-08              1e-04
  plant_step vdp_matlab, switched                4.74e-08              1e-04
  plant_step tank                                7.17e-08              1e-04
  plant_step tank, switched                      7.44e-08              1e-04
  offline_fit [A B]                              1.60e-05              1e-03
  offline_fit C                                  1.49e-05              1e-03
  shared model [A B]                             9.76e-05              1e-03
  shared model C                                 1.10e-05              1e-03
  shared-model u_k, 2 steps                      2.66e-04              5e-03
  mpc_solve fun (per-trajectory models, no P_N)  6.77e-08              1e-04
  mpc_solve fun (per-trajectory models, P_N)     2.83e-07              1e-04
  mpc_solve fun (one model, no P_N)              1.58e-07              1e-04
  mpc_solve fun (one model, P_N)                 1.60e-07              1e-04
"""
import functools

import numpy as np
import pytest

from oracle import koopman_oracle as ko

F = np.float32
ULP16 = 16.0 * 2.0 ** -24
CAP_LIFT = CAP_CONDENSE = CAP_PLANT = 1e-4
CAP_MODEL = CAP_KKT = 1e-3
CAP_U = 5e-3


def _f32(a):
    """the float64 array whose values are exactly representable in float32"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ====================================================================================================================
# the oracle's formulas once more in float32 (every operand cast, every eye / zeros created as float32)
# ====================================================================================================================
def mlp_lift32(weights, X):
    """ko.mlp_lift"""
    H = np.asarray(X, dtype=F)
    if H.ndim == 1:
        H = H[:, None]
    for k, (W, b) in enumerate(weights):
        H = np.asarray(W, dtype=F) @ H + np.asarray(b, dtype=F).reshape(-1, 1)
        if k + 1 < len(weights):
            H = np.maximum(H, F(0))
    return H


def mlp_lift_offset32(weights, X, form):
    """ko.mlp_lift_offset"""
    X = np.asarray(X, dtype=F)
    E = mlp_lift32(weights, X) - mlp_lift32(weights, np.zeros((X.shape[0], 1), dtype=F))
    return E if form == "psi0" else np.concatenate([X, E], axis=0)


def rbf_lift32(X, cx, eps=1e-4, form="python"):
    """ko.rbf_lift"""
    X = np.asarray(X, dtype=F)
    if X.ndim == 1:
        X = X[:, None]
    cx = np.asarray(cx, dtype=F)
    if form == "python":
        xx = np.sum(X * X, axis=0)[None, :]
        cc = np.sum(cx * cx, axis=1)[:, None]
        d2 = np.maximum(xx - F(2) * (cx @ X) + cc, F(0))
        d = np.sqrt(d2)
        return d * d * np.log(d + F(eps))
    r2 = np.sum((X[None, :, :] - cx[:, :, None]) ** 2, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = r2 * np.log(np.sqrt(r2))
    y[np.isnan(y)] = F(0)
    return y


def rls_update_gain32(K, P, z, y):
    """ko.rls_update_gain, lam = 1"""
    z = np.asarray(z, dtype=F).reshape(-1, 1)
    y = np.asarray(y, dtype=F).reshape(-1, 1)
    Pz = P @ z
    d = F(1) + (z.T @ Pz)[0, 0]
    g = Pz / d
    return K + (y - K @ z) @ g.T, P - Pz @ Pz.T / d


def condense32(A, B, Co, psi, r, N, Qw, Rw, PN=None):
    """ko.condense -> H, f, const"""
    A = np.asarray(A, dtype=F)
    L = A.shape[0]
    B = np.asarray(B, dtype=F).reshape(L, 1)
    Co = np.eye(L, dtype=F) if Co is None else np.asarray(Co, dtype=F)
    q = Co.shape[0]
    Gam = np.zeros((q * N, L), dtype=F)
    Phi = np.zeros((q * N, N), dtype=F)
    M = Co.copy()
    g = []
    for j in range(N):
        g.append(M @ B)
        M = M @ A
        Gam[q * j: q * (j + 1), :] = M
    for i in range(N):
        for j in range(i + 1):
            Phi[q * i: q * (i + 1), j: j + 1] = g[i - j]
    Qbar = F(Qw) * np.eye(q * N, dtype=F)
    if PN is not None:
        Qbar[-q:, -q:] = np.asarray(PN, dtype=F)
    H = Phi.T @ Qbar @ Phi + F(Rw) * np.eye(N, dtype=F)
    H = F(0.5) * (H + H.T)
    e = Gam @ np.asarray(psi, dtype=F).reshape(-1, 1) - np.asarray(r, dtype=F).T.reshape(-1, 1)
    f = F(2) * (Phi.T @ Qbar @ e).reshape(-1)
    return H, f, (e.T @ Qbar @ e)[0, 0]


def cost_function32(u, r, AB, C, x0, Qw, Rw):
    """ko.cost_function"""
    x = np.asarray(x0, dtype=F).reshape(-1, 1)
    AB = np.asarray(AB, dtype=F)
    r = np.asarray(r, dtype=F)
    u = np.asarray(u, dtype=F).reshape(-1)
    J = F(0)
    for k in range(u.size):
        x = AB @ np.concatenate([x, u[k].reshape(1, 1)], axis=0)
        y = x if C is None else np.asarray(C, dtype=F) @ x
        e = y - r[:, k].reshape(-1, 1)
        J = J + F(Qw) * np.sum(e * e)
    return J + F(Rw) * np.sum(u * u)


def qp_exact32(H, f, lb, ub):
    """ko.qp_exact (primal active set) in float32.  Its two thresholds are those of the float64 original scaled to the format:
    a Newton step counts as zero below 16 ulps of the iterate, a multiplier as of the right sign within 64 ulps of the gradient's
    terms.  Returns the last iterate when the iteration cap is reached (the companion test judges it by its KKT residual)."""
    H = np.asarray(H, dtype=F)
    f = np.asarray(f, dtype=F).reshape(-1)
    n = f.size
    lb = np.broadcast_to(np.asarray(lb, dtype=F), (n,)).copy()
    ub = np.broadcast_to(np.asarray(ub, dtype=F), (n,)).copy()
    x = np.clip(np.zeros(n, dtype=F), lb, ub)
    act = np.zeros(n, dtype=int)
    act[x <= lb] = -1
    act[x >= ub] = 1
    eps = F(2.0 ** -24)
    gscale = np.abs(f) + F(2) * (np.abs(H) @ np.maximum(np.abs(lb), np.abs(ub)))
    at_min = False
    for _ in range(20 * n + 20):
        Fm = act == 0
        grad = F(2) * (H @ x) + f
        p = np.zeros(n, dtype=F)
        if Fm.any() and not at_min:
            p[Fm] = np.linalg.solve(F(2) * H[np.ix_(Fm, Fm)], -grad[Fm])
        if at_min or np.max(np.abs(p)) <= F(16) * eps * max(F(1), np.max(np.abs(x))):
            viol = np.where(act == -1, -grad, np.where(act == 1, grad, F(0))) / np.maximum(gscale, F(1e-30))
            j = int(np.argmax(viol))
            if viol[j] <= F(64) * eps:
                return x
            act[j] = 0
            at_min = False
            continue
        alpha, blk = F(1), -1
        for i in np.nonzero(Fm)[0]:
            if p[i] < 0 and x[i] + p[i] < lb[i]:
                a = (lb[i] - x[i]) / p[i]
                if a < alpha:
                    alpha, blk = a, i
            elif p[i] > 0 and x[i] + p[i] > ub[i]:
                a = (ub[i] - x[i]) / p[i]
                if a < alpha:
                    alpha, blk = a, i
        x = np.clip(x + alpha * p, lb, ub)  # (the clip only removes the rounding of alpha * p: the step ends inside the box by construction)
        at_min = blk < 0
        if blk >= 0:
            x[blk] = lb[blk] if p[blk] < 0 else ub[blk]
            act[blk] = -1 if p[blk] < 0 else 1
    return x


def plant_step32(kind, x, u, h=0.05, switched=False):
    """ko.plant_step / ko.tank_step"""
    x = np.asarray(x, dtype=F)
    u = np.asarray(u, dtype=F)
    h = F(h)
    if kind == "tank":
        if switched:
            xn = np.stack([x[0] - F(0.53) * np.sqrt(x[0]) + F(0.3) * u, x[1] + F(0.1) * np.sqrt(x[0]) - F(0.35) * np.sqrt(x[1])])
        else:
            xn = np.stack([x[0] - F(0.5) * np.sqrt(x[0]) + F(0.4) * u, x[1] + F(0.2) * np.sqrt(x[0]) - F(0.3) * np.sqrt(x[1])])
        return np.maximum(xn, F(0))
    matlab = kind.endswith("_matlab")
    base = kind[:-7] if matlab else kind
    if base == "duffing":
        if switched:
            f = lambda x: np.stack([x[1], -F(10.0) * F(0.5) * x[1] + F(2.0) * x[0] - F(0.5) * x[0] ** F(3.0) + u])
        else:
            f = lambda x: np.stack([x[1], -F(0.5) * x[1] + x[0] - x[0] ** F(3.0) + u])
    else:
        if switched:
            f = lambda x: np.stack([x[1], -F(3.0) * x[1] - F(10.0) * x[0] ** F(2.0) * x[1] - F(3.0) * x[0] + u])
        else:
            f = lambda x: np.stack([F(2.0) * x[1], F(2.0) * x[1] - F(10.0) * x[0] ** F(2.0) * x[1] - F(0.8) * x[0] + u])
    k1 = f(x)
    k2 = f(x + F(0.5) * h * k1)
    k3 = f(x + F(0.5) * h * k2)
    k4 = f(x + h * (k1 if matlab else k3))
    return x + (h / F(6.0)) * (k1 + F(2.0) * k2 + F(2.0) * k3 + k4)


def gram_fit32(PX, PY, U, X, ridge):
    """the Gram-form solve of ko.SharedEdmd.model (Koopman_update.m:94-101) with both ridges = ridge"""
    PX, PY, X = np.asarray(PX, dtype=F), np.asarray(PY, dtype=F), np.asarray(X, dtype=F)
    L = PX.shape[0]
    Z = np.concatenate([PX, np.asarray(U, dtype=F).reshape(1, -1)], axis=0)
    G, YZ, XZ = Z @ Z.T, PY @ Z.T, X @ Z.T
    K = np.linalg.solve(G + F(ridge) * np.eye(L + 1, dtype=F), YZ.T).T
    C = np.linalg.solve(G[:L, :L] + F(ridge) * np.eye(L, dtype=F), XZ[:, :L].T).T
    return K, C


def gram_fit64(PX, PY, U, X, ridge):
    L = PX.shape[0]
    Z = np.concatenate([PX, np.reshape(U, (1, -1))], axis=0)
    G, YZ, XZ = Z @ Z.T, PY @ Z.T, X @ Z.T
    K = np.linalg.solve(G + ridge * np.eye(L + 1), YZ.T).T
    C = np.linalg.solve(G[:L, :L] + ridge * np.eye(L), XZ[:, :L].T).T
    return K, C


# ====================================================================================================================
# bounds
# ====================================================================================================================
class Ref:
    """one compared quantity: the float64 oracle's value, the float32 oracle's value, the cap of its bound"""

    def __init__(self, name, w64, w32, cap):
        self.name, self.w64, self.w32, self.cap = name, np.asarray(w64, dtype=np.float64), np.asarray(w32), cap

    def cut(self, idx):
        return Ref(self.name, self.w64[idx], self.w32[idx], self.cap)

    def scale(self):
        return float(np.abs(self.w64).max())

    def deviation(self):
        return float(np.abs(self.w32.astype(np.float64) - self.w64).max()) / self.scale()

    def bound(self):
        return max(8.0 * self.deviation(), ULP16)

    def check(self, got, what=""):
        got = np.asarray(got)
        assert got.dtype == np.float32, (self.name, got.dtype)  # the kernel's own panel, not a conversion
        assert got.shape == self.w64.shape, (self.name, got.shape, self.w64.shape)
        err = float(np.abs(got.astype(np.float64) - self.w64).max()) / self.scale()
        print("%-34s %-26s float32 oracle %.2e -> bound %.2e, kernel %.2e" % (self.name, what, self.deviation(), self.bound(), err))
        assert np.isfinite(err) and err <= self.bound(), (self.name, what, err, self.bound())


class KktRef:
    """the box QP is judged by its optimality: ko.kkt_residual in float64, relative to max|f|, per problem"""

    def __init__(self, name, H, f, lb, ub, U32):
        self.name, self.H, self.f, self.lb, self.ub, self.U32, self.cap = name, H, f, lb, ub, U32, CAP_KKT

    def kkt(self, U):
        U = np.asarray(U, dtype=np.float64)
        return max(ko.kkt_residual(self.H[b], self.f[b], self.lb[b], self.ub[b], U[:, b]) / np.abs(self.f[b]).max() for b in range(self.H.shape[0]))

    def cut(self, idx):
        return KktRef(self.name, self.H[idx], self.f[idx], self.lb[idx], self.ub[idx], self.U32[:, idx])

    def deviation(self):
        return self.kkt(self.U32)

    def bound(self):
        return max(8.0 * self.deviation(), ULP16)

    def check(self, U, status, what=""):
        U = np.asarray(U)
        assert U.dtype == np.float32
        assert int(np.max(status)) == 0, (self.name, what, status)
        U = U.astype(np.float64)
        assert np.all(U >= self.lb.T) and np.all(U <= self.ub.T), (self.name, what, "outside the box")  # no slack
        err = self.kkt(U)
        print("%-34s %-26s float32 oracle %.2e -> bound %.2e, kernel %.2e (relative KKT residual)" % (self.name, what, self.deviation(), self.bound(), err))
        assert np.isfinite(err) and err <= self.bound(), (self.name, what, err, self.bound())


# ====================================================================================================================
# 1. lifts
# ====================================================================================================================
MLP_SETS = [(2, 37, 2, 5), (2, 100, 2, 10), (1, 128, 3, 64), (4, 112, 3, 33), (3, 113, 2, 16)]  # (n, hidden, layers, L)
MLP_BATCHES = [1, 16, 17, 16400]
OFFSET_SETS = [(4, 120, 3, 9), (1, 37, 2, 9)]  # (n, hidden, layers, encoder outputs)
RBF_SETS = [(2, 8), (1, 33), (4, 4)]  # (n, L)
RBF_B = 17


def _mlp_weights(n, hidden, layers, Lout, seed):
    rng = np.random.RandomState(seed)
    dims = [n] + [hidden] * layers + [Lout]
    return [(_f32(rng.randn(dims[k + 1], dims[k]) / np.sqrt(dims[k])), _f32(0.1 * rng.randn(dims[k + 1]))) for k in range(len(dims) - 1)]


@functools.lru_cache(maxsize=None)
def mlp_case(n, hidden, layers, L):
    """weights, 16400 distinct random states, both oracles on all of them (every batch of the set is a prefix)"""
    w = _mlp_weights(n, hidden, layers, L, 1000 + hidden + L)
    X = _f32(4 * np.random.RandomState(hidden).rand(n, max(MLP_BATCHES)) - 2)
    return w, X, Ref("mlp_lift (%d, %d, %d, %d)" % (n, hidden, layers, L), ko.mlp_lift(w, X), mlp_lift32(w, X), CAP_LIFT)


@functools.lru_cache(maxsize=None)
def offset_case(n, hidden, layers, Lenc, form):
    w = _mlp_weights(n, hidden, layers, Lenc, 2000 + hidden)
    X = _f32(4 * np.random.RandomState(hidden + 1).rand(n, 17) - 2)
    X[:, 0] = 0.0
    return w, X, Ref("mlp_lift_offset %s (%d, %d)" % (form, n, hidden), ko.mlp_lift_offset(w, X, form), mlp_lift_offset32(w, X, form), CAP_LIFT)


@functools.lru_cache(maxsize=None)
def rbf_case(n, L, form):
    rng = np.random.RandomState(3000 + 10 * n + L)
    cx = _f32(4 * rng.rand(L, n) - 2)
    X = np.concatenate([_f32(4 * rng.rand(n, RBF_B) - 2), cx.T], axis=1)  # the centres themselves: r = 0 exactly at [j, RBF_B + j]
    return cx, X, Ref("rbf_lift %s (%d, %d)" % (form, n, L), ko.rbf_lift(X, cx, 1e-4, form), rbf_lift32(X, cx, 1e-4, form), CAP_LIFT)


# ====================================================================================================================
# 2. step kernels
# ====================================================================================================================
# (L, N, output, delta-u): register-state; the 8 x 8 grid with y = psi; L = 32 with the tank's delta-u on Cx row 1; four waves.
# Start of the estimator: P0 = 1e4, barQ0 = 100, unit-variance transitions (duffing.py:929-930, 946).
STEP_SETS = {
    "reg": dict(L=8, N=10, output="Cx"),
    "psi": dict(L=8, N=30, output="lift"),
    "du32": dict(L=32, N=40, output="Cx", delta_u=True, out_row0=1, out_rows=1, lb=-0.5, ub=0.5, umin=-0.75, umax=0.75, Qw=10.0, Rw=1e-3),
    "w4": dict(L=64, N=50, output="Cx"),
}
STEP_B = 33  # one workgroup plus a tail; the B = 5 handle takes its first five trajectories (a partial workgroup)
P0, BARQ0 = 1e4, 100.0


def _set_kw(name):
    kw = dict(lb=-2.0, ub=2.0, umin=-8.0, umax=8.0, Qw=100.0, Rw=1e-4, delta_u=False, out_row0=0, out_rows=0)
    kw.update(STEP_SETS[name])
    return kw


def _stable_model(rng, L, n):
    return _f32(0.9 * np.linalg.qr(rng.randn(L, L))[0]), _f32(rng.randn(L, 1)), _f32(rng.randn(n, L) / np.sqrt(L))


def _du_problem(kw, A, B, C, psi, uprev):
    """the increment form (ko.OracleDeltaUController.qp): A~ = [A B; 0 I], B~ = [B; I], Co = row cy0 of [C 0], x~ = [psi; u_prev]"""
    L = A.shape[0]
    dt = A.dtype
    At = np.block([[A, B], [np.zeros((1, L), dtype=dt), np.eye(1, dtype=dt)]])
    Bt = np.concatenate([B, np.ones((1, 1), dtype=dt)], axis=0)
    Ct = np.concatenate([C, np.zeros((C.shape[0], 1), dtype=dt)], axis=1)
    return At, Bt, Ct[kw["out_row0"]: kw["out_row0"] + kw["out_rows"]], np.concatenate([psi, [uprev]]).astype(dt)


def _box(kw, N, uprev):
    """[lb, ub]^N, the first increment also inside [umin - u_prev, umax - u_prev] (Tank_System.m:182-188)"""
    lbv, ubv = np.full(N, kw["lb"]), np.full(N, kw["ub"])
    if kw["delta_u"]:
        lbv[0], ubv[0] = max(kw["lb"], kw["umin"] - uprev), min(kw["ub"], kw["umax"] - uprev)
    return lbv, ubv


@functools.lru_cache(maxsize=None)
def step_case(name):
    kw = _set_kw(name)
    L, N, n, B = kw["L"], kw["N"], 2, STEP_B
    lift_out = kw["output"] == "lift"
    q = L if lift_out else (kw["out_rows"] or n)
    rng = np.random.RandomState(sum(map(ord, name)))
    d = dict(kw=kw, cx=_f32(4 * rng.rand(L, n) - 2))
    # three successive updates on random transitions
    d["trans"] = [(_f32(rng.randn(L, B)), _f32(rng.randn(B)), _f32(rng.randn(L, B)), _f32(rng.randn(n, B))) for _ in range(3)]
    K64, C64, K32, C32 = np.zeros((B, L, L + 1)), np.zeros((B, n, L)), np.zeros((B, L, L + 1), dtype=F), np.zeros((B, n, L), dtype=F)
    for b in range(B):
        K, P, Cm, Q = np.zeros((L, L + 1)), P0 * np.eye(L + 1), np.zeros((n, L)), BARQ0 * np.eye(L)
        k32, p32, c32, q32 = np.zeros((L, L + 1), dtype=F), F(P0) * np.eye(L + 1, dtype=F), np.zeros((n, L), dtype=F), F(BARQ0) * np.eye(L, dtype=F)
        for psi, u, psin, xn in d["trans"]:
            z = np.concatenate([psi[:, b], [u[b]]])
            K, P = ko.rls_update_gain(K, P, z, psin[:, b])
            Cm, Q = ko.rls_update_gain(Cm, Q, psi[:, b], xn[:, b])
            k32, p32 = rls_update_gain32(k32, p32, z, psin[:, b])
            c32, q32 = rls_update_gain32(c32, q32, psi[:, b], xn[:, b])
        K64[b], C64[b], K32[b], C32[b] = K, Cm, k32, c32
    d["K"] = Ref("%s: [A B] after 3 updates" % name, K64, K32, CAP_MODEL)
    d["C"] = None if lift_out else Ref("%s: C after 3 updates" % name, C64, C32, CAP_MODEL)
    # condensed QP of a stable random model
    A0, B0, C0 = _stable_model(rng, L, n)
    d["model"] = (A0, B0, C0)
    d["psi"] = _f32(rng.randn(L, B))
    d["r"] = _f32(rng.randn(q, N))
    d["uprev"] = np.round(0.3 * rng.randn(B) * 64) / 64 if kw["delta_u"] else np.zeros(B)  # (multiples of 1/64: umin - u_prev is exact in both formats)
    H64, f64, c64 = np.zeros((B, N, N)), np.zeros((B, N)), np.zeros(B)
    H32, f32, c32 = np.zeros((B, N, N), dtype=F), np.zeros((B, N), dtype=F), np.zeros(B, dtype=F)
    for b in range(B):
        if kw["delta_u"]:
            a64 = _du_problem(kw, A0, B0, C0, d["psi"][:, b], d["uprev"][b])
            a32 = _du_problem(kw, A0.astype(F), B0.astype(F), C0.astype(F), d["psi"][:, b].astype(F), F(d["uprev"][b]))
        else:
            a64 = (A0, B0, None if lift_out else C0, d["psi"][:, b])
            a32 = a64
        _, _, H64[b], f64[b], c64[b] = ko.condense(*a64, d["r"], N, kw["Qw"], kw["Rw"])
        H32[b], f32[b], c32[b] = condense32(*a32, d["r"], N, kw["Qw"], kw["Rw"])
    d["H"], d["f"], d["c"] = Ref("%s: H" % name, H64, H32, CAP_CONDENSE), Ref("%s: f" % name, f64, f32, CAP_CONDENSE), Ref("%s: cost constant" % name, c64, c32, CAP_CONDENSE)
    # box QPs with cond(H) = 1e3
    Hq, fq = np.zeros((B, N, N)), _f32(30 * rng.randn(B, N))
    for b in range(B):
        Qo = np.linalg.qr(rng.randn(N, N))[0]
        Hb = Qo @ np.diag(np.logspace(0, 3, N)) @ Qo.T
        Hq[b] = _f32(0.5 * (Hb + Hb.T))
    lbq, ubq = [np.stack(v) for v in zip(*[_box(kw, N, d["uprev"][b]) for b in range(B)])]
    U32 = np.stack([qp_exact32(Hq[b], fq[b], lbq[b], ubq[b]) for b in range(B)], axis=1)
    d["qp"] = KktRef("%s: box QP, cond(H) = 1e3" % name, Hq, fq, lbq, ubq, U32)
    return d


# the closed loop (kmpc_step): gentler weights than the defaults, a target the box cannot reach (the inputs saturate, the delta-u set runs
# into its absolute range), the estimator started closer to its data (P0 = barQ0 = 100)
LOOP_KW = dict(psi=dict(Qw=1.0, Rw=0.1), du32=dict(Qw=10.0, Rw=1e-3))
LOOP_P0 = 100.0
LOOP_STEPS = 3
PLANT_A, PLANT_B_COL = np.array([[0.9, 0.1], [-0.2, 0.8]]), np.array([0.0, 0.5])  # the host plant of the closed-loop and fit cases


class Loop:
    """ko.OracleController(rls="gain") / ko.OracleDeltaUController (c_skip_first off) in either precision: dt = float64 calls the
    oracle's functions, dt = float32 their restatements above"""

    def __init__(self, dt, kw, cx, model):
        self.dt, self.kw, self.cx = dt, kw, cx
        L, n = kw["L"], 2
        self.A, self.B, self.C = [np.asarray(m, dtype=dt) for m in model]
        self.K, self.P = np.zeros((L, L + 1), dtype=dt), dt(LOOP_P0) * np.eye(L + 1, dtype=dt)
        self.Cg, self.Q = np.zeros((n, L), dtype=dt), dt(LOOP_P0) * np.eye(L, dtype=dt)
        self.prev, self.u = None, dt(0)

    def step(self, x, r):
        kw, dt = self.kw, self.dt
        f64 = dt is np.float64
        psi = (ko.rbf_lift if f64 else rbf_lift32)(np.reshape(x, (-1, 1)), self.cx).reshape(-1)
        if self.prev is not None:
            ppsi, pu = self.prev
            upd = ko.rls_update_gain if f64 else rls_update_gain32
            self.K, self.P = upd(self.K, self.P, np.concatenate([ppsi, [pu]]).astype(dt), psi)
            self.Cg, self.Q = upd(self.Cg, self.Q, ppsi, np.asarray(x, dtype=dt).reshape(-1))
            self.A, self.B, self.C = self.K[:, :-1].copy(), self.K[:, -1:].copy(), self.Cg.copy()
        if kw["delta_u"]:
            args = _du_problem(kw, self.A, self.B, self.C, psi, self.u)
        else:
            args = (self.A, self.B, None if kw["output"] == "lift" else self.C, psi)
        if f64:
            _, _, H, f, _ = ko.condense(*args, r, kw["N"], kw["Qw"], kw["Rw"])
        else:
            H, f, _ = condense32(*args, r, kw["N"], kw["Qw"], kw["Rw"])
        lbv, ubv = np.full(kw["N"], dt(kw["lb"])), np.full(kw["N"], dt(kw["ub"]))
        if kw["delta_u"]:
            lbv[0], ubv[0] = max(dt(kw["lb"]), dt(kw["umin"]) - self.u), min(dt(kw["ub"]), dt(kw["umax"]) - self.u)
        U = ko.qp_exact(H, f, lbv, ubv)[0] if f64 else qp_exact32(H, f, lbv, ubv)
        self.u = (self.u + U[0]) if kw["delta_u"] else U[0]
        self.prev = (psi, self.u)
        return self.u


@functools.lru_cache(maxsize=None)
def loop_case(name):
    kw = _set_kw(name)
    kw.update(LOOP_KW[name])
    L, N, n, B = kw["L"], kw["N"], 2, STEP_B
    q = L if kw["output"] == "lift" else (kw["out_rows"] or n)
    rng = np.random.RandomState(7 + sum(map(ord, name)))
    cx = _f32(4 * rng.rand(L, n) - 2)
    model = _stable_model(rng, L, n)
    r = _f32(np.tile(3.0 + rng.rand(q, 1), (1, N)))
    # the states every side is given: a slow stable plant driven by the float64 oracle's own controls, rounded to float32 (successive
    # states stay close, so the rank-one model of the first update -- A ~ psi_k psi_{k-1}' / |z|^2 -- has its eigenvalue near one
    # and the condensed QP of the 40-step horizon stays representable)
    Xs = [_f32(4 * rng.rand(n, B) - 2)] + [np.zeros((n, B)) for _ in range(LOOP_STEPS - 1)]
    u64, u32 = np.zeros((LOOP_STEPS, B)), np.zeros((LOOP_STEPS, B), dtype=F)
    for b in range(B):
        c64, c32 = Loop(np.float64, kw, cx, model), Loop(np.float32, kw, cx, model)
        for k in range(LOOP_STEPS):
            u64[k, b], u32[k, b] = c64.step(Xs[k][:, b], r), c32.step(Xs[k][:, b], r)
            if k + 1 < LOOP_STEPS:
                Xs[k + 1][:, b] = _f32(PLANT_A @ Xs[k][:, b] + PLANT_B_COL * u64[k, b])
    # (the oracle's own classes give the same float64 controls: the companion test checks Loop against them)
    return dict(kw=kw, cx=cx, model=model, r=r, Xs=Xs, u=Ref("%s: u_k over %d closed-loop steps" % (name, LOOP_STEPS), u64, u32, CAP_U))


# ====================================================================================================================
# 3. the remaining entry points
# ====================================================================================================================
SOLVE_L, SOLVE_N, SOLVE_B = 8, 10, 17
PN_SOLVE = np.array([[300.0, 20.0], [20.0, 150.0]])


@functools.lru_cache(maxsize=None)
def solve_case(shared):
    L, N, B, n = SOLVE_L, SOLVE_N, SOLVE_B, 2
    rng = np.random.RandomState(40 + shared)
    models = [_stable_model(rng, L, n) for _ in range(1 if shared else B)]
    return dict(models=models, psi=_f32(rng.randn(L, B)), r=_f32(rng.randn(n, N)))


def solve_fun_ref(case, U, with_pn):
    """`fun` at the RETURNED sequences U (N, B; float64 values of the kernel's float32 panel): ko.cost_function, and with a terminal
    block -- which cost_function does not have -- the condensed form u'Hu + f'u + c of ko.condense(PN=...), its equal"""
    B = SOLVE_B
    J64, J32 = np.zeros(B), np.zeros(B, dtype=F)
    for b in range(B):
        A, Bm, Cm = case["models"][0 if len(case["models"]) == 1 else b]
        if with_pn:
            _, _, H, f, c = ko.condense(A, Bm, Cm, case["psi"][:, b], case["r"], SOLVE_N, 100.0, 1e-4, PN=PN_SOLVE)
            J64[b] = U[:, b] @ H @ U[:, b] + f @ U[:, b] + c
            H3, f3, c3 = condense32(A, Bm, Cm, case["psi"][:, b], case["r"], SOLVE_N, 100.0, 1e-4, PN=PN_SOLVE)
            u3 = U[:, b].astype(F)
            J32[b] = u3 @ H3 @ u3 + f3 @ u3 + c3
        else:
            AB = np.concatenate([A, Bm], axis=1)
            J64[b] = ko.cost_function(U[:, b], case["r"], AB, Cm, case["psi"][:, b], 100.0, 1e-4)
            J32[b] = cost_function32(U[:, b], case["r"], AB, Cm, case["psi"][:, b], 100.0, 1e-4)
    return Ref("mpc_solve fun (%s, %s)" % ("one model" if len(case["models"]) == 1 else "per-trajectory models", "P_N" if with_pn else "no P_N"), J64, J32, CAP_CONDENSE)


PLANTS = ["duffing", "duffing_matlab", "vdp", "vdp_matlab", "tank"]
PLANT_B = 17


@functools.lru_cache(maxsize=None)
def plant_case(kind, switched):
    rng = np.random.RandomState(50 + PLANTS.index(kind))
    X = _f32(0.5 + 4 * rng.rand(2, PLANT_B)) if kind == "tank" else _f32(4 * rng.rand(2, PLANT_B) - 2)
    U = _f32(4 * rng.rand(PLANT_B) - 2)
    w64 = ko.tank_step(X, U, switched) if kind == "tank" else ko.plant_step(kind, X, U, 0.05, switched)
    return X, U, Ref("plant_step %s%s" % (kind, ", switched" if switched else ""), w64, plant_step32(kind, X, U, 0.05, switched), CAP_PLANT)


FIT_M, FIT_L, FIT_RIDGE = 600, 8, 1e-6


@functools.lru_cache(maxsize=None)
def fit_case():
    """M = 600 samples of a stable linear plant, L = 8 RBF observables, ridge 1e-6.  The float64 side is the Gram-form solve on the
    float32-ROUNDED lifts (the lift's own rounding is item 1's business); the float32 side lifts, sums and solves in float32."""
    n, L, M = 2, FIT_L, FIT_M
    rng = np.random.RandomState(60)
    # states and centres in [-1, 1]^2: the thin-plate observables stay O(1) beside u and cond(V V') = 9e2 (on [-2, 2]^2 it is 6e3 to
    # 5e5 with the centres' draw, and float32 Gram sums of 600 samples lose the fit to 1e-3 .. 2e-2: the CPU companion says so)
    cx = _f32(2 * rng.rand(L, n) - 1)
    X, U = _f32(2 * rng.rand(n, M) - 1), _f32(4 * rng.rand(M) - 2)
    Y = _f32(PLANT_A @ X + PLANT_B_COL[:, None] * U[None, :])
    PX, PY = _f32(ko.rbf_lift(X, cx)), _f32(ko.rbf_lift(Y, cx))
    K64, C64 = gram_fit64(PX, PY, U, X, FIT_RIDGE)
    K32, C32 = gram_fit32(rbf_lift32(X, cx), rbf_lift32(Y, cx), U, X, FIT_RIDGE)
    return dict(cx=cx, X=X, Y=Y, U=U, K=Ref("offline_fit [A B]", K64, K32, CAP_MODEL), C=Ref("offline_fit C", C64, C32, CAP_MODEL))


SHARED_KW = dict(L=10, N=20, output="Cx", delta_u=True, out_row0=1, out_rows=1, lb=-0.5, ub=0.5, umin=-0.75, umax=0.75, Qw=10.0, Rw=1e-3)
SHARED_B, SHARED_P0 = 37, 100.0


@functools.lru_cache(maxsize=None)
def shared_case():
    """two steps of the shared-model loop: step 0 solves with the offline model (no transition yet), step 1 with the model pooled
    from the batch's 37 transitions (ko.SharedEdmd), each trajectory's delta-u QP as ko.OracleDeltaUController.qp writes it.  The
    input applied after step 0 is the float64 oracle's u_0 rounded to float32, on every side (kmpc_set_applied_input)."""
    kw = dict(SHARED_KW)
    L, N, n, B = kw["L"], kw["N"], 2, SHARED_B
    rng = np.random.RandomState(70)
    cx = _f32(2 * rng.rand(L, n) - 1)  # (states and centres in [-1, 1]^2 as in fit_case: 37 samples for an 11 x 11 Gram matrix)
    model = _stable_model(rng, L, n)
    r = _f32(np.full((1, N), 0.2))
    Xs = [_f32(2 * rng.rand(n, B) - 1) for _ in range(2)]

    def solve(dt, A, Bm, Cm, psi, uprev):
        args = _du_problem(kw, A.astype(dt), np.reshape(Bm, (L, 1)).astype(dt), Cm.astype(dt), psi.astype(dt), dt(uprev))
        lbv, ubv = np.full(N, dt(kw["lb"])), np.full(N, dt(kw["ub"]))
        lbv[0], ubv[0] = max(dt(kw["lb"]), dt(kw["umin"]) - dt(uprev)), min(dt(kw["ub"]), dt(kw["umax"]) - dt(uprev))
        if dt is np.float64:
            _, _, H, f, _ = ko.condense(*args, r, N, kw["Qw"], kw["Rw"])
            return dt(uprev) + ko.qp_exact(H, f, lbv, ubv)[0][0]
        H, f, _ = condense32(*args, r, N, kw["Qw"], kw["Rw"])
        return dt(uprev) + qp_exact32(H, f, lbv, ubv)[0]

    P64 = [ko.rbf_lift(X, cx) for X in Xs]
    P32 = [rbf_lift32(X, cx) for X in Xs]
    u64, u32 = np.zeros((2, B)), np.zeros((2, B), dtype=F)
    for b in range(B):
        u64[0, b] = solve(np.float64, *model, P64[0][:, b], 0.0)
        u32[0, b] = solve(np.float32, *model, P32[0][:, b], 0.0)
    sh = ko.SharedEdmd(L, n, P0=SHARED_P0, barQ0=SHARED_P0)
    ua = _f32(u64[0])  # the input every side applies after step 0 (kmpc_set_applied_input on the handle): the hand-over stays exact
    sh.add(*ko.SharedEdmd.gram(P64[0], ua, P64[1], Xs[1]))
    A1, B1, C1 = sh.model()
    K32, C32 = gram_fit32(P32[0], P32[1], ua, Xs[1], 1.0 / SHARED_P0)
    for b in range(B):
        u64[1, b] = solve(np.float64, A1, B1, C1, P64[1][:, b], ua[b])
        u32[1, b] = solve(np.float32, K32[:, :L], K32[:, L:], C32, P32[1][:, b], ua[b])
    return dict(kw=kw, cx=cx, model=model, r=r, Xs=Xs, ua=ua, K=Ref("shared model [A B]", np.concatenate([A1, B1], axis=1), K32, CAP_MODEL),
                C=Ref("shared model C", C1, C32, CAP_MODEL), u=Ref("shared-model u_k, 2 steps", u64, u32, CAP_U))


# ====================================================================================================================
# 4. the companion: the reference arithmetic itself, on the CPU
# ====================================================================================================================
def all_refs():
    for s in MLP_SETS:
        yield mlp_case(*s)[2]
    for s in OFFSET_SETS:
        for form in ("psi0", "x_psi0"):
            yield offset_case(*s, form)[2]
    for s in RBF_SETS:
        for form in ("python", "matlab"):
            yield rbf_case(*s, form)[2]
    for name in STEP_SETS:
        d = step_case(name)
        for key in ("K", "C", "H", "f", "c", "qp"):
            if d[key] is not None:
                yield d[key]
                yield d[key].cut(slice(0, 5))
    for name in LOOP_KW:
        yield loop_case(name)["u"]
    for kind in PLANTS:
        for sw in (False, True):
            yield plant_case(kind, sw)[2]
    yield fit_case()["K"]
    yield fit_case()["C"]
    for key in ("K", "C", "u"):
        yield shared_case()[key]


def test_float32_oracle_deviations_stay_under_their_caps():
    """no GPU: the float32 evaluations really are float32 arrays, and every derived bound (8 x the float32 oracle's deviation from
    the float64 oracle, at least 16 float32 ulps) stays under its cap -- so no GPU case can pass on a bound that means nothing"""
    worst = {}
    for ref in all_refs():
        w32 = ref.U32 if isinstance(ref, KktRef) else ref.w32
        assert isinstance(w32, np.ndarray) and w32.dtype == np.float32, ref.name
        dev, bound = ref.deviation(), ref.bound()
        print("%-46s float32 oracle %.2e  bound %.2e  cap %.0e" % (ref.name, dev, bound, ref.cap))
        assert np.isfinite(dev) and bound <= ref.cap, (ref.name, dev, bound, ref.cap)
        worst[ref.name] = dev
    # `fun` of kmpc_mpc_solve is compared at the sequence the kernel returns; here at the float64 minimisers
    for shared in (0, 1):
        case = solve_case(shared)
        U = np.zeros((SOLVE_N, SOLVE_B))
        for b in range(SOLVE_B):
            A, Bm, Cm = case["models"][0 if shared else b]
            _, _, H, f, _ = ko.condense(A, Bm, Cm, case["psi"][:, b], case["r"], SOLVE_N, 100.0, 1e-4)
            U[:, b] = _f32(ko.qp_exact(H, f, -2.0, 2.0)[0])
        for with_pn in (False, True):
            ref = solve_fun_ref(case, U, with_pn)
            assert ref.w32.dtype == np.float32
            print("%-46s float32 oracle %.2e  bound %.2e  cap %.0e" % (ref.name, ref.deviation(), ref.bound(), ref.cap))
            assert ref.bound() <= ref.cap, (ref.name, ref.deviation())


def test_loop_restatement_is_the_oracle_controller():
    """no GPU: Loop(float64) above IS ko.OracleController(rls="gain") / ko.OracleDeltaUController on the closed-loop cases"""
    for name in LOOP_KW:
        c = loop_case(name)
        kw, (A0, B0, C0) = c["kw"], c["model"]
        lift = lambda x: ko.rbf_lift(x, c["cx"])
        for b in (0, STEP_B - 1):
            if kw["delta_u"]:
                ctl = ko.OracleDeltaUController(lift, kw["L"], 2, kw["N"], A0, B0, C0, cy0=kw["out_row0"], q=kw["out_rows"], lb=kw["lb"], ub=kw["ub"],
                                                umin=kw["umin"], umax=kw["umax"], P0=LOOP_P0, barQ0=LOOP_P0, Qw=kw["Qw"], Rw=kw["Rw"], c_skip_first=False)
            else:
                ctl = ko.OracleController(lift, kw["L"], 2, kw["N"], kw["lb"], kw["ub"], A0, B0, C0, P0=LOOP_P0, barQ0=LOOP_P0, Qw=kw["Qw"], Rw=kw["Rw"],
                                          output=kw["output"], rls="gain")
            for k in range(LOOP_STEPS):
                assert ctl.step(c["Xs"][k][:, b], c["r"])[0] == c["u"].w64[k, b], (name, b, k)


# ====================================================================================================================
# the GPU cases
# ====================================================================================================================
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def KM(torch_mod):
    from koopmpc import KoopmanMPC

    def make(**kw):
        m = KoopmanMPC(dtype=torch_mod.float32, device="cuda:0", **kw)
        code, text = m.rollout_plugin_status()
        assert code in (0, 2), (code, text)  # a built-in instantiation or no fused roll-out: no case compiles a plug-in
        return m

    return make


def _t(torch, a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda:0").contiguous()


def _np(t):
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n,hidden,layers,L", MLP_SETS)
def test_mlp_lift(torch_mod, KM, n, hidden, layers, L):
    """lift_mlp_kernel<float, ..> at B = 1, 16, 17 and 16400 (1025 tiles on a grid of 1024: block 0 runs the tile loop twice, and
    with two layers the NHH == 1 barrier between the tiles).  The 16400 states are all different, so a tile that reads the previous
    tile's activations gives a wrong value; first and last 16 columns must also be a B = 16 launch of those states bit for bit."""
    w, X, ref = mlp_case(n, hidden, layers, L)
    m = KM(n=n, L=L, N=2, batch=1, weights=w, hidden=hidden, layers=layers, output="lift")
    for B in MLP_BATCHES:
        got = _np(m.Encoder(_t(torch_mod, X[:, :B])))
        ref.cut((slice(None), slice(0, B))).check(got, "B = %d" % B)
    Bmax = max(MLP_BATCHES)
    big = _np(m.Encoder(_t(torch_mod, X)))
    first, last = _np(m.Encoder(_t(torch_mod, X[:, :16]))), _np(m.Encoder(_t(torch_mod, X[:, Bmax - 16:])))
    assert np.array_equal(big[:, :16], first) and np.array_equal(big[:, Bmax - 16:], last)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["psi0", "x_psi0"])
@pytest.mark.parametrize("n,hidden,layers,Lenc", OFFSET_SETS)
def test_mlp_lift_offset(torch_mod, KM, n, hidden, layers, Lenc, form):
    """psi(x) - psi(0) and [x; psi(x)] - [0; psi(0)] (hidden + 2n = 128 at (4, 120)), X[:, 0] = 0; the x rows bit for bit"""
    w, X, ref = offset_case(n, hidden, layers, Lenc, form)
    L = Lenc + (n if form == "x_psi0" else 0)
    m = KM(n=n, L=L, N=2, batch=1, weights=w, hidden=hidden, layers=layers, output="lift", lift_offset=form)
    got = _np(m.Encoder(_t(torch_mod, X)))
    ref.check(got, "B = %d" % X.shape[1])
    if form == "x_psi0":
        assert np.array_equal(got[:n], X.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["python", "matlab"])
@pytest.mark.parametrize("n,L", RBF_SETS)
def test_rbf_lift(torch_mod, KM, n, L, form):
    """lift_rbf_kernel<float>: the generic branch also at n = 2 (the bit-for-bit n == 2 branch is double only); the centres are
    among the states, so r = 0 occurs exactly: 0.0 in the MATLAB form, 0 * log(eps) = 0 in the Python form"""
    cx, X, ref = rbf_case(n, L, form)
    m = KM(n=n, L=L, N=2, batch=1, lift="rbf" if form == "python" else "rbf_matlab", centres=cx, output="lift")
    got = _np(m.Encoder(_t(torch_mod, X)))
    ref.check(got, "B = %d" % X.shape[1])
    at_centre = got[np.arange(L), RBF_B + np.arange(L)]
    assert np.all(at_centre == 0.0), at_centre


def _step_handle(KM, kw, B, cx, P0=P0, barQ0=BARQ0):
    return KM(n=2, L=kw["L"], N=kw["N"], batch=B, lift="rbf", centres=cx, output=kw["output"], P0=P0, barQ0=barQ0, Qw=kw["Qw"], Rw=kw["Rw"],
              lb=kw["lb"], ub=kw["ub"], umin=kw["umin"], umax=kw["umax"], delta_u=kw["delta_u"], out_row0=kw["out_row0"], out_rows=kw["out_rows"])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, STEP_B])
@pytest.mark.parametrize("name", list(STEP_SETS))
def test_step_kernels(torch_mod, KM, name, B):
    """the float step kernels of one kernel family: three successive Koopman_update calls on random transitions (after the first, P
    is no multiple of the identity any more) -> A, B, C against ko.rls_update_gain carried on the host; condense and condense_cost
    with its constant on a stable random model against ko.condense; qp_solve on H with cond(H) = 1e3, judged by its KKT residual,
    exact feasibility and status 0"""
    d = step_case(name)
    kw, sl = d["kw"], slice(0, B)
    m = _step_handle(KM, kw, B, d["cx"])
    for psi, u, psin, xn in d["trans"]:
        A, Bm, C = m.Koopman_update(psi[:, sl], u[sl], psin[:, sl], xn[:, sl])
    d["K"].cut(sl).check(np.concatenate([_np(A), _np(Bm)], axis=2), "B = %d" % B)
    if d["C"] is not None:
        d["C"].cut(sl).check(_np(C), "B = %d" % B)
    m.set_model(*d["model"])
    if kw["delta_u"]:
        m.set_applied_input(d["uprev"][sl])
    H, f, c = m.condense(d["psi"][:, sl], d["r"], return_const=True)
    H2, f2 = m.condense(d["psi"][:, sl], d["r"])
    assert torch_mod.equal(H, H2) and torch_mod.equal(f, f2)
    d["H"].cut(sl).check(_np(H), "B = %d" % B)
    d["f"].cut(sl).check(_np(f), "B = %d" % B)
    d["c"].cut(sl).check(_np(c), "B = %d" % B)
    qp = d["qp"].cut(sl)
    U, st, _ = m.qp_solve(qp.H, qp.f)
    qp.check(_np(U), _np(st), "B = %d" % B)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LOOP_KW))
def test_closed_loop_steps(torch_mod, KM, name):
    """kmpc_step for three steps on the two float32 routes that have no float64 core behind them (y = psi; delta-u) against the
    oracle's controllers; delta-u: umin <= u_k <= umax exactly"""
    c = loop_case(name)
    kw = c["kw"]
    m = _step_handle(KM, kw, STEP_B, c["cx"], P0=LOOP_P0, barQ0=LOOP_P0)
    m.set_model(*c["model"])
    u = np.zeros((LOOP_STEPS, STEP_B), dtype=np.float32)
    for k in range(LOOP_STEPS):
        u[k] = _np(m.step(_t(torch_mod, c["Xs"][k]), c["r"]))
        assert int(m.status.max().item()) == 0, k
    if kw["delta_u"]:
        assert np.all(u >= np.float32(kw["umin"])) and np.all(u <= np.float32(kw["umax"])), (u.min(), u.max())
        assert np.any(u == np.float32(kw["umax"]))  # (the case does run into its absolute range)
    else:
        assert np.all(u >= np.float32(kw["lb"])) and np.all(u <= np.float32(kw["ub"]))
    c["u"].check(u)


@pytest.mark.gpu
@pytest.mark.parametrize("with_pn", [False, True])
@pytest.mark.parametrize("shared", [0, 1])
def test_mpc_solve(torch_mod, KM, shared, with_pn):
    """kmpc_mpc_solve with per-trajectory models and with model_shared = 1, with and without PN_host, L = 8, N = 10, B = 17: `fun` is
    the oracle's cost at the returned sequence, U0 is U[0], the sequence is feasible and optimal (KKT as for qp_solve)"""
    case = solve_case(shared)
    L, N, B = SOLVE_L, SOLVE_N, SOLVE_B
    m = KM(n=2, L=L, N=N, batch=B, lift="rbf", centres=np.zeros((L, 2)))
    if shared:
        A, Bm, Cm = case["models"][0]
    else:
        A, Bm, Cm = [np.stack(v) for v in zip(*case["models"])]
    U, u0, st, fun = m.mpc_solve(A, Bm, Cm, case["psi"], case["r"], -2.0, 2.0, 100.0, 1e-4, PN_SOLVE if with_pn else None)
    U, u0, fun = _np(U), _np(u0), _np(fun)
    assert np.array_equal(u0, U[0])
    solve_fun_ref(case, U.astype(np.float64), with_pn).check(fun)
    Hs, fs, U32 = np.zeros((B, N, N)), np.zeros((B, N)), np.zeros((N, B), dtype=F)
    for b in range(B):
        mod = case["models"][0 if shared else b]
        _, _, Hs[b], fs[b], _ = ko.condense(*mod, case["psi"][:, b], case["r"], N, 100.0, 1e-4, PN=PN_SOLVE if with_pn else None)
        H3, f3, _ = condense32(*mod, case["psi"][:, b], case["r"], N, 100.0, 1e-4, PN=PN_SOLVE if with_pn else None)
        U32[:, b] = qp_exact32(H3, f3, -2.0, 2.0)
    KktRef("mpc_solve U", Hs, fs, np.full((B, N), -2.0), np.full((B, N), 2.0), U32).check(U, _np(st))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PLANTS)
def test_plant_step(torch_mod, KM, kind):
    """kmpc_plant_step: all three plants, nominal and switched parameters, the MATLAB Runge-Kutta step for Duffing and Van der Pol"""
    m = KM(n=2, L=8, N=10, batch=PLANT_B, lift="rbf", centres=np.zeros((8, 2)))
    for sw in (False, True):
        X, U, ref = plant_case(kind, sw)
        ref.check(_np(m.plant_step(kind, _t(torch_mod, X), U, switched=sw)))


@pytest.mark.gpu
def test_offline_fit(torch_mod, KM):
    """kmpc_offline_fit, M = 600, L = 8, ridge 1e-6, against the same Gram-form solve in float64 on the float32-rounded lifts"""
    c = fit_case()
    m = KM(n=2, L=FIT_L, N=10, batch=3, lift="rbf", centres=c["cx"])
    A, Bm, Cm = [_np(t) for t in m.offline_fit(c["X"], c["Y"], c["U"], ridge=FIT_RIDGE)]
    c["K"].check(np.concatenate([A, Bm], axis=1))
    c["C"].check(Cm)
    A2, B2, C2 = [_np(t) for t in m.get_model()]
    assert np.array_equal(A2[2], A) and np.array_equal(B2[2], Bm) and np.array_equal(C2[2], Cm)  # handed to every trajectory


@pytest.mark.gpu
def test_shared_model_steps(torch_mod, KM):
    """shared-model mode on a float32 handle (offered for KMPC_F32: Gram sums in float64 over float32 lifts, float kernels for the
    model, the condensed QP and the solve), L = 10, N = 20, delta-u, B = 37: two shared_steps against ko.SharedEdmd and the QP of
    ko.OracleDeltaUController per trajectory"""
    c = shared_case()
    kw = c["kw"]
    m = KM(n=2, L=kw["L"], N=kw["N"], batch=SHARED_B, lift="rbf", centres=c["cx"], output="Cx", P0=SHARED_P0, barQ0=SHARED_P0, Qw=kw["Qw"], Rw=kw["Rw"],
           lb=kw["lb"], ub=kw["ub"], umin=kw["umin"], umax=kw["umax"], delta_u=True, out_row0=1, out_rows=1)
    m.set_model(*c["model"])
    u = np.zeros((2, SHARED_B), dtype=np.float32)
    for k in range(2):
        u[k] = _np(m.shared_step(_t(torch_mod, c["Xs"][k]), c["r"]))
        assert int(m.status.max().item()) == 0, k
        if k == 0:
            m.set_applied_input(c["ua"])
    A, Bm, Cm = [_np(t) for t in m.shared_model()]
    c["K"].check(np.concatenate([A, Bm], axis=1))
    c["C"].check(Cm)
    assert np.all(u >= np.float32(kw["umin"])) and np.all(u <= np.float32(kw["umax"]))
    c["u"].check(u)
