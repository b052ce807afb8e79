"""The inputs of tests/test_gpu_shared_mode_options.py, judged from the oracle alone (no GPU).

The shared-model mode (kmpc_shared_local_gram / kmpc_shared_solve[_plant] / kmpc_shared_rollout) is compared with the oracle elsewhere only at
lambda = 1, y = C x and a reference that is one column tiled along the horizon and held from step to step.  The cases below set lambda < 1,
y = psi, and a reference that moves along the horizon, across rows and from step to step, at shapes that reach each of the three model
routes of csrc/api.hip shared_solve_impl.  This module holds the case table and the oracle side of the comparison (SharedOracle:
ko.mlp_lift / ko.rbf_lift -> ko.SharedEdmd(lam) -> ko.condense -> ko.qp_exact -> ko.plant_step / ko.tank_step), and proves from the oracle
alone, free-running over 8 steps with the plant switched from step 5 on, that the inputs are fit for the comparison:

  mix          at least 1/4 of the QPs have the whole sequence strictly inside the box (shared_fast_kernel's work) and at least 1/5 have
               some component on it (the solve-only kernel on the tableau T_in); du_tank counts the increments against the first-move box.
  conditioning cond(H) <= 1e6 for every QP (du_tank: the filter cond(H) < 1e10 of test_shared_model_delta_u_tank_vs_oracle, at least 3 B
               QPs left).
  model bound  beside SharedEdmd.model() (normal equations) the same discounted ridge regression is solved in square-root form:
               np.linalg.lstsq on the samples weighted by sqrt(lambda^age), stacked on the ridge rows I / sqrt(P0) (I / sqrt(barQ0) for C).
               That form does not square the condition number.  bound = 8 x max(two-form deviation, cond(G + I/P0) eps), relative to the
               largest element as test_shared_model_closed_loop_vs_oracle measures it: 8 is the margin tests/test_gpu_float32.py gives a
               kernel over a restatement, cond eps is the forward error of any backward-stable solve of the Gram system.  It must stay
               below 1e-7, the bound of the lambda = 1 test (with P0 = 1e4 the case L64 is not fit, cond 3e9: hence P0 = 100 there).
  sensitivity  on the case's own states three perturbations must each move some input by at least 1e-2, four orders above the 1e-6 the
               inputs are held to: the oracle with lambda = 1 from the third step on, the reference shifted one step along the horizon,
               the reference held at its first column.  Without this a test of lambda, or of a horizon index, proves nothing.

The moving reference at step k has the rows sin(0.3 j), 0.5 cos(0.2 j), j = k .. k + N - 1; y = psi takes the lift of those columns (L, N),
du_tank (one output row, C x row 1) the second row.  MLP weights random_mlp_weights(2, 100, 3, L, seed=7), RBF centres
4 RandomState(L + N).rand(L, 2) - 2, offline model koopmpc.synth.offline_edmd on the case's plant, start initial_states(B, seed=11).
du_tank takes weights_tank.npz, the offline fit, box and weights of test_shared_model_delta_u_tank_vs_oracle and starts from the absolute
values of those states (a tank level is not negative).

Measured here (printed by `python -m pytest tests/test_shared_mode_cases_cpu.py -s`):
    case      (L, N)    B   lift, plant   y      lam   box    Qw, Rw     P0    interior / on box   cond(H)  cond(G+I/P0)  two forms  model bound | moved by: lam = 1, shifted, held
    m2_17     (16, 12)  24  MLP, duffing  C x    0.95  +-2    10, 1      1e4   107 / 85            3.0e0    1.1e6         8.2e-13    1.9e-9      | 0.15   0.61   2.6
    m2_33     (20, 20)  24  MLP, duffing  C x    0.90  +-2    10, 1      1e4    77 / 115           5.4e1    1.3e6         2.3e-12    2.3e-9      | 0.38   0.49   3.5
    m2_33w    (32, 40)  16  MLP, duffing  C x    0.95  +-2    5, 1       1e4    88 / 40            4.6e0    1.6e6         4.0e-12    2.8e-9      | 0.48   0.18   1.9
    r3_short  (8, 10)   24  RBF, vdp      C x    0.95  +-6    100, 1     1e4   106 / 86            8.2e0    7.7e4         1.7e-12    1.4e-10     | 0.44   2.0    6.8
    r3_wide   (40, 12)  24  MLP, duffing  C x    0.95  +-2    10, 1      1e4   108 / 84            3.3e0    2.7e6         6.3e-12    4.7e-9      | 0.17   0.50   2.6
    psi8      (8, 10)   24  RBF, vdp      psi    0.95  +-6    100, 1     1e4    67 / 125           4.6e2    3.8e4         1.8e-12    6.7e-11     | 0.95   5.7    12
    psi20     (20, 20)  24  MLP, duffing  psi    0.95  +-2    1000, 1    1e4    78 / 114           1.2e1    1.4e6         2.5e-12    2.5e-9      | 0.18   0.44   3.1
    L64       (64, 10)  24  RBF, duffing  C x    0.95  +-2    20, 1      100    84 / 108           3.7e0    3.2e7         9.1e-10    5.6e-8      | 0.34   0.91   3.7
    du_tank   (10, 15)  24  tank, tank    C x 1  0.95  +-0.5  10, 0.3    1e4    95 / 97            6.4e3    3.0e5         1.1e-11    5.3e-10     | 0.038  0.38   1.0
du_tank: Rw = 0.3 instead of the 1e-3 of test_shared_model_delta_u_tank_vs_oracle, with which 7 of the 192 increment sequences are interior
(Rw = 0.1: 61, 1: 152); every one of its QPs has cond(H) < 1e10, so all 192 are compared.  The variants the GPU module also runs (the
reference of step 0 held over a roll-out; m2_17 and psi8 with terminal_block()) stay below cond(H) 5.7e2 and a model bound of 5.7e-8.
"""
import functools
import os

import numpy as np
import pytest

from oracle import koopman_oracle as ko

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEPS, SWITCH = 8, 5

# name -> shape, lift, plant, output, forgetting factor, box, weights, RLS scales; `route` is what csrc/api.hip takes at that shape
CASES = {
    "m2_17": dict(L=16, N=12, B=24, lift="mlp", plant="duffing", output="Cx", lam=0.95, lb=-2.0, ub=2.0, Qw=10.0, Rw=1.0, P0=1e4,
                  route="shared_model2_kernel<17>, shared_fast_kernel 2 tiles"),
    "m2_33": dict(L=20, N=20, B=24, lift="mlp", plant="duffing", output="Cx", lam=0.90, lb=-2.0, ub=2.0, Qw=10.0, Rw=1.0, P0=1e4,
                  route="shared_model2_kernel<33>, shared_fast_kernel 2 tiles"),
    "m2_33w": dict(L=32, N=40, B=16, lift="mlp", plant="duffing", output="Cx", lam=0.95, lb=-2.0, ub=2.0, Qw=5.0, Rw=1.0, P0=1e4,
                   route="shared_model2_kernel<33>, shared_fast_kernel 3 tiles"),
    "r3_short": dict(L=8, N=10, B=24, lift="rbf", plant="vdp", output="Cx", lam=0.95, lb=-6.0, ub=6.0, Qw=100.0, Rw=1.0, P0=1e4,
                     route="shared_model_kernel (N < 12)"),
    "r3_wide": dict(L=40, N=12, B=24, lift="mlp", plant="duffing", output="Cx", lam=0.95, lb=-2.0, ub=2.0, Qw=10.0, Rw=1.0, P0=1e4,
                    route="shared_model_kernel (L > 33), shared_fast_kernel 4 tiles"),
    "psi8": dict(L=8, N=10, B=24, lift="rbf", plant="vdp", output="lift", lam=0.95, lb=-6.0, ub=6.0, Qw=100.0, Rw=1.0, P0=1e4,
                 route="shared_solve_kernel + shared_condense_kernel"),
    "psi20": dict(L=20, N=20, B=24, lift="mlp", plant="duffing", output="lift", lam=0.95, lb=-2.0, ub=2.0, Qw=1000.0, Rw=1.0, P0=1e4,
                  route="shared_solve_kernel + shared_condense_kernel, 80 KB of LDS (above the 64 KB a kernel has without the attribute)"),
    "L64": dict(L=64, N=10, B=24, lift="rbf", plant="duffing", output="Cx", lam=0.95, lb=-2.0, ub=2.0, Qw=20.0, Rw=1.0, P0=100.0,
                route="shared_solve_kernel (133 KB of LDS) + shared_condense_kernel by shape: L + 1 > 64"),
    # (Rw: with the 1e-3 of test_shared_model_delta_u_tank_vs_oracle 7 of the 192 increment sequences are interior; 0.1 gives 61, 0.3 95, 1 152)
    "du_tank": dict(L=10, N=15, B=24, lift="tank", plant="tank", output="Cx", lam=0.95, lb=-0.5, ub=0.5, Qw=10.0, Rw=0.3, P0=1e4,
                    barQ0=1e4, delta_u=True, umin=-8.0, umax=8.0, route="shared_model2_kernel<17>, L~ = 11"),
}
INTERIOR_SHARE, ON_BOX_SHARE = 1.0 / 4.0, 1.0 / 5.0
COND_MAX = 1e6           # cond(H) of every QP: the minimiser is then unique to far below the 1e-6 bound on the inputs
COND_DU = 1e10           # du_tank: the filter of test_shared_model_delta_u_tank_vs_oracle
MODEL_BOUND_MAX = 1e-7   # the model bound of test_shared_model_closed_loop_vs_oracle; a case bound above it says the inputs are unfit
MARGIN = 8.0             # what tests/test_gpu_float32.py gives a kernel over a restatement
INPUT_BOUND = 1e-6       # the project's bound for inputs against qp_exact
SENSITIVITY_MIN = 1e-2   # what each perturbation must move some input by
EPS = float(np.finfo(np.float64).eps)


def terminal_block(case):
    """A symmetric positive definite P_N (q, q) for kmpc_set_terminal_weight: Qw (I + M M' / q), M uniform in [0, 1)."""
    c = CASES[case]
    q = c["L"] if c["output"] == "lift" else 2
    M = np.random.RandomState(q).rand(q, q)
    return c["Qw"] * (np.eye(q) + M @ M.T / q)


def moving_reference(k, N):
    j = np.arange(k, k + N, dtype=np.float64)
    return np.stack([np.sin(0.3 * j), 0.5 * np.cos(0.2 * j)])


def model_deviation(got, want):
    """The measure of test_shared_model_closed_loop_vs_oracle: [A B] relative to its largest element, C to max(1e-3, |C|max); C is left
    out where either side has none (y = psi)."""
    scale = max(np.abs(want[0]).max(), np.abs(want[1]).max())
    d = max(np.abs(got[0] - want[0]).max(), np.abs(np.reshape(got[1], -1) - np.reshape(want[1], -1)).max()) / scale
    if got[2] is not None and want[2] is not None:
        d = max(d, np.abs(got[2] - want[2]).max() / max(1e-3, np.abs(want[2]).max()))
    return float(d)


@functools.lru_cache(maxsize=None)
def setup(case):
    """lift, offline model and initial states of a case: (lift_fn, constructor options for KoopmanMPC, (A0, B0, C0), X0)."""
    from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights, vdp_rk4

    c = CASES[case]
    L, N, B = c["L"], c["N"], c["B"]
    X0 = initial_states(B, seed=11)
    if c["lift"] == "tank":
        npz = np.load(os.path.join(GOLDEN, "weights_tank.npz"))
        w = ko.load_mlp_weights(npz)
        lift_fn = lambda x: ko.mlp_lift(w, x)
        kw = dict(weights=w, layers=2)
        # the offline fit of test_shared_model_delta_u_tank_vs_oracle: 100 x 100 tank samples, pinv
        rng = np.random.RandomState(L + N)
        Ub = 10 * rng.rand(100, 100) - 5
        xc = np.maximum(4 * rng.rand(2, 100) - 2, 0.0)
        Xs, Ys, Us = [], [], []
        for i in range(100):
            xn = ko.tank_step(xc, Ub[i])
            Xs.append(xc); Ys.append(xn); Us.append(Ub[i][None, :]); xc = xn
        Xd, Yd, Ud = np.concatenate(Xs, 1), np.concatenate(Ys, 1), np.concatenate(Us, 1)
        V = np.concatenate([lift_fn(Xd), Ud], 0)
        M = np.concatenate([lift_fn(Yd), Xd], 0) @ V.T @ np.linalg.pinv(V @ V.T)
        model0 = (M[:L, :L].copy(), M[:L, L:].copy(), M[L:, :L].copy())
        return lift_fn, kw, model0, np.abs(X0)
    if c["lift"] == "mlp":
        w = random_mlp_weights(2, 100, 3, L, seed=7)
        lift_fn = lambda x: ko.mlp_lift(w, x)
        kw = dict(weights=w, layers=3)
    else:
        cx = 4 * np.random.RandomState(L + N).rand(L, 2) - 2
        lift_fn = lambda x: ko.rbf_lift(x, cx)
        kw = dict(lift="rbf", centres=cx)
    model0 = offline_edmd(lift_fn, plant=duffing_rk4 if c["plant"] == "duffing" else vdp_rk4)
    return lift_fn, kw, model0, X0


def handle_options(case):
    """Keyword arguments of KoopmanMPC for the case (the GPU module's side of setup())."""
    c = CASES[case]
    kw = dict(n=2, L=c["L"], N=c["N"], batch=c["B"], output=c["output"], lam=c["lam"], P0=c["P0"], barQ0=c.get("barQ0", 100.0),
              Qw=c["Qw"], Rw=c["Rw"], lb=c["lb"], ub=c["ub"])
    if c.get("delta_u"):
        kw.update(delta_u=True, out_row0=1, out_rows=1, umin=c["umin"], umax=c["umax"])
    kw.update(setup(case)[1])
    return kw


class SharedOracle:
    """The oracle side of a shared-model loop, one step at a time on states the caller gives: solve(X, r) updates the pooled model with
    the transitions that ended in X and returns the exact input sequences (N, B) of the condensed QPs; commit(u) names the inputs that
    were applied (they are what the next update regresses on; in the delta-u form they are absolute)."""

    def __init__(self, case, PN=None):
        c = self.c = CASES[case]
        self.lift, _, model0, _ = setup(case)
        self.model = tuple(np.array(m) for m in model0)
        self.sh = ko.SharedEdmd(c["L"], 2, c["P0"], c.get("barQ0", 100.0), c["lam"])
        self.PN, self.du = PN, bool(c.get("delta_u"))
        self.uabs = np.zeros(c["B"])
        self.prev, self.samples, self.k = None, [], 0
        self.Psi = None

    def reference(self, k, mode="moving"):
        c = self.c
        r2 = moving_reference(k + 1 if mode == "shifted" else k, c["N"])
        if mode == "held":
            r2 = np.tile(r2[:, :1], (1, c["N"]))
        if c["output"] == "lift":
            return self.lift(r2)
        return r2[1:2].copy() if self.du else r2

    def plant_step(self, X, u, k):
        if self.c["plant"] == "tank":
            return ko.tank_step(X, u, switched=(k >= SWITCH))
        return ko.plant_step(self.c["plant"], X, u, switched=(k >= SWITCH))

    def box(self, b):
        c, N = self.c, self.c["N"]
        lbv, ubv = np.full(N, c["lb"]), np.full(N, c["ub"])
        if self.du:  # the first-move box (Tank_System.m:182-188)
            lbv[0] = max(c["lb"], c["umin"] - self.uabs[b]); ubv[0] = min(c["ub"], c["umax"] - self.uabs[b])
        return lbv, ubv

    def qps(self, model, Psi, r):
        """H (shared) and the exact minimisers (N, B) of the condensed QPs of `model` at the lifted states Psi."""
        c = self.c
        A, Bm, C = model
        N, Bn = c["N"], Psi.shape[1]
        U, H = np.zeros((N, Bn)), None
        ctl = ko.OracleDeltaUController(self.lift, c["L"], 2, N, A, Bm, C) if self.du else None
        for b in range(Bn):
            if self.du:
                ctl.u = float(self.uabs[b])
                At, Bt, Co, xt = ctl.qp(Psi[:, b])
                _, _, H, f, _ = ko.condense(At, Bt, Co, xt, r, N, c["Qw"], c["Rw"], PN=self.PN)
            else:
                _, _, H, f, _ = ko.condense(A, Bm, None if c["output"] == "lift" else C, Psi[:, b], r, N, c["Qw"], c["Rw"], PN=self.PN)
            lbv, ubv = self.box(b)
            U[:, b] = ko.qp_exact(H, f, lbv, ubv)[0]
        return H, U

    def update(self, X):
        """lift X; with a previous transition, pool the batch's transitions and solve for the model (both forms are available after it)"""
        self.Psi = Psi = self.lift(X)
        if self.prev is not None:
            self.sh.add(*ko.SharedEdmd.gram(self.prev[0], self.prev[1], Psi, X))
            self.samples.append((self.prev[0], self.prev[1], Psi, np.array(X)))
            self.model = self.sh.model()
        return Psi

    def solve(self, X, r):
        Psi = self.update(X)
        return self.qps(self.model, Psi, r)

    def first_inputs(self, U):
        return self.uabs + U[0] if self.du else U[0].copy()

    def commit(self, u):
        self.prev = (self.Psi, np.array(u, dtype=np.float64))
        if self.du:
            self.uabs = np.array(u, dtype=np.float64)
        self.k += 1

    # ---- the model bound
    def sqrt_form_model(self):
        """The discounted ridge regression of SharedEdmd.model() from the samples themselves: rows sqrt(lambda^age) [psi; u]' stacked on
        I / sqrt(P0) (I / sqrt(barQ0) for C), least squares by np.linalg.lstsq -- the Gram matrix is never formed."""
        c, L = self.c, self.c["L"]
        n_s = len(self.samples)
        Zs, Ys, Xs = [], [], []
        for i, (Psi, u, PsiN, XN) in enumerate(self.samples):
            wgt = np.sqrt(c["lam"] ** (n_s - 1 - i))
            Zs.append(wgt * np.concatenate([Psi, u[None, :]], 0)); Ys.append(wgt * PsiN); Xs.append(wgt * XN)
        Z, Y, Xn = np.concatenate(Zs, 1), np.concatenate(Ys, 1), np.concatenate(Xs, 1)
        p = L + 1
        K = np.linalg.lstsq(np.concatenate([Z.T, np.eye(p) / np.sqrt(c["P0"])], 0), np.concatenate([Y.T, np.zeros((p, L))], 0), rcond=None)[0].T
        Cm = np.linalg.lstsq(np.concatenate([Z[:L].T, np.eye(L) / np.sqrt(c.get("barQ0", 100.0))], 0),
                             np.concatenate([Xn.T, np.zeros((L, 2))], 0), rcond=None)[0].T
        return K[:, :L], K[:, L:], Cm

    def model_terms(self):
        """(two-form deviation, cond(G + I/P0)) of the current model; (0, 1) before the first transition"""
        if not self.samples:
            return 0.0, 1.0
        want = self.model if self.c["output"] != "lift" else (self.model[0], self.model[1], None)
        return model_deviation(self.sqrt_form_model(), want), float(np.linalg.cond(self.sh.G + np.eye(self.sh.p) / self.c["P0"]))


def model_bound(dev, cond_g):
    return MARGIN * max(dev, cond_g * EPS)


@functools.lru_cache(maxsize=None)
def oracle_alone(case, held=False, terminal=False, sensitivity=False):
    """The case free-running on the oracle over STEPS steps.  held: the reference of step 0 at every step (what a roll-out takes);
    terminal: with terminal_block(case); sensitivity: also the three perturbed solves on the same states."""
    c = CASES[case]
    B, N = c["B"], c["N"]
    orc = SharedOracle(case, PN=terminal_block(case) if terminal else None)
    alt = ko.SharedEdmd(c["L"], 2, c["P0"], c.get("barQ0", 100.0), c["lam"])  # (lambda = 1 from the third step on)
    X = setup(case)[3].copy()
    out = dict(total=0, interior=0, on_box=0, cond=0.0, cond_g=0.0, dev=0.0, compared=0, s_lam=0.0, s_shift=0.0, s_held=0.0)
    for k in range(STEPS):
        r = orc.reference(0 if held else k)
        prev = orc.prev
        H, U = orc.solve(X, r)
        cond = float(np.linalg.cond(H))
        out["cond"] = max(out["cond"], cond)
        if cond < (COND_DU if orc.du else COND_MAX):
            out["compared"] += B
        for b in range(B):
            lbv, ubv = orc.box(b)
            inside = bool(np.all((U[:, b] > lbv) & (U[:, b] < ubv)))
            assert inside or bool(np.any((U[:, b] == lbv) | (U[:, b] == ubv)))
            out["interior"] += inside; out["on_box"] += not inside; out["total"] += 1
        dev, cond_g = orc.model_terms()
        out["dev"], out["cond_g"] = max(out["dev"], dev), max(out["cond_g"], cond_g)
        if sensitivity:
            if prev is not None:
                if k >= 2:
                    alt.lam = 1.0
                alt.add(*ko.SharedEdmd.gram(prev[0], prev[1], orc.Psi, X))
                out["s_lam"] = max(out["s_lam"], float(np.abs(orc.qps(alt.model(), orc.Psi, r)[1] - U).max()))
            out["s_shift"] = max(out["s_shift"], float(np.abs(orc.qps(orc.model, orc.Psi, orc.reference(k, "shifted"))[1] - U).max()))
            out["s_held"] = max(out["s_held"], float(np.abs(orc.qps(orc.model, orc.Psi, orc.reference(k, "held"))[1] - U).max()))
        u = orc.first_inputs(U)
        orc.commit(u)
        X = orc.plant_step(X, u, k)
    out["model_bound"] = model_bound(out["dev"], out["cond_g"])
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_inputs_meet_the_conditions_of_the_case(case):
    c, res = CASES[case], oracle_alone(case, sensitivity=True)
    print("%-8s (%2d, %2d) B=%2d lam=%.2f: interior %3d / %3d, on the box %3d, max cond(H) %.1e, cond(G + I/P0) %.1e, two forms %.1e, "
          "model bound %.1e | moved by lambda = 1: %.2e, shifted reference: %.2e, held reference: %.2e"
          % (case, c["L"], c["N"], c["B"], c["lam"], res["interior"], res["total"], res["on_box"], res["cond"], res["cond_g"], res["dev"],
             res["model_bound"], res["s_lam"], res["s_shift"], res["s_held"]))
    assert res["interior"] + res["on_box"] == res["total"] == c["B"] * STEPS
    assert res["interior"] >= INTERIOR_SHARE * res["total"]
    assert res["on_box"] >= ON_BOX_SHARE * res["total"]
    if c.get("delta_u"):
        assert res["compared"] >= 3 * c["B"]
    else:
        assert res["cond"] <= COND_MAX
    assert res["model_bound"] < MODEL_BOUND_MAX
    assert min(res["s_lam"], res["s_shift"], res["s_held"]) >= SENSITIVITY_MIN


@pytest.mark.parametrize("case,held,terminal", [(c, True, False) for c in CASES] + [("m2_17", False, True), ("psi8", False, True)])
def test_variants_keep_conditioning_and_model_bound(case, held, terminal):
    """The two variants the GPU module also runs -- the reference of step 0 held over a roll-out, a terminal block with the moving
    reference -- stay inside the conditioning and the model bound (they visit other states than the case itself)."""
    c, res = CASES[case], oracle_alone(case, held=held, terminal=terminal)
    print("%-8s %s: interior %3d / %3d, max cond(H) %.1e, model bound %.1e"
          % (case, "held reference" if held else "terminal block", res["interior"], res["total"], res["cond"], res["model_bound"]))
    if c.get("delta_u"):
        assert res["compared"] >= 3 * c["B"]
    else:
        assert res["cond"] <= COND_MAX
    assert res["model_bound"] < MODEL_BOUND_MAX


def test_the_refused_shape_is_the_one_the_formula_names():
    """The LDS the condensed QP of the two-kernel route asks for (csrc/kernels.h shared_condense_lds_bytes), in the figures the GPU
    module's refusal test and the case table rely on: y = psi at (30, 30) is past 160 KiB, psi20 is past the 64 KiB a kernel has without
    the attribute and inside 160 KiB, L64 fits."""
    lds = lambda L, q, N: (L * L + L + q * L + (N + 1) * q * L + 2 * N * q) * 8
    assert lds(30, 30, 30) == 252240 > 160 * 1024
    assert 64 * 1024 < lds(20, 20, 20) == 80160 <= 160 * 1024
    assert lds(8, 8, 10) <= 64 * 1024 and lds(64, 2, 10) <= 64 * 1024
    assert (65 * 66 + 66 * 65 + 65 * 65 + 64 * 65) * 8 == 135720 <= 160 * 1024  # shared_solve_kernel with its refinement step at L = 64, n = 2
