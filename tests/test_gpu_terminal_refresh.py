"""The refreshed terminal blocks (kmpc_set_terminal_refresh) on every route that refreshes them.

THE DETECTOR.  kmpc_condense forms H, f with the handle's current per-trajectory blocks, so after any call the blocks a launch left are
read back through the condensed QP of an arbitrary fixed (psi, r): for every trajectory of the batch, H and f must equal
ko.condense(A[b], B[b], Co_b, psi[:, b], r, N, PN=Co* solve_dare(A*, B*, Qd, Rd, maxiter, eps) Co*') with the device's own final model
(A, B, C) and the device's own model (A*, B*, C*) right after the step that last refreshed -- 1e-9 relative where the oracle's Riccati
iteration converged, 1e-6 where it ran into maxiter (the tolerances of test_terminal_from_dare; rounding is amplified along a diverging
iteration).  Both sides start from identical inputs, only the order of summation differs, and an active box plays no part.

CONTROLS.  A twin handle walks the same loop with kmpc_step: its whole Useq against the oracle's minimiser (1e-6; gain-form RLS driven
by the device's applied inputs and states, solve_dare + terminal_block at the refresh steps), its U0 against the launch's U_log (1e-9),
the states against the oracle's plant (1e-9).  Steps with cond(H) >= 1e9 are counted, not compared.

CASES AND THE CODE PATHS THEY EXECUTE (rollout_kernel.hip TERM branch, api.hip step_impl / rollout_fused):
  psi12     (12, 12) y = psi, MLP 3 layers, B = 20, every 1, 6 steps split 4 + 2         dense-block form with the identity for Q_ == L_
  lds36     (36, 24) q = 2, MLP 3 layers, B = 20, every 3, 8 steps split 4 + 3 + 1       dense-block form, Kb / Cb reads (LDS step, L + 2 > 32);
                                                                                         term_count carried from call to call; held blocks
  row1/row0 (16, 24) q = 1, out_row0 = 1 / 0, MLP 2 layers, B = 32, every 2, 9 = 5 + 4   wave-image form with cy0 != 0 and q = 1; the second
                                                                                         call runs under the placement table of the first
  rbf26     (26, 34) q = 2, RBF from the offline samples, B = 20, every 1, 5 steps       fused eight-wave RBF kernel; the twin's kmpc_step is the
                                                                                         per-step route (RLS launch, dare_kernel, QP launch)
  rbf26r    the same set, estimator restarted from a contractive start model             ... with well-conditioned QPs (rbf26 has none: below)
  four64    (64, 50) hidden 128, threads = 256, B = 5, every 2, 5 steps                  per-step route of a four-wave set, once as kmpc_step +
                                                                                         kmpc_plant_step, once as kmpc_rollout (3 + 1 + 1) with the
                                                                                         plant inside the step kernel (a1.plant = -1)
  n3        n = 3, (20, 20), rows 1..2 of C, B = 5, every 2, 5 steps, host plant         per-step route, n != 2
  du10      tank set (10, 20), q = 1, row 1, delta-u, B = 5, every 2, 6 steps            delta-u (see below)
  off       row1's set, kmpc_set_online_update(h, 0), every 1, 3 steps                   the refresh without the online update
  max7      row1's set, maxiter = 7, eps = 1e-12, every 1, 3 steps                       maxiter reached on purpose (every refresh stops at 7)
  ckpt      row1's set, state_dict / load_state_dict while armed, every 1 and 2          a checkpoint taken while the refresh is armed

DELTA-U.  kmpc_set_terminal_refresh ACCEPTS a delta-u handle.  The Riccati iteration runs on the un-augmented [A B] (dare_blocks passes
dK; wave_dare reads the same rows), the q x q block Co P Co' enters the augmented condensed QP ([A B; 0 1], [B; 1], [Co 0]) as the
terminal block of its output weight.  The tank set (10, 20, 1) has a fused roll-out, so kmpc_step of this MLP set is a one-step launch
of the TERM plug-in and kmpc_rollout one launch; both are held here.

CHECKPOINTS.  The blob carries the blocks, not the period's count.  kmpc_set_terminal_refresh zeroes the count and kmpc_state_import
leaves it alone: a freshly armed handle refreshes at its FIRST step after the import and at every `every`-th after it, whatever the
exporter's phase was; the steps in between use the blocks of the blob.  A blob with ONE block (or none) imported into an armed handle:
kmpc_state_import hands that block (or Qw I) to every trajectory -- before this module it filled trajectory 0 only and a fused launch
read B blocks, B - 1 of them stale (test_checkpoint_with_one_shared_block_into_an_armed_handle).

INPUTS.  A contractive start model A = randn 0.5 / sqrt(L), B, C = 0.3 randn (the RBF set: the offline fit), Qd = 10 I, Rd = 0.01, bounds
+-2 (delta-u: increments +-0.5), x0 ~ U[-0.5, 0.5]^n (tank levels U[0, 1]), r = the rows of [1; 0] the output map selects (psi([1; 0]) for
y = psi; row1: the zero row), or a constant where that reference leaves the conditions unmet from the oracle alone (row0 0.4: with 1 the
box is active at 7 steps of 8; four64, du10 0.5; off, max7 0.2).  rbf26 as the issue states it -- continued from the offline samples --
cannot meet them: the fitted model has spectral radius 0.9985, the Riccati iteration is still growing at 500 iterations (blocks of
1e11) and every H is numerically singular; its blocks, split and plant are held, the Useq and route controls are rbf26r's.  A trajectory
leaves a comparison between two routes at its first numerically singular QP (_route_dev).  test_case_inputs (no GPU) asserts from
the oracle loop alone, self-driven, over every trajectory and step of a case: at most a quarter of the steps left out (cond(H) >= 1e9),
in at least a third of the compared steps the oracle's Useq moves by more than 1e-4 when the block is replaced by Qw I, and in at most
a quarter of the refreshes the Riccati iteration reaches maxiter (max7: all of them, by design).  Measured shares (self-driven oracle):

  case     steps  left out  Useq moved / compared  maxiter reached / refreshes
  psi12      120         0        98 / 120                 7 / 120
  lds36      160         0        94 / 160                 3 / 60
  row1       288         0       123 / 288                18 / 160
  row0       288         0        97 / 288                17 / 160
  rbf26      100       100         0 / 0                 100 / 100     (the case as stated: conditions NOT met, see test_case_inputs)
  rbf26r     100        10        73 / 90                  0 / 100
  four64      25         0        16 / 25                  1 / 15
  n3          25         0        13 / 25                  0 / 15
  du10        30         0        12 / 30                  0 / 15
  off         96         0        96 / 96                  0 / 96
  max7        96         0        62 / 96                 65 / 96      (by design; the 32 refreshes of the start model all stop at 7)

MEASURED ON THE MI355X (worst over every trajectory, step and detector call; block = the detector's deviation of H or f as a FRACTION
of its tolerance, 1e-9 or 1e-6: 1.4e-06 is 1.4e-15 relative at 1e-9; split = the split roll-out against one launch of a twin):
  case     block     Useq vs oracle  U0 vs launch  x vs plant  split     left out
  psi12    1.41e-06  8.07e-13        0.00e+00      5.55e-17    0.00e+00    0 / 120
  lds36    1.48e-06  1.99e-10        0.00e+00      5.55e-17    0.00e+00    0 / 160
  row1     1.13e-06  4.17e-11        0.00e+00      5.55e-17    1.11e-14    0 / 288
  row0     2.98e-06  2.92e-10        0.00e+00      1.11e-16    0.00e+00    0 / 288
  rbf26    3.02e-03  (none)          1.14 (n/a)    1.11e-16    0.00e+00  100 / 100
  rbf26r   9.95e-06  1.97e-07        1.13e-13      5.55e-17    0.00e+00   10 / 100
  du10     1.95e-06  1.58e-11        0.00e+00      1.11e-16    0.00e+00    0 / 30
  max7     1.21e-06  7.25e-12        0.00e+00      5.55e-17    0.00e+00    0 / 96
  four64   1.44e-06  6.99e-12        0.00e+00      5.55e-17    (kmpc_rollout against kmpc_step + kmpc_plant_step: 0.00e+00)
  n3       8.09e-07  1.14e-12        -             1.11e-16
  off      7.14e-07  2.60e-14        2.78e-16      5.55e-17    (against the twin without the refresh: 0.00e+00)
  ckpt     1.91e-06  (exporter and importer bit for bit at every = 1)
  ckpt3    1.09e-06  (held step of the importer against the exporter's: 0.00e+00)
"""
import functools
import os

import numpy as np
import pytest

from oracle import koopman_oracle as ko

G = os.path.join(os.path.dirname(__file__), "golden")
RD = 0.01


# ====================================================================================================================
# the cases: everything that does not involve the device
# ====================================================================================================================
_ROW = dict(L=16, N=24, layers=2, out_rows=1, B=32, every=2, steps=9, split=(5, 4), seed=316)
CASES = {
    "psi12": dict(L=12, N=12, layers=3, output="lift", B=20, every=1, steps=6, split=(4, 2), seed=112),
    "lds36": dict(L=36, N=24, layers=3, B=20, every=3, steps=8, split=(4, 3, 1), seed=136),
    "row1": dict(_ROW, out_row0=1),
    "row0": dict(_ROW, out_row0=0, ref=0.4),
    "rbf26": dict(L=26, N=34, lift="rbf", B=20, every=1, steps=5, split=(5,), seed=126, plant="vdp"),
    "rbf26r": dict(L=26, N=34, lift="rbf", B=20, every=1, steps=5, split=(5,), seed=126, plant="vdp", restart=True),
    "four64": dict(L=64, N=50, layers=3, hidden=128, threads=256, B=5, every=2, steps=5, split=(3, 1, 1), seed=164, ref=0.5),
    "n3": dict(n=3, L=20, N=20, layers=3, out_rows=2, out_row0=1, B=5, every=2, steps=5, split=None, seed=320, plant="host"),
    "du10": dict(L=10, N=20, layers=2, out_rows=1, out_row0=1, B=5, every=2, steps=6, split=(3, 1, 1, 1), seed=210, plant="tank", delta_u=True,
                 lb=-0.5, ub=0.5, Qw=10.0, Rw=1e-3, P0=1e4, barQ0=1e4, ref=0.5),
    "off": dict(_ROW, out_row0=1, every=1, steps=3, split=(3,), update=False, ref=0.2),
    "max7": dict(_ROW, out_row0=1, every=1, steps=3, split=(3,), maxiter=7, eps=1e-12, ref=0.2),
}


class _Set:
    """One case: constructor arguments, oracle lift, start model, reference, initial states, and the oracle's pieces."""

    def __init__(self, name, **c):
        from koopmpc.synth import offline_data, random_mlp_weights, vdp_rk4

        self.name = name
        self.n, self.L, self.N, self.B = c.get("n", 2), c["L"], c["N"], c["B"]
        n, L, N = self.n, self.L, self.N
        self.output = c.get("output", "Cx")
        self.rows, self.row0 = c.get("out_rows", 0), c.get("out_row0", 0)
        self.q = L if self.output == "lift" else (self.rows or n)
        self.every, self.steps, self.split = c["every"], c["steps"], c["split"]
        self.maxiter, self.eps = c.get("maxiter", 500), c.get("eps", 0.01)
        self.du, self.update = c.get("delta_u", False), c.get("update", True)
        self.lb, self.ub = c.get("lb", -2.0), c.get("ub", 2.0)
        self.umin, self.umax = -8.0, 8.0
        self.Qw, self.Rw, self.P0, self.barQ0 = c.get("Qw", 100.0), c.get("Rw", 1e-4), c.get("P0", 1e4), c.get("barQ0", 100.0)
        self.plant = c.get("plant", "duffing")
        self.rbf = c.get("lift", "mlp") == "rbf"
        self.sw = c.get("switched", False)  # the plant with the parameters the reference switches to (vanderpol.py:923-931), throughout
        self.Qd = 10.0 * np.eye(L)
        self.status_ok = 1 if (self.output == "lift" or c.get("lift", "mlp") == "rbf") else 0  # (y = psi / RBF: ill-conditioned H, the cap may be met)
        rng = np.random.RandomState(c["seed"])
        kw = dict(n=n, L=L, N=N, output=self.output, lb=self.lb, ub=self.ub, Qw=self.Qw, Rw=self.Rw, P0=self.P0, barQ0=self.barQ0)
        if self.rows:
            kw.update(out_rows=self.rows, out_row0=self.row0)
        if "threads" in c:
            kw.update(threads=c["threads"])
        if self.du:
            kw.update(delta_u=True, umin=self.umin, umax=self.umax)
        if self.rbf:  # (as vanderpol_RBF.py: centres from the data, the estimator continues from the offline samples, :434-438)
            Xo, Yo, Uo = offline_data(plant=(lambda x, u: ko.plant_step("vdp", x, u, switched=True)) if self.sw else vdp_rk4)
            cx = Xo[:, np.random.RandomState(0).choice(Xo.shape[1], L, replace=False)].T.copy()
            kw.update(lift="rbf", centres=cx)
            self.lift = lambda x: ko.rbf_lift(x, cx)
            self.offline = (Xo, Yo, Uo)
            PX, PY = self.lift(Xo), self.lift(Yo)
            Z = np.concatenate([PX, Uo[None, :]], 0)
            gP = np.linalg.inv(Z @ Z.T); gK = (PY @ Z.T) @ gP
            gQ = np.linalg.inv(PX @ PX.T); gC = (Xo @ PX.T) @ gQ
            self.g0 = (gK, gP, gC, gQ)
            self.A0, self.B0, self.C0 = gK[:, :-1].copy(), gK[:, -1:].copy(), gC.copy()
            if c.get("restart"):  # (the estimator restarted from a contractive start model, as the MLP sets)
                self.g0, self.offline = None, None
                self.A0, self.B0, self.C0 = rng.randn(L, L) * 0.5 / np.sqrt(L), rng.randn(L, 1) * 0.3, rng.randn(n, L) * 0.3
        else:
            hidden, layers = c.get("hidden", 100), c["layers"]
            w = ko.load_mlp_weights(np.load(os.path.join(G, "weights_tank.npz"))) if self.plant == "tank" else \
                random_mlp_weights(n, hidden, layers, L, seed=5)
            kw.update(weights=w, hidden=hidden, layers=layers)
            self.lift = lambda x: ko.mlp_lift(w, x)
            self.g0 = None
            self.A0 = rng.randn(L, L) * 0.5 / np.sqrt(L)
            self.B0 = rng.randn(L, 1) * 0.3
            self.C0 = None if self.output == "lift" else rng.randn(n, L) * 0.3
        self.kw = kw
        if self.plant == "host":  # (x+ = A_d x + b_d u, as tests/test_gpu_state_dims.py: the device's plants have two states)
            Qo, _ = np.linalg.qr(rng.randn(n, n))
            self.Ad, self.bd = 0.95 * Qo, 0.3 * rng.randn(n)
        self.X0 = np.abs(rng.rand(n, self.B)) if self.plant == "tank" else rng.rand(n, self.B) - 0.5
        e1 = np.zeros((n, 1)); e1[0] = 1.0
        if self.output == "lift":
            self.r = np.tile(self.lift(e1), (1, N))   # vanderpol.py:668-675
        elif self.plant == "tank":
            self.r = np.ones((1, N))
        else:
            self.r = np.tile(e1[self.row0:self.row0 + self.q], (1, N))  # (the rows of [1; 0 ..] the output map selects)
        if "ref" in c:
            self.r = np.full((self.q, N), c["ref"])
        self.probe = (0.5 * rng.randn(L, self.B), rng.randn(self.q, N))  # the detector's arbitrary fixed (psi, r)

    # ---- the oracle's pieces
    def Co(self, C):
        return None if self.output == "lift" else C[self.row0:self.row0 + self.q]

    def block(self, A, Bm, C):
        """(Co P Co', iterations) of the reference's Riccati iteration on the un-augmented model"""
        P, it = ko.solve_dare(A, Bm, self.Qd, RD, self.maxiter, self.eps)
        return ko.terminal_block(np.eye(self.L) if self.output == "lift" else self.Co(C), P), it

    def Hf(self, A, Bm, C, psi, uprev, r, PN):
        """the condensed QP the device forms: plain, or on the increment form [A B; 0 1], [B; 1], [Co 0] with state [psi; u_prev]"""
        Co = self.Co(C)
        if self.du:
            L = self.L
            At = np.block([[A, Bm], [np.zeros((1, L)), np.eye(1)]])
            Bt = np.concatenate([Bm, [[1.0]]], axis=0)
            Cot = np.concatenate([Co, np.zeros((self.q, 1))], axis=1)
            _, _, H, f, _ = ko.condense(At, Bt, Cot, np.concatenate([psi, [uprev]]), r, self.N, self.Qw, self.Rw, PN=PN)
        else:
            _, _, H, f, _ = ko.condense(A, Bm, Co, psi, r, self.N, self.Qw, self.Rw, PN=PN)
        return H, f

    def box(self, uprev):
        lbv, ubv = np.full(self.N, self.lb), np.full(self.N, self.ub)
        if self.du:
            lbv[0] = max(self.lb, self.umin - uprev); ubv[0] = min(self.ub, self.umax - uprev)
        return lbv, ubv

    def plant_cpu(self, x, u):
        if self.plant == "host":
            return self.Ad @ x + self.bd * u
        if self.plant == "tank":
            return ko.tank_step(x, u)
        return ko.plant_step(self.plant, x, u, switched=self.sw)


@functools.lru_cache(maxsize=None)
def _set(name):
    return _Set(name, **CASES[name])


def _walk(S, b, drive=None, model0=None, steps=None):
    """The oracle loop for trajectory b: gain-form RLS, at every S.every-th step solve_dare + terminal_block on the updated model, the
    condensed QP with that block and its exact minimiser.  drive = None: self-driven (its own inputs, its own plant); drive = (U, X)
    ([steps][B], [steps][n][B]): it regresses on the device's applied inputs and continues from the device's states.  One record per
    step: U (None where cond(H) >= 1e9), moved = max |U - U(Qw I)|, it (at refresh steps), dx (driven: |plant(x, u) - X|)."""
    n, L = S.n, S.L
    A, Bm, C = model0 if model0 is not None else (S.A0, S.B0, S.C0)
    if S.g0 is not None:
        gK, gP, gC, gQ = S.g0
    else:
        gK, gP, gC, gQ = np.zeros((L, L + 1)), S.P0 * np.eye(L + 1), np.zeros((n, L)), S.barQ0 * np.eye(L)
    prev, uabs, x, PN, out = None, 0.0, S.X0[:, b].copy(), None, []
    for k in range(S.steps if steps is None else steps):
        psi = S.lift(x.reshape(n, 1)).reshape(-1)
        if prev is not None and S.update:
            ppsi, pu = prev
            gK, gP = ko.rls_update_gain(gK, gP, np.concatenate([ppsi, [pu]]), psi)
            A, Bm = gK[:, :-1].copy(), gK[:, -1:].copy()
            if S.output != "lift":
                gC, gQ = ko.rls_update_gain(gC, gQ, ppsi, x)
                C = gC.copy()
        rec = dict(k=k, model=(A, Bm, C), it=None)
        if k % S.every == 0:  # K = -dlqr(A, B, ...) / P with the UPDATED model; Q_bar(end) = C*P*C'   (Koopman_update.m:215, 381)
            PN, rec["it"] = S.block(A, Bm, C)
        rec["PN"] = PN
        H, f = S.Hf(A, Bm, C, psi, uabs, S.r, PN)
        lbv, ubv = S.box(uabs)
        rec["cond"] = np.linalg.cond(H)
        if rec["cond"] < 1e9:
            U, _ = ko.qp_exact(H, f, lbv, ubv)
            H0, f0 = S.Hf(A, Bm, C, psi, uabs, S.r, None)
            U0, _ = ko.qp_exact(H0, f0, lbv, ubv)
            rec["U"], rec["moved"] = U, float(np.abs(U - U0).max())
        else:  # (numerically singular: no minimiser to compare with; a self-driven loop applies the projected gradient step's sign)
            U = np.clip(-f, lbv, ubv)
            rec["U"], rec["moved"] = None, 0.0
        u = float(drive[0][k, b]) if drive is not None else (uabs + float(U[0]) if S.du else float(U[0]))
        xo = S.plant_cpu(x, u)
        rec["dx"] = float(np.abs(drive[1][k, :, b] - xo).max()) if drive is not None else 0.0
        x = drive[1][k, :, b].copy() if drive is not None else xo
        prev, uabs = (psi, u), u
        out.append(rec)
    return out


def _dev(H, f, Ho, fo):
    """the detector's two figures, relative as test_terminal_from_dare takes them"""
    return float(np.abs(H - Ho).max() / np.abs(Ho).max()), float(np.abs(f - fo).max() / max(1.0, np.abs(fo).max()))


def _tol(S, it):
    # (max7 stops every refresh at 7 iterations on purpose: seven iterations amplify nothing)
    return 1e-6 if (it >= S.maxiter and S.maxiter > 100) else 1e-9


@functools.lru_cache(maxsize=None)
def _self_driven(name):
    S = _set(name)
    return [_walk(S, b) for b in range(S.B)]


# ====================================================================================================================
# CPU companions (no GPU marker)
# ====================================================================================================================
@pytest.mark.parametrize("name", list(CASES))
def test_case_inputs(name):
    """The conditions on a case's inputs, from the oracle loop alone (self-driven, every trajectory): at most a quarter of the steps
    left out, the block moves the oracle's Useq by more than 1e-4 in at least a third of the compared steps, the Riccati iteration
    reaches maxiter in at most a quarter of the refreshes (max7: in all of them)."""
    S = _set(name)
    recs = [r for w in _self_driven(name) for r in w]
    steps = len(recs)
    assert steps == S.B * S.steps
    compared = [r for r in recs if r["U"] is not None]
    moved = sum(r["moved"] > 1e-4 for r in compared)
    its = [r["it"] for r in recs if r["it"] is not None]
    hit = sum(it >= S.maxiter for it in its)
    print("%-7s %5d  %8d  %5d / %-5d          %4d / %d" % (name, steps, steps - len(compared), moved, len(compared), hit, len(its)))
    assert len(its) == S.B * len([k for k in range(S.steps) if k % S.every == 0])
    if name == "rbf26":
        # The case as the issue states it -- the estimator continued from the offline samples -- CANNOT meet the conditions: the fitted
        # RBF model has spectral radius 0.9985 (a near-constant dictionary function), the Riccati iteration is still growing after
        # 500 iterations (|P| 1e11) and every H is numerically singular with such a block.  Pinned here as it is; the detector still
        # holds its blocks (1e-6: maxiter reached), and rbf26r -- the same set, estimator restarted -- carries the Useq controls.
        assert hit == len(its) and not compared
        return
    assert 4 * (steps - len(compared)) <= steps
    assert 3 * moved >= len(compared)
    if name == "max7":
        # every refresh of the start model (step 0) stops at 7; the rank-one models the first update after a restart leaves converge
        # below 1e-12 in 4 to 6 iterations, so not every later one does
        assert all(w[0]["it"] == 7 for w in _self_driven(name)) and 2 * hit >= len(its)
    else:
        assert 4 * hit <= len(its)
    if S.every > 1 and S.update:  # (a held block is visible only where the model moves on between two refreshes)
        w = _self_driven(name)[0]
        assert np.abs(w[1]["model"][0] - w[0]["model"][0]).max() > 1e-3


def test_the_two_output_rows_give_different_blocks():
    """row0 / row1 differ in out_row0 alone: their blocks differ, so a dropped cy0 cannot pass by symmetry"""
    a, b = _self_driven("row0"), _self_driven("row1")
    for wa, wb in zip(a, b):
        PNa, PNb = wa[0]["PN"], wb[0]["PN"]  # (step 0: the same start model on both sides)
        assert np.abs(PNa - PNb).max() > 1e-2 * max(np.abs(PNa).max(), np.abs(PNb).max())


def _mutants(S, final, star, before):
    """Deliberately wrong oracle-side blocks for the model `star` that last refreshed (`before`: the refresh before it); None where a
    mutation is the identity for this case (out_row0 = 0; y = psi, where Co = I and P is symmetric)."""
    A, Bm, C = star
    P, _ = ko.solve_dare(A, Bm, S.Qd, RD, S.maxiter, S.eps)
    PN, _ = S.block(A, Bm, C)
    I = np.eye(S.q)
    out = {}
    if S.output != "lift":
        out["out_row0 ignored"] = ko.terminal_block(C[0:S.q], P) if S.row0 else None
        Ct = C.reshape(S.L, S.n).T  # C read with the indices of its transpose
        out["Co' for Co"] = ko.terminal_block(Ct[S.row0:S.row0 + S.q], P)
    else:
        out["out_row0 ignored"] = out["Co' for Co"] = None
    out["block of the previous refresh"] = S.block(*before)[0] if before is not None else None
    out["- Qw I applied twice"] = PN - S.Qw * I
    out["- Qw I not applied"] = PN + S.Qw * I
    try:  # (without B nothing stabilises an unstable A: the iteration may leave the floating-point range -- a block no tolerance accepts)
        with np.errstate(all="ignore"):
            P0, _ = ko.solve_dare(A, np.zeros_like(Bm), S.Qd, RD, S.maxiter, S.eps)
        out["A without B in the iteration"] = ko.terminal_block(np.eye(S.L) if S.output == "lift" else S.Co(C), P0)
    except np.linalg.LinAlgError:
        out["A without B in the iteration"] = np.full((S.q, S.q), np.inf)
    return PN, out


@pytest.mark.parametrize("name", list(CASES))
def test_the_detector_rejects_wrong_blocks(name):
    """The power of the block comparison, on the case's own inputs and at the case's own tolerance: with the right block on the
    'device' side (the oracle stands in for it), each deliberately wrong oracle-side block -- out_row0 ignored, Co' for Co, the block of
    the previous refresh, P_N without '- Qw I' applied twice or not at all, A without B in the Riccati iteration -- is rejected for
    EVERY trajectory of the batch."""
    S = _set(name)
    psi, rq = S.probe
    applicable = set()
    for b, w in enumerate(_self_driven(name)):
        refreshes = [r for r in w if r["it"] is not None]
        star, it = refreshes[-1]["model"], refreshes[-1]["it"]
        before = refreshes[-2]["model"] if (len(refreshes) > 1 and S.update) else None
        final = w[-1]["model"]
        PN, muts = _mutants(S, final, star, before)
        H, f = S.Hf(*final, psi[:, b], 0.3, rq, PN)
        tol = _tol(S, it)
        assert max(_dev(H, f, *S.Hf(*final, psi[:, b], 0.3, rq, PN.copy()))) == 0.0
        for what, PNw in muts.items():
            if PNw is None:
                continue
            applicable.add(what)
            if not np.isfinite(PNw).all():
                continue
            d = max(_dev(H, f, *S.Hf(*final, psi[:, b], 0.3, rq, PNw)))
            if name == "rbf26" and "Qw I" in what:
                # (the one blind spot, and only of the case as the issue states it: its blocks are 1e11, Qw = 100 is 1e-9 of them and the
                #  iteration that reached maxiter is held to 1e-6; rbf26r sees both)
                assert np.abs(PN).max() > 1e8 * S.Qw and d < tol
                continue
            assert d > 10 * tol, (name, b, what)
    assert {"- Qw I applied twice", "- Qw I not applied", "A without B in the iteration"} <= applicable
    if name in ("row1", "lds36", "n3", "du10", "four64"):
        assert "Co' for Co" in applicable and "block of the previous refresh" in applicable
    if name in ("row1", "n3", "du10"):
        assert "out_row0 ignored" in applicable


# ====================================================================================================================
# GPU cases
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

    return KoopmanMPC


def _t(torch, a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda:0").contiguous()


def _model(m):
    return [t.cpu().numpy() if t is not None else None for t in m.get_model()]


def _handle(S, KM, arm=True):
    """a controller of the case with its start model (the RBF set: the offline fit, estimator continued), armed as the case says"""
    m = KM(batch=S.B, **S.kw)
    if S.rbf and S.offline is not None:
        m.offline_fit(*S.offline, init_rls=True)
    else:
        m.set_model(S.A0, S.B0, S.C0)
    if not S.update:
        m.set_online_update(False)
    if arm:
        m.set_terminal_refresh(S.every, S.Qd, RD, S.maxiter, S.eps)
    return m


def _model0(S, m):
    """the model the oracle starts from: the handle's own (the device's offline fit for the RBF set)"""
    A, Bm, C = _model(m)
    return A[0], Bm[0], None if C is None else C[0]


def _detect(S, m, star, uprev=None):
    """THE DETECTOR (module docstring): H, f of kmpc_condense against the oracle's with the block of the model `star`, for every
    trajectory, each held to its tolerance; returns the worst deviation as a fraction of its tolerance."""
    psi, rq = S.probe
    A, Bm, C = _model(m)
    H, f = [t.cpu().numpy() for t in m.condense(psi, rq)]
    up = np.zeros(S.B) if uprev is None else np.asarray(uprev.cpu().numpy() if hasattr(uprev, "cpu") else uprev, dtype=np.float64)
    worst = 0.0
    for b in range(S.B):
        PN, it = S.block(star[0][b], star[1][b], None if star[2] is None else star[2][b])
        Ho, fo = S.Hf(A[b], Bm[b], None if C is None else C[b], psi[:, b], float(up[b]), rq, PN)
        dH, df = _dev(H[b], f[b], Ho, fo)
        tol = _tol(S, it)
        worst = max(worst, dH / tol, df / tol)
        assert dH <= tol and df <= tol, (S.name, b, it, dH, df)
    return worst


def _sw(S):
    return 0 if S.sw else 10 ** 6


def _rollout_split(S, torch, m, split):
    """the case's steps as the calls of `split`; the global step that refreshes last is the last step of its call, get_model() there
    is the starred model of the blocks every later detector call must find.  Returns (U_log, X_log, worst block deviation)."""
    X = _t(torch, S.X0)
    done, star, worst, Us, Xs = 0, None, 0.0, [], []
    for cnt in split:
        Ul, Xl = m.rollout(S.plant, X, S.r, cnt, step0=done, switch_step=_sw(S), log=True)
        done += cnt
        if (done - 1) % S.every == 0:
            star = _model(m)
        else:
            assert not [g for g in range(done - cnt, done) if g % S.every == 0], "the split must end a call on the refreshing step"
        worst = max(worst, _detect(S, m, star, uprev=Ul[-1]))
        Us.append(Ul); Xs.append(Xl)
    return torch.cat(Us), torch.cat(Xs), worst


def _step_walk(S, torch, s, every_step=False):
    """the case's loop with kmpc_step (+ kmpc_plant_step, or the host's plant); the detector after the last step (after every step
    with every_step).  Returns (U0 [steps][B], Useq [steps][N][B], X [steps][n][B], worst block deviation) as NumPy arrays."""
    X = S.X0.copy() if S.plant == "host" else _t(torch, S.X0)
    star, worst, U0s, Useqs, Xs = None, 0.0, [], [], []
    for k in range(S.steps):
        u = s.step(X, S.r).clone()
        assert int(s.status.max().item()) <= S.status_ok, (S.name, k)
        Useqs.append(s.Useq.cpu().numpy().copy())
        if S.plant == "host":
            X = S.Ad @ X + S.bd[:, None] * u.cpu().numpy()[None, :]
            Xs.append(X.copy())
        else:
            X = s.plant_step(S.plant, X, u, switched=S.sw)
            Xs.append(X.cpu().numpy().copy())
        U0s.append(u.cpu().numpy().copy())
        if k % S.every == 0:
            star = _model(s)
        if every_step or k == S.steps - 1:
            worst = max(worst, _detect(S, s, star, uprev=u))
    return np.array(U0s), np.array(Useqs), np.array(Xs), worst


def _controls(S, model0, U0s, Useqs, Xs):
    """the oracle loop driven by the device's applied inputs and states: worst |Useq - Useq_oracle| over the compared steps, worst
    |x - plant(x, u)|, the number of steps left out (cond(H) >= 1e9), and per trajectory the first such step (S.steps: none).  A
    numerically singular QP has no minimiser for two routes to agree on, and from there on they regress on different inputs: a
    trajectory leaves a comparison between two routes at its first one (_route_dev)."""
    worst_u = worst_x = 0.0
    left, first = 0, np.full(S.B, S.steps)
    for b in range(S.B):
        for rec in _walk(S, b, drive=(U0s, Xs), model0=model0):
            worst_x = max(worst_x, rec["dx"])
            if rec["U"] is None:
                left += 1
                first[b] = min(first[b], rec["k"])
            else:
                worst_u = max(worst_u, float(np.abs(Useqs[rec["k"]][:, b] - rec["U"]).max()))
    return worst_u, worst_x, left, first


def _route_dev(a, b, first):
    """max |a - b| of two routes' logs ([steps][B] or [steps][n][B]) over the steps before each trajectory's first singular QP"""
    a, b = [np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for v in (a, b)]
    keep = np.arange(a.shape[0])[:, None] < first[None, :]
    d = np.abs(a - b)
    return float((d * (keep if d.ndim == 2 else keep[:, None, :])).max())


def _plant_dev(S, U0s, Xs):
    """max |x_k - plant(x_{k-1}, u_k)| over a route's logs: the oracle's plant on the device's own states and inputs"""
    worst, x = 0.0, S.X0
    for k in range(len(U0s)):
        worst = max(worst, max(float(np.abs(Xs[k][:, b] - S.plant_cpu(x[:, b], float(U0s[k][b]))).max()) for b in range(S.B)))
        x = Xs[k]
    return worst


def _report(name, **figs):
    print("terminal refresh %-7s " % name + ", ".join("%s %.2e" % kv if isinstance(kv[1], float) else "%s %s" % kv for kv in figs.items()))


FUSED = ["psi12", "lds36", "row1", "row0", "rbf26", "rbf26r", "du10", "max7"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED)
def test_fused_rollout_blocks_and_controls(torch_mod, KM, name):
    """A fused set: the roll-out split into calls (detector after every call: fresh and held blocks, term_count carried, the second
    call of row1 / row0 under the placement table of the first) against ONE launch of a twin (1e-9), and the kmpc_step walk of a
    third handle (MLP: one-step launches of the TERM plug-in; RBF: the per-step route) -- its blocks, its Useq against the oracle's
    minimiser (1e-6), its U0 against the launch (1e-9), the states against the oracle's plant (1e-9)."""
    torch = torch_mod
    S = _set(name)
    m, t, s = _handle(S, KM), _handle(S, KM), _handle(S, KM)
    code, text = m.rollout_plugin_status()
    print(text)
    assert code == 1 and "_term_" in text and m.rollout_is_fused()
    Ul, Xl, worst_split = _rollout_split(S, torch, m, S.split)
    assert int(m.status.max().item()) <= S.status_ok
    Xt = _t(torch, S.X0)
    Ut, Xlt = t.rollout(S.plant, Xt, S.r, S.steps, switch_step=_sw(S), log=True)
    worst_one = _detect(S, t, _model(t), uprev=Ut[-1]) if (S.steps - 1) % S.every == 0 else 0.0
    d_split = max(float((Ul - Ut).abs().max()), float((Xl - Xlt).abs().max()))
    model0 = _model0(S, s)
    U0s, Useqs, Xs, worst_step = _step_walk(S, torch, s)
    worst_x = max(_plant_dev(S, U0s, Xs), _plant_dev(S, Ut.cpu().numpy(), Xlt.cpu().numpy()))
    if name == "rbf26":
        # (every H of this case is numerically singular -- cond 5e10, blocks of 1e11, test_case_inputs --: there is no minimiser for the
        #  oracle or for the two routes to agree on, 1.1 measured between them; its blocks, its split and its plant are held here, rbf26r
        #  holds the rest)
        worst_u, left, d_launch = 0.0, S.B * S.steps, float("nan")
    else:
        worst_u, _, left, first = _controls(S, model0, U0s, Useqs, Xs)
        d_launch = _route_dev(U0s, Ut, first)
    _report(name, block=max(worst_split, worst_one, worst_step), Useq=worst_u, U0_vs_launch=d_launch, x=worst_x, split_vs_one=d_split,
            left_out="%d / %d" % (left, S.B * S.steps))
    assert d_split < 1e-9
    assert worst_u < 1e-6 and worst_x < 1e-9
    if name != "rbf26":
        assert d_launch < 1e-9
        assert 4 * left <= S.B * S.steps


@pytest.mark.gpu
def test_the_two_output_rows_leave_different_blocks(torch_mod, KM):
    """row0 / row1 on the device: the same start model, out_row0 alone differs -- H of the probe differs after the first step"""
    Hs = []
    for name in ("row0", "row1"):
        S = _set(name)
        m = _handle(S, KM)
        m.rollout(S.plant, _t(torch_mod, S.X0), S.r, 1)
        Hs.append(m.condense(*_set("row1").probe)[0].cpu().numpy())
    assert np.abs(Hs[0] - Hs[1]).max() > 1e-3 * np.abs(Hs[0]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["four64", "n3"])
def test_per_step_route_blocks_and_controls(torch_mod, KM, name):
    """A set without a fused roll-out (four waves per trajectory; n = 3): RLS-only launch, dare_kernel every second step, QP-only launch.
    kmpc_step walk with the detector after EVERY step (fresh and held blocks) and the oracle controls; four64 also as kmpc_rollout
    (3 + 1 + 1 steps, the plant inside the step kernel): the two loops agree to 1e-9 -- the RLS-only launch leaves the plant alone."""
    torch = torch_mod
    S = _set(name)
    s = _handle(S, KM)
    assert not s.rollout_is_fused()
    U0s, Useqs, Xs, worst_step = _step_walk(S, torch, s, every_step=True)
    worst_u, worst_x, left, first = _controls(S, (S.A0, S.B0, S.C0), U0s, Useqs, Xs)
    d_ro, worst_ro = 0.0, 0.0
    if S.split:
        m = _handle(S, KM)
        Ul, Xl, worst_ro = _rollout_split(S, torch, m, S.split)
        assert int(m.status.max().item()) <= S.status_ok
        d_ro = max(_route_dev(Ul, U0s, first), _route_dev(Xl, Xs, first))
    _report(name, block=max(worst_step, worst_ro), Useq=worst_u, U0_vs_launch=d_ro, x=worst_x, left_out="%d / %d" % (left, S.B * S.steps))
    assert d_ro < 1e-9
    assert worst_u < 1e-6 and worst_x < 1e-9
    assert 4 * left <= S.B * S.steps


@pytest.mark.gpu
def test_refresh_with_the_online_update_off(torch_mod, KM):
    """kmpc_set_online_update(h, 0) with the refresh armed: every trajectory's block is solve_dare of the model kmpc_set_model gave,
    and U_log equals (1e-9) that of a twin WITHOUT the refresh whose one block came from kmpc_terminal_from_dare(per_trajectory = 0)."""
    torch = torch_mod
    S = _set("off")
    m, t = _handle(S, KM), _handle(S, KM, arm=False)
    t.terminal_from_dare(S.Qd, RD, per_trajectory=False)
    star = [np.tile(a[None], (S.B, 1, 1)) for a in (S.A0, S.B0, S.C0)]
    Xm, Xt = _t(torch, S.X0), _t(torch, S.X0)
    Um, Xlm = m.rollout(S.plant, Xm, S.r, S.steps, log=True)
    worst = _detect(S, m, star)
    Ut, Xlt = t.rollout(S.plant, Xt, S.r, S.steps, log=True)
    assert m.rollout_is_fused() and int(m.status.max().item()) == 0
    d = max(float((Um - Ut).abs().max()), float((Xlm - Xlt).abs().max()))
    # the same through kmpc_step (one-step launches)
    s = _handle(S, KM)
    U0s, Useqs, Xs, worst_s = _step_walk(S, torch, s, every_step=True)
    for a, b in zip(_model(s), star):
        assert np.array_equal(a, b)  # the model stays
    worst_u, worst_x, left, _ = _controls(S, (S.A0, S.B0, S.C0), U0s, Useqs, Xs)
    _report("off", block=max(worst, worst_s), Useq=worst_u, U0_vs_launch=float(np.abs(U0s - Um.cpu().numpy()).max()), x=worst_x, vs_twin_without=d)
    assert d < 1e-9 and float(np.abs(U0s - Um.cpu().numpy()).max()) < 1e-9
    assert worst_u < 1e-6 and worst_x < 1e-9 and left == 0


@pytest.mark.gpu
def test_checkpoint_while_armed(torch_mod, KM):
    """state_dict() / load_state_dict() with the refresh armed (row1's set).  every = 1: the blocks of the importer equal the exporter's
    before any step, and the next 3 steps of exporter and importer agree bit for bit (as the checkpoint round trips of handles without
    the refresh do).  every = 2: the blob does not carry the count -- the exporter (3 steps done) holds its block at its next step, the
    freshly armed importer refreshes at its FIRST step and holds at its second; both are pinned with the detector."""
    torch = torch_mod
    S1 = _Set("ckpt1", **dict(CASES["row1"], every=1, steps=3, split=(3,)))
    a = _handle(S1, KM)
    X = _t(torch, S1.X0)
    Ua, _ = a.rollout(S1.plant, X, S1.r, 3, log=True)
    star = _model(a)
    sd = a.state_dict()
    b = _handle(S1, KM)
    b.load_state_dict(sd)
    worst = max(_detect(S1, b, star, uprev=Ua[-1]), _detect(S1, a, star, uprev=Ua[-1]))
    Xa, Xb = X.clone(), X.clone()
    Ua2, Xla = a.rollout(S1.plant, Xa, S1.r, 3, step0=3, log=True)
    Ub2, Xlb = b.rollout(S1.plant, Xb, S1.r, 3, step0=3, log=True)
    assert torch.equal(Ua2, Ub2) and torch.equal(Xla, Xlb)
    worst = max(worst, _detect(S1, b, _model(b), uprev=Ub2[-1]))
    # every = 2
    S2 = _Set("ckpt2", **dict(CASES["row1"], every=2, steps=3, split=(3,)))
    a = _handle(S2, KM)
    X = _t(torch, S2.X0)
    Ua, _ = a.rollout(S2.plant, X, S2.r, 3, log=True)   # refreshes at steps 0 and 2
    star2 = _model(a)
    sd = a.state_dict()
    b = _handle(S2, KM)
    b.load_state_dict(sd)
    worst = max(worst, _detect(S2, b, star2, uprev=Ua[-1]))       # the blob's blocks, before any step
    Xa, Xb = X.clone(), X.clone()
    ua, _ = a.rollout(S2.plant, Xa, S2.r, 1, step0=3, log=True)   # exporter: step 3 holds the block of step 2
    worst = max(worst, _detect(S2, a, star2, uprev=ua[-1]))
    ub, _ = b.rollout(S2.plant, Xb, S2.r, 1, step0=3, log=True)   # importer: count 0, its first step refreshes
    star_b = _model(b)
    worst = max(worst, _detect(S2, b, star_b, uprev=ub[-1]))
    assert float((ua - ub).abs().max()) > 0.0                       # (another block, another input)
    ub, _ = b.rollout(S2.plant, Xb, S2.r, 1, step0=4, log=True)   # ... its second step holds that block
    worst = max(worst, _detect(S2, b, star_b, uprev=ub[-1]))
    assert np.abs(_model(b)[0] - star_b[0]).max() > 0.0
    _report("ckpt", block=worst)


@pytest.mark.gpu
def test_checkpoint_with_one_shared_block_into_an_armed_handle(torch_mod, KM):
    """A blob with ONE Riccati block for the batch (kmpc_terminal_from_dare(per_trajectory = 0) on a handle without the refresh) imported
    into an armed handle whose next step HOLDS (every = 2, one step done): the fused launch reads B blocks, so the import hands the
    blob's block to every trajectory -- the detector finds it B times, and the held step equals the exporter's next step (1e-9)."""
    torch = torch_mod
    S = _Set("ckpt3", **dict(CASES["row1"], every=2, steps=2, split=(2,)))
    g = _handle(S, KM, arm=False)
    g.terminal_from_dare(S.Qd, RD, per_trajectory=False)
    X = _t(torch, S.X0)
    Ug, _ = g.rollout(S.plant, X, S.r, 1, log=True)
    sd = g.state_dict()
    b = _handle(S, KM)
    b.set_model(2.0 * S.A0, S.B0, S.C0)  # (another model: the blocks of its own first refresh are not the blob's)
    b.rollout(S.plant, _t(torch, S.X0), S.r, 1)
    b.load_state_dict(sd)
    star = [np.tile(a_[None], (S.B, 1, 1)) for a_ in (S.A0, S.B0, S.C0)]
    worst = _detect(S, b, star, uprev=Ug[-1])
    Xg, Xb = X.clone(), X.clone()
    Ug2, Xlg = g.rollout(S.plant, Xg, S.r, 1, step0=1, log=True)
    Ub2, Xlb = b.rollout(S.plant, Xb, S.r, 1, step0=1, log=True)   # count 1 of 2: held
    assert b.rollout_is_fused()
    d = max(float((Ug2 - Ub2).abs().max()), float((Xlg - Xlb).abs().max()))
    worst = max(worst, _detect(S, b, star, uprev=Ub2[-1]))
    _report("ckpt3", block=worst, held_step_vs_exporter=d)
    assert d < 1e-9
