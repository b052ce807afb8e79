"""Trajectories between handles of any batch size on the device: kmpc_state_pack / kmpc_state_unpack / kmpc_state_transfer
(KoopmanMPC.pack_state / unpack_state / transfer_state) and koopmpc.sharding.regroup.
Runs on the MI355X box:  python -m pytest tests/test_gpu_state_rows.py -m gpu

A packed row is one trajectory's share of the per-trajectory sections of the state blob (the format comments in csrc/api.hip):

    P[sP] K[sK] Q[sQ] C[sC] psi_prev[L] warm[N] u_prev[1] have_prev rls_fresh 0...   (row_elems: a multiple of 16 bytes)

Dimension sets (n, L, N), chosen so that every alignment case of the copy kernels occurs at the smallest size:
    mlp64  (2, 20, 20) MLP, float64        the built-in fused roll-out, state in its wave image
    rbf64  (2, 8, 30)  thin-plate, float64 built-in fused; p p = 81 is odd, sP carries a padding element
    rbf3   (3, 9, 5)   thin-plate, float64 per-step launches (no three-state plant on the device: a linear host-side plant, evaluated
                       element by element so that a column's arithmetic does not depend on the batch); n L = 27 and L = 9 are odd
    mlp32  (2, 20, 20) MLP, float32        the float64 core behind float32 blocks; segments aligned to 8 bytes only
Every test starts from handles that ran six closed-loop steps (the estimator is past its restart, warm is non-zero, have_prev = 1).
Continuations are compared with torch.equal: a trajectory's arithmetic depends neither on its slot nor on the batch
(include/koopmpc.h, kmpc_set_rollout_workgroup), and checkpoints continue bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SETS = ["mlp64", "rbf64", "rbf3", "mlp32"]
PRE, MORE = 6, 5  # steps of the preamble, steps of a continuation
IDX16 = [31, 0, 17, 5, 22, 9, 30, 1, 12, 28, 3, 19, 7, 26, 14, 11]  # neither sorted nor contiguous


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


def even_up(v):
    return (v + 1) & ~1


class Case:
    """One dimension set: how to make a handle of any batch, its offline model, reference and initial states, and how to advance a
    closed loop by `steps` (fused roll-out with the device plant for n = 2; step() and the host-side linear plant for n = 3)."""

    def __init__(self, torch, KM, name):
        from koopmpc.synth import duffing_rk4, initial_states, offline_edmd, random_mlp_weights

        self.torch, self.KM, self.name = torch, KM, name
        self.n, self.L, self.N = {"mlp64": (2, 20, 20), "rbf64": (2, 8, 30), "rbf3": (3, 9, 5), "mlp32": (2, 20, 20)}[name]
        self.tdt, self.dt = (torch.float32, np.float32) if name == "mlp32" else (torch.float64, np.float64)
        rng = np.random.RandomState(11)
        if name.startswith("mlp"):
            self.kw = dict(weights=random_mlp_weights(2, 100, 3, self.L, seed=5))
        else:
            self.kw = dict(lift="rbf", centres=4 * rng.rand(self.L, self.n) - 2)
        self.kw.update(dtype=self.tdt)
        n, L, N = self.n, self.L, self.N
        probe = self.make(4, model=False)
        if n == 2:
            self.model = offline_edmd(lambda X: np.asarray(probe.Encoder(X), dtype=np.float64), plant=duffing_rk4)
            self.r = np.tile(np.array([[1.0], [0.0]]), (1, N))
        else:
            Qo, _ = np.linalg.qr(rng.randn(n, n))
            self.Ad, self.bd = 0.95 * Qo, 0.3 * rng.randn(n)
            Xs, Us = 4 * rng.rand(n, 2000) - 2, 4 * rng.rand(1, 2000) - 2
            Ys = self.Ad @ Xs + self.bd[:, None] * Us
            PX, PY = probe.Encoder(Xs), probe.Encoder(Ys)
            K = PY @ np.linalg.pinv(np.concatenate([PX, Us], 0))
            self.model = (K[:, :-1].copy(), K[:, -1:].copy(), Xs @ np.linalg.pinv(PX))
            self.r = np.tile(0.5 * rng.randn(n, 1), (1, N))
        self.X0 = initial_states(48, seed=3, n=n)
        self.X0b = initial_states(48, seed=8, n=n)
        p = L + 1
        self.strides = (even_up(p * p), even_up(L * p), even_up(L * L), even_up(n * L))
        per16 = 16 // np.dtype(self.dt).itemsize
        self.flag_off = sum(self.strides) + L + N + 1
        self.row_elems = (self.flag_off + 2 + per16 - 1) // per16 * per16

    def make(self, B, model=True, **extra):
        kw = dict(self.kw)
        kw.update(extra)
        m = self.KM(n=self.n, L=self.L, N=self.N, batch=B, **kw)
        if model:
            m.set_model(*self.model)
        return m

    def states(self, X0, cols=None):
        X = X0 if cols is None else X0[:, cols]
        return self.torch.tensor(np.ascontiguousarray(X), dtype=self.tdt, device="cuda:0")

    def advance(self, m, X, steps, step0):
        """`steps` closed-loop steps of m on X (advanced in place) -> (U_log (steps, B), X_log (steps, n, B))"""
        torch = self.torch
        if self.n == 2:
            Ul, Xl = m.rollout("duffing", X, self.r, steps, step0=step0, log=True)
            assert m.rollout_is_fused(), self.name  # (the three two-state sets have built-in fused kernels)
            return Ul, Xl
        Ul, Xl = [], []
        for _ in range(steps):
            u = m.step(X, self.r).clone()
            # (element by element: no library GEMM whose summation could depend on the number of columns)
            Xn = torch.stack([sum(float(self.Ad[i, j]) * X[j] for j in range(self.n)) + float(self.bd[i]) * u for i in range(self.n)])
            X.copy_(Xn)
            Ul.append(u)
            Xl.append(Xn)
        assert not m.rollout_is_fused(), self.name
        return torch.stack(Ul), torch.stack(Xl)

    def stepped(self, B, X0, cols=None):
        """a handle of batch B after the preamble on columns `cols` of X0 -> (handle, X)"""
        m = self.make(B)
        X = self.states(X0, cols if cols is not None else list(range(B)))
        self.advance(m, X, PRE, 0)
        return m, X

    def parse(self, blob, B):
        """(header ints, per-trajectory sections) of a state blob of batch B, by the format comment above BlobHeader in api.hip"""
        raw = np.ascontiguousarray(blob, dtype=np.uint8).tobytes()
        ints = np.frombuffer(raw[:64], dtype=np.int32)
        o, isz, out = 80, np.dtype(self.dt).itemsize, []
        for rows, cols in [(B, s) for s in self.strides] + [(B, self.L), (self.N, B), (1, B)]:
            out.append(np.frombuffer(raw[o:o + rows * cols * isz], dtype=self.dt).reshape(rows, cols))
            o += rows * cols * isz
        assert o == len(raw), (o, len(raw))  # (no shared-model or terminal section on these handles)
        return ints, out

    def rows_of_blob(self, blob, B, idx):
        """the packed rows of trajectories idx, assembled from the blob"""
        ints, (P, K, Q, Cc, psi, warm, u) = self.parse(blob, B)
        rows = np.zeros((len(idx), self.row_elems), dtype=self.dt)
        for r, b in enumerate(idx):
            body = np.concatenate([P[b], K[b], Q[b], Cc[b], psi[b], warm[:, b], u[0, b:b + 1], np.array([ints[7], ints[8]], dtype=self.dt)])
            rows[r, :body.size] = body
        return rows


_cases = {}


@pytest.fixture(params=SETS)
def case(request, torch_mod, KM):
    if request.param not in _cases:
        _cases[request.param] = Case(torch_mod, KM, request.param)
    return _cases[request.param]


def blob_of(m):
    return m.state_dict()["blob"].tobytes()


def same(torch, a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


# ------------------------------------------------------------------ 1. layout
def test_rows_are_the_blob_slices_of_their_trajectories(torch_mod, case):
    """pack_state(idx) after the preamble: every row equals, byte for byte, that trajectory's slices of the kmpc_state_export blob --
    the full strides with their padding element, the warm column of the [N][B] panel, u_prev, the two flags, zero padding."""
    B = 32
    m, _ = case.stepped(B, case.X0)
    assert m.state_row_elems() == case.row_elems and (case.row_elems * np.dtype(case.dt).itemsize) % 16 == 0
    for idx in (IDX16, [17], [4, 4, 31, 4], None):
        rows = m.pack_state(idx)
        blob = m.state_dict()["blob"]
        want = case.rows_of_blob(blob, B, list(range(B)) if idx is None else idx)
        got = rows.cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (case.name, idx)
        assert got.tobytes() == want.tobytes(), (case.name, idx, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4])
    # the preamble left something to tell the segments apart: flags 1 / 0, a warm start and a previous transition that are not zero
    ints, (P, K, Q, Cc, psi, warm, u) = case.parse(blob, B)
    assert ints[7] == 1 and ints[8] == 0 and warm.any() and psi.any() and u.any(), case.name
    assert not np.array_equal(K[0], K[1]), case.name
    assert not np.array_equal(warm.ravel(), np.ascontiguousarray(warm.T).ravel()), case.name  # (a panel that tells [N][B] from [B][N])


# ------------------------------------------------------------------ 2. whole-handle round trip
def test_whole_handle_round_trip_reproduces_the_blob(torch_mod, case):
    """unpack_state(pack_state()) into a fresh handle of the same batch: its blob equals the source's byte for byte, header included
    (a call that fills the whole handle adopts the flags)."""
    B = 32
    m, _ = case.stepped(B, case.X0)
    fresh = case.make(B, model=False)
    assert fresh.estimator_status()[0] is False
    fresh.unpack_state(m.pack_state())
    assert blob_of(fresh) == blob_of(m), case.name
    assert fresh.estimator_status()[:2] == m.estimator_status()[:2] == (True, False), case.name


# ------------------------------------------------------------------ 3. continuation of a subset
@pytest.mark.parametrize("count", [16, 1])
def test_subset_continues_as_in_the_large_handle(torch_mod, case, count):
    """A (B = 32) takes state_dict() -- the synchronisation point -- and rows idx go to a fresh S (B = 16, B = 1); both run five more
    steps, A on X and S on X[:, idx]: controls and states of S are A's columns idx, bit for bit."""
    torch = torch_mod
    idx = IDX16 if count == 16 else [17]
    A, X = case.stepped(32, case.X0)
    A.state_dict()
    S = case.make(count)
    S.transfer_state(A, src_idx=idx)
    Xs = X[:, idx].clone().contiguous()
    Ua, Xa = case.advance(A, X, MORE, PRE)
    Us, Xsl = case.advance(S, Xs, MORE, PRE)
    du = float((Us - Ua[:, idx]).abs().max())
    dx = float((Xsl - Xa[:, :, idx]).abs().max())
    print("subset %s 32 -> %d: max |dU| = %.3e, max |dX| = %.3e" % (case.name, count, du, dx))
    assert same(torch, Us, Ua[:, idx].contiguous()), (case.name, count, du)
    assert same(torch, Xsl, Xa[:, :, idx].contiguous()), (case.name, count, dx)
    assert float(Ua.abs().max()) > 0.0 and not same(torch, Ua[:, 0], Ua[:, 1])
    # ... and the state they arrive at: S's rows are A's rows idx
    assert same(torch, S.pack_state(), A.pack_state(idx)), (case.name, count)


# ------------------------------------------------------------------ 4. scatter into a running handle
def test_scatter_into_a_running_handle(torch_mod, case):
    """A and D (B = 32 each) run the preamble from different initial states; eight rows of A go to eight rows of D.  D continues: the
    eight behave as A's do on the same states, the other 24 equal a twin of D that took state_dict() at the same point, bit for bit."""
    torch = torch_mod
    ia, idd = [31, 2, 17, 8, 9, 25, 0, 13], [5, 30, 1, 16, 22, 7, 11, 28]
    others = [b for b in range(32) if b not in idd]
    A, XA = case.stepped(32, case.X0)
    D, XD = case.stepped(32, case.X0b)
    T, XT = case.stepped(32, case.X0b)
    T.state_dict()
    D.transfer_state(A, src_idx=ia, dst_idx=torch.tensor(idd, device="cuda:0"))
    XD[:, idd] = XA[:, ia]
    Ua, Xa = case.advance(A, XA, MORE, PRE)
    Ud, Xd = case.advance(D, XD, MORE, PRE)
    Ut, Xt = case.advance(T, XT, MORE, PRE)
    assert same(torch, Ud[:, idd].contiguous(), Ua[:, ia].contiguous()), case.name
    assert same(torch, Xd[:, :, idd].contiguous(), Xa[:, :, ia].contiguous()), case.name
    assert same(torch, Ud[:, others].contiguous(), Ut[:, others].contiguous()), case.name
    assert same(torch, Xd[:, :, others].contiguous(), Xt[:, :, others].contiguous()), case.name
    assert not same(torch, Ud[:, idd].contiguous(), Ut[:, idd].contiguous()), case.name  # (the eight did change hands)


# ------------------------------------------------------------------ 5. clone inside one handle
def test_clone_inside_one_handle_with_overlapping_lists(torch_mod, case):
    """transfer_state(m, src_idx=[0, 1, 2], dst_idx=[1, 2, 3]): rows 1, 2, 3 hold the OLD rows 0, 1, 2; every other row stays."""
    torch = torch_mod
    m, _ = case.stepped(32, case.X0)
    before = m.pack_state().clone()
    m.transfer_state(m, src_idx=[0, 1, 2], dst_idx=[1, 2, 3])
    after = m.pack_state()
    assert same(torch, after[1:4], before[0:3]), case.name
    assert same(torch, after[0], before[0]) and same(torch, after[4:], before[4:]), case.name
    assert not same(torch, before[1], before[0]), case.name
    # one to many: a row may be read more than once
    m.transfer_state(m, src_idx=np.array([7, 7, 7]), dst_idx=[20, 8, 31])
    last = m.pack_state()
    for b in (20, 8, 31):
        assert same(torch, last[b], after[7]), (case.name, b)
    keep = [b for b in range(32) if b not in (20, 8, 31)]
    assert same(torch, last[keep], after[keep]), case.name


# ------------------------------------------------------------------ 6. regroup
def test_regroup_two_handles_of_24_into_three_of_16(torch_mod, case):
    """48 trajectories run as two handles of 24, then koopmpc.sharding.regroup into three of 16 (the middle one is assembled from both):
    the continuation equals the unsharded 48-trajectory handle column by column."""
    torch = torch_mod
    from koopmpc.sharding import regroup, reshard_plan

    W, XW = case.stepped(48, case.X0)
    W.state_dict()
    olds = [case.stepped(24, case.X0, list(range(24 * k, 24 * k + 24))) for k in range(2)]
    assert same(torch, torch.cat([x for _, x in olds], dim=1), XW), case.name  # (the preamble does not depend on the batch either)
    news = [case.make(16, model=False) for _ in range(3)]
    assert [len(reshard_plan(48, 2, 3, k)) for k in range(3)] == [1, 2, 1]
    regroup([m for m, _ in olds], news)
    Uw, Xw = case.advance(W, XW, MORE, PRE)
    Xcat = torch.cat([x for _, x in olds], dim=1)
    for k, m in enumerate(news):
        Xk = Xcat[:, 16 * k:16 * k + 16].clone().contiguous()
        Uk, Xkl = case.advance(m, Xk, MORE, PRE)
        assert same(torch, Uk, Uw[:, 16 * k:16 * k + 16].contiguous()), (case.name, k)
        assert same(torch, Xkl, Xw[:, :, 16 * k:16 * k + 16].contiguous()), (case.name, k)


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_destination_unchanged(torch_mod, KM):
    torch = torch_mod
    from koopmpc._ffi import KmpcError

    if "rbf3" not in _cases:
        _cases["rbf3"] = Case(torch, KM, "rbf3")
    case = _cases["rbf3"]  # (float64 without a fused roll-out: arming the terminal refresh compiles nothing)
    B = 8
    A, X = case.stepped(B, case.X0)
    D, _ = case.stepped(B, case.X0b)
    rows = A.pack_state([0, 1])
    ref = blob_of(D)

    def refused(call, match, dst=D, want=None):
        with pytest.raises(KmpcError, match=match):
            call()
        assert blob_of(dst) == (ref if want is None else want), match

    # an index outside [0, B) -- on a destination and on a source
    refused(lambda: D.unpack_state(rows, idx=[0, B]), "outside")
    refused(lambda: D.unpack_state(rows, idx=[-1, 3]), "outside")
    refused(lambda: D.transfer_state(A, src_idx=[0, B], dst_idx=[0, 1]), "outside")
    refused(lambda: D.transfer_state(A, src_idx=[0, 1], dst_idx=[B, 1]), "outside")
    with pytest.raises(KmpcError, match="outside"):
        A.pack_state([B])
    with pytest.raises(KmpcError, match="outside"):
        A.pack_state([-1])
    # a destination named twice
    refused(lambda: D.unpack_state(rows, idx=[3, 3]), "twice")
    refused(lambda: D.transfer_state(A, src_idx=[0, 1, 2], dst_idx=[4, 2, 4]), "twice")
    # more rows than trajectories (the binding checks the shape itself; the library refuses the count)
    with pytest.raises(ValueError):
        D.unpack_state(A.pack_state(list(range(B)) + [0]))
    with pytest.raises(ValueError):
        D.unpack_state(rows[:, :-1])
    with pytest.raises(ValueError):
        D.unpack_state(rows, idx=[1, 2, 3])
    refused(lambda: D.transfer_state(A, src_idx=[0] * (B + 1)), "more rows")
    # rows of a stepped handle into PART of a fresh one: the flags are the handle's
    F = case.make(B)
    fresh = blob_of(F)
    refused(lambda: F.unpack_state(rows, idx=[0, 1]), "flags", dst=F, want=fresh)
    refused(lambda: F.transfer_state(A, src_idx=[0, 1, 2], dst_idx=[5, 6, 7]), "flags", dst=F, want=fresh)
    # ... and rows that carry different flags cannot fill a handle either
    mixed = torch.cat([A.pack_state(list(range(B - 1))), F.pack_state([0])])
    refused(lambda: F.unpack_state(mixed), "different", dst=F, want=fresh)
    bad = A.pack_state()
    bad[2, case.flag_off] = 0.5
    refused(lambda: F.unpack_state(bad), "not 0 or 1", dst=F, want=fresh)
    # handles that differ in L
    other = KM(n=case.n, L=case.L - 1, N=case.N, batch=B, lift="rbf", centres=case.kw["centres"][:-1])
    refused(lambda: D.transfer_state(other), "differ")
    with pytest.raises(ValueError):
        D.unpack_state(other.pack_state([0, 1]), idx=[0, 1])
    # count == 0 succeeds and does nothing
    D.unpack_state(rows[:0], idx=[])
    assert A.pack_state([]).shape == (0, case.row_elems)
    D.transfer_state(A, src_idx=[], dst_idx=[])
    assert blob_of(D) == ref
    # a handle with per-trajectory terminal blocks: the terminal refresh armed
    Tm, _ = case.stepped(B, case.X0)
    Tm.set_terminal_refresh(1)
    armed = blob_of(Tm)
    refused(lambda: Tm.unpack_state(rows, idx=[0, 1]), "terminal", dst=Tm, want=armed)
    refused(lambda: Tm.pack_state(), "terminal", dst=Tm, want=armed)
    refused(lambda: Tm.transfer_state(A, src_idx=[0], dst_idx=[0]), "terminal", dst=Tm, want=armed)
    refused(lambda: D.transfer_state(Tm, src_idx=[0], dst_idx=[0]), "terminal")
    with pytest.raises(KmpcError, match="terminal"):
        Tm.state_row_elems()
    # a handle after shared_step: its model is pooled over the batch
    Sm, Xs = case.stepped(B, case.X0)
    Sm.shared_step(Xs, case.r)
    pooled = blob_of(Sm)
    refused(lambda: Sm.unpack_state(rows, idx=[0, 1]), "shared-model", dst=Sm, want=pooled)
    refused(lambda: Sm.pack_state([0]), "shared-model", dst=Sm, want=pooled)
    refused(lambda: Sm.transfer_state(A, src_idx=[0], dst_idx=[0]), "shared-model", dst=Sm, want=pooled)
    refused(lambda: D.transfer_state(Sm, src_idx=[0], dst_idx=[0]), "shared-model")
    # after all that D still takes rows
    D.unpack_state(rows, idx=[6, 2])
    assert same(torch, D.pack_state([6, 2]), rows)
