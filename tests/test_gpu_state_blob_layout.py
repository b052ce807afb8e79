"""The byte layout of the state blob (kmpc_state_export, version 2) as csrc/api.hip documents it above BlobHeader, parsed in
NumPy and held bit for bit against what the public getters return.  The other checkpoint tests are round trips (export, then
import) or compare one blob with another: they cannot see the two sides move together.  This file pins the bytes.
Runs on the MI355X box:  python -m pytest tests/test_gpu_state_blob_layout.py -m gpu

    header   16 int32: magic 0x4b4d5043, version 2, dtype, n, L, N, B, have_prev, rls_fresh, has_shared, shared_has_samples,
             have_wterm, wterm_from_dare, wterm_per_traj, wterm_blocks, reserved; then 2 float64: P0, barQ0           80 bytes
    P        [B][sP]  p x p row-major at the head of every stride, p = L + 1, sP = even_up(p p)                         T
    K        [B][sK]  L x p row-major, [A B], sK = even_up(L p)                                                         T
    Q        [B][sQ]  L x L, sQ = even_up(L L)                                                                          T
    C        [B][sC]  n x L, sC = even_up(n L)                                                                          T
    psi_prev [B][L]                                                                                                     T
    warm     [N][B]   the last minimiser                                                                                T
    u_prev   [B]                                                                                                        T
    shared   Gram (p + L + n) x p float64, shared K (L x p) and C (n x L) as T            -- when has_shared
    terminal wterm_blocks blocks q x q of PN - Qw I: T, or float64 when wterm_from_dare   -- when have_wterm

The handle is n = 2, L = 3, N = 3, batch = 3 with thin-plate RBFs and y = C x: L L = 9 is odd, so sQ = 10 carries a padding
element (its content is not part of the format and is not read here).  kmpc_get_prev_transition refuses a float32 handle that
runs its roll-outs on a float64 core (the default at this dimension set), so the float32 case runs twice: as created by default,
with psi_{k-1} and u_{k-1} held against kmpc_lift of the stepped states and the returned inputs, and without the core
(KMPC_NO_IO32_ROLLOUT), against the getter.  The float64 case is held against both.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

n, L, N, B = 2, 3, 3, 3
p, q = L + 1, n
P0, BARQ0, QW, RW = 3.5, 0.75, 1.5, 0.5  # (weights that keep most moves of the step inside the box)
HEADER_BYTES = 16 * 4 + 2 * 8


def even_up(v):
    return (v + 1) & ~1


sP, sK, sQ, sC = even_up(p * p), even_up(L * p), even_up(L * L), even_up(n * L)


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device; there is no CPU fallback")
    return torch


def parse(blob, dt):
    """-> (header dict, sections dict) by the documented layout; asserts that the sections fill the blob exactly"""
    raw = np.ascontiguousarray(blob, dtype=np.uint8).tobytes()
    ints = np.frombuffer(raw[:64], dtype=np.int32)
    names = ("magic", "version", "dtype", "n", "L", "N", "B", "have_prev", "rls_fresh", "has_shared", "shared_has_samples",
             "have_wterm", "wterm_from_dare", "wterm_per_traj", "wterm_blocks", "reserved")
    hd = dict(zip(names, (int(v) for v in ints)))
    hd["P0"], hd["barQ0"] = (float(v) for v in np.frombuffer(raw[64:HEADER_BYTES], dtype=np.float64))
    o = [HEADER_BYTES]

    def take(dtype, *shape):
        nb = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert o[0] + nb <= len(raw), (o[0], nb, len(raw))
        a = np.frombuffer(raw[o[0]:o[0] + nb], dtype=dtype).reshape(shape)
        o[0] += nb
        return a

    s = {}
    s["P"] = take(dt, B, sP)[:, :p * p].reshape(B, p, p)
    s["K"] = take(dt, B, sK)[:, :L * p].reshape(B, L, p)
    s["Q"] = take(dt, B, sQ)[:, :L * L].reshape(B, L, L)
    s["C"] = take(dt, B, sC)[:, :n * L].reshape(B, n, L)
    s["psi_prev"] = take(dt, B, L)
    s["warm"] = take(dt, N, B)
    s["u_prev"] = take(dt, B)
    if hd["has_shared"]:
        s["gram"] = take(np.float64, p + L + n, p)
        s["Ks"] = take(dt, L, p)
        s["Cs"] = take(dt, n, L)
    if hd["have_wterm"]:
        s["wterm"] = take(np.float64 if hd["wterm_from_dare"] else dt, hd["wterm_blocks"], q, q)
    assert o[0] == len(raw), (o[0], len(raw))
    return hd, s


def export(m):
    """the blob of state_dict(), whose length is kmpc_state_bytes"""
    blob = m.state_dict()["blob"]
    assert blob.size == m.lib.kmpc_state_bytes(m.h)
    return blob


def model_of(m):
    """([A B] (B, L, p), C (B, n, L)) from kmpc_get_model"""
    A, Bm, Cm = [t.cpu().numpy() for t in m.get_model()]
    return np.concatenate([A, Bm], axis=2), Cm


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", ["float64", "float32", "float32-no-core"])
def test_blob_layout_against_the_public_getters(torch_mod, monkeypatch, case):
    torch = torch_mod
    from koopmpc import KoopmanMPC, _ffi

    f64 = case == "float64"
    tdt, dt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
    if case == "float32-no-core":
        monkeypatch.setenv("KMPC_NO_IO32_ROLLOUT", "1")  # (read when the handle is created)
    rng = np.random.RandomState(5)
    cx = 4 * rng.rand(L, n) - 2
    m = KoopmanMPC(n=n, L=L, N=N, batch=B, lift="rbf", centres=cx, output="Cx", dtype=tdt, Qw=QW, Rw=RW)
    want_hd = dict(magic=0x4b4d5043, version=2, dtype=_ffi.KMPC_F64 if f64 else _ffi.KMPC_F32, n=n, L=L, N=N, B=B, have_prev=0,
                   rls_fresh=1, has_shared=0, shared_has_samples=0, have_wterm=0, wterm_from_dare=0, wterm_per_traj=0,
                   wterm_blocks=0, reserved=0, P0=P0, barQ0=BARQ0)
    base_bytes = HEADER_BYTES + np.dtype(dt).itemsize * (B * (sP + sK + sQ + sC) + L * B + N * B + B)

    # P, Q: the diagonal fills of state_init; K = [A B], C: what get_model returns, for three models in turn
    m.state_init(P0, BARQ0)
    for k in range(3):
        A0 = 0.5 * rng.randn(L, L)
        B0, C0 = 0.1 * rng.randn(L, 1), 0.5 * rng.randn(n, L)
        m.set_model(A0, B0, C0)
        blob = export(m)
        assert blob.size == base_bytes
        hd, s = parse(blob, dt)
        assert hd == want_hd, (case, k, hd)
        Kg, Cg = model_of(m)
        for b in range(B):
            assert same_bits(s["P"][b], (P0 * np.eye(p)).astype(dt)), (case, k, b)
            assert same_bits(s["Q"][b], (BARQ0 * np.eye(L)).astype(dt)), (case, k, b)
            assert same_bits(s["K"][b], Kg[b]) and same_bits(s["K"][b], np.concatenate([A0, B0], axis=1).astype(dt)), (case, k, b)
            assert same_bits(s["C"][b], Cg[b]) and same_bits(s["C"][b], C0.astype(dt)), (case, k, b)
        assert not s["psi_prev"].any() and not s["warm"].any() and not s["u_prev"].any(), (case, k)

    # one step: psi_{k-1}, u_{k-1}, the minimiser in its [N][B] order
    X = torch.tensor(4 * rng.rand(n, B) - 2, dtype=tdt, device="cuda:0")
    r = np.tile(0.5 * rng.randn(q, 1), (1, N))
    u = m.step(X, r).cpu().numpy().copy()
    Useq = m.Useq.cpu().numpy().copy()
    assert int(m.status.max().item()) == 0
    assert Useq.shape == (N, B) and len(set(Useq.ravel().tolist())) > B, Useq  # (a sequence that tells [N][B] from [B][N])
    blob = export(m)
    assert blob.size == base_bytes
    hd, s = parse(blob, dt)
    want_hd.update(have_prev=1)
    assert hd == want_hd, (case, hd)
    psi_lift = m.Encoder(X).cpu().numpy().T  # (B, L)
    if case != "float32":
        psi_g, u_g = torch.empty(B, L, dtype=tdt, device="cuda:0"), torch.empty(B, dtype=tdt, device="cuda:0")
        m._chk(m.lib.kmpc_get_prev_transition(m.h, C.c_void_p(psi_g.data_ptr()), C.c_void_p(u_g.data_ptr()), m._stream()),
               "kmpc_get_prev_transition")
        assert same_bits(s["psi_prev"], psi_g.cpu().numpy()), case
        assert same_bits(s["u_prev"], u_g.cpu().numpy()), case
    assert same_bits(s["psi_prev"], np.ascontiguousarray(psi_lift)), case
    assert same_bits(s["u_prev"], u), case
    assert same_bits(s["warm"], Useq), case
    assert same_bits(s["warm"][0], u), case

    # a second step runs the update: every trajectory now has its own model, still what get_model returns
    X2 = torch.tensor(4 * rng.rand(n, B) - 2, dtype=tdt, device="cuda:0")
    m.step(X2, r)
    hd, s = parse(export(m), dt)
    want_hd.update(rls_fresh=0)
    assert hd == want_hd, (case, hd)
    Kg, Cg = model_of(m)
    assert same_bits(s["K"], Kg) and same_bits(s["C"], Cg), case
    assert not same_bits(s["K"][0], s["K"][1]) and not same_bits(s["C"][1], s["C"][2]), case

    # the shared-model section
    X3 = torch.tensor(4 * rng.rand(n, B) - 2, dtype=tdt, device="cuda:0")
    m.shared_step(X3, r)
    assert int(m.status.max().item()) == 0
    shared_bytes = 8 * (p + L + n) * p + np.dtype(dt).itemsize * (L * p + n * L)
    blob = export(m)
    assert blob.size == base_bytes + shared_bytes
    hd, s = parse(blob, dt)
    want_hd.update(has_shared=1, shared_has_samples=1)
    assert hd == want_hd, (case, hd)
    As, Bs, Cs = [t.cpu().numpy() for t in m.shared_model()]
    assert same_bits(s["Ks"], np.concatenate([As, Bs], axis=1)) and same_bits(s["Cs"], Cs), case
    assert s["gram"].any(), case

    # the terminal section: one block of T behind the shared-model section
    G = rng.randn(q, q)
    PN = 3.0 * (G @ G.T / q + 0.1 * np.eye(q)) + QW * np.eye(q)
    m.set_terminal_weight(PN)
    blob = export(m)
    assert blob.size == base_bytes + shared_bytes + np.dtype(dt).itemsize * q * q
    hd, s = parse(blob, dt)
    want_hd.update(have_wterm=1, wterm_blocks=1)
    assert hd == want_hd, (case, hd)
    assert same_bits(s["wterm"][0], (PN - QW * np.eye(q)).astype(dt)), case
    assert same_bits(s["Ks"], np.concatenate([As, Bs], axis=1)), case

    if f64:
        # the Riccati blocks: B blocks of float64.  kmpc_terminal_from_dare hands back P_N = block + Qw I, formed on the host in
        # float64: off the diagonal the block itself, on it block + Qw exactly as rounded there
        PNd, _ = m.terminal_from_dare(per_trajectory=True)
        assert PNd.shape == (B, q, q)
        blob = export(m)
        assert blob.size == base_bytes + shared_bytes + 8 * B * q * q
        hd, s = parse(blob, dt)
        want_hd.update(wterm_from_dare=1, wterm_per_traj=1, wterm_blocks=B)
        assert hd == want_hd, (case, hd)
        w = s["wterm"]
        assert w.dtype == np.float64
        assert same_bits(w + QW * np.eye(q)[None], PNd), case
        off = ~np.eye(q, dtype=bool)
        assert same_bits(w[:, off], PNd[:, off]), case
        assert np.abs(w - (PNd - QW * np.eye(q)[None])).max() <= 2.0 ** -52 * (QW + np.abs(PNd).max()), case
        assert not same_bits(w[0], w[1]), case

    # a fresh handle that imports the blob exports the same bytes
    m2 = KoopmanMPC(n=n, L=L, N=N, batch=B, lift="rbf", centres=cx, output="Cx", dtype=tdt, Qw=QW, Rw=RW)
    m2.load_state_dict({"blob": blob})
    assert export(m2).tobytes() == blob.tobytes(), case
