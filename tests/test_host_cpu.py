"""CPU-side checks: the C-ABI library loads and exports every symbol include/koopmpc.h declares,
the product fails loudly without a GPU (no CPU path), and the multi-GPU host logic (batch
sharding + max-over-ranks timing) works over gloo with world_size 2.  No compute kernels run."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "koopman-online-updated-mpc_amd")


@pytest.fixture(scope="module")
def lib():
    from koopmpc import _ffi

    if not os.path.exists(_ffi.LIB_PATH):
        subprocess.check_call(["make", "-C", PKG, "-j4"])
    return _ffi.load()


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "koopmpc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kmpc_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(lib):
    from koopmpc import _ffi

    names = _declared_symbols()
    assert len(names) >= 20
    assert sorted(_ffi.SIGNATURES) == names  # the ctypes table binds exactly the header's API
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.kmpc_version() >= 100


def test_config_struct_layout_matches_header():
    from koopmpc import _ffi

    src = open(os.path.join(ROOT, "include", "koopmpc.h")).read()
    body = re.search(r"typedef struct kmpc_config \{(.*?)\} kmpc_config;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        for nm in names.split(","):
            fields.append((nm.strip(), typ))
    got = [(n if n != "lam" else "lambda", {ctypes.c_int32: "int32_t", ctypes.c_double: "double"}[t]) for n, t in _ffi.KmpcConfig._fields_]
    assert got == fields


def test_no_gpu_means_loud_failure(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the failure path is not reachable")
    from koopmpc import _ffi

    cfg = _ffi.KmpcConfig(n=2, m=1, L=8, N=10, hidden=100, layers=3, batch=4, dtype=1, lam=1.0, P0=1e4, barQ0=100.0,
                          Qw=100.0, Rw=1e-4, lb=-2.0, ub=2.0, rbf_eps=1e-4)
    h = ctypes.c_void_p()
    rc = lib.kmpc_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc != 0 and not h.value
    assert b"no HIP device" in lib.kmpc_last_error(None)
    from koopmpc import KoopmanMPC

    with pytest.raises(RuntimeError):
        KoopmanMPC(n=2, L=8, N=10, batch=4)


def test_product_never_imports_the_oracle():
    bad = []
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "koopman_oracle" in txt:
                    bad.append(f)
    assert not bad, bad


def test_shard_range_partitions_the_batch():
    from koopmpc import shard_range

    for total in (1, 7, 4096, 262144, 65537):
        for world in (1, 2, 3, 8):
            spans = [shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            for (a, b), (c, d) in zip(spans, spans[1:]):
                assert b == c
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_range(10, 2, 2)


_WORKER = r"""
import os, sys
sys.path.insert(0, {pkg!r})
import torch, torch.distributed as dist
from koopmpc import shard_range, max_over_ranks
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=int(sys.argv[1]), world_size=2)
rank = dist.get_rank()
lo, hi = shard_range(4097, rank, 2)
# every rank owns a disjoint contiguous slice: gather the spans and check the cover
spans = [None, None]
dist.all_gather_object(spans, (lo, hi))
assert spans[0][0] == 0 and spans[0][1] == spans[1][0] and spans[1][1] == 4097, spans
t = max_over_ranks(1.0 + rank)        # bench.py's timing rule: max over ranks
assert t == 2.0, t
# whole-job value = units of all ranks / max time
units = torch.tensor([float(hi - lo)], dtype=torch.float64)
dist.all_reduce(units)
assert units.item() == 4097.0
# shared-model mode: the ONLY collective of the path is the sum of the per-rank Gram blocks
# (KoopmanMPC.shared_step does dist.all_reduce(delta) between its two stages).  Same arithmetic on the
# oracle: per-shard Gram sums, all-reduced, equal the Gram sums of the whole batch.
sys.path.insert(0, {root!r})
import numpy as np
from oracle import koopman_oracle as ko
rng = np.random.RandomState(0)
L, Bt = 6, 101
Psi, U, PsiN, XN = rng.randn(L, Bt), rng.randn(Bt), rng.randn(L, Bt), rng.randn(2, Bt)
lo, hi = shard_range(Bt, rank, 2)
G, YZ, XZ = ko.SharedEdmd.gram(Psi[:, lo:hi], U[lo:hi], PsiN[:, lo:hi], XN[:, lo:hi])
delta = torch.tensor(np.concatenate([G, YZ, XZ], axis=0))
dist.all_reduce(delta, op=dist.ReduceOp.SUM)
Gf, YZf, XZf = ko.SharedEdmd.gram(Psi, U, PsiN, XN)
assert np.allclose(delta.numpy(), np.concatenate([Gf, YZf, XZf], axis=0), rtol=1e-12, atol=1e-12)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_two_rank_gloo_sharding_and_timing(tmp_path):
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "w.py"
    script.write_text(_WORKER.format(pkg=PKG, port=port, root=ROOT))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


_UID_WORKER = r"""
import os, sys
sys.path.insert(0, {pkg!r})
import torch.distributed as dist
from koopmpc.sharding import exchange_unique_id
rank = int(sys.argv[1])
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="{port}", RANK=str(rank), WORLD_SIZE="2")
dist.init_process_group("gloo")
idb = bytes(range(128))
try:
    got = exchange_unique_id(idb if rank == 0 else None)
    assert got == idb
    print("rank", rank, "same id")
except RuntimeError as e:
    print("rank", rank, "refused:", e)
    dist.destroy_process_group()
    sys.exit(3)
dist.destroy_process_group()
"""


@pytest.mark.parametrize("corrupt", [None, 1])
def test_two_rank_unique_id_exchange_is_validated(tmp_path, corrupt):
    """koopmpc.sharding.exchange_unique_id (the RCCL id hand-over of NcclCommunicator, world > 1) over gloo, world size 2: both ranks
    end with rank 0's 128 bytes; when one rank's copy differs, EVERY rank raises before ncclCommInitRank could hang (exit code 3,
    never a re-exec) -- VERDICT r4 item 6b."""
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "u.py"
    script.write_text(_UID_WORKER.format(pkg=PKG, port=port))
    env = dict(os.environ)
    env.pop("KMPC_TEST_CORRUPT_UID_RANK", None)
    if corrupt is not None:
        env["KMPC_TEST_CORRUPT_UID_RANK"] = str(corrupt)
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env) for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == (0 if corrupt is None else 3), o
        assert ("same id" in o) if corrupt is None else ("refused" in o and "differs between the ranks" in o), o


def test_synth_workload_is_deterministic():
    from koopmpc.synth import initial_states, random_mlp_weights

    a = random_mlp_weights(2, 100, 3, 20)
    b = random_mlp_weights(2, 100, 3, 20)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert [w.shape for w, _ in a] == [(100, 2), (100, 100), (100, 100), (20, 100)]
    assert np.abs(a[1][0]).max() <= 0.1 + 1e-12
    x = initial_states(4096)
    assert x.shape == (2, 4096) and np.abs(x).max() <= 2.0


def test_mat_io_roundtrip(tmp_path):
    """.mat compatibility with the reference's weight files and log dumps (Encoder_Duffing.m:2-6, duffing.py:61-64, :1015)."""
    import scipy.io as sio

    from koopmpc import io as kio
    from koopmpc.synth import random_mlp_weights

    w = random_mlp_weights(2, 100, 3, 8)
    f = str(tmp_path / "weights.mat")
    kio.save_encoder_mat(f, w)
    d = sio.loadmat(f)
    assert d["W1"].shape == (100, 2) and d["b1"].shape == (1, 100) and d["W4"].shape == (8, 100)  # the reference's layout
    w2 = kio.load_encoder_mat(f)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(w, w2))
    # the committed golden weights came from the reference's .mat: same loader semantics as the oracle's
    g = np.load(os.path.join(ROOT, "tests", "golden", "weights_tank.npz"))
    kio.save_encoder_mat(f, [(g["W%d" % k], g["b%d" % k]) for k in (1, 2, 3)])
    assert len(kio.load_encoder_mat(f)) == 3
    logX, logU = np.random.rand(7, 2, 3), np.random.rand(7, 3)
    f2 = str(tmp_path / "DuffingPlotrealtime.mat")
    kio.save_closed_loop_mat(f2, logX, logU, r=np.array([[1.0], [0.0]]) * np.ones((1, 10)), traj=1)
    d = sio.loadmat(f2)
    assert d["logXloc"].shape == (2, 7) and d["logUloc"].shape == (1, 7) and d["logR"].shape == (2, 7)
    assert np.array_equal(d["logXloc"][:, 3], logX[3, :, 1]) and np.allclose(d["tspan"].ravel(), 0.05 * np.arange(7))


# --------------------------------------------------------------------------------------
# bench.py host logic (no GPU): every configuration's workload builds, and the CPU baseline leg -- the oracle run the
# reference's way, the only place outside tests/ and smoke() that may use it -- produces trajectory-steps for each of them
# --------------------------------------------------------------------------------------
def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg3-L20", "cfg4", "cfg5"])
def test_bench_workloads_build(name):
    bench = _bench()
    c = bench.CONFIGS[name]
    w = bench.workload_inputs(name, c["L"], c["N"])
    assert w["L"] == c["L"] and w["N"] == c["N"]
    X, Y, U = w["data"]
    assert X.shape == Y.shape and X.shape[0] == 2 and U.shape == (X.shape[1],)
    if c.get("lift") == "rbf":
        assert w["weights"] is None and w["centres"].shape == (c["L"], 2)
    else:
        assert w["centres"] is None and w["weights"][-1][0].shape[0] == c["L"]  # output layer rows = lift dimension
    q = 1 if name == "cfg4" else 2
    assert w["ref"].shape == (q, c["N"])
    x0 = bench.initial_states_for(name, 8, 101)
    assert x0.shape == (2, 8) and np.isfinite(x0).all()
    assert np.array_equal(x0, bench.initial_states_for(name, 8, 101))  # seeded


@pytest.mark.parametrize("name,solver", [("cfg2", "lbfgsb"), ("cfg3", "exact"), ("cfg4", "exact")])
def test_bench_cpu_baseline_worker_makes_steps(name, solver):
    bench = _bench()
    c = bench.CONFIGS[name]
    x0 = bench.initial_states_for(name, 4, 101)
    # (name, L, N, x0, budget, solver, settle steps that are set-up, first steps timed as the post-reset transient)
    done, secs, tdone, tsecs = bench._cpu_worker((name, c["L"], c["N"], x0, 1.5, solver, 3, 2))
    assert done >= 1 and secs > 0.0 and tdone >= 2 and tsecs > 0.0


@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg4"])
def test_bench_parity_probe_worker_on_the_host(name, tmp_path, capsys):
    """The oracle half of bench.py's parity probe (a child process of the cpu_baseline leg; round 4) on files made here: inputs that
    ARE the exact minimisers' first moves for the given models and states must come back with error 0, a perturbed one with exactly
    the perturbation -- so the number in the bench line is the device's distance from the oracle and nothing else."""
    import json

    from oracle import koopman_oracle as ko

    bench = _bench()
    c = bench.CONFIGS[name]
    L, N = c["L"], c["N"]
    w = bench.workload_inputs(name, L, N)
    lift = (lambda x: ko.rbf_lift(x, w["centres"])) if c.get("lift") == "rbf" else (lambda x: ko.mlp_lift(w["weights"], x))
    rng = np.random.RandomState(5)
    nb = 3
    X = np.abs(rng.rand(2, nb)) if name == "cfg4" else 4 * rng.rand(2, nb) - 2
    A = rng.randn(nb, L, L) * 0.2 / np.sqrt(L)
    Bm = rng.randn(nb, L, 1) * 0.1
    Cm = rng.randn(nb, 2, L) * 0.3
    uprev = rng.randn(nb) * 0.2 if name == "cfg4" else np.zeros(nb)
    u = np.zeros(nb)
    for i in range(nb):
        psi = lift(X[:, i:i + 1]).reshape(-1)
        if name == "cfg4":
            ctl = ko.OracleDeltaUController(lift, L, 2, N, A[i], Bm[i], Cm[i])
            ctl.u = float(uprev[i])
            At, Bt, Co, xt = ctl.qp(psi)
            _, _, H, f, _ = ko.condense(At, Bt, Co, xt, w["ref"], N, ctl.Qw, ctl.Rw)
            lbv = np.full(N, ctl.lb); ubv = np.full(N, ctl.ub)
            lbv[0] = max(ctl.lb, ctl.umin - ctl.u); ubv[0] = min(ctl.ub, ctl.umax - ctl.u)
            u[i] = ctl.u + float(ko.qp_exact(H, f, lbv, ubv)[0][0])
        else:
            _, _, H, f, _ = ko.condense(A[i], Bm[i], Cm[i], psi, w["ref"], N, 100.0, 1e-4)
            u[i] = float(ko.qp_exact(H, f, c["lb"], c["ub"])[0][0])
    for delta in (0.0, 3e-5):
        path = str(tmp_path / ("probe_%s_%g.npz" % (name, delta)))
        ug = u.copy(); ug[1] += delta
        np.savez(path, name=name, L=L, N=N, X=X, A=A, B=Bm, C=Cm, u=ug, uprev=uprev)
        bench._probe_worker(path)
        out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert out["n"] == nb and abs(out["max_abs_u_err"] - delta) <= 1e-12


def test_bench_flop_and_byte_counts():
    """SURVEY 8d's algorithmic flop formulas as bench.py evaluates them (the table's totals at 100 Newton solves) and the executed
    count beside them (never above the algorithmic one for the per-trajectory modes: the Toeplitz build is cheaper than the dense H)."""
    bench = _bench()
    # SURVEY 8d totals at iters = 100: cfg1/2 224 806, cfg5 2 527 302
    assert bench.algorithmic_flops("cfg2", 20, 20, 2, 100) == 224806
    assert bench.algorithmic_flops("cfg5", 64, 50, 2, 100) == 2527302
    for name, q in (("cfg2", 2), ("cfg3", 2), ("cfg3-L20", 2), ("cfg5", 2)):
        c = bench.CONFIGS[name]
        ex, al = bench.executed_flops(name, c["L"], c["N"], q, 1.1), bench.algorithmic_flops(name, c["L"], c["N"], q, 1.1)
        assert 0 < ex < al


# ------------------------------------------------------------------ roll-out plug-ins (no device needed: hipcc cross-compiles)
def test_rollout_plugin_is_built_cached_and_self_contained(lib, tmp_path, monkeypatch):
    """csrc/rollout_plugin.hip without a GPU: kmpc_rollout_plugin_prebuild for a dimension set libkoopmpc.so has no instantiation
    for (7, 9, 2) compiles csrc/rollout_jit.hip with hipcc into $KMPC_KERNEL_CACHE (code 1, the text names the file and the seconds);
    the object exports the three plug-in entry points and needs no symbol of libkoopmpc.so (it is loaded with RTLD_LOCAL into
    processes that may hold another build of the library); a built-in set answers 0 and compiles nothing; a set the fused kernel
    cannot take (four waves per trajectory: L = 64) answers 2; bad arguments -3."""
    from koopmpc import _ffi

    monkeypatch.setenv("KMPC_KERNEL_CACHE", str(tmp_path))
    buf = ctypes.create_string_buffer(1024)

    def pre(n, L, N, rows, lift, hidden, B, dtype):
        rc = lib.kmpc_rollout_plugin_prebuild(n, L, N, rows, lift, hidden, B, dtype, buf, len(buf))
        return rc, buf.value.decode()

    rc, text = pre(2, 7, 9, 0, _ffi.KMPC_LIFT_RBF_PY, 0, 100, _ffi.KMPC_F64)
    assert rc == 1 and "compiled with hipcc" in text and str(tmp_path) in text, (rc, text)
    objs = [f for f in os.listdir(tmp_path) if f.endswith(".so")]
    assert len(objs) == 1 and objs[0].startswith("rollout_L7_N9_q2_nw16_ksm1_f64_"), objs
    assert not [f for f in os.listdir(tmp_path) if ".tmp." in f or ".log." in f]
    path = os.path.join(str(tmp_path), objs[0])
    dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for sym in ("kmpc_rollout_plugin_abi", "kmpc_rollout_plugin_args_bytes", "kmpc_rollout_plugin_launch"):
        assert sym in dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True).stdout
    assert "kmpc" not in und, und
    # the same request again: the process table, no second object
    rc2, text2 = pre(2, 7, 9, 0, _ffi.KMPC_LIFT_RBF_PY, 0, 100, _ffi.KMPC_F64)
    assert (rc2, text2) == (rc, text)
    assert pre(2, 20, 20, 0, _ffi.KMPC_LIFT_MLP, 100, 4096, _ffi.KMPC_F64)[0] == 0      # BASELINE cfg2: inside the library
    assert pre(2, 64, 50, 0, _ffi.KMPC_LIFT_MLP, 100, 64, _ffi.KMPC_F64)[0] == 2        # cfg5: four waves per trajectory, per-step kernels
    assert pre(2, 7, 9, 0, _ffi.KMPC_LIFT_MLP, 0, 100, _ffi.KMPC_F64)[0] == -3
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".so")]) == 1


def test_rollout_plugin_failure_is_reported_not_fatal(lib, tmp_path, monkeypatch):
    """No compiler: the plug-in cannot be made; the entry point says so (code -1, the compiler's name in the text) -- a handle of such
    a set then works with per-step launches (kmpc_rollout_is_fused = 0; kmpc_rollout_plugin_status carries the same text)."""
    from koopmpc import _ffi

    monkeypatch.setenv("KMPC_KERNEL_CACHE", str(tmp_path))
    monkeypatch.setenv("KMPC_HIPCC", "/nonexistent/hipcc")
    buf = ctypes.create_string_buffer(1024)
    rc = lib.kmpc_rollout_plugin_prebuild(2, 9, 7, 0, _ffi.KMPC_LIFT_RBF_PY, 0, 10, _ffi.KMPC_F64, buf, len(buf))
    assert rc == -1 and "/nonexistent/hipcc" in buf.value.decode(), (rc, buf.value)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".so")]


def test_rollout_plugin_requested_by_several_processes_at_once(tmp_path):
    """The ranks of a node create their controllers at the same moment: three processes ask for the same plug-in with an empty cache.
    The file lock lets ONE of them compile; the others wait and load its object (code 1 for all, "compiled" in exactly one text,
    "built by another process" or "kernel cache" in the others, one object and no left-overs in the directory)."""
    code = (
        "import ctypes, os, sys\n"
        "sys.path.insert(0, %r)\n"
        "from koopmpc import _ffi\n"
        "lib = _ffi.load()\n"
        "buf = ctypes.create_string_buffer(1024)\n"
        "rc = lib.kmpc_rollout_plugin_prebuild(2, 6, 11, 0, _ffi.KMPC_LIFT_RBF_PY, 0, 64, _ffi.KMPC_F64, buf, len(buf))\n"
        "print(rc, buf.value.decode())\n"
    ) % os.path.join(ROOT, "koopman-online-updated-mpc_amd")
    env = dict(os.environ, KMPC_KERNEL_CACHE=str(tmp_path))
    procs = [subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for _ in range(3)]
    outs = [p.communicate(timeout=600) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-400:] for o in outs]
    texts = [o[0].strip().splitlines()[-1] for o in outs]
    assert all(t.startswith("1 ") for t in texts), texts
    assert sum("compiled with hipcc" in t for t in texts) == 1, texts
    assert sum(("built by another process" in t) or ("loaded from the kernel cache" in t) for t in texts) == 2, texts
    files = os.listdir(tmp_path)
    assert len([f for f in files if f.endswith(".so")]) == 1, files
    assert not [f for f in files if ".tmp." in f or ".log." in f], files
    # the lock file stays (every process locks the same inode), and a fourth process loads the object without compiling
    assert len([f for f in files if f.endswith(".so.lock")]) == 1, files
    [(rc, text)] = _prebuild_in(env, (2, 6, 11, 0, 1, 0, 64, 1))
    assert rc == 1 and "loaded from the kernel cache" in text, text
    assert sorted(os.listdir(tmp_path)) == sorted(files)


# (the plug-in tests below run the library in fresh processes, from a copy whose own <library dir>/kernel_cache is the test's)
_RBF, _F64 = 1, 1  # (koopmpc._ffi.KMPC_LIFT_RBF_PY, KMPC_F64)
_HIPCC = "/opt/rocm/bin/hipcc" if os.access("/opt/rocm/bin/hipcc", os.X_OK) else shutil.which("hipcc")


def _plugin_sandbox(root, **env):
    """libkoopmpc.so and its plug-in sources copied to root/lib, and an environment whose every kernel cache directory lies under root
    ($HOME, $XDG_CACHE_HOME, $TMPDIR; $KMPC_KERNEL_CACHE and $KMPC_HIPCC only as given): a process started with it is hermetic."""
    lib = root / "lib"
    lib.mkdir()
    shutil.copy(os.path.join(PKG, "libkoopmpc.so"), lib)
    shutil.copytree(os.path.join(PKG, "csrc"), lib / "csrc", ignore=shutil.ignore_patterns("*.o"))
    for d in ("home", "tmp"):
        (root / d).mkdir(mode=0o700)
    e = {k: v for k, v in os.environ.items() if k not in ("KMPC_KERNEL_CACHE", "KMPC_HIPCC")}
    e.update(KMPC_LIB=str(lib / "libkoopmpc.so"), HOME=str(root / "home"), XDG_CACHE_HOME=str(root / "home" / "xdg"), TMPDIR=str(root / "tmp"))
    e.update(env)
    return e


def _hipcc_wrapper(path, version=None, compile_=None):
    """A compiler for KMPC_HIPCC: `--version` and compiles go to the real hipcc unless replaced by the given shell lines."""
    path.write_text("#!/bin/sh\nif [ \"$1\" = --version ]; then\n%s\nelse\n%s\nfi\n"
                    % (version or '%s --version' % _HIPCC, compile_ or '%s "$@"' % _HIPCC))
    path.chmod(0o755)
    return str(path)


def _prebuild_in(env, *sets):
    """kmpc_rollout_plugin_prebuild of each set in one fresh process: [(code, text)]."""
    code = (
        "import ctypes, sys\n"
        "sys.path.insert(0, %r)\n"
        "from koopmpc import _ffi\n"
        "lib = _ffi.load()\n"
        "buf = ctypes.create_string_buffer(4096)\n"
        "for a in %r:\n"
        "    print(lib.kmpc_rollout_plugin_prebuild(*a, buf, len(buf)), buf.value.decode())\n"
    ) % (PKG, list(sets))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return [(int(line.split(" ", 1)[0]), line.split(" ", 1)[1]) for line in p.stdout.strip().splitlines()]


def test_rollout_plugin_cache_directories_must_be_trusted(tmp_path):
    """A plug-in is code the process runs: a kernel cache directory that is world-writable, a symbolic link (here to a trusted
    directory) or owned by another user is skipped -- a valid object under the exact expected name there is not loaded, nothing is
    written there, and the status text names the directory and why."""
    S = (2, 5, 9, 0, _RBF, 0, 64, _F64)
    env = _plugin_sandbox(tmp_path)
    good = tmp_path / "good"
    good.mkdir(mode=0o700)
    [(rc, text)] = _prebuild_in(dict(env, KMPC_KERNEL_CACHE=str(good)), S)
    assert rc == 1 and "compiled with hipcc" in text and str(good) in text, text
    [obj] = [f for f in os.listdir(good) if f.endswith(".so")]
    own = tmp_path / "lib" / "kernel_cache"  # (the trusted place the processes below find the object in)
    own.mkdir(mode=0o700)
    shutil.copy(good / obj, own)
    wide, link, other = tmp_path / "wide", tmp_path / "link", tmp_path / "other"
    wide.mkdir()
    shutil.copy(good / obj, wide)
    wide.chmod(0o777)
    link.symlink_to(good)
    cases = [(wide, "writable by group or others"), (link, "a symbolic link")]
    if os.geteuid() == 0:
        other.mkdir(mode=0o755)
        shutil.copy(good / obj, other)
        os.chown(other, 65534, 65534)
        cases.append((other, "owned by uid 65534"))
    else:
        cases.append(("/usr", "owned by uid %d" % os.stat("/usr").st_uid))
    for d, why in cases:
        before = sorted(os.listdir(d))
        [(rc, text)] = _prebuild_in(dict(env, KMPC_KERNEL_CACHE=str(d)), S)
        assert rc == 1 and "loaded from the kernel cache" in text and str(own / obj) in text, (d, text)
        assert "skipped %s: %s" % (d, why) in text, (d, text)
        assert sorted(os.listdir(d)) == before, d


def test_rollout_plugin_cache_directory_modes(tmp_path):
    """A cache directory the library makes has mode 0700; a pre-existing $TMPDIR/koopmpc-<uid> that fails the trust rule is refused
    (the compiler here answers --version and fails every compile: no object is needed to see where it would go)."""
    S = (2, 5, 10, 0, _RBF, 0, 64, _F64)
    cc = _hipcc_wrapper(tmp_path / "cc", compile_="echo no compiles in this test; exit 1")
    env = _plugin_sandbox(tmp_path, KMPC_HIPCC=cc)
    made = tmp_path / "new" / "cache"
    [(rc, text)] = _prebuild_in(dict(env, KMPC_KERNEL_CACHE=str(made)), S)
    assert rc == -1 and "no compiles in this test" in text, text
    assert os.stat(made).st_mode & 0o777 == 0o700
    assert not [f for f in os.listdir(made) if ".tmp." in f or f.endswith(".so")]
    # only the temporary directory is left: the library's own cache is world-writable, $HOME and $XDG_CACHE_HOME are unset
    (tmp_path / "lib" / "kernel_cache").mkdir()
    (tmp_path / "lib" / "kernel_cache").chmod(0o777)
    last = tmp_path / "tmp" / ("koopmpc-%d" % os.geteuid())
    last.mkdir()
    last.chmod(0o777)
    env = dict(env, HOME="", XDG_CACHE_HOME="")
    [(rc, text)] = _prebuild_in(env, S)
    assert rc == -1 and "no usable kernel cache directory" in text and "skipped %s: writable by group or others" % last in text, text
    assert os.listdir(last) == []
    last.rmdir()
    [(rc, text)] = _prebuild_in(env, S)
    assert rc == -1 and "no compiles in this test" in text, text
    assert os.stat(last).st_mode & 0o777 == 0o700


def test_rollout_plugin_compile_does_not_block_other_sets(tmp_path):
    """The process-wide table is not locked across a compile: while one thread waits for hipcc on set X (a compiler that sleeps
    first), another thread's request for set Y -- already in the kernel cache -- is answered at once."""
    X, Y = (2, 5, 11, 0, _RBF, 0, 64, _F64), (2, 5, 12, 0, _RBF, 0, 64, _F64)
    cache = tmp_path / "cache"
    cache.mkdir(mode=0o700)
    env = _plugin_sandbox(tmp_path, KMPC_KERNEL_CACHE=str(cache))
    assert _prebuild_in(env, Y)[0][0] == 1
    slow = _hipcc_wrapper(tmp_path / "slow_cc", compile_='sleep 4; %s "$@"' % _HIPCC)
    code = (
        "import ctypes, os, sys, threading, time\n"
        "sys.path.insert(0, %r)\n"
        "from koopmpc import _ffi\n"
        "lib = _ffi.load()\n"
        "def pre(a):\n"
        "    buf = ctypes.create_string_buffer(4096)\n"
        "    return lib.kmpc_rollout_plugin_prebuild(*a, buf, len(buf)), buf.value.decode()\n"
        "os.environ['KMPC_HIPCC'] = %r\n"
        "out = {}\n"
        "t = threading.Thread(target=lambda: out.update(x=pre(%r)))\n"
        "t.start()\n"
        "time.sleep(1.5)\n"
        "t0 = time.time()\n"
        "y = pre(%r)\n"
        "dt, busy = time.time() - t0, t.is_alive()\n"
        "t.join()\n"
        "print(repr((y, dt, busy, out['x'])))\n"
    ) % (PKG, slow, X, Y)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    y, dt, busy, x = eval(p.stdout.strip().splitlines()[-1])
    assert y[0] == 1 and "loaded from the kernel cache" in y[1], y
    assert busy and dt < 0.5, (dt, busy)
    assert x[0] == 1 and "compiled with hipcc" in x[1], x


def test_rollout_plugin_name_carries_the_compiler(tmp_path):
    """The object's hash covers the compiler's --version: with the real hipcc two fresh processes agree on the name (the second loads
    the first one's object); a compiler that says it is another version gets an object of its own."""
    S = (2, 5, 13, 0, _RBF, 0, 64, _F64)
    cache = tmp_path / "cache"
    cache.mkdir(mode=0o700)
    env = _plugin_sandbox(tmp_path, KMPC_KERNEL_CACHE=str(cache))
    [(rc1, t1)], [(rc2, t2)] = _prebuild_in(env, S), _prebuild_in(env, S)
    assert rc1 == 1 and "compiled with hipcc" in t1 and rc2 == 1 and "loaded from the kernel cache" in t2, (t1, t2)
    [obj] = [f for f in os.listdir(cache) if f.endswith(".so")]
    assert obj in t1 and obj in t2
    other = _hipcc_wrapper(tmp_path / "other_cc", version="echo 'HIP version: 0.0.0'; echo 'clang version 0.0.0'")
    [(rc3, t3)] = _prebuild_in(dict(env, KMPC_HIPCC=other), S)
    assert rc3 == 1 and "compiled with hipcc" in t3, t3
    objs = sorted(f for f in os.listdir(cache) if f.endswith(".so"))
    assert len(objs) == 2 and objs[0][:-20] == objs[1][:-20], objs  # (same set, different _<hash>.so)


def test_plugins_prune_keeps_current_objects_and_other_files(tmp_path):
    """koopmpc.plugins.prune (what __graft_entry__.build() runs on the tree's kernel cache): objects and lock files of other hashes
    go, those of the current ones and every unrelated file stay."""
    from koopmpc import plugins

    cur, old = "0123456789abcdef", "fedcba9876543210"
    names = ["rollout_L10_N10_q2_nw8_ks0_f64_%s.so" % cur, "rollout_L10_N10_q2_nw8_ks0_f64_%s.so.lock" % cur,
             "rollout_L7_N9_q2_nw16_ksm1_f64_term_%s.so" % cur, "rollout_L10_N10_q2_nw8_ks0_f64_%s.so" % old,
             "rollout_L10_N10_q2_nw8_ks0_f64_%s.so.lock" % old, "rollout_L7_N9_q2_nw16_ksm1_f32_%s.so" % old, "README", "notes.so"]
    for n in names:
        (tmp_path / n).write_text("x")
    gone = plugins.prune(str(tmp_path), {cur})
    assert sorted(gone) == sorted(n for n in names if old in n)
    assert sorted(os.listdir(tmp_path)) == sorted(n for n in names if old not in n)


def test_device_buffer_type_on_a_failing_host_allocator(tmp_path):
    """csrc/devbuf.h (the owning buffers of api.hip) on the CPU: tests/devbuf_check.cpp instantiates DevBuf with a host allocator that
    counts its blocks and refuses the k-th request, built as a program of its own with AddressSanitizer and UBSan.  It checks that
    destruction, reset and moves free every block exactly once; that a refused grow returns the error and leaves pointer and capacity;
    that three buffers grown together (the shape of Impl::dare_buffers, on the header's replace_together) free what the call had
    allocated and keep the old blocks when request 1, 2 or 3 is refused; that ensure on a non-empty buffer makes no request."""
    # (ROCm's clang, which hipcc itself runs, links the sanitizer runtimes statically)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(_HIPCC)))
    rocm_clang = os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    cxx = rocm_clang if os.access(rocm_clang, os.X_OK) else (shutil.which("clang++") or shutil.which("g++"))
    exe = str(tmp_path / "devbuf_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(PKG, "csrc"),
                            os.path.join(ROOT, "tests", "devbuf_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "devbuf ok" in run.stdout, (run.stdout, run.stderr[-3000:])


def test_handle_state_types_against_the_flags_they_replaced(tmp_path):
    """csrc/state_home.h (where a handle's state is valid, the estimator's progress, the kind of terminal block) on the CPU:
    tests/state_home_check.cpp, built as a program of its own with AddressSanitizer and UBSan, holds the flag statements api.hip had
    before as reference models.  Every sequence of up to six of the operations dense-read, dense-write, take-fast, dense-overwritten,
    drop-fast and steps-0 prepare, with and without a fast form: StateHome asks for the same conversions at the same points as the two
    booleans did, never without a fast form, and has no state for the pair (false, false) that the booleans could reach.
    Progress::advance(steps, on) equals `steps` applications of the one-step rule (steps 0..5, update on and off, every start);
    term_from_flags accepts exactly the four triples a handle can write and round-trips."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(_HIPCC)))
    rocm_clang = os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    cxx = rocm_clang if os.access(rocm_clang, os.X_OK) else (shutil.which("clang++") or shutil.which("g++"))
    exe = str(tmp_path / "state_home_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "state_home_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "state_home ok" in run.stdout, (run.stdout, run.stderr[-3000:])


def test_tools_scripts_compile():
    """VERDICT r5 hygiene: every script under tools/ is at least well-formed -- Python files byte-compile, shell scripts pass `bash -n` --
    and none of them refers to a compile-time experiment switch that no longer exists in the product headers."""
    gone = ("KMPC_EXP_", "KMPC_DEV_LIFT")
    n = 0
    for dirpath, _, files in os.walk(os.path.join(ROOT, "tools")):
        for f in files:
            path = os.path.join(dirpath, f)
            if f.endswith(".py"):
                compile(open(path).read(), path, "exec")
            elif f.endswith(".sh"):
                assert subprocess.run(["bash", "-n", path]).returncode == 0, path
            else:
                continue
            n += 1
            src = open(path).read()
            for g in gone:
                assert g not in src, (path, g)
    assert n >= 10
