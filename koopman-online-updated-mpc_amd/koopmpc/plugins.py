"""Roll-out plug-ins from Python: fill the kernel cache ahead of the first controller of a dimension set.

libkoopmpc.so holds the fused roll-out kernel for the dimension sets BASELINE.json and the reference's scripts use; a controller
of any other set gets its kernel when it is created (csrc/rollout_plugin.hip: kernel cache on disk, else hipcc on
csrc/rollout_jit.hip, 4-8 s).  `prebuild` does that step without a device -- `__graft_entry__.build()` calls it for DEFAULT_SETS
so that the objects travel with the tree, and `prune` then drops the objects of older sources or compilers from the tree's cache."""
from __future__ import annotations

import ctypes as C
import os
import re

from . import _ffi

# rollout_L.._N.._q.._nw.._ks.._f64|f32[_term][_diag]_<hash>.so and its lock file; the hash covers the sources, the flags and the compiler
_OBJECT = re.compile(r"^rollout_\w+_([0-9a-f]{16})\.so(\.lock)?$")

# (n, L, N, out_rows, lift, effective hidden width, batch, dtype)
#   the MATLAB twin of the reference: liftFun = [x; Encoder(x)] - [0; Encoder(0)], L = 10, N = 10 (Koopman_update.m:67, 70, 113) --
#   lift_offset "x_psi0" carries x through the encoder on 2 n extra hidden units: 104
DEFAULT_SETS = [
    (2, 10, 10, 0, "mlp", 104, 64, "f64"),
    (2, 10, 10, 0, "mlp", 104, 4096, "f64"),
    (2, 10, 10, 0, "mlp", 100, 4096, "f64"),
    # rbf.m's gauss / invquad / invmultquad / polyharmonic dictionaries at BASELINE cfg3's set and at the reference's (8, 10)
    (2, 8, 30, 0, "rbf_gauss", 0, 4096, "f64"),
    (2, 8, 30, 0, "rbf_gauss", 0, 4096, "f32"),  # (... behind float32 panels: a KMPC_F32 handle of that set)
    (2, 8, 10, 0, "rbf_gauss", 0, 64, "f64"),
]
# The diagnostics variants of the fused roll-out (kmpc_set_rollout_diagnostics; always plug-ins, float64), in the form of DEFAULT_SETS:
# the dtype field reads "f64+diag", or "f64+term+diag" for the variant that also holds the terminal refresh.  The reference's set
# (8, 10), BASELINE cfg2 (20, 20) and cfg3 (8, 30, RBF).
DIAG_SETS = [
    (2, 8, 10, 0, "mlp", 100, 64, "f64+diag"),
    (2, 8, 10, 0, "mlp", 100, 64, "f64+term+diag"),
    (2, 20, 20, 0, "mlp", 100, 4096, "f64+diag"),
    (2, 8, 30, 0, "rbf", 0, 4096, "f64+diag"),
    (2, 8, 10, 0, "rbf_gauss", 0, 64, "f64+diag"),  # (rbf.m's other kinds at the reference's set)
]
_KIND = {"mlp": _ffi.KMPC_LIFT_MLP, "rbf": _ffi.KMPC_LIFT_RBF_PY, "rbf_matlab": _ffi.KMPC_LIFT_RBF_MATLAB,
         # (rbf.m's other kernels: ONE object for the four -- ..._ksm2_... beside the thin plates' ..._ksm1_... --, always a plug-in,
         #  also for the built-in dimension sets; which of the four, its width and k are launch arguments)
         "rbf_gauss": _ffi.KMPC_LIFT_RBF_GAUSS, "rbf_invquad": _ffi.KMPC_LIFT_RBF_INVQUAD,
         "rbf_invmultquad": _ffi.KMPC_LIFT_RBF_INVMULTQUAD, "rbf_polyharmonic": _ffi.KMPC_LIFT_RBF_POLYHARMONIC}


def prebuild(sets=None, verbose=False):
    """Make (or find) the plug-ins of the given configurations; returns [(set, code, text)] with code as kmpc_rollout_plugin_status
    (a diagnostics set: 1 plug-in, 2 no fused variant -- per-step launches --, -1 failed).
    NOTE: without `sets` this is DEFAULT_SETS followed by DIAG_SETS -- five more objects, 5-6 s of hipcc each on a cold cache.
    `__graft_entry__.build()` calls it this way, so that the diagnostics plug-ins of the reference's and the BASELINE sets travel with
    the tree and `prune` keeps them."""
    lib = _ffi.load()
    out = []
    for st in ((DEFAULT_SETS + DIAG_SETS) if sets is None else sets):
        n, L, N, out_rows, lift, hidden, batch, dtype = st
        buf = C.create_string_buffer(1024)
        if dtype.endswith("+diag"):
            fn, last = lib.kmpc_rollout_diag_plugin_prebuild, int("+term" in dtype)
        else:
            fn, last = lib.kmpc_rollout_plugin_prebuild, _ffi.KMPC_F64 if dtype == "f64" else _ffi.KMPC_F32
        code = int(fn(n, L, N, out_rows, _KIND[lift], hidden, batch, last, buf, len(buf)))
        text = buf.value.decode("utf-8", "replace")
        if verbose:
            print("plug-in %s: %d %s" % (st, code, text))
        out.append((st, code, text))
    return out


def object_hash(path):
    """The hash suffix of a plug-in object's file name, or None."""
    m = _OBJECT.match(os.path.basename(path))
    return m.group(1) if m else None


def prune(cache_dir, keep_hashes):
    """Remove the plug-in objects (and their lock files) in `cache_dir` whose hash is not in `keep_hashes`; every other file stays.
    Returns the names removed."""
    gone = []
    for f in sorted(os.listdir(cache_dir)):
        h = object_hash(f)
        if h is not None and h not in keep_hashes:
            os.remove(os.path.join(cache_dir, f))
            gone.append(f)
    return gone
