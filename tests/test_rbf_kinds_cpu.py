"""rbf.m's dictionary kinds without a GPU: the header's enumerators, the ctypes constants, the plug-in table and the name map of
KoopmanMPC agree, and the module-level rbf(X, cx, type=...) handles its arguments as rbf.m:10-17, 41 does.  No handle is created."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_NAMES = {  # KoopmanMPC(lift=...) -> the header's enumerator
    "mlp": "KMPC_LIFT_MLP", "rbf": "KMPC_LIFT_RBF_PY", "rbf_matlab": "KMPC_LIFT_RBF_MATLAB", "rbf_gauss": "KMPC_LIFT_RBF_GAUSS",
    "rbf_invquad": "KMPC_LIFT_RBF_INVQUAD", "rbf_invmultquad": "KMPC_LIFT_RBF_INVMULTQUAD", "rbf_polyharmonic": "KMPC_LIFT_RBF_POLYHARMONIC",
}


def _header_enum():
    src = open(os.path.join(ROOT, "include", "koopmpc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(KMPC_LIFT_(?:MLP|RBF_[A-Z]+))\s*=\s*(\d+)", src)}


def test_header_ffi_and_plugin_table_agree():
    from koopmpc import _ffi, plugins

    enum = _header_enum()
    assert enum == {"KMPC_LIFT_MLP": 0, "KMPC_LIFT_RBF_PY": 1, "KMPC_LIFT_RBF_MATLAB": 2, "KMPC_LIFT_RBF_GAUSS": 3, "KMPC_LIFT_RBF_INVQUAD": 4,
                    "KMPC_LIFT_RBF_INVMULTQUAD": 5, "KMPC_LIFT_RBF_POLYHARMONIC": 6}
    for name, value in enum.items():
        assert getattr(_ffi, name) == value, name
    assert plugins._KIND == {lift: enum[e] for lift, e in _NAMES.items()}
    assert "kmpc_set_rbf_order" in _ffi.SIGNATURES


def test_controller_name_map_covers_the_six_rbf_names():
    from koopmpc import KoopmanMPC

    enum = _header_enum()
    assert KoopmanMPC.LIFT_KINDS == {lift: enum[e] for lift, e in _NAMES.items()}
    assert sum(name.startswith("rbf") for name in KoopmanMPC.LIFT_KINDS) == 6


def test_module_level_rbf_arguments():
    from koopmpc import api

    # without `type`: the Python scripts' rbf(X, cx) as before
    assert api._rbf_arguments(None, "python", None, 1) == ("rbf", 1e-4, 1)
    assert api._rbf_arguments(1e-3, "matlab", None, 1) == ("rbf_matlab", 1e-3, 1)
    # with `type`: rbf.m -- eps defaults to 1 (rbf.m:12-14), the name is lower-cased (rbf.m:11), 'thinplate' is form="matlab"
    assert api._rbf_arguments(None, "python", "gauss", 1) == ("rbf_gauss", 1.0, 1)
    assert api._rbf_arguments(0.5, "python", "InvQuad", 1) == ("rbf_invquad", 0.5, 1)
    assert api._rbf_arguments(None, "python", "ThinPlate", 1) == ("rbf_matlab", 1.0, 1)
    assert api._rbf_arguments(None, "python", "invmultquad", 5) == ("rbf_invmultquad", 1.0, 1)  # (k is read by the polyharmonic only)
    assert api._rbf_arguments(None, "python", "POLYHARMONIC", 3) == ("rbf_polyharmonic", 1.0, 3)
    for k in (0, 9, 2.5):
        with pytest.raises(ValueError):
            api._rbf_arguments(None, "python", "polyharmonic", k)
    with pytest.raises(ValueError, match="RBF type not recognize"):  # rbf.m:41
        api._rbf_arguments(None, "python", "bogus", 1)
    # ... and the public function raises it before it looks for a device
    with pytest.raises(ValueError, match="RBF type not recognize"):
        api.rbf([[0.0], [0.0]], [[0.0, 1.0]], type="bogus")


def test_prebuild_entry_points_refuse_an_unknown_lift_kind():
    """kmpc_create refuses a lift_kind outside 0..6; the two prebuild entry points (no device needed) agree with it"""
    import ctypes

    from koopmpc import _ffi

    lib = _ffi.load()
    buf = ctypes.create_string_buffer(512)
    for kind in (7, 99, -1):
        assert lib.kmpc_rollout_plugin_prebuild(2, 8, 30, 0, kind, 0, 64, _ffi.KMPC_F64, buf, len(buf)) == -3 and b"lift_kind" in buf.value
        assert lib.kmpc_rollout_diag_plugin_prebuild(2, 8, 30, 0, kind, 0, 64, 0, buf, len(buf)) == -3 and b"lift_kind" in buf.value
    # the built-in set with a thin plate needs no object (0); the same set with one of rbf.m's other kinds is a plug-in (1)
    assert lib.kmpc_rollout_plugin_prebuild(2, 8, 30, 0, _ffi.KMPC_LIFT_RBF_MATLAB, 0, 64, _ffi.KMPC_F64, buf, len(buf)) == 0
    assert lib.kmpc_rollout_plugin_prebuild(2, 8, 30, 0, _ffi.KMPC_LIFT_RBF_INVQUAD, 0, 64, _ffi.KMPC_F64, buf, len(buf)) == 1 and b"ksm2" in buf.value
