"""Host side of the packed-row calls (kmpc_state_pack / _unpack / _transfer): the re-sharding plan of koopmpc.sharding, the ctypes
signatures, and the segment table of csrc/state_rows.h on the CPU under AddressSanitizer and UBSan.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "koopman-online-updated-mpc_amd")


def test_reshard_plan_tiles_the_batch_exactly_once():
    """For every total in 0..40 and old / new worlds in 1..5: the segments of all new ranks tile [0, total) exactly once, every
    segment lies inside one old slice and one new slice (both shard_range cuts), and they come in ascending order."""
    from koopmpc.sharding import reshard_plan, shard_range

    for total in range(41):
        for ow in range(1, 6):
            for nw in range(1, 6):
                cover = [0] * total
                last_end = 0
                for nr in range(nw):
                    lo, hi = shard_range(total, nr, nw)
                    at = 0  # local index the next segment must start at
                    prev_old = -1
                    for orank, olo, nlo, cnt in reshard_plan(total, ow, nw, nr):
                        assert cnt > 0 and 0 <= orank < ow and orank > prev_old, (total, ow, nw, nr)
                        prev_old = orank
                        a, b = shard_range(total, orank, ow)
                        assert 0 <= olo and olo + cnt <= b - a, (total, ow, nw, nr)   # inside the old rank's slice
                        assert nlo == at and nlo + cnt <= hi - lo, (total, ow, nw, nr)  # contiguous inside the new one
                        assert a + olo == lo + nlo == last_end, (total, ow, nw, nr)      # the same global trajectories, ascending
                        for g in range(a + olo, a + olo + cnt):
                            cover[g] += 1
                        at += cnt
                        last_end += cnt
                    assert at == hi - lo, (total, ow, nw, nr)
                assert cover == [1] * total, (total, ow, nw)


def test_ctypes_signatures_of_the_four_row_calls():
    from koopmpc import _ffi

    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    want = {
        "kmpc_state_row_elems": (i64, [vp]),
        "kmpc_state_pack": (i32, [vp, vp, i32, vp, vp]),
        "kmpc_state_unpack": (i32, [vp, vp, i32, vp, vp]),
        "kmpc_state_transfer": (i32, [vp, vp, vp, vp, i32, vp]),
    }
    for name, sig in want.items():
        assert _ffi.SIGNATURES[name] == sig, name
    src = open(os.path.join(ROOT, "include", "koopmpc.h")).read()
    for name in want:
        assert name + "(" in src, name
    lib = _ffi.load()
    for name in want:
        assert getattr(lib, name).argtypes == want[name][1]
    assert lib.kmpc_state_row_elems(None) == -1 and lib.kmpc_state_pack(None, None, 0, None, None) == -1


def test_segment_table_under_address_sanitizer(tmp_path):
    """tests/state_rows_check.cpp: build_row_plan (csrc/state_rows.h, the one implementation of the row layout) on lists shaped as
    Impl::sections makes them, for the four dimension sets of tests/test_gpu_state_rows.py -- offsets, lengths, row_elems, and a walk
    over every address the row kernels form from the table, on host blocks of exactly the sections' sizes.  A program of its own,
    built with AddressSanitizer and UBSan."""
    hipcc = "/opt/rocm/bin/hipcc" if os.access("/opt/rocm/bin/hipcc", os.X_OK) else shutil.which("hipcc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    rocm_clang = os.path.join(rocm, "lib", "llvm", "bin", "clang++")  # (ROCm's clang links the sanitizer runtimes statically)
    cxx = rocm_clang if os.access(rocm_clang, os.X_OK) else (shutil.which("clang++") or shutil.which("g++"))
    exe = str(tmp_path / "state_rows_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(PKG, "csrc"),
                            os.path.join(ROOT, "tests", "state_rows_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "state rows ok" in run.stdout, (run.stdout, run.stderr[-3000:])
