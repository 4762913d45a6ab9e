"""The debug tests' one harness around the DEBUG library (make -C fs-nerf_amd/csrc debug -> libfsnerf_hip_dbg.so: the
checked kernels record an index outside their arrays per translation unit, csrc/common.hpp; include/fsnerf_hip.h lists
the units and the record's four words).  A test calls run_worker(script): the worker runs its cases through the debug
library in a fresh child process and emit()s the records it took, "all" (every registered unit, read last) among them."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fs-nerf_amd", "csrc")
DBG = os.path.join(CSRC, "libfsnerf_hip_dbg.so")
TAG = "DEBUG_REPORT "


# ---------------------------------------------------------------- parent side
def build_debug_library():
    if not os.path.exists(DBG):  # (__graft_entry__.build() makes it; a bare checkout builds it here)
        r = subprocess.run(["make", "-C", CSRC, "-j4", "debug"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return DBG


def run_worker(script, timeout=600):
    """Runs tests/<script> against the debug library in a child process; returns what it emitted."""
    env = dict(os.environ, FSN_LIB_PATH=build_debug_library())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script)], capture_output=True, text=True, env=env,
                         cwd=ROOT, timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith(TAG)][-1]
    return json.loads(line[len(TAG):])


def assert_no_other_unit_recorded(rep):
    """rep["all"] is read after the worker took its own units: a count left there is a violation in a unit that the
    worker did not think it exercised (a shared header, a kernel pulled in indirectly)."""
    hit = {unit: rec for unit, rec in rep["all"].items() if rec[0] != 0}
    assert not hit, f"units that recorded a violation: {hit} (count, line, index, extent)"


# ---------------------------------------------------------------- worker side
def open_debug_library():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib
    assert "dbg" in os.path.basename(_lib.LIB_PATH), _lib.LIB_PATH
    return _lib


def take(unit):
    """The unit's record (count, source line, index, extent); the call clears it."""
    from fs_nerf_amd import _lib
    buf = (C.c_uint32 * 4)()
    _lib.check(_lib.lib().fsn_debug_report(unit.encode(), buf), "fsn_debug_report")
    return list(buf)


def take_all():
    from fs_nerf_amd import _lib
    return {unit: take(unit) for unit in _lib.lib().fsn_debug_units().decode().split(",")}


def emit(obj):
    print(TAG + json.dumps(obj), flush=True)
