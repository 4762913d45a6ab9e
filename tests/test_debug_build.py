"""-m gpu: the DEBUG build of the library (make -C fs-nerf_amd/csrc debug: -DFSN_DEBUG, SURVEY 5 "LDS bounds asserts in
debug builds", VERDICT r3 next #6 iv).  GPU AddressSanitizer is not available on this pool and a trapping kernel can take
a node down, so the debug build RECORDS an index outside one of the render kernels' LDS arrays (RenderLds / OccLds) and
clamps it; here small-shape parity cases of every BASELINE shape, ragged single-pass shapes, the launch-shape variants
and the occupancy kernel run through it in a child process and the record must stay empty - after a negative control
has shown that the checks fire."""
import pytest

import debug_lib


def test_release_library_says_it_is_not_a_debug_build():
    import ctypes as C
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib as L
    buf = (C.c_uint32 * 4)()
    for unit in (b"render", b"occ"):
        assert L.lib().fsn_debug_report(unit, buf) == -2 and b"not a debug build" in L.lib().fsn_last_error()
    assert L.lib().fsn_debug_selftest() == -2


@pytest.mark.gpu
def test_render_kernels_keep_inside_their_lds_arrays():
    rep = debug_lib.run_worker("debug_build_worker.py", timeout=1200)
    clean = {"render": [0] * 4, "occ": [0] * 4}
    st = rep["selftest"]["render"]
    assert st[0] == 2 and st[3] == 32 and st[2] in (32, 34) and rep["selftest"]["occ"] == [0, 0, 0, 0], \
        f"negative control: {rep['selftest']}"
    assert rep["after_selftest"] == clean, "the report clears the record"
    assert rep["render"] == clean, f"k_render_fused indexed outside an LDS array: {rep['render']} (count, line, index, extent)"
    assert rep["occ"] == clean, f"k_render_occ indexed outside an LDS array: {rep['occ']}"
    debug_lib.assert_no_other_unit_recorded(rep)
