"""The single-pass occupancy refresh without a device: the C-ABI's argument checks, the golden of the reference's refresh
arithmetic under autocast (tests/golden/g7_refresh_autocast.npz, written by make_golden_refresh.py) pinned to the oracle,
the conditions test_refresh_gpu.py relies on asserted for the reference alone, and the Python surface's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import fsnerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# share of the points that may lie within 2 x dev_ref of the threshold (test_refresh_gpu.py excuses flipped decisions there)
BAND_CAP = {"fp16": 0.01, "bf16": 0.10}


def golden_refresh():
    g = np.load(os.path.join(GOLDEN, "g7_refresh_autocast.npz"))
    g4 = np.load(os.path.join(GOLDEN, "g4_nerf_8x256.npz"))
    sd = {k[3:]: torch.from_numpy(g4[k]) for k in g4.files if k.startswith("sd.")}
    sd["sigma.weight"], sd["sigma.bias"] = torch.from_numpy(g["sigma_weight"]), torch.from_numpy(g["sigma_bias"])
    return g, sd


def test_refresh_entry_point_is_declared_mirrored_and_validates():
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib as L
    from fs_nerf_amd import ops
    hdr = open(os.path.join(ROOT, "include", "fsnerf_hip.h")).read()
    for name in ("fsn_occgrid_refresh", "fsn_occgrid_apply_pending"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES
    lib = L.lib()
    d = ops.make_desc(8, 256, (4,), [2.0 ** i for i in range(10)], [2.0 ** i for i in range(4)])
    aabb = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    seeds = (C.c_uint64 * 4)(1, 2, 3, 4)
    one = C.c_void_p(64)  # a non-null "device pointer" for calls that must fail before anything is launched
    call = lambda prec, blob, bits, all_cells, nu, no, sd, pend, desc=d, ab=aabb: lib.fsn_occgrid_refresh(
        C.byref(desc) if desc is not None else None, prec, blob, None, bits, 8, 4, ab, all_cells, nu, no, sd, 5e-3, None,
        pend, None, None)
    for prec in (L.FSN_PREC_FP16, L.FSN_PREC_BF16):
        assert call(prec, None, None, 0, 0, 0, None, None) == 0, lib.fsn_last_error()  # zero draws: a no-op
    for prec in (L.FSN_PREC_FP16X3, L.FSN_PREC_BF16X3, L.FSN_PREC_FP16X3U, L.FSN_PREC_FP16X2):
        assert call(prec, one, one, 1, 0, 0, seeds, one) == -2  # FSN_E_UNSUPPORTED: the parity modes
        assert b"single-pass" in lib.fsn_last_error()
    assert call(L.FSN_PREC_FP16, None, None, 1, 0, 0, None, None) == -1 and b"null" in lib.fsn_last_error()
    assert call(L.FSN_PREC_FP16, one, one, 1, 0, 0, seeds, None) == -1        # no pending array
    assert call(L.FSN_PREC_BF16, one, one, 0, 128, 128, seeds, one) == -1     # occupied draws without the prefix scratch
    assert call(L.FSN_PREC_FP16, one, one, 0, -1, 0, seeds, one) == -1
    assert call(L.FSN_PREC_FP16, one, one, 1, 0, 0, seeds, one, desc=None) == -1
    assert call(L.FSN_PREC_FP16, one, one, 1, 0, 0, seeds, one, ab=None) == -1
    assert lib.fsn_occgrid_apply_pending(None, 0, None, 0.95, None) == 0
    assert lib.fsn_occgrid_apply_pending(None, 64, None, 0.95, None) == -1


def test_golden_is_the_oracles_float64_density():
    """The stored float64 column is the oracle's float64 density on the stored points and network times the step: the
    golden (the reference's own NeRF) and the oracle agree to float64 rounding."""
    g, sd = golden_refresh()
    x = torch.from_numpy(g["x"])
    assert x.shape == (16384, 3) and x.dtype == torch.float32 and float(x.abs().max()) <= 1.5
    want = O.nerf_forward({k: v.double() for k, v in sd.items()}, x.double(), None, n_layers=8, skip=[4], n_freqs=10,
                          n_freqs_dir=4).reshape(-1) * float(g["step"])
    assert g["occ_f64"].dtype == np.float64
    assert float(np.abs(want.numpy() - g["occ_f64"]).max()) <= 1e-12
    assert float(np.abs(g["occ_f32"].astype(np.float64) - g["occ_f64"]).max()) <= 1e-6


@pytest.mark.parametrize("mode", ["fp16", "bf16"])
def test_golden_conditions_hold_for_the_reference_alone(mode):
    """What the GPU tests ask of the fused path, asked of the reference's own autocast output: dev_ref is its largest
    deviation; its flipped threshold decisions all lie within its own dev_ref of the threshold; the band that excuses
    flips (2 x dev_ref either side) holds at most 1 % (fp16) / 10 % (bf16) of the points, so a changed golden cannot
    loosen the GPU test silently; the values straddle the threshold (20-40 % occupied) and are finite."""
    g, _ = golden_refresh()
    occ64, ac, thre, dev_ref = g["occ_f64"], g["occ_ac_" + mode], float(g["thre"]), float(g["dev_ref_" + mode])
    assert np.isfinite(occ64).all() and np.isfinite(ac).all() and ac.dtype == np.float32
    assert float(g["step"]) == 5e-3 and thre == 1e-2
    assert 0.2 <= float((occ64 > thre).mean()) <= 0.4
    assert float(np.abs(ac.astype(np.float64) - occ64).max()) == dev_ref > 0.0
    flips = (ac > thre) != (occ64 > thre)
    assert not bool((flips & (np.abs(occ64 - thre) > dev_ref)).any())
    band = np.abs(occ64 - thre) <= 2.0 * dev_ref
    print(f"{mode}: dev_ref {dev_ref:.3e}, {int(flips.sum())} flips, {100 * band.mean():.2f} % inside the band")
    assert float(band.mean()) <= BAND_CAP[mode]


def test_python_surface_checks_its_arguments_without_a_device():
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd.core.models import NeRF, OccEvalFn
    m = NeRF(3, 3, 8, 256, (4,), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    assert m.autocast_precision is None and m.cull_precision is None
    fn = m.occ_eval_fn(5e-3)
    assert isinstance(fn, OccEvalFn) and fn.precision == "fp16" and fn.model is m and fn.render_step_size == 5e-3
    assert m.occ_eval_fn(5e-3, "bf16").precision == "bf16"
    for bad in ("fp16x3", "bf16x3", "fp32", None):
        with pytest.raises(ValueError):
            m.occ_eval_fn(5e-3, bad)
        with pytest.raises(ValueError):
            m.packed_single(bad)
    m.autocast_precision = "fp16x3"
    with pytest.raises(ValueError, match="autocast_precision"):
        with torch.no_grad():
            m(torch.zeros(4, 3))
    m.cull_precision = "fp16"
    with pytest.raises(ValueError, match="cull_precision"):
        m.packed_cull()
