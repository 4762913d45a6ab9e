"""Worker of tests/test_raydata_gpu.py: runs the smallest identity-order case and one shuffled epoch of it (every batch
also through the explicit-index order, all indices valid) through the DEBUG library (FSN_LIB_PATH ->
libfsnerf_hip_dbg.so: k_ray_batch records an explicit index outside the dataset) and prints the record as JSON."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib as L
    from fs_nerf_amd.nerfdata import RayLoader
    assert "dbg" in os.path.basename(L.LIB_PATH), L.LIB_PATH
    import test_raydata_gpu as T
    dev = torch.device("cuda:0")
    T.test_identity_order_is_the_ray_tables_and_the_reference_colours(dev, (7, 9), 3, False, False)
    ds = T.small_dataset(dev, ndc=True)
    seen = []
    for o, d, rgb, index in RayLoader(ds, 64, seed=7, with_index=True):
        eo, ed, ec = ds[index]
        assert torch.equal(o, eo) and torch.equal(d, ed) and torch.equal(rgb, ec)
        seen.append(index)
    assert torch.equal(torch.cat(seen).sort().values.cpu(), torch.arange(len(ds)))
    torch.cuda.synchronize()
    buf = (C.c_uint32 * 4)()
    L.check(L.lib().fsn_debug_report_raydata(buf), "fsn_debug_report_raydata")
    print("RAYDATA_DEBUG_REPORT " + json.dumps(list(buf)), flush=True)


if __name__ == "__main__":
    main()
