"""Worker of tests/test_raydata_gpu.py: runs the smallest identity-order case and one shuffled epoch of it (every batch
also through the explicit-index order, all indices valid) through the DEBUG library (FSN_LIB_PATH ->
libfsnerf_hip_dbg.so: k_ray_batch records an explicit index outside the dataset) and prints the record as JSON."""
import torch

import debug_lib as D


def main():
    D.open_debug_library()
    from fs_nerf_amd.nerfdata import RayLoader
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
    D.emit({"raydata": D.take("raydata"), "all": D.take_all()})


if __name__ == "__main__":
    main()
