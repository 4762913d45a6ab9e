"""Worker of tests/test_occ_cone_fused_gpu.py::test_lds_indices_stay_inside_with_cone_and_bounds: the carry case (rays
with more than half a batch of candidates, cone regime) and a per-ray bounds case in both regimes run through all three
modes of the occupancy kernel in the DEBUG library (FSN_LIB_PATH -> libfsnerf_hip_dbg.so: every LDS index of k_render_occ
range-checked, csrc/common.hpp); prints the violation record as JSON."""
import torch

import debug_lib as D


def main():
    D.open_debug_library()
    import test_occ_cone_fused_gpu as T
    from test_occ_cone_gpu import BOX1, N_RAYS, STEP, estimator, field, mixed_rays
    dev = torch.device("cuda:0")
    D.take("render"), D.take("occ")  # (clears the records)
    o, d = mixed_rays()
    m = T.thin_model(dev)
    est, ms = T.carry_case(dev)
    _, _, n_cand = T.three_modes(est, m, o, d, dev, 0.005, ms, "debug build, carry", cone=0.002)
    est = estimator(BOX1, 16, 3, field("random"), dev)
    t_min, t_max = T.ray_bounds()
    u = torch.rand(N_RAYS, generator=torch.Generator().manual_seed(1))
    for cone in (0.0, 0.02):
        T.three_modes(est, m, o, d, dev, STEP, est.max_steps(STEP, cone), f"debug build, bounds cone {cone}", cone=cone, u=u,
                      t_min=t_min, t_max=t_max, athre=1e-3)
    D.emit({"render": D.take("render"), "occ": D.take("occ"), "carried": int((n_cand > 1024).sum()), "all": D.take_all()})


if __name__ == "__main__":
    main()
