"""Worker of tests/test_pose_refine_gpu.py: fsn_ray_pose_grad through the DEBUG library (FSN_LIB_PATH ->
libfsnerf_hip_dbg.so: its kernel, k_ray_view_grad<false>, records an index outside the dataset) - first a valid list,
then the same list with two entries outside [0, N) appended - and prints the records as JSON."""
import torch

import debug_lib as D


def main():
    D.open_debug_library()
    from fs_nerf_amd import ops
    import test_pose_refine_gpu as T
    dev = torch.device("cuda:0")
    out = {}
    for ndc in (False, True):
        P0, xi, index, go, gd = (t.to(dev) for t in T.grad_case(3, 192, ndc, 0.3, seed=7))
        n_rays = 3 * T.H * T.W
        good = ops.ray_pose_grad(P0, xi, T.H, T.W, T.FOCAL, index, go, gd, ndc=ndc)
        torch.cuda.synchronize()
        valid = D.take("pose_refine")
        # (at the end of the list, so that no other entry changes its place in the summation)
        bad = torch.cat([index, torch.tensor([n_rays + 5, -1], device=dev)])
        pad = torch.ones(2, 3, device=dev)
        got = ops.ray_pose_grad(P0, xi, T.H, T.W, T.FOCAL, bad, torch.cat([go, pad]), torch.cat([gd, pad]), ndc=ndc)
        torch.cuda.synchronize()
        rec = D.take("pose_refine")
        equal = bool(torch.equal(got, good))
        if not out:
            out = {"valid": valid, "bad": rec, "n_rays": n_rays, "first_bad": n_rays + 5, "equal_without_the_entries": equal}
        else:  # the NDC pass must say the same
            assert valid == out["valid"] and rec[0] == out["bad"][0] and rec[3] == out["bad"][3], (valid, rec)
            out["equal_without_the_entries"] = out["equal_without_the_entries"] and equal
    out["all"] = D.take_all()
    D.emit(out)


if __name__ == "__main__":
    main()
