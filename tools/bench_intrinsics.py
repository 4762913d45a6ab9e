#!/usr/bin/env python3
"""Time one training batch with learnable intrinsics - change of phi, the batch, and the backward from the rays' gradients
to phi.grad (and, jointly, to xi.grad) - through nerfdata.IntrinsicsRefiner (RayLoader(intrinsics=[, cameras=]):
fsn_intrinsics_compose when phi changed, fsn_ray_batch_k, fsn_ray_camera_grad, fsn_intrinsics_grad) against the torch
spelling a user writes without it: the index from the plain loader's launch, exp of the log focal, a gather of pixel
coordinates, normalise, (matrix_exp and) an einsum with the gathered poses, the NDC map under autograd, and autograd's
backward of all that (index_add_: float atomics, not reproducible).  Shapes: --rays 4096 per batch over 8 and 100 views
of --hw 64 x 64 pixels, world and NDC rays.  Two more variants run code that the intrinsics did not change, for an A/B
against another checkout: `plain_batch` (one RayLoader batch) and `pose_only` (the cameras=-only step).  --baseline
times these two alone; --root DIR imports the package from another tree (the parent commit's), so

    python tools/bench_intrinsics.py --baseline --root ../parent --tag parent
    python tools/bench_intrinsics.py --baseline --tag this

in one session give the two sides; compare their difference with the spread of either side's own rounds.  The timed call
is change + batch + backward.  Schedule: interleaved (tools/benchlib.py), --rounds 3 rounds, us.  There is no pass or
fail on these times. Appends one JSON line to profiles/bench_intrinsics.jsonl (--out) and prints it.

    timeout -k 10 300 python tools/bench_intrinsics.py [--iters 20] [--warmup 5] [--rays 4096] [--hw 64] [--tag NAME]
"""
import argparse
import os
import sys

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=5, rounds=3, out="bench_intrinsics.jsonl")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--hw", type=int, default=64)
    ap.add_argument("--baseline", action="store_true", help="only the variants whose code the intrinsics did not change")
    ap.add_argument("--root", default=benchlib.ROOT, help="the tree to import the package (and tests/pose_refine_ref.py) from")
    args = ap.parse_args()
    import torch
    sys.path.insert(0, os.path.join(benchlib.package(args.root), "tests"))
    from fs_nerf_amd import nerfdata
    from fs_nerf_amd.nerfdata import CameraRefiner, RayDataset, RayLoader
    import pose_refine_ref as PR  # the fixtures' poses
    dev = torch.device("cuda:0")
    H = W = args.hw
    focal, B = 1.1 * W, args.rays
    gen = torch.Generator(device=dev).manual_seed(0)
    co, cd = torch.randn(B, 3, device=dev, generator=gen), torch.randn(B, 3, device=dev, generator=gen)
    pix = torch.arange(H * W, device=dev)
    col, row = (pix % W).float(), (pix // W).float()
    sx, sy = -1.0 / (W / (2.0 * focal)), -1.0 / (H / (2.0 * focal))

    def ndc_map(o, d):
        tt = -(1.0 + o[:, 2]) / d[:, 2]
        q = o + tt[:, None] * d
        return (torch.stack([sx * q[:, 0] / q[:, 2], sy * q[:, 1] / q[:, 2], 1.0 + 2.0 / q[:, 2]], -1),
                torch.stack([sx * (d[:, 0] / d[:, 2] - q[:, 0] / q[:, 2]), sy * (d[:, 1] / d[:, 2] - q[:, 1] / q[:, 2]),
                             -2.0 / q[:, 2]], -1))

    def case(n_views, ndc):
        imgs = torch.zeros(n_views, H, W, 3, dtype=torch.uint8)
        poses = PR.forward_poses(n_views, 1) if ndc else PR.world_poses(n_views, 1)
        ds = RayDataset(imgs, poses, (H, W, focal), near=0.0 if ndc else 2.0, far=1.0 if ndc else 6.0, ndc=ndc, device=dev)
        P0 = ds.poses12.view(-1, 3, 4)
        xi_step = 1e-4 * torch.randn(n_views, 6, device=dev, generator=gen)
        phi_step = 1e-4 * torch.randn(1, 4, device=dev, generator=gen)
        cam_only = CameraRefiner(ds)
        loaders = {"plain": RayLoader(ds, B, seed=0), "pose": RayLoader(ds, B, seed=0, cameras=cam_only),
                   "index": RayLoader(ds, B, seed=0, with_index=True)}
        state = {}

        def batch(which):
            try:
                return next(state[which])
            except (StopIteration, KeyError):
                state[which] = iter(loaders[which])
                return next(state[which])

        def plain_batch():
            return batch("plain")

        def pose_only():
            with torch.no_grad():
                cam_only.xi.add_(xi_step)
            o, d, _ = batch("pose")
            return torch.autograd.grad([o, d], [cam_only.xi], [co[:o.shape[0]], cd[:o.shape[0]]])[0]

        fns = {"plain_batch": plain_batch, "pose_only": pose_only}
        if args.baseline:
            return fns
        intr = nerfdata.IntrinsicsRefiner(ds, learn_principal_point=True)
        cam, intr_j = CameraRefiner(ds), nerfdata.IntrinsicsRefiner(ds, learn_principal_point=True)
        loaders["intr"] = RayLoader(ds, B, seed=0, intrinsics=intr)
        loaders["joint"] = RayLoader(ds, B, seed=0, cameras=cam, intrinsics=intr_j)
        phi_t = torch.zeros(1, 4, device=dev, requires_grad=True)
        phi_tj, xi_t = torch.zeros(1, 4, device=dev, requires_grad=True), torch.zeros(n_views, 6, device=dev, requires_grad=True)

        def intr_kernel():
            with torch.no_grad():
                intr.phi.add_(phi_step)
            o, d, _ = batch("intr")
            return torch.autograd.grad([o, d], [intr.phi], [co[:o.shape[0]], cd[:o.shape[0]]])[0]

        def joint_kernel():
            with torch.no_grad():
                intr_j.phi.add_(phi_step)
                cam.xi.add_(xi_step)
            o, d, _ = batch("joint")
            return torch.autograd.grad([o, d], [cam.xi, intr_j.phi], [co[:o.shape[0]], cd[:o.shape[0]]])

        def spelled(phi, xi):
            _, _, _, index = batch("index")
            view, p = index // (H * W), index % (H * W)
            fx = focal * torch.exp(phi[0, 0])  # (a shared tied focal)
            c = torch.stack([(col[p] - (W * 0.5 + W * phi[0, 2])) / fx, -(row[p] - (H * 0.5 + H * phi[0, 3])) / fx,
                             -torch.ones_like(col[p])], -1)
            c = c / c.norm(dim=-1, keepdim=True)
            if xi is None:
                R, t = P0[:, :, :3], P0[:, :, 3]
            else:
                R, t = torch.linalg.matrix_exp(PR.skew(xi[:, :3])) @ P0[:, :, :3], P0[:, :, 3] + xi[:, 3:]
            d = torch.einsum("bij,bj->bi", R[view], c)
            o = t[view]
            if ndc:
                o, d = ndc_map(o, d)
            n = o.shape[0]
            if xi is None and not ndc:  # (the origins do not depend on phi)
                return torch.autograd.grad([d], [phi], [cd[:n]])[0]
            return torch.autograd.grad([o, d], [phi] if xi is None else [xi, phi], [co[:n], cd[:n]])

        def intr_torch():
            with torch.no_grad():
                phi_t.add_(phi_step)
            return spelled(phi_t, None)

        def joint_torch():
            with torch.no_grad():
                phi_tj.add_(phi_step)
                xi_t.add_(xi_step)
            return spelled(phi_tj, xi_t)

        fns.update(intr_kernel=intr_kernel, intr_torch=intr_torch, joint_kernel=joint_kernel, joint_torch=joint_torch)
        return fns

    cases = {f"{'ndc' if ndc else 'world'}_{n}views": case(n, ndc) for n in (8, 100) for ndc in (False, True)}
    variants = {f"{c}_{which}": fn for c, fns in cases.items() for which, fn in fns.items()}
    rounds = benchlib.interleaved(variants, args.iters, args.warmup, args.rounds)
    out = {**benchlib.header("bench_intrinsics", args.tag), "rays": B,
           "image": [H, W], "iters": args.iters, "rounds": args.rounds, "baseline_only": bool(args.baseline),
           "what": "change of phi (xi) + batch + backward to dL/dphi (dL/dxi), device events, us",
           "variants": {name: benchlib.rounds_summary(r, "us") for name, r in rounds.items()}}
    benchlib.emit(out, args.out)


if __name__ == "__main__":
    main()
