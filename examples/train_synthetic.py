#!/usr/bin/env python3
"""A run-nerf.py-shaped driver on the drop-in modules (no dataset files, no network): a teacher NeRF renders the
"photographs" of a Lego-style orbit, a student is trained on them with the reference's loop structure
(src/run-nerf.py:216-299: ray batch -> render_rays(train=True) -> MSE -> backward -> Adam -> ExponentialDecay ->
estimator.update_every_n_steps) and evaluated with render_frame + PSNR and SSIM (run-nerf.py:140-190).

    python examples/train_synthetic.py [--estimator occgrid|stratified|propnet] [--iters 400] [--hw 64] [--u8-dataset]
                                       [--depth-weight W] [--distortion-weight W] [--cone-angle A] [--near-plane T]
                                       [--mark-invisible] [--min-views K] [--ssim-weight W --patch P --patches B]
                                       [--lpips-weight W --lpips-weights FILE]
                                       [--entropy-weight W] [--depth-kl-weight W --depth-kl-var V]
                                       [--depth-smooth-weight W] [--unseen-views shell|box]
                                       [--warp-weight W --warp-kind l1|l2]
                                       [--refine-poses --pose-noise-rot DEG --pose-noise-trans X --pose-lr LR
                                        --c2f-until K]
                                       [--refine-intrinsics --focal-noise PCT --intrinsics-lr LR --per-view-intrinsics
                                        --learn-principal-point]

--u8-dataset: the teacher's frames become uint8 "photographs" (R.to8b) held in a device-resident RayDataset; the loop
takes its batches from a RayLoader the way run-nerf.py:236-240 takes them from its DataLoader, and the held-out view
comes from a FrameLoader (fs_nerf_amd.nerfdata).

--depth-weight / --distortion-weight (both 0 by default: the loop is then the one above): few-shot regularisers on the
renderer's other outputs through render_rays(full_grad=True) - an MSE between the rendered depth and the teacher's on
the rays where the teacher hit something (with --u8-dataset the depth is an aux plane of the dataset), and the distortion
loss of the compositor's weights (core.loss.DistortionLoss).

--entropy-weight / --depth-kl-weight / --depth-smooth-weight (all 0 by default: the loop is then the one above): the
few-shot geometry losses of core.loss, through render_rays(full_grad=True).  --entropy-weight: RayEntropyLoss on
extras["alphas"], the rays masked by the rendered opacity (InfoNeRF's ray entropy).  --depth-kl-weight, with
--depth-kl-var V (default 0.01): DepthKLLoss on extras["weights"] against the teacher's depth on the rays where the
teacher hit something (DS-NeRF's depth term; with --u8-dataset from the aux plane, as --depth-weight).  --depth-smooth-weight:
PatchDepthSmoothnessLoss on the rendered depth of --patches B patches of --patch P x P rays from a random orbit pose no
photograph was taken from (RegNeRF's depth smoothness); their rays come from get_rays and ride in the same render_rays
call, behind the ray batch and the SSIM / LPIPS patches.  --unseen-views shell|box: those patches are instead --patches
freshly drawn poses' patches from nerfdata.UnseenPatchLoader, one launch per step, its pose distribution fitted to the
training poses (UnseenViewSampler.from_poses); with --entropy-weight alone the entropy term covers their rays too.

--ray-kl-weight W [--ray-kl-bins N] (0 by default: the loop is then the one above): the KL divergence between the
termination distributions of neighbouring rays (core.loss.NeighborRayKLLoss, InfoNeRF's second term) on
extras["weights"] through render_rays(full_grad=True).  Each patch ray's samples are binned into a histogram of N
(default 64) bins over [near, far] and adjacent pixels of a patch are compared bin by bin, pixels masked by the
rendered opacity.  It acts on the patches that --depth-smooth-weight renders - the orbit pose's or the --unseen-views
ones, which sit behind every other ray of the call (first_ray = their offset) - and has them rendered when nothing
else does; with --ssim-weight / --lpips-weight and no unseen patches it acts on the photographs' patches instead.

--warp-weight W [--warp-kind l1|l2] (0 by default; needs --u8-dataset): the depth-warp consistency term
(core.loss.WarpConsistencyLoss over nerfdata.WarpSource, through render_rays(full_grad=True)): a ray's rendered colour
against the colour a training photograph shows at its rendered 3-D point, rays masked by the rendered opacity.  With
--unseen-views the term is put on those patches, each against the training view nearest to its pose
(WarpSource.nearest_views of the poses the loader reports); otherwise on the batch's own rays, each against the view
nearest to its own (the view is index // (H W), the source WarpSource.other_views).

--cone-angle / --near-plane (both 0 by default): `sampling_kwargs` of render_rays / render_frame / render_path - the
occupancy march's step grows with distance, dt = max(t * cone_angle, step), and nothing is sampled in front of the near
plane - in training, evaluation and the path render alike.

--estimator propnet: a learned proposal in the estimator slot (render/propnet.py) - one 4x128 proposal network,
prop_samples=(128,), num_samples=64, uniform in disparity between near and far, its own Adam; after the main step
`estimator.update_every_n_steps(extras["trans"].reshape(n_rays, 64), requires_grad=True)` takes the interlevel loss's
step on the proposal network.

--ssim-weight W (0 by default: the loop is then the one above; needs --u8-dataset): a structural (D-SSIM) term on
rendered patches.  A PatchLoader serves --patches B patches of --patch P x P pixels per step; their rays are concatenated
to the ray batch for ONE render_rays call, and the rendered tail, reshaped to [B, P, P, 3], goes through
core.loss.SSIMLoss against the photographs' patches: loss = MSE(ray batch) + W * (1 - SSIM(patches)).

--lpips-weight W --lpips-weights FILE (0 by default; needs --u8-dataset and --patch of at least 16): the perceptual term
on the same patches, loss += W * LPIPSLoss(patches) (core.loss.LPIPSLoss on metrics.LPIPS, VGG16).  FILE is a local
torch.save'd state dict in the `lpips` package's layout; nothing is downloaded.

--refine-poses (off by default; needs --u8-dataset): joint pose and field optimisation.  The training poses are
perturbed by --pose-noise-rot DEG (a rotation of that angle about a random axis per view) and --pose-noise-trans X (a
step of that length in a random direction); a nerfdata.CameraRefiner holds a correction xi per view, the RayLoader (and
the PatchLoader) serve their batches over the corrected poses, loss.backward() fills xi.grad in one launch, and
torch.optim.Adam steps xi (--pose-lr, default 1e-3) beside the network.  --c2f-until K ramps the frequency mask of both
encodings from the lowest frequency to all of them over the first K steps (BARF's coarse-to-fine schedule through
NeRF.set_freq_mask).  At the end nerfdata.pose_error prints the rotation and translation error of the perturbed and of
the refined poses against the true ones, after a similarity alignment.  (Intrinsics: --refine-intrinsics.  The teacher
is a random network: its photographs are smooth and constrain the cameras only weakly, so expect the rotation error to shrink by a
part, not to vanish - 5.4 -> 3.1 degrees in 800 steps at --hw 64 --estimator stratified --pose-noise-rot 5
--pose-noise-trans 0.1 --c2f-until 200.)

--refine-intrinsics (off by default; needs --u8-dataset; alone or with --refine-poses): the loop is told a focal length
wrong by --focal-noise PCT percent; a nerfdata.IntrinsicsRefiner holds phi (log focal factor, principal-point offset in
image sizes), the loaders serve their batches over its camera table, loss.backward() fills phi.grad, and
torch.optim.Adam steps phi (--intrinsics-lr, default 1e-3).  --per-view-intrinsics: one row per view instead of a shared
one; --learn-principal-point: off by default, since with learnable poses the principal point is nearly degenerate with
the rotation.  At the end the learned K and the focal's relative error are printed.  The held-out frame and the path
are rendered with the true focal.

--mono-depth-weight W [--mono-depth-kind ssi|rank] [--mono-depth-space depth|disparity] (0 by default; needs
--u8-dataset): a monocular depth prior.  The teacher's depth frames (their reciprocal with --mono-depth-space disparity)
become one auxiliary plane of the RayDataset, each view multiplied and shifted by its own random affine pair, as a
monocular estimator would deliver it, with NaN where the teacher saw background; a PatchLoader(with_aux=True) serves
--patches patches of --patch x --patch pixels with their prior in the batch's own launch, their rays ride behind the rest
in the ONE render_rays call, and core.loss.ScaleShiftDepthLoss (ssi: a scale-and-shift-invariant fit per patch) or
core.loss.DepthRankingLoss (rank: only the prior's ordering) goes on their rendered depth.  With --u8-dataset the
teacher's metric depth is an auxiliary plane as well, so --depth-weight and --depth-kl-weight take their targets from
the aux column the RayLoader serves (with_aux=True) instead of a float table.

--mark-invisible (off by default): before the first step the occupancy estimator takes every cell that fewer than
--min-views K (default 1) training views see out of the grid for good (OccGridEstimator.mark_invisible_from_views: a
conservative frustum / box test); no later refresh switches such a cell on.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fs_nerf_amd  # noqa: E402,F401
from fs_nerf_amd.core import metrics  # noqa: E402
from fs_nerf_amd.core import models as M  # noqa: E402
from fs_nerf_amd.core.loss import (DepthKLLoss, DepthRankingLoss, DistortionLoss, LPIPSLoss, NeighborRayKLLoss,  # noqa: E402
                                   PatchDepthSmoothnessLoss, RayEntropyLoss, ScaleShiftDepthLoss, SSIMLoss, WarpConsistencyLoss,
                                   WeightNormRegularizer)
from fs_nerf_amd.core.optim import FusedAdam  # noqa: E402
from fs_nerf_amd.core.scheduler import ExponentialDecay  # noqa: E402
from fs_nerf_amd.nerfdata import (CameraRefiner, FrameLoader, IntrinsicsRefiner, PatchLoader, RayDataset, RayLoader, UnseenPatchLoader,  # noqa: E402
                                  UnseenViewSampler, WarpSource, pose_error)
from fs_nerf_amd.render import rendering as R  # noqa: E402
from fs_nerf_amd.render.occgrid import OccGridEstimator  # noqa: E402
from fs_nerf_amd.render.propnet import PropNetEstimator  # noqa: E402
from fs_nerf_amd.utils import utilities as U  # noqa: E402


def orbit_pose(phi_deg, theta_deg=50.0, radius=4.0311289):
    th, ph = theta_deg / 180.0 * math.pi, phi_deg / 180.0 * math.pi
    tr = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1.0]])
    rt = torch.tensor([[1, 0, 0, 0], [0, math.cos(th), -math.sin(th), 0], [0, math.sin(th), math.cos(th), 0], [0, 0, 0, 1.0]])
    rp = torch.tensor([[math.cos(ph), -math.sin(ph), 0, 0], [math.sin(ph), math.cos(ph), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    return rp @ (rt @ tr)


def perturbed(poses, rot_deg, trans, gen):
    """[n,4,4]: every pose turned by rot_deg about a random axis (world frame) and moved by `trans` in a random direction."""
    n = poses.shape[0]
    axis = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, dtype=torch.float64), dim=-1)
    w = axis * math.radians(rot_deg)
    z = torch.zeros(n, dtype=torch.float64)
    K = torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                     torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)
    out = poses.double().clone()
    out[:, :3, :3] = torch.linalg.matrix_exp(K) @ out[:, :3, :3]
    out[:, :3, 3] += trans * torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, dtype=torch.float64), dim=-1)
    return out.float()


def c2f_mask(d_in, n_freqs, progress, dev):
    """BARF's coarse-to-fine weights in the encoder's block order (x, sin f0, cos f0, sin f1, ...): frequency k has
    weight (1 - cos(pi clamp(progress * n_freqs - k, 0, 1))) / 2, the identity block 1."""
    k = torch.arange(n_freqs, dtype=torch.float32)
    w = 0.5 * (1.0 - torch.cos(math.pi * (progress * n_freqs - k).clamp(0.0, 1.0)))
    return torch.cat([torch.ones(d_in), w.repeat_interleave(2 * d_in)]).to(dev)


def make_model(seed, dev):
    torch.manual_seed(seed)
    m = M.NeRF(3, 3, 8, 256, (4,), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    with torch.no_grad():
        m.sigma.weight.mul_(64.0)
        m.sigma.bias.add_(3.0)
    return m.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--estimator", choices=("occgrid", "stratified", "propnet"), default="occgrid")
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--hw", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--cull-bf16", action="store_true",
                    help="opt-in: the occupancy estimator's visibility cull in single-pass bf16 (NeRF.cull_precision; not the parity mode)")
    ap.add_argument("--refresh-precision", choices=("fp16", "bf16"), default=None,
                    help="opt-in: the occupancy-grid refresh in that single-pass mode, one fused launch for all levels "
                         "(NeRF.occ_eval_fn: the project's equivalent of the reference's autocast around it; default: "
                         "the plain closure in the model's own mode)")
    ap.add_argument("--u8-dataset", action="store_true",
                    help="train on uint8 images through the device-resident RayDataset / RayLoader (epochs without "
                         "replacement, one launch per batch) instead of float tables indexed with torch.randint")
    ap.add_argument("--depth-weight", type=float, default=0.0,
                    help="opt-in: weight of a depth-supervision term against the teacher's depth (render_rays(full_grad=True))")
    ap.add_argument("--distortion-weight", type=float, default=0.0,
                    help="opt-in: weight of the distortion loss on the compositor's weights (render_rays(full_grad=True))")
    ap.add_argument("--entropy-weight", type=float, default=0.0,
                    help="opt-in: weight of the ray entropy of the compositor's alphas, rays masked by opacity "
                         "(core.loss.RayEntropyLoss; render_rays(full_grad=True))")
    ap.add_argument("--depth-kl-weight", type=float, default=0.0,
                    help="opt-in: weight of the depth KL term of the compositor's weights against the teacher's depth "
                         "(core.loss.DepthKLLoss; render_rays(full_grad=True))")
    ap.add_argument("--depth-kl-var", type=float, default=0.01, help="with --depth-kl-weight: the variance around the teacher's depth")
    ap.add_argument("--mono-depth-weight", type=float, default=0.0,
                    help="opt-in: weight of a monocular-depth-prior term on the rendered depth of --patches patches of "
                         "--patch x --patch pixels, the prior served as an aux plane by a PatchLoader(with_aux=True); needs "
                         "--u8-dataset (core.loss.ScaleShiftDepthLoss / DepthRankingLoss; render_rays(full_grad=True))")
    ap.add_argument("--mono-depth-kind", choices=("ssi", "rank"), default="ssi",
                    help="with --mono-depth-weight: the scale-and-shift-invariant fit, or the ordinal ranking term")
    ap.add_argument("--mono-depth-space", choices=("depth", "disparity"), default="depth",
                    help="with --mono-depth-weight: the prior is an affine map of the depth, or of its reciprocal")
    ap.add_argument("--depth-smooth-weight", type=float, default=0.0,
                    help="opt-in: weight of the depth smoothness of --patches patches of --patch x --patch rays from a random "
                         "unseen orbit pose (core.loss.PatchDepthSmoothnessLoss; render_rays(full_grad=True))")
    ap.add_argument("--ray-kl-weight", type=float, default=0.0,
                    help="opt-in: weight of the KL divergence between the termination histograms of neighbouring rays of "
                         "the --patches patches of --patch x --patch rays that --depth-smooth-weight renders (or of the "
                         "photographs' patches of --ssim-weight / --lpips-weight when only those are rendered), rays masked "
                         "by opacity (core.loss.NeighborRayKLLoss over [near, far]; render_rays(full_grad=True))")
    ap.add_argument("--ray-kl-bins", type=int, default=64, help="with --ray-kl-weight: the histograms' bins over [near, far]")
    ap.add_argument("--unseen-views", choices=("shell", "box"), default=None,
                    help="opt-in: the rays of --depth-smooth-weight / --ray-kl-weight (and --entropy-weight on them) come from "
                         "nerfdata.UnseenPatchLoader, one launch per step, its pose distribution fitted to the training "
                         "poses (UnseenViewSampler.from_poses) - instead of the hard-coded orbit and a host generator")
    ap.add_argument("--warp-weight", type=float, default=0.0,
                    help="opt-in: weight of the depth-warp consistency of the rendered colour and depth with the nearest "
                         "training photograph (core.loss.WarpConsistencyLoss; needs --u8-dataset; render_rays(full_grad=True))")
    ap.add_argument("--warp-kind", choices=("l1", "l2"), default="l1", help="with --warp-weight: the photometric penalty")
    ap.add_argument("--cone-angle", type=float, default=0.0,
                    help="opt-in: the occupancy march's step grows with distance, dt = max(t * cone_angle, step) "
                         "(sampling_kwargs of render_rays / render_frame; nerfacc uses 0.004 for unbounded scenes)")
    ap.add_argument("--near-plane", type=float, default=0.0,
                    help="opt-in: no samples in front of this distance (sampling_kwargs, any estimator)")
    ap.add_argument("--mark-invisible", action="store_true",
                    help="opt-in: cells outside the training views' frusta leave the occupancy grid before the first step "
                         "(OccGridEstimator.mark_invisible_from_views)")
    ap.add_argument("--min-views", type=int, default=1,
                    help="with --mark-invisible: a cell stays only if at least this many training views see it (few-shot: 2)")
    ap.add_argument("--ssim-weight", type=float, default=0.0,
                    help="opt-in: weight of 1 - SSIM on rendered patches (core.loss.SSIMLoss; needs --u8-dataset)")
    ap.add_argument("--patch", type=int, default=16, help="with --ssim-weight: the patches are PATCH x PATCH pixels (at least 11)")
    ap.add_argument("--patches", type=int, default=8, help="with --ssim-weight: patches per step")
    ap.add_argument("--lpips-weight", type=float, default=0.0,
                    help="opt-in: weight of LPIPS-VGG on rendered patches (core.loss.LPIPSLoss; needs --u8-dataset, "
                         "--lpips-weights and --patch >= 16)")
    ap.add_argument("--lpips-weights", default=None, metavar="FILE",
                    help="with --lpips-weight: a local torch.save'd state dict of the lpips package's LPIPS(net='vgg')")
    ap.add_argument("--refine-poses", action="store_true",
                    help="opt-in: learn a correction per training camera beside the network (nerfdata.CameraRefiner; needs "
                         "--u8-dataset)")
    ap.add_argument("--pose-noise-rot", type=float, default=0.0, metavar="DEG",
                    help="with --refine-poses: the training poses are turned by this angle about random axes")
    ap.add_argument("--pose-noise-trans", type=float, default=0.0, metavar="X",
                    help="with --refine-poses: the training cameras are moved by this distance in random directions")
    ap.add_argument("--pose-lr", type=float, default=1e-3, help="with --refine-poses: Adam's learning rate for the corrections")
    ap.add_argument("--c2f-until", type=int, default=0, metavar="K",
                    help="ramp the frequency mask of both encodings up over the first K steps (coarse-to-fine; 0: off)")
    ap.add_argument("--refine-intrinsics", action="store_true",
                    help="opt-in: learn the focal length (and the principal point) beside the network "
                         "(nerfdata.IntrinsicsRefiner; needs --u8-dataset)")
    ap.add_argument("--focal-noise", type=float, default=0.0, metavar="PCT",
                    help="with --refine-intrinsics: the loop starts from a focal length wrong by this many percent")
    ap.add_argument("--intrinsics-lr", type=float, default=1e-3, help="with --refine-intrinsics: Adam's learning rate for phi")
    ap.add_argument("--per-view-intrinsics", action="store_true", help="with --refine-intrinsics: one camera row per view")
    ap.add_argument("--learn-principal-point", action="store_true",
                    help="with --refine-intrinsics: learn the principal point too (nearly degenerate with learnable rotations)")
    a = ap.parse_args()
    if a.refine_intrinsics and not a.u8_dataset:
        ap.error("--refine-intrinsics learns the camera table behind the device-resident loaders: add --u8-dataset")
    if (a.focal_noise or a.per_view_intrinsics or a.learn_principal_point) and not a.refine_intrinsics:
        ap.error("--focal-noise / --per-view-intrinsics / --learn-principal-point belong to --refine-intrinsics")
    if a.refine_poses and not a.u8_dataset:
        ap.error("--refine-poses learns the poses behind the device-resident loaders: add --u8-dataset")
    if (a.pose_noise_rot or a.pose_noise_trans) and not a.refine_poses:
        ap.error("--pose-noise-rot / --pose-noise-trans belong to --refine-poses")
    if a.lpips_weight:
        if not a.u8_dataset:
            ap.error("--lpips-weight takes its patches from the device-resident dataset: add --u8-dataset")
        if not a.lpips_weights:
            ap.error("--lpips-weight needs --lpips-weights FILE (a local state dict; nothing is downloaded)")
        if a.patch < 16:
            ap.error("--lpips-weight needs --patch of at least 16 (LPIPS-VGG has four 2x2 pools)")
    if a.ssim_weight and not a.u8_dataset:
        ap.error("--ssim-weight takes its patches from the device-resident dataset: add --u8-dataset")
    if a.cone_angle and a.estimator != "occgrid":
        ap.error("--cone-angle belongs to the occupancy estimator")
    if a.mark_invisible and a.estimator != "occgrid":
        ap.error("--mark-invisible belongs to the occupancy estimator")
    sampling_kwargs = {k: v for k, v in (("cone_angle", a.cone_angle), ("near_plane", a.near_plane)) if v != 0.0} or None
    if a.mono_depth_weight and not a.u8_dataset:
        ap.error("--mono-depth-weight takes its prior from the device-resident dataset's aux planes: add --u8-dataset")
    if a.mono_depth_weight and a.patch < 2:
        ap.error("--mono-depth-weight needs --patch of at least 2")
    if a.unseen_views and not (a.depth_smooth_weight or a.entropy_weight or a.warp_weight or a.ray_kl_weight):
        ap.error("--unseen-views serves the rays of --depth-smooth-weight / --entropy-weight / --warp-weight / --ray-kl-weight: "
                 "set one of them")
    if a.warp_weight and not a.u8_dataset:
        ap.error("--warp-weight samples the device-resident photographs: add --u8-dataset")
    if (a.depth_smooth_weight or a.ray_kl_weight) and a.patch < 2:
        ap.error("--depth-smooth-weight / --ray-kl-weight need --patch of at least 2")
    if a.ray_kl_weight and not 1 <= a.ray_kl_bins <= 4096:
        ap.error("--ray-kl-bins is between 1 and 4096")
    full_grad = any(w != 0.0 for w in (a.depth_weight, a.distortion_weight, a.entropy_weight, a.depth_kl_weight,
                                       a.depth_smooth_weight, a.warp_weight, a.ray_kl_weight, a.mono_depth_weight))
    dev = torch.device("cuda:0")
    hwf = (a.hw, a.hw, 0.5 * a.hw / math.tan(0.5 * 0.6911112))
    near, far, step = 2.0, 6.0, 2e-2
    teacher = make_model(1, dev).eval()
    t_est = R.StratifiedEstimator(near, far, 64, 128)
    poses = [orbit_pose(phi) for phi in range(0, 360, 45)]
    ro, rd, gt, gd = [], [], [], []
    with torch.no_grad():  # the "dataset": rays of every view (blender.py:174-191) and their colours
        for p in poses:
            o, d = U.get_rays(p, hwf, dev)
            ro.append(o.reshape(-1, 3))
            rd.append(d.reshape(-1, 3))
            frame, frame_depth = R.render_frame(hwf, near, far, p, 1 << 20, t_est, teacher, white_bkgd=True, device=dev)
            gt.append(frame.reshape(-1, 3))
            gd.append(frame_depth.reshape(-1, 1))
    ro, rd, gt, gd = torch.cat(ro), torch.cat(rd), torch.cat(gt), torch.cat(gd)
    held_out = orbit_pose(22.5)
    if a.u8_dataset:  # the frames as photographs: bytes, resident; the float tables above are dropped
        frames8 = R.to8b(gt).reshape(len(poses), a.hw, a.hw, 3)
        true_poses = torch.stack(poses)
        start_poses = true_poses
        if a.refine_poses:  # the photographs are those of the true poses; the loop is told the perturbed ones
            start_poses = perturbed(true_poses, a.pose_noise_rot, a.pose_noise_trans, torch.Generator().manual_seed(5))
        # (with --refine-intrinsics the photographs are those of the true focal; the loop is told a wrong one)
        start_hwf = (hwf[0], hwf[1], hwf[2] * (1.0 + a.focal_noise / 100.0)) if a.refine_intrinsics else hwf
        # aux planes: the teacher's metric depth (--depth-weight / --depth-kl-weight) and, with --mono-depth-weight, the
        # prior a monocular estimator would deliver: each view under its own affine map, NaN where nothing was hit
        depth_frames = gd.reshape(len(poses), a.hw, a.hw, 1)
        planes = [depth_frames]
        if a.mono_depth_weight:
            aff = torch.Generator().manual_seed(6)
            scale = (0.5 + 1.5 * torch.rand(len(poses), 1, 1, 1, generator=aff)).to(dev)
            shift = (2.0 * torch.rand(len(poses), 1, 1, 1, generator=aff) - 1.0).to(dev)
            base = 1.0 / depth_frames if a.mono_depth_space == "disparity" else depth_frames
            planes.append(torch.where(depth_frames > near, scale * base + shift, torch.full_like(base, float("nan"))))
        train_set = RayDataset(frames8, start_poses, start_hwf, near=near, far=far, device=dev, aux=torch.cat(planes, dim=-1))
        ray_aux = bool(a.depth_weight or a.depth_kl_weight)  # the batch's depth targets ride in its own launch
        cameras = CameraRefiner(train_set) if a.refine_poses else None
        intrinsics = None
        if a.refine_intrinsics:
            intrinsics = IntrinsicsRefiner(train_set, per_view=a.per_view_intrinsics,
                                           learn_principal_point=a.learn_principal_point)
        # (the warp term on the batch's own rays needs to know which view each came from: the loader reports the index)
        warp_own = bool(a.warp_weight) and not a.unseen_views
        train_loader = RayLoader(train_set, a.batch, shuffle=True, seed=0, cameras=cameras, intrinsics=intrinsics,
                                 with_index=warp_own, with_aux=ray_aux)
        iterator = iter(train_loader)
        if a.mono_depth_weight:
            mono_loader = PatchLoader(train_set, a.patch, a.patches, shuffle=True, seed=2, cameras=cameras,
                                      intrinsics=intrinsics, with_aux=True)
            mono_iterator = iter(mono_loader)
            if a.mono_depth_kind == "ssi":
                mono_loss = ScaleShiftDepthLoss(space=a.mono_depth_space, threshold=0.5)
            else:
                mono_loss = DepthRankingLoss(prior_is_disparity=a.mono_depth_space == "disparity", threshold=0.5)
        if a.warp_weight:
            warp_source = WarpSource(train_set, cameras=cameras, intrinsics=intrinsics)
            warp_loss = WarpConsistencyLoss(a.warp_kind, threshold=0.5)
        if a.ssim_weight or a.lpips_weight:
            patch_loader = PatchLoader(train_set, a.patch, a.patches, shuffle=True, seed=1, cameras=cameras,
                                       intrinsics=intrinsics)
            patch_iterator = iter(patch_loader)
        if a.ssim_weight:
            ssim_loss = SSIMLoss(gaussian_weights=True, data_range=1.0, channel_axis=-1)
        if a.lpips_weight:
            lpips_net = metrics.LPIPS(net="vgg")
            lpips_net.load_state_dict(torch.load(a.lpips_weights, map_location="cpu"))
            lpips_loss = LPIPSLoss(lpips_net.to(dev).eval(), normalize=True, channel_axis=-1)
        with torch.no_grad():
            ref8 = R.to8b(R.render_frame(hwf, near, far, held_out, 1 << 20, t_est, teacher, white_bkgd=True, device=dev)[0])
        val_loader = FrameLoader(RayDataset(ref8.reshape(1, a.hw, a.hw, 3), held_out[None], hwf, near=near, far=far, device=dev))
        del ro, rd, gt, gd

    model = make_model(2, dev).train()
    if a.cull_bf16:
        model.cull_precision = "bf16"
    if a.estimator == "occgrid":
        estimator = OccGridEstimator(roi_aabb=torch.tensor([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]), resolution=64, levels=1).to(dev)
    elif a.estimator == "propnet":
        torch.manual_seed(3)
        proposal = M.NeRF(3, 3, 4, 128, (), pos_fn={"n_freqs": 10, "log_space": True},
                          dir_fn={"n_freqs": 4, "log_space": True}).to(dev).train()
        estimator = PropNetEstimator(torch.optim.Adam(proposal.parameters(), lr=5e-4), prop_models=[proposal],
                                     prop_samples=(128,), num_samples=64, near_plane=near, far_plane=far)
    else:
        estimator = R.StratifiedEstimator(near, far, 64, 128)
    estimator.train()
    if a.mark_invisible:  # once, before the first step (nerfacc's mark_invisible_cells, on the reference's cameras)
        if a.u8_dataset:
            estimator.mark_invisible_from_views(train_set.poses, train_set.hwf, ndc=train_set.ndc, min_views=a.min_views)
        else:
            estimator.mark_invisible_from_views(torch.stack(poses), hwf, min_views=a.min_views)
        print(f"marked: {100.0 * (1.0 - float(estimator.visible.float().mean())):.1f} % of the grid's cells are seen by fewer "
              f"than {a.min_views} of the {len(poses)} training views", flush=True)
    optimizer = FusedAdam(model.parameters(), lr=5e-4)  # torch.optim.Adam's arithmetic, one launch over flat arenas
    pose_optimizer = torch.optim.Adam([cameras.xi], lr=a.pose_lr) if a.refine_poses else None
    intrinsics_optimizer = torch.optim.Adam([intrinsics.phi], lr=a.intrinsics_lr) if a.refine_intrinsics else None
    wnorm = WeightNormRegularizer(model.named_parameters(), reg="l2", reg_ratio=0.5, Td=a.iters)  # run-nerf.py:266-279
    alpha = 1e-5
    distortion = DistortionLoss()
    ray_entropy, depth_kl, depth_smooth = RayEntropyLoss(), DepthKLLoss(), PatchDepthSmoothnessLoss()
    ray_kl = NeighborRayKLLoss(a.ray_kl_bins, t_min=near, t_max=far)
    # its patches: the unseen ones where they are rendered, else the photographs' (--ssim-weight / --lpips-weight), else
    # it has the unseen orbit patches of --depth-smooth-weight rendered for itself
    ray_kl_on_seen = bool(a.ray_kl_weight) and bool(a.ssim_weight or a.lpips_weight) and not (a.unseen_views or a.depth_smooth_weight)
    pose_gen = torch.Generator().manual_seed(4)  # the unseen poses of --depth-smooth-weight
    if a.unseen_views:
        unseen_loader = UnseenPatchLoader(UnseenViewSampler.from_poses(torch.stack(poses), a.unseen_views, device=dev), hwf,
                                          a.patch, a.patches, seed=4, with_poses=bool(a.warp_weight))
    scheduler = ExponentialDecay(optimizer, a.iters, 5e-4, r=0.1)
    gen = torch.Generator(device=dev).manual_seed(0)

    def occ_eval_fn(x):
        return model(x) * step

    if a.refresh_precision:
        occ_eval_fn = model.occ_eval_fn(step, a.refresh_precision)

    t0 = time.perf_counter()
    for k in range(a.iters):
        if a.c2f_until and k <= a.c2f_until:  # (the last of these steps leaves the mask at all ones)
            progress = k / a.c2f_until
            model.set_freq_mask(c2f_mask(3, 10, progress, dev), c2f_mask(3, 4, progress, dev))
        if a.u8_dataset:
            try:  # (run-nerf.py:236-240)
                rays_o, rays_d, rgb_gt, *more = next(iterator)
            except StopIteration:
                iterator = iter(train_loader)
                rays_o, rays_d, rgb_gt, *more = next(iterator)
            ray_index = more[:1] if warp_own else []
            gd_batch = more[-1][:, :1] if ray_aux else None  # (aux column 0: the teacher's depth of the batch's rays)
        else:
            idx = torch.randint(0, ro.shape[0], (a.batch,), device=dev, generator=gen)
            rays_o, rays_d, rgb_gt = ro[idx], rd[idx], gt[idx]
            gd_batch = gd[idx]
        n_batch = rays_o.shape[0]
        if a.ssim_weight or a.lpips_weight:  # the patches' rays ride in the same render_rays call, behind the ray batch
            try:
                patch_o, patch_d, patch_gt = next(patch_iterator)
            except StopIteration:
                patch_iterator = iter(patch_loader)
                patch_o, patch_d, patch_gt = next(patch_iterator)
            rays_o, rays_d = torch.cat([rays_o, patch_o]), torch.cat([rays_d, patch_d])
        n_seen = rays_o.shape[0]
        if a.unseen_views:  # B patches of P x P rays of B freshly drawn poses in one launch, behind the rest
            o, d, *unseen_poses = next(unseen_loader)  # (+ the poses, for the warp term's source views)
            rays_o, rays_d = torch.cat([rays_o, o]), torch.cat([rays_d, d])
        elif a.depth_smooth_weight or (a.ray_kl_weight and not ray_kl_on_seen):  # B windows of P x P rays of one random pose between the training views, behind the rest
            phi, theta = 360.0 * float(torch.rand((), generator=pose_gen)), 40.0 + 20.0 * float(torch.rand((), generator=pose_gen))
            o, d = U.get_rays(orbit_pose(phi, theta), hwf, dev)
            corner = torch.randint(0, a.hw - a.patch + 1, (a.patches, 2), generator=pose_gen)
            rows = (corner[:, :1] + torch.arange(a.patch))[:, :, None].expand(-1, -1, a.patch).to(dev)
            cols = (corner[:, 1:] + torch.arange(a.patch))[:, None, :].expand(-1, a.patch, -1).to(dev)
            rays_o = torch.cat([rays_o, o[rows, cols].reshape(-1, 3)])
            rays_d = torch.cat([rays_d, d[rows, cols].reshape(-1, 3)])
        n_geo = rays_o.shape[0]  # (the unseen patches end here)
        if a.mono_depth_weight:  # B patches of the photographs with their prior, one launch, behind everything else
            try:
                mono_o, mono_d, _, mono_aux = next(mono_iterator)
            except StopIteration:
                mono_iterator = iter(mono_loader)
                mono_o, mono_d, _, mono_aux = next(mono_iterator)
            rays_o, rays_d = torch.cat([rays_o, mono_o]), torch.cat([rays_d, mono_d])
        (rgb, opacity, depth, extras), ray_indices, _ = R.render_rays(rays_o, rays_d, estimator, model, train=True,
                                                                      white_bkgd=True, render_step_size=step, device=dev,
                                                                      full_grad=full_grad, sampling_kwargs=sampling_kwargs)
        loss = torch.nn.functional.mse_loss(rgb[:n_batch], rgb_gt)
        if a.ssim_weight:
            loss = loss + a.ssim_weight * ssim_loss(rgb[n_batch:n_seen].view(-1, a.patch, a.patch, 3),
                                                    patch_gt.view(-1, a.patch, a.patch, 3))
        if a.lpips_weight:
            loss = loss + a.lpips_weight * lpips_loss(rgb[n_batch:n_seen].view(-1, a.patch, a.patch, 3),
                                                      patch_gt.view(-1, a.patch, a.patch, 3))
        if a.depth_weight and depth.requires_grad:  # (an all-background batch renders no samples: nothing to supervise)
            hit = (gd_batch > near).float()  # render_frame clamps depth to [near, far]: `near` = the teacher saw background
            loss = loss + a.depth_weight * (hit * (depth[:n_batch] - gd_batch) ** 2).sum() / hit.sum().clamp(min=1.0)
        if a.distortion_weight and extras is not None and extras["weights"].requires_grad:
            loss = loss + a.distortion_weight * distortion(extras["weights"], extras["t_starts"], extras["t_ends"],
                                                           ray_indices, rays_o.shape[0])
        if a.entropy_weight and extras is not None and extras["alphas"].requires_grad:
            loss = loss + a.entropy_weight * ray_entropy(extras["alphas"], ray_indices, rays_o.shape[0], opacity=opacity)
        if a.depth_kl_weight and extras is not None and extras["weights"].requires_grad:
            target = torch.zeros(rays_o.shape[0], device=dev)  # 0: no depth known (background, the patches' rays)
            target[:n_batch] = torch.where(gd_batch > near, gd_batch, torch.zeros_like(gd_batch)).reshape(-1)
            loss = loss + a.depth_kl_weight * depth_kl(extras["weights"], extras["t_starts"], extras["t_ends"], ray_indices,
                                                       rays_o.shape[0], target, a.depth_kl_var)
        if a.depth_smooth_weight and depth.requires_grad:
            loss = loss + a.depth_smooth_weight * depth_smooth(depth[n_seen:n_geo].view(-1, a.patch, a.patch))
        if a.mono_depth_weight and depth.requires_grad:
            shape = (-1, a.patch, a.patch)
            loss = loss + a.mono_depth_weight * mono_loss(depth[n_geo:].view(shape), mono_aux[:, -1].reshape(shape),
                                                          opacity=opacity[n_geo:].view(shape))
        if a.ray_kl_weight and extras is not None and extras["weights"].requires_grad:
            first_ray = n_batch if ray_kl_on_seen else n_seen  # the patches sit behind the batch's rays
            loss = loss + a.ray_kl_weight * ray_kl(extras["weights"], extras["t_starts"], extras["t_ends"], ray_indices,
                                                   rays_o.shape[0], (a.patches, a.patch, a.patch), first_ray=first_ray,
                                                   opacity=opacity)
        if a.warp_weight and depth.requires_grad:
            if a.unseen_views:  # the unseen patches, each against the training view nearest to its pose
                rows = slice(n_seen, n_geo)
                src_view = warp_source.nearest_views(unseen_poses[0]).repeat_interleave(a.patch * a.patch)
            else:  # the batch's own rays, each against the view nearest to its own
                rows = slice(0, n_batch)
                own_view = torch.div(ray_index[0], a.hw * a.hw, rounding_mode="floor")
                src_view = warp_source.other_views(1)[own_view, 0]
            loss = loss + a.warp_weight * warp_loss(rgb[rows], depth[rows].reshape(-1), rays_o[rows], rays_d[rows], src_view,
                                                    warp_source, opacity=opacity[rows])
        if wnorm.active(k):
            loss = loss + alpha * wnorm()
        loss.backward()
        optimizer.step()
        scheduler.step()
        optimizer.zero_grad()
        if pose_optimizer is not None:
            pose_optimizer.step()
            pose_optimizer.zero_grad()
        if intrinsics_optimizer is not None:
            intrinsics_optimizer.step()
            intrinsics_optimizer.zero_grad()
        if a.estimator == "propnet":  # the proposal network's own step, on the interlevel loss
            prop_loss = estimator.update_every_n_steps(extras["trans"].reshape(rays_o.shape[0], estimator.num_samples),
                                                       requires_grad=estimator.proposal_requires_grad)
            if not math.isfinite(prop_loss):
                raise RuntimeError(f"iter {k}: the proposal loss is {prop_loss}")
        else:
            estimator.update_every_n_steps(step=k, occ_eval_fn=occ_eval_fn, occ_thre=1e-2)
        if k % 100 == 0 or k == a.iters - 1:
            lv = float(loss.detach())
            if not math.isfinite(lv):
                raise RuntimeError(f"iter {k}: the loss is {lv}")
            print(f"iter {k:5d}  loss {lv:.5f}  psnr {-10 * math.log10(max(lv, 1e-10)):.2f} dB"
                  + (f"  proposal loss {prop_loss:.3e}" if a.estimator == "propnet" else ""), flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    model.eval()
    estimator.eval()
    with torch.no_grad():
        img, _ = R.render_frame(hwf, near, far, held_out, 1 << 20, estimator, model, white_bkgd=True,
                                render_step_size=step, device=dev, sampling_kwargs=sampling_kwargs)
        if a.u8_dataset:
            ref = next(iter(val_loader))[0][0]  # (rgb_gt [1,H,W,3], pose [1,4,4]) as evaluation() consumes them
        else:
            ref, _ = R.render_frame(hwf, near, far, held_out, 1 << 20, t_est, teacher, white_bkgd=True, device=dev)
    # a short camera path (rendering.py:180-248), with the same sampling options
    frames, _ = R.render_path(torch.stack([orbit_pose(phi) for phi in (10.0, 20.0)]), hwf, near, far, 1 << 20, model, estimator,
                              white_bkgd=True, render_step_size=step, device=dev, sampling_kwargs=sampling_kwargs)
    psnr = float(metrics.psnr(img, ref))  # run-nerf.py:157-160
    ssim = float(metrics.ssim(img, ref, channel_axis=-1, data_range=1.0, gaussian_weights=True))  # run-nerf.py:180-189
    print(f"{a.iters} iterations of {a.batch} rays in {dt:.1f} s ({a.iters * a.batch / dt:,.0f} rays/s); held-out view PSNR "
          f"{psnr:.2f} dB, SSIM {ssim:.4f}; frame as uint8: {tuple(R.to8b(img).shape)}; path frames {frames.shape}")
    if a.refine_poses:  # up to the joint problem's gauge: after a similarity alignment of the camera centres
        for name, p in (("perturbed", start_poses), ("refined", cameras.poses())):
            rot, trans = pose_error(p, true_poses)
            print(f"{name} poses: rotation error {float(rot.mean()):.3f} deg (max {float(rot.max()):.3f}), translation error "
                  f"{float(trans.mean()):.4f} (max {float(trans.max()):.4f})")
    if a.refine_intrinsics:
        K = intrinsics.K().cpu()
        rel = (K[:, :2] / hwf[2] - 1.0).abs().max()
        print(f"learned K (fx, fy, cx, cy) per row: {[[round(v, 4) for v in row] for row in K.tolist()]}; true focal "
              f"{hwf[2]:.4f}, started at {start_hwf[2]:.4f} ({a.focal_noise:+.2f} %); focal relative error "
              f"{100.0 * float(rel):.3f} % (largest over rows and axes)")


if __name__ == "__main__":
    main()
