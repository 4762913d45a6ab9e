"""CPU oracle for the fs-nerf ray-rendering hot path.  TEST INFRASTRUCTURE ONLY.

This file restates, with plain PyTorch CPU ops, the arithmetic of the reference
(a-lemus96/fs-nerf) for the path  get_rays -> sampling -> positional encoding ->
NeRF MLP -> volume integration.  It exists so that `tests/`, `__graft_entry__.smoke()`
and the `cpu_baseline` leg of `bench.py` can check / time the HIP path against it.
Nothing under `fs-nerf_amd/` imports it; the product path fails loudly without the
HIP library.

Pinning status ("Oracle"):
  * get_rays, to_ndc, get_chunks, posenc, nerf_forward are PINNED: they are checked
    against golden vectors produced by importing the reference's own modules
    (`tests/golden/make_golden.py`, fixtures `tests/golden/*.npz`).
  * composite / rendering_packed follow nerfacc 0.5.3 (`environment.yaml:341`), which
    is a third-party dependency NOT present under /root/reference.  Its published
    algorithm is restated here and anchored on the reference's call sites
    (`src/render/rendering.py:66-74, 89-96`).  PARITY UNPINNED for these.
  * stratified_edges, sample_pdf, merge_edges, freq_mask are this build's own
    definitions of what `north_star` asks for (fixed-count stratified sampling,
    hierarchical 64+128 sampling, frequency mask); the reference has no such
    code.  PARITY UNPINNED; with mask == 1 and one network they reduce to the
    reference formulas.
  * occgrid_march, packed_visibility, occgrid_select, occgrid_update (end of file) restate this build's definition of the
    estimator contract the reference fills with nerfacc's OccGridEstimator.  PARITY UNPINNED.

All functions take / return torch CPU tensors; `dtype` follows the inputs so the
same code runs in float32 (parity oracle, CPU baseline) and float64 (truth for
error budgets).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch
from torch import Tensor

FLT_EPS = 1.1920928955078125e-07  # torch.finfo(torch.float32).eps


# --------------------------------------------------------------------------- rays
def get_rays(pose: Tensor, hwf: Tuple[int, int, float]) -> Tuple[Tensor, Tensor]:
    """Pinhole rays in world space.  Follows `src/utils/utilities.py:36-82`.

    pixel (h, w): d_cam = [(w - W/2)/f, -(h - H/2)/f, -1], normalised to unit length
    (`:66-72`), rotated by pose[:3,:3] (`:75-78`); origin = pose[:3,-1] (`:80`).
    No half-pixel offset.  Returns ([H,W,3], [H,W,3]).
    """
    H, W, focal = hwf
    dt = torch.float32
    pose = pose.to(dt)
    ww = torch.arange(W, dtype=dt)[None, :].expand(H, W)
    hh = torch.arange(H, dtype=dt)[:, None].expand(H, W)
    d_cam = torch.stack([(ww - W * 0.5) / focal, -(hh - H * 0.5) / focal,
                         -torch.ones(H, W, dtype=dt)], dim=-1)
    d_cam = d_cam / torch.norm(d_cam, dim=-1, keepdim=True)
    # d_w[k] = sum_c d_cam[c] * R[k, c]   (same reduction order as the reference)
    d_w = torch.sum(d_cam[..., None, :] * pose[:3, :3], dim=-1)
    o_w = pose[:3, -1].expand(d_w.shape)
    return o_w, d_w


def to_ndc(rays_o: Tensor, rays_d: Tensor, hwf, near: float) -> Tuple[Tensor, Tensor]:
    """Forward-facing NDC warp.  Follows `src/utils/utilities.py:84-120`."""
    H, W, focal = hwf
    t = -(near + rays_o[..., 2]) / rays_d[..., 2]
    o = rays_o + t[..., None] * rays_d
    sx = -1.0 / (W / (2.0 * focal))
    sy = -1.0 / (H / (2.0 * focal))
    o0 = sx * o[..., 0] / o[..., 2]
    o1 = sy * o[..., 1] / o[..., 2]
    o2 = 1.0 + 2.0 * near / o[..., 2]
    d0 = sx * (rays_d[..., 0] / rays_d[..., 2] - o[..., 0] / o[..., 2])
    d1 = sy * (rays_d[..., 1] / rays_d[..., 2] - o[..., 1] / o[..., 2])
    d2 = -2.0 * near / o[..., 2]
    return torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, d2], -1)


def get_chunks(t: Tensor, chunksize: int):
    """Row slices.  Follows `src/utils/utilities.py:122-134`."""
    return [t[i:i + chunksize] for i in range(0, t.shape[0], chunksize)]


def pose_from_spherical(radius: float, theta_deg: float, phi_deg: float) -> Tensor:
    """Orbit pose.  Follows `src/nerfdata/datasets/blender.py:20-69`
    (rot_phi(phi) @ rot_theta(theta) @ trans_t(radius)), float32 like the reference."""
    th, ph = theta_deg / 180.0 * math.pi, phi_deg / 180.0 * math.pi
    tr = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1]], dtype=torch.float32)
    rt = torch.tensor([[1, 0, 0, 0], [0, math.cos(th), -math.sin(th), 0],
                       [0, math.sin(th), math.cos(th), 0], [0, 0, 0, 1]], dtype=torch.float32)
    rp = torch.tensor([[math.cos(ph), -math.sin(ph), 0, 0], [math.sin(ph), math.cos(ph), 0, 0],
                       [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32)
    return rp @ (rt @ tr)


# ------------------------------------------------------------------- encoding
def pe_freqs(n_freqs: int, log_space: bool) -> Tensor:
    """Frequency bands.  Follows `src/core/models.py:31-34` (float32 values)."""
    if log_space:
        return 2.0 ** torch.linspace(0.0, n_freqs - 1, n_freqs)
    return torch.linspace(2.0 ** 0.0, 2.0 ** (n_freqs - 1), n_freqs)


def posenc(x: Tensor, n_freqs: int, log_space: bool, mask: Optional[Tensor] = None) -> Tensor:
    """[x, sin(f0 x), cos(f0 x), sin(f1 x), ...] -> [N, d*(1+2n)].
    Follows `src/core/models.py:28,37-39,50` (block order, x*freq before sin).
    `mask` ([d*(1+2n)], optional) multiplies the encoded features: the build's
    frequency mask (not in the reference; mask == 1 is the reference)."""
    fr = pe_freqs(n_freqs, log_space).to(x.dtype)
    parts = [x]
    for k in range(n_freqs):
        parts.append(torch.sin(x * fr[k]))
        parts.append(torch.cos(x * fr[k]))
    y = torch.cat(parts, dim=-1)
    if mask is not None:
        y = y * mask.to(y.dtype)
    return y


def freq_mask(d_in: int, n_freqs: int, ratio: float) -> Tensor:
    """Build's definition (FreeNeRF-style linear schedule): band k gets
    clamp(L*ratio - k, 0, 1); the identity block is always 1.  Layout = posenc layout."""
    m = [torch.ones(d_in)]
    for k in range(n_freqs):
        v = min(max(n_freqs * ratio - k, 0.0), 1.0)
        m.append(torch.full((2 * d_in,), v))
    return torch.cat(m).to(torch.float32)


# ------------------------------------------------------------------------ MLP
def round_to(t: Tensor, fmt: Optional[str]) -> Tensor:
    """Round every element to the nearest bfloat16 / float16 value (ties to even) and return it in t's dtype: the
    rounding a 16-bit MFMA operand undergoes.  `fmt` None = identity."""
    if fmt is None:
        return t
    return t.to({"bf16": torch.bfloat16, "fp16": torch.float16}[fmt]).to(t.dtype)


def round_e4m3_blocks(t: Tensor, block: int = 32) -> Tensor:
    """Round to OCP e4m3 under one power-of-two scale per block of `block` consecutive values of the last axis (the
    operand format of v_mfma_scale_f32_16x16x128_f8f6f4): block maximum scaled into [128, 256)."""
    n = t.shape[-1]
    pad = (-n) % block
    tp = torch.nn.functional.pad(t, (0, pad))
    b = tp.reshape(*tp.shape[:-1], -1, block)
    mx = b.abs().amax(-1, keepdim=True).clamp_min(1e-38)
    sc = torch.exp2(torch.floor(torch.log2(mx)) - 7.0)
    q = (b / sc).to(torch.float32).to(torch.float8_e4m3fn).to(t.dtype) * sc
    return q.reshape(tp.shape)[..., :n]


def split_linear(h: Tensor, W: Tensor, scheme: str) -> Tensor:
    """h @ W.T as a split-precision matrix-core GEMM would form it (products exact, sums in h's dtype):
      "fp16x3"   ah.wh + 2^-11 (al'.wh + ah.wl'), low parts scaled by 2^11 (this build's parity mode, csrc/mlp_layout.hpp)
      "fp16x3u"  ah.wh + al.wh + ah.wl with UNSCALED fp16 low parts (rounds 1-2; round 4's FSN_PREC_FP16X3U, which runs it
                 on the network scaled by scale_state_dict so that every layer's activations sit at 2^4 .. 2^10)
      "bf16x3"   the same on bfloat16 parts, unscaled
      "fp16x2"   ah.wh + 2^-11 al'.wh: "fp16x3" with the weights' low parts dropped (FSN_PREC_FP16X2, inference only)
      "fp16+f8"  ah.wh in fp16, the two correction products with every operand in block-scaled e4m3 (VERDICT r2 item 4:
                 a candidate mode, measured in tools/emulate_split.py and DESIGN.md 4.3; NOT built)"""
    fmt = "bf16" if scheme == "bf16x3" else "fp16"
    K = 2048.0 if scheme in ("fp16x3", "fp16x2") else 1.0  # ("fp16x3u": unscaled low parts - meant for the SCALED network, below)
    ah, wh = round_to(h, fmt), round_to(W, fmt)
    ar, wr = h - ah, W - wh
    if scheme == "fp16x2":
        return ah @ wh.T + (round_to(ar * K, fmt) @ wh.T) / K
    if scheme == "fp16+f8":
        corr = round_e4m3_blocks(ar) @ round_e4m3_blocks(wh).T + round_e4m3_blocks(ah) @ round_e4m3_blocks(wr).T
        return ah @ wh.T + corr
    al, wl = round_to(ar * K, fmt), round_to(wr * K, fmt)
    return ah @ wh.T + (al @ wh.T + ah @ wl.T) / K


def nerf_forward(sd: Dict[str, Tensor], x: Tensor, dirs: Optional[Tensor], *,
                 n_layers: int, skip: Sequence[int], n_freqs: int, n_freqs_dir: int,
                 log_space: bool = True, log_space_dir: Optional[bool] = None,
                 pos_mask: Optional[Tensor] = None, dir_mask: Optional[Tensor] = None,
                 emulate: Optional[str] = None) -> Tensor:
    """NeRF MLP forward from a reference-format state_dict.
    Follows `src/core/models.py:111-143`: relu(layer_i(h)); after layer i in `skip`
    h = cat([h, x_in]); sigma head without activation; connection (no activation);
    cat([feat, dir_enc]); relu(branch); sigmoid(rgb); returns [N,1] or [N,4]=[rgb,sigma].
    `emulate` = "fp16x3" / "bf16x3" / "fp16x2" / "fp16+f8": the split-precision schemes of split_linear (float32 x only).
    `emulate` = "bf16" / "fp16" (BASELINE config 5, "bf16 weights/activations"): the same math with the operand
    rounding of a single-pass 16-bit matrix-core kernel restated on the CPU - every Linear layer's weight and input
    are rounded to that format before the product, products and sums are taken in x's dtype (the kernel accumulates
    in float32), biases, activations and the two heads (sigma: 256 -> 1, rgb: 128 -> 3, evaluated on the unrounded
    accumulators) stay in x's dtype.  None = the reference arithmetic."""
    if log_space_dir is None:
        log_space_dir = log_space
    dt = x.dtype
    W = lambda k: sd[k].to(dt)
    q = lambda t: round_to(t, emulate)
    if emulate in ("fp16x3", "fp16x3u", "bf16x3", "fp16x2", "fp16+f8"):  # split-precision schemes (see split_linear)
        lin = lambda h, k: split_linear(h, W(k + ".weight"), emulate) + W(k + ".bias")
    else:
        lin = lambda h, k: q(h) @ q(W(k + ".weight")).T + W(k + ".bias")  # a matrix-core GEMM
    x_in = posenc(x, n_freqs, log_space, pos_mask)
    h = x_in
    for i in range(n_layers):
        h = torch.relu(lin(h, f"layers.{i}"))
        if i in skip:
            h = torch.cat([h, x_in], dim=-1)
    sigma = h @ W("sigma.weight").T + W("sigma.bias")  # fp32 dot product on the accumulators
    if dirs is None:
        return sigma
    f = lin(h, "connection")
    d_in = posenc(dirs, n_freqs_dir, log_space_dir, dir_mask)
    f = torch.cat([f, d_in], dim=-1)
    f = torch.relu(lin(f, "branch"))
    rgb = torch.sigmoid(f @ W("rgb.weight").T + W("rgb.bias"))
    return torch.cat([rgb, sigma], dim=-1)


# ---------------------------------------------------------------- the scaled network (round 4, FSN_PREC_FP16X3U)
# Restatement of the packer's transformation (csrc/mlp_pack.hpp: fill_scales, pack_piece, aux_value) and of NeRF.calibrate
# (exponents: core/range_guard.py:choose_exponents) on state dicts: with a power of two s_g = 2^e_g per GEMM (hidden layers 0..L-1, connection, branch) the scaled network's
# GEMM g produces s_g x the reference's activations and the same outputs (src/core/models.py:111-143), exactly.
def layer_maxima(sd: Dict[str, Tensor], x: Tensor, dirs: Tensor, *, n_layers: int, skip: Sequence[int], n_freqs: int,
                 n_freqs_dir: int, log_space: bool = True) -> list:
    """Largest |output after its activation| of every GEMM over the samples (what fsn_mlp_layer_maxima reports)."""
    W = lambda k: sd[k].double()
    x_in = posenc(x.double(), n_freqs, log_space)
    h, mx = x_in, []
    for i in range(n_layers):
        h = torch.relu(h @ W(f"layers.{i}.weight").T + W(f"layers.{i}.bias"))
        mx.append(float(h.abs().max()))
        if i in skip:
            h = torch.cat([h, x_in], dim=-1)
    f = h @ W("connection.weight").T + W("connection.bias")
    mx.append(float(f.abs().max()))
    f = torch.relu(torch.cat([f, posenc(dirs.double(), n_freqs_dir, log_space)], dim=-1) @ W("branch.weight").T + W("branch.bias"))
    mx.append(float(f.abs().max()))
    return mx


def calibrate_exps(maxima: Sequence[float], target_exp: int = 10) -> list:
    """e_g = target - ceil(log2 max_g): the layer's maximum lands in (2^(target-1), 2^target] (core/range_guard.py:choose_exponents)."""
    import math
    return [0 if v <= 0.0 else max(-60, min(60, target_exp - math.ceil(math.log2(v)))) for v in maxima]


def scale_state_dict(sd: Dict[str, Tensor], exps: Sequence[int], *, n_layers: int, skip: Sequence[int], d_hidden: int) -> Dict[str, Tensor]:
    """The network fsn_mlp_pack_scaled packs: weight columns fed by activations x s_g / s_(g-1), columns fed by an
    encoding x s_g, biases x s_g, sigma.weight / s_(L-1), rgb.weight / s_branch (all powers of two: exact)."""
    L, D = n_layers, d_hidden
    out = {k: v.clone() for k, v in sd.items()}
    p2 = lambda e: 2.0 ** e
    for g in range(L):
        w = out[f"layers.{g}.weight"]
        if g == 0:
            w *= p2(exps[0])
        else:
            w[:, :D] *= p2(exps[g] - exps[g - 1])
            if (g - 1) in skip:
                w[:, D:] *= p2(exps[g])
        out[f"layers.{g}.bias"] *= p2(exps[g])
    out["sigma.weight"] *= p2(-exps[L - 1])
    out["connection.weight"] *= p2(exps[L] - exps[L - 1])
    out["connection.bias"] *= p2(exps[L])
    wb = out["branch.weight"]
    wb[:, :D] *= p2(exps[L + 1] - exps[L])
    wb[:, D:] *= p2(exps[L + 1])
    out["branch.bias"] *= p2(exps[L + 1])
    out["rgb.weight"] *= p2(-exps[L + 1])
    return out


def init_nerf_state_dict(n_layers: int, d_hidden: int, skip: Sequence[int], n_freqs: int,
                         n_freqs_dir: int, seed: int, d_pos: int = 3, d_dir: int = 3) -> Dict[str, Tensor]:
    """Default nn.Linear init, created in the reference's construction order
    (`src/core/models.py:96-108`: layers[1..], then layers[0], sigma, connection, branch, rgb)
    so that torch.manual_seed(seed) reproduces the reference's parameters bit for bit."""
    from torch import nn
    torch.manual_seed(seed)
    d_pe, d_de = d_pos * (1 + 2 * n_freqs), d_dir * (1 + 2 * n_freqs_dir)
    hidden = [nn.Linear(d_hidden + d_pe, d_hidden) if i in skip else nn.Linear(d_hidden, d_hidden)
              for i in range(n_layers - 1)]
    first = nn.Linear(d_pe, d_hidden)
    mods = {"sigma": nn.Linear(d_hidden, 1), "connection": nn.Linear(d_hidden, d_hidden),
            "branch": nn.Linear(d_hidden + d_de, d_hidden // 2), "rgb": nn.Linear(d_hidden // 2, 3)}
    sd = {}
    for i, m in enumerate([first] + hidden):
        sd[f"layers.{i}.weight"], sd[f"layers.{i}.bias"] = m.weight.detach().clone(), m.bias.detach().clone()
    for k, m in mods.items():
        sd[f"{k}.weight"], sd[f"{k}.bias"] = m.weight.detach().clone(), m.bias.detach().clone()
    return sd


# -------------------------------------------------------------------- sampling
def stratified_edges(near: float, far: float, n_samples: int, n_rays: int,
                     u: Optional[Tensor] = None, dtype=torch.float32) -> Tensor:
    """Build's definition of the fixed-count sampler that fills the reference's
    `estimator.sampling` slot (`src/render/rendering.py:66-74`).  Returns S+1 sorted interval
    edges per ray, [R, S+1]; interval i = [e_i, e_{i+1}], sample position = its midpoint
    (`rendering.py:61`).  step = (far-near)/S.
      u is None            -> e_i = near + i*step                     (stratified=False)
      u shape [R] / [R,1]  -> e_i = near + (i + u_r)*step             (one shift per ray: the
                              nerfacc `stratified=True` behaviour the reference trains with)
      u shape [R, S+1]     -> per-edge jitter inside [mid_{i-1}, mid_i] (mip-NeRF style):
                              lo_i = near + max(i-0.5, 0)*step, hi_i = near + min(i+0.5, S)*step,
                              e_i = lo_i + (hi_i - lo_i)*u_i
    """
    S = n_samples
    step = torch.tensor((far - near) / S, dtype=dtype)
    i = torch.arange(S + 1, dtype=dtype)[None, :]
    nr = torch.tensor(near, dtype=dtype)
    if u is None:
        return (nr + i * step).expand(n_rays, S + 1).contiguous()
    u = u.to(dtype)
    if u.numel() == n_rays:
        return nr + (i + u.reshape(n_rays, 1)) * step
    assert u.shape == (n_rays, S + 1)
    lo = nr + torch.clamp(i - 0.5, min=0.0) * step
    hi = nr + torch.clamp(i + 0.5, max=float(S)) * step
    return lo + (hi - lo) * u


def edges_to_packed(edges: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """[R,S+1] edges -> nerfacc-style packed (ray_indices int64 [N], t_starts [N], t_ends [N])."""
    R, S1 = edges.shape
    ri = torch.arange(R, dtype=torch.int64)[:, None].expand(R, S1 - 1).reshape(-1)
    return ri, edges[:, :-1].reshape(-1), edges[:, 1:].reshape(-1)


def sample_pdf(edges: Tensor, weights: Tensor, n_importance: int, u: Optional[Tensor] = None) -> Tensor:
    """Inverse-CDF importance sampling (NeRF-paper `sample_pdf`, restated for interval edges).
    edges [R,S+1], weights [R,S] -> new t values [R,n_importance].
    pdf = (max(w,0)+1e-5)/sum; cdf = [0, cumsum(pdf)]; u = linspace(0,1,n) if None (det) else
    given [R,n]; idx = searchsorted(cdf, u, right=True); below = max(idx-1,0), above = min(idx,S);
    denom = cdf[above]-cdf[below] (1 if < 1e-5); t = e_below + (u-cdf_below)/denom*(e_above-e_below).
    The clamp max(w,0) is the build's addition: the reference network emits raw, possibly
    negative sigma (`models.py:127`), which would make the cdf non-monotone."""
    R, S = weights.shape
    dt = edges.dtype
    w = torch.clamp(weights, min=0.0) + 1e-5
    pdf = w / torch.sum(w, dim=-1, keepdim=True)
    cdf = torch.cat([torch.zeros(R, 1, dtype=dt), torch.cumsum(pdf, dim=-1)], dim=-1)
    if u is None:
        u = torch.linspace(0.0, 1.0, n_importance, dtype=dt)[None, :].expand(R, n_importance)
    u = u.contiguous().to(dt)
    idx = torch.searchsorted(cdf.contiguous(), u, right=True)
    below = torch.clamp(idx - 1, min=0)
    above = torch.clamp(idx, max=S)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    e0, e1 = torch.gather(edges, 1, below), torch.gather(edges, 1, above)
    denom = c1 - c0
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    return e0 + (u - c0) / denom * (e1 - e0)


def merge_edges(edges: Tensor, t_new: Tensor) -> Tensor:
    """Sorted union of coarse edges [R,S+1] and importance samples [R,n] -> [R,S+1+n]."""
    return torch.sort(torch.cat([edges, t_new], dim=-1), dim=-1).values


# ----------------------------------------------------------------- compositing
def composite(sigmas: Tensor, rgbs: Tensor, t_starts: Tensor, t_ends: Tensor,
              bkgd: Optional[Tensor] = None):
    """Dense [R,S] volume integration = nerfacc 0.5.3 `volrend.rendering` arithmetic
    (call site `src/render/rendering.py:89-96`; nerfacc source NOT in /root/reference — PARITY
    UNPINNED): dt = t1-t0; alpha = 1-exp(-sigma dt); T = exp(-exclusive_cumsum(sigma dt));
    w = T alpha; colors = sum w rgb; opacity = sum w; depth = sum w (t0+t1)/2 / max(opacity, eps);
    colors += bkgd (1-opacity).  No clamp on sigma (the reference net emits raw sigma).
    Returns colors [R,3], opacity [R,1], depth [R,1], extras dict with [R,S] entries."""
    sdt = sigmas * (t_ends - t_starts)
    alphas = 1.0 - torch.exp(-sdt)
    excl = torch.cumsum(sdt, dim=-1) - sdt
    trans = torch.exp(-excl)
    w = trans * alphas
    colors = torch.sum(w[..., None] * rgbs, dim=-2)
    opacity = torch.sum(w, dim=-1, keepdim=True)
    depth = torch.sum(w * (t_starts + t_ends) / 2.0, dim=-1, keepdim=True)
    depth = depth / torch.clamp(opacity, min=FLT_EPS)
    if bkgd is not None:
        colors = colors + bkgd.to(colors.dtype) * (1.0 - opacity)
    extras = {"weights": w, "alphas": alphas, "trans": trans, "sigmas": sigmas, "rgbs": rgbs}
    return colors, opacity, depth, extras


def rendering_packed(t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int,
                     rgb_sigma_fn: Callable, render_bkgd: Optional[Tensor] = None):
    """Packed / variable-length form with the nerfacc call signature used at
    `src/render/rendering.py:89-96` (samples of a ray are contiguous and sorted by ray).
    Raises AssertionError on the shape violations nerfacc asserts (caught at `rendering.py:97`)."""
    rgbs, sigmas = rgb_sigma_fn(t_starts, t_ends, ray_indices)
    assert rgbs.shape[-1] == 3, f"rgbs must have 3 channels, got {rgbs.shape}"
    assert sigmas.shape == t_starts.shape, f"sigmas must have shape of (N,)! Got {sigmas.shape}"
    N = t_starts.shape[0]
    dt = t_starts.dtype
    sdt = sigmas * (t_ends - t_starts)
    alphas = 1.0 - torch.exp(-sdt)
    # exclusive sum restarted at every ray boundary: a PER-RAY running sum, as nerfacc's scan computes it (a global
    # cumsum minus the segment's start value cancels catastrophically in float32 after ~1e4 samples)
    first = torch.ones(N, dtype=torch.bool)
    if N > 1:
        first[1:] = ray_indices[1:] != ray_indices[:-1]
    seg_id = torch.cumsum(first.to(torch.int64), 0) - 1
    excl = torch.zeros(N, dtype=dt)
    if N > 0:
        seg_first = torch.nonzero(first).reshape(-1)
        pos = torch.arange(N) - seg_first[seg_id]
        n_seg, m = int(seg_id[-1]) + 1, int(pos.max()) + 1
        dense = torch.zeros(n_seg, m, dtype=dt)
        dense[seg_id, pos] = sdt
        run = torch.cumsum(dense, dim=1) - dense
        excl = run[seg_id, pos]
    trans = torch.exp(-excl)
    w = trans * alphas
    colors = torch.zeros(n_rays, 3, dtype=dt).index_add_(0, ray_indices, w[:, None] * rgbs)
    opacity = torch.zeros(n_rays, 1, dtype=dt).index_add_(0, ray_indices, w[:, None])
    depth = torch.zeros(n_rays, 1, dtype=dt).index_add_(0, ray_indices, (w * (t_starts + t_ends) / 2.0)[:, None])
    depth = depth / torch.clamp(opacity, min=FLT_EPS)
    if render_bkgd is not None:
        colors = colors + render_bkgd.to(dt) * (1.0 - opacity)
    extras = {"weights": w, "alphas": alphas, "trans": trans, "sigmas": sigmas, "rgbs": rgbs}
    return colors, opacity, depth, extras


# ------------------------------------------------------------- whole hot path
def render_rays_oracle(rays_o: Tensor, rays_d: Tensor, sd_coarse: Dict[str, Tensor],
                       sd_fine: Optional[Dict[str, Tensor]], cfg: dict, *, near: float, far: float,
                       n_samples: int, n_importance: int = 0, u: Optional[Tensor] = None,
                       u_fine: Optional[Tensor] = None, white_bkgd: bool = False,
                       pos_mask: Optional[Tensor] = None, dir_mask: Optional[Tensor] = None,
                       edges_override: Optional[Tensor] = None, emulate: Optional[str] = None):
    """The whole path in the reference's operator order (`src/render/rendering.py:58-107`):
      1. intervals from `stratified_edges` (fills the `estimator.sampling` slot, `:66-74`);
      2. density-only pass sigma_fn: x = o + d*(t0+t1)/2; sigma = model(x)       (`:58-64`)
         -> weights (same alpha/T arithmetic as step 4)        [only if n_importance > 0]
      3. `sample_pdf` + sorted union -> S+n_importance intervals [only if n_importance > 0]
      4. full pass rgb_sigma_fn: out = model(x, d); rgbs = out[:, :3]; sigmas = out[:, -1]
         (`:76-84`), `composite` with bkgd = white_bkgd*ones(3) (`:86, 89-96`);
      5. t_vals = (t0+t1)/2 (`:105`).
    `sd_fine is None` uses one network for both passes, as the reference does.
    Returns ((rgb [R,3], opacity [R,1], depth [R,1], extras), ray_indices [N], t_vals [N]);
    extras additionally holds "edges" [R,S'+1] and, when hierarchical, "weights_coarse" [R,S].
    `edges_override` [R,S'+1] replaces the result of steps 1-3 for step 4 (tests use it to check the
    full pass + integration on exactly the sample set another implementation produced, because
    inverse-CDF resampling is ill-conditioned where the coarse pdf is ~0).  `emulate`: see nerf_forward."""
    R = rays_o.shape[0]
    dt = rays_o.dtype
    mk = dict(n_layers=cfg["n_layers"], skip=cfg["skip"], n_freqs=cfg["n_freqs"],
              n_freqs_dir=cfg["n_freqs_dir"], log_space=cfg.get("log_space", True),
              pos_mask=pos_mask, dir_mask=dir_mask, emulate=emulate)
    edges = stratified_edges(near, far, n_samples, R, u, dtype=dt)
    w_coarse = None
    if n_importance > 0:
        t0, t1 = edges[:, :-1], edges[:, 1:]
        x = rays_o[:, None, :] + rays_d[:, None, :] * (t0 + t1)[..., None] / 2.0
        sig = nerf_forward(sd_coarse, x.reshape(-1, 3), None, **mk).reshape(R, n_samples)
        sdt = sig * (t1 - t0)
        w_coarse = torch.exp(-(torch.cumsum(sdt, -1) - sdt)) * (1.0 - torch.exp(-sdt))
        edges = merge_edges(edges, sample_pdf(edges, w_coarse, n_importance, u_fine))
    if edges_override is not None:
        edges = edges_override.to(dt)
    sd = sd_fine if sd_fine is not None else sd_coarse
    t0, t1 = edges[:, :-1], edges[:, 1:]
    S = t0.shape[1]
    x = rays_o[:, None, :] + rays_d[:, None, :] * (t0 + t1)[..., None] / 2.0
    d = rays_d[:, None, :].expand(R, S, 3)
    out = nerf_forward(sd, x.reshape(-1, 3), d.reshape(-1, 3), **mk).reshape(R, S, 4)
    bk = float(white_bkgd) * torch.ones(3, dtype=dt)
    colors, opacity, depth, extras = composite(out[..., 3], out[..., :3], t0, t1, bk)
    extras["edges"] = edges
    if w_coarse is not None:
        extras["weights_coarse"] = w_coarse
    ri, ts, te = edges_to_packed(edges)
    return (colors, opacity, depth, extras), ri, (ts + te) / 2.0


# ------------------------------------------------------------------ occupancy-grid sampler
# PARITY UNPINNED: nerfacc (OccGridEstimator) is not part of the reference and is not installed; these functions
# restate THIS build's definition of the estimator contract (DESIGN.md "occupancy sampler"), operation for
# operation in float32, for the kernels in csrc/occgrid.hip.  Call sites they serve: src/render/rendering.py:66-74.
def occgrid_march(rays_o: Tensor, rays_d: Tensor, aabb: Sequence[float], res: int, levels: int, binaries: Tensor,
                  near_plane: float, far_plane: float, step: float, u: Optional[Tensor] = None,
                  max_steps: int = 16384) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (ray_indices int64 [N], t_starts [N], t_ends [N]); binaries bool [levels,res,res,res]."""
    import numpy as np
    f = np.float32
    o_all, d_all = rays_o.numpy().astype(f), rays_d.numpy().astype(f)
    amin, amax = np.array(aabb[:3], f), np.array(aabb[3:], f)
    c, h = (amin + amax) / f(2), (amax - amin) / f(2)
    bins = binaries.numpy().reshape(levels, -1)
    step, near_plane, far_plane = f(step), f(near_plane), f(far_plane)
    sc = f(1 << (levels - 1))
    ri, ts_out, te_out = [], [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for r in range(o_all.shape[0]):
            o, d = o_all[r], d_all[r]
            tmin, tmax, miss = f(-np.inf), f(np.inf), False
            for a in range(3):
                hh = h[a] * sc
                lo, hi = c[a] - hh, c[a] + hh
                if d[a] == 0:
                    miss = miss or o[a] < lo or o[a] > hi
                else:
                    ta, tb = (lo - o[a]) / d[a], (hi - o[a]) / d[a]
                    tmin, tmax = max(tmin, min(ta, tb)), min(tmax, max(ta, tb))
            near_r = near_plane + f(u[r]) * step if u is not None else near_plane
            t_lo, t_hi = max(tmin, near_r), min(tmax, far_plane)
            if miss or not (t_hi > t_lo):
                continue
            k0 = max(int(np.ceil((t_lo - near_r) / step)), 0)
            k = np.arange(k0, k0 + max_steps, dtype=np.int64)
            ts = near_r + k.astype(f) * step
            te = ts + step
            rng = (ts >= t_lo) & (ts < t_hi)
            # the kernel stops at the first 64-block whose first lattice point is past the box; points beyond are
            # out of range anyway
            tm = (ts + te) / f(2)
            p = o[None, :] + d[None, :] * tm[:, None]
            keep = np.zeros(len(k), bool)
            done = np.zeros(len(k), bool)
            s = f(1)
            for l in range(levels):
                lo, hi = c - h * s, c + h * s
                inside = np.all((p >= lo) & (p <= hi), axis=1) & ~done
                q = np.floor((p - lo) / (hi - lo) * f(res)).astype(np.int64)
                q = np.clip(q, 0, res - 1)
                cell = (q[:, 0] * res + q[:, 1]) * res + q[:, 2]
                keep |= inside & bins[l][cell]
                done |= inside
                s = s * f(2)
            keep &= rng
            n = int(keep.sum())
            ri.append(np.full(n, r, np.int64))
            ts_out.append(ts[keep])
            te_out.append(te[keep])
    cat = lambda xs, dt: torch.from_numpy(np.concatenate(xs) if xs else np.zeros(0, dt))
    return cat(ri, np.int64), cat(ts_out, f), cat(te_out, f)


def packed_visibility(sigmas: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int,
                      early_stop_eps: float = 1e-4, alpha_thre: float = 0.0) -> Tensor:
    """keep[i] = T_i >= eps and alpha_i >= alpha_thre with T = exp(-exclusive per-ray sum of sigma*dt) (float64)."""
    sdt = (sigmas * (t_ends - t_starts)).double()
    keep = torch.zeros(sdt.shape[0], dtype=torch.bool)
    for r in range(n_rays):
        m = ray_indices == r
        if not bool(m.any()):
            continue
        s = sdt[m]
        T = torch.exp(-(torch.cumsum(s, 0) - s))
        keep[m] = (T >= early_stop_eps) & ((1.0 - torch.exp(-s)) >= alpha_thre)
    return keep


# ---------------------------------------------------------------- occupancy-grid update: cell selection (round 4)
# Build's own definition (nerfacc is absent: parity unpinned) of which cells OccGridEstimator.update_every_n_steps
# (call site src/run-nerf.py:288-295) re-evaluates and where: csrc/occgrid.hip (occ_rand, k_occ_select) restated with numpy
# integers.  Test infrastructure only.
def _occ_mix(x):
    import numpy as np
    x = x.astype(np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def occ_rand(i, k: int, seed: int):
    """draw i (array) of stream k of the update with 64-bit `seed` -> uint32 values (as uint64 array)."""
    import numpy as np
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    i = np.asarray(i, dtype=np.uint64)
    return _occ_mix(_occ_mix((i + lo) & 0xFFFFFFFF) ^ np.uint64((hi + 0x9E3779B9 * (k + 1)) & 0xFFFFFFFF))


def occgrid_select(binaries_lvl: Tensor, aabb_lvl, res: int, all_cells: bool, n_uniform: int, n_occupied: int, seed: int):
    """-> (cells int64 [n] indices inside the level, x float32 [n,3]).  binaries_lvl: [res,res,res] bool of the level
    (cell index (ix*res + iy)*res + iz), aabb_lvl = (lo[3], hi[3]) of the level's box.
    Past the warm-up the first n_uniform draws are uniform over the level's cells (with replacement).  The occupied half
    follows nerfacc's rule (OccGridEstimator._sample_uniform_and_occupied_cells): with m <= n_occupied occupied cells,
    draw n_uniform + q is the q-th occupied cell in ascending order for q < m and the sentinel -1 for q >= m; with
    m > n_occupied the draws are uniform over the occupied cells, with replacement.  Every draw, a sentinel one too, gets
    a point inside a cell of the level's box: its own cell, or for a sentinel its uniform cell r(i, 0) % res^3."""
    import numpy as np
    res3 = res ** 3
    n = res3 if all_cells else n_uniform + n_occupied
    i = np.arange(n, dtype=np.uint64)
    unused = np.zeros(n, bool)
    if all_cells:
        cell = i.copy()
    else:
        r = occ_rand(i, 0, seed)
        occ_idx = np.flatnonzero(binaries_lvl.reshape(-1).cpu().numpy())  # ascending = (word, bit) order of the bit field
        cell = r % np.uint64(res3)
        m = occ_idx.size
        if n_occupied > 0 and m > n_occupied:
            j = (r[n_uniform:] % np.uint64(m)).astype(np.int64)
            cell[n_uniform:] = occ_idx[j].astype(np.uint64)
        elif n_occupied > 0:
            cell[n_uniform:n_uniform + m] = occ_idx.astype(np.uint64)
            unused[n_uniform + m:] = True
    cell = cell.astype(np.int64)  # (a sentinel draw keeps its uniform cell here: its point lies in it)
    ix, iy, iz = cell // (res * res), (cell // res) % res, cell % res
    u = [(occ_rand(i, k, seed) >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) for k in (1, 2, 3)]
    lo, hi = [np.float32(v) for v in aabb_lvl[0]], [np.float32(v) for v in aabb_lvl[1]]
    fr = np.float32(res)
    x = np.stack([lo[a] + ((c.astype(np.float32) + u[a]) / fr) * (hi[a] - lo[a]) for a, c in enumerate((ix, iy, iz))], -1)
    cells = np.where(unused, -1, cell)
    return torch.from_numpy(cells), torch.from_numpy(x.astype(np.float32))


def occgrid_update(occs: Tensor, cells: Tensor, vals: Tensor, decay: float = 0.95, occ_thre: float = 1e-2):
    """One update_every_n_steps over all levels, after the selection: `cells` int64 [n] global cell indices (the levels'
    draws concatenated; -1 = an unused draw, skipped), `vals` [n] the occ_eval_fn values of the draws.  Float32: every
    touched cell once, occs = max(occs * decay, max over the cell's draws) (NaN values are skipped, as the kernel does);
    threshold = min(mean(occs), occ_thre) with the mean in float64; binaries = occs > threshold (in float32).
    -> (occs float32 [n_cells], touched bool [n_cells], threshold float, binaries bool [n_cells])."""
    import numpy as np
    f = np.float32
    occ = occs.detach().cpu().numpy().astype(f).copy()
    c = cells.detach().cpu().numpy().astype(np.int64).reshape(-1)
    v = vals.detach().cpu().numpy().astype(f).reshape(-1)
    ok = (c >= 0) & ~np.isnan(v)
    best = np.full(occ.shape[0], -np.inf, f)
    np.maximum.at(best, c[ok], v[ok])
    touched = np.zeros(occ.shape[0], bool)
    touched[c[ok]] = True
    occ[touched] = np.maximum(occ[touched] * f(decay), best[touched])
    thr = min(float(occ.astype(np.float64).mean()), float(occ_thre))
    return torch.from_numpy(occ), torch.from_numpy(touched), thr, torch.from_numpy(occ > f(thr))
