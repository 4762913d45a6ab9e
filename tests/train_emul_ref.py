"""Float64 restatement of the single-pass (fp16 / bf16) training step of NeRF.forward(x, d): the forward and the backward
of oracle.fsnerf_oracle.nerf_forward with every operand rounded to 16 bits where the training kernels round it, sums in
float64.  Written as torch.autograd.Functions, so autograd also carries the gradient through the two encoders to the
sample positions and directions.  `fmt` = "fp16", "bf16" or None (no rounding: float64 autograd of the reference).

Where each rounding point was read (fs-nerf_amd/csrc):

  forward, MFMA layers   mlp_dev.hpp, pair_epilogue: the accumulators start from the fp32 bias (NoHook::kZeroInit = false),
                         ReLU on the fp32 sums, then split_store -> the next GEMM's B operand: y = q(h) @ q(W).T + b, the
                         encodings (encode<>: split_store of the fp32 features) rounded like any other input.
  forward, heads         pair_epilogue, EPI_LAST_* / EPI_RGB: fp32 fma of w_sigma / w_rgb (aux area, fp32) with v[], the
                         fp32 values after the ReLU and before the split: no rounded operand.
  saved activations      train_fused.hip, FwdSaver::Hook::store -> store_pair_parts<false>: the 16-bit part of the fp32
                         value after its activation, i.e. q(h): the operand the next layer consumed.  The ReLU mask is
                         v > 0 on the fp32 value (Hook::post).
  d heads                k_train_bwd: dz = (d_rgb * scale) * rgb * (1 - rgb) and dsig = d_sigma * scale in fp32 from the
                         forward's own fp32 output; stored unrounded (dhead).
  d Bo                   k_train_bwd, branch block: (dz . w_rgb) in fp32, masked by Bo > 0, split_store -> stored q(dBo),
                         and q(dBo) is the B operand of the next GEMM.
  d feat, d Pre_l        k_train_bwd: gemm_layer<..., EPI_CVT> on the transposed-weight stream (kStreamBwd, pack_piece: half_rne(W) =
                         q(W)) with BwdStoreHook / BwdMaskHook: dH = q(dY) @ q(W)[:, :D]; the sigma head's dsig * w_sigma
                         (fp32) is added and the ReLU mask applied in post(), before the split: stored q(dPre), which is
                         the next GEMM's operand and the weight-gradient GEMM's.
  weight gradients       k_wgrad, !X3: mfma32(af.hi, bfr.hi) on the stored parts: dW = q(dPre).T @ q(h_in) (encoding
                         columns: the saved q(encoding), launches WG_ENC / WG_BD); bias: frag_sum of the stored parts of A:
                         db = sum q(dPre).
  head weight gradients  k_heads_wgrad: accS += ds * h with ds from dhead (fp32) and h = from_h(stored part) = q(h_{L-1});
                         accR the same with q(Bo); biases: accB sums of dhead (fp32).
  input gradient         input_grad.hip: the slices' stream (kStreamInputGrad, pack_piece) rounds the encoding columns of W_0, the skip-fed layers and
                         the branch layer (half_rne), ig_job multiplies them with the stored q(dPre_l) / q(dBo):
                         d enc = q(dY) @ q(W)[:, encoding columns]; enc_bwd is fp32 (sincos_f32 of the sample position).
  fp16 gradient scale    k_train_bwd multiplies d_out by `scale` on entry, k_wgrad_reduce / k_heads_reduce / k_input_grad
                         divide by it at the end: `scale` is an argument here, so that the roundings above - fp16's
                         underflow and overflow included - happen at the scaled magnitude.  grad_scale restates
                         fsn_grad_scale (ops.grad_scale_for).  The per-stage factors of the delayed scaling are 1 (the
                         tests hand the kernels no stage arrays).

Every MFMA Linear is therefore one Function (_QLinear): forward q(h) @ q(W).T + b; backward with g = q(dY): dH = g @ q(W),
dW = g.T @ q(h), db = sum g.  A head is another (_Head): forward h @ W.T + b on the unrounded h; backward dH = dY @ W and
db = sum dY unrounded, dW = dY.T @ q(h).  Test infrastructure only."""
import math

import torch

from oracle import fsnerf_oracle as O


class _QLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, W, b, fmt):
        qh, qW = O.round_to(h, fmt), O.round_to(W, fmt)
        ctx.save_for_backward(qh, qW)
        ctx.fmt = fmt
        return qh @ qW.T + b

    @staticmethod
    def backward(ctx, dy):
        qh, qW = ctx.saved_tensors
        g = O.round_to(dy, ctx.fmt)
        return g @ qW, g.T @ qh, g.sum(0), None


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, W, b, fmt):
        ctx.save_for_backward(O.round_to(h, fmt), W)
        return h @ W.T + b

    @staticmethod
    def backward(ctx, dy):
        qh, W = ctx.saved_tensors
        return dy @ W, dy.T @ qh, dy.sum(0), None


def cfg_of(net):
    """net = (n_layers, d_hidden, skip, n_freqs, n_freqs_dir) -> keyword arguments of O.nerf_forward."""
    L, D, skip, nf, nfd = net
    return dict(n_layers=L, skip=list(skip), n_freqs=nf, n_freqs_dir=nfd, log_space=True)


def forward(sd, x, d, net, fmt, pre=None):
    """O.nerf_forward(sd, x, d, emulate=fmt) in float64 through the Functions above -> [N, 4] = [rgb, sigma].  `pre`: a
    list that receives every ReLU pre-activation (hidden layers, then the branch layer)."""
    L, D, skip, nf, nfd = net
    W = lambda k: sd[k].double()
    x_in = O.posenc(x.double(), nf, True)
    h = x_in
    for i in range(L):
        z = _QLinear.apply(h, W(f"layers.{i}.weight"), W(f"layers.{i}.bias"), fmt)
        if pre is not None:
            pre.append(z.detach())
        h = torch.relu(z)
        if i in skip:
            h = torch.cat([h, x_in], dim=-1)
    sigma = _Head.apply(h, W("sigma.weight"), W("sigma.bias"), fmt)
    f = _QLinear.apply(h, W("connection.weight"), W("connection.bias"), fmt)
    f = torch.cat([f, O.posenc(d.double(), nfd, True)], dim=-1)
    z = _QLinear.apply(f, W("branch.weight"), W("branch.bias"), fmt)
    if pre is not None:
        pre.append(z.detach())
    rgb = torch.sigmoid(_Head.apply(torch.relu(z), W("rgb.weight"), W("rgb.bias"), fmt))
    return torch.cat([rgb, sigma], dim=-1)


def grad_scale(c):
    """fsn_grad_scale: 2^clamp(floor(log2(1024 / max|d_out|)), -40, 60); 1 when the maximum is 0, inf or NaN."""
    m = float(c.abs().max())
    if not (0.0 < m < math.inf):
        return 1.0
    return 2.0 ** max(-40, min(60, math.floor(math.log2(1024.0 / m))))


def gradients(sd, inputs, c, net, fmt, scale=1.0):
    """Gradients of (out * c).sum() as a single-pass training step in `fmt` forms them.  `inputs`: {"x", "d"} (point
    form) or {"o", "d", "ri", "t0", "t1"} (ray form: sample = midpoint of [t0, t1) on ray ri).  `scale`: the factor the
    cotangent carries through the backward (fp16: grad_scale(c)).  -> (out [N,4], {parameter name: gradient, "d_x" /
    "d_dirs" or "d_rays_o" / "d_rays_d": input gradients}), float64."""
    par = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    if "ri" in inputs:
        a, b = leaf(inputs["o"]), leaf(inputs["d"])
        ri = inputs["ri"]
        mid = ((inputs["t0"].double() + inputs["t1"].double()) / 2.0)[:, None]
        x, d = a[ri] + b[ri] * mid, b[ri]
        names = ("d_rays_o", "d_rays_d")
    else:
        a, b = leaf(inputs["x"]), leaf(inputs["d"])
        x, d = a, b
        names = ("d_x", "d_dirs")
    out = forward(par, x, d, net, fmt)
    (out * (c.double() * scale)).sum().backward()
    g = {k: v.grad / scale for k, v in par.items()}
    g[names[0]], g[names[1]] = a.grad / scale, b.grad / scale
    return out.detach(), g


def preacts(sd, x, d, net, fmt=None):
    """Every ReLU pre-activation of the network on the samples, [N, L * D + D / 2] float64 (hidden layers, branch)."""
    pre = []
    with torch.no_grad():
        forward(sd, x, d, net, fmt, pre)
    return torch.cat(pre, dim=-1)


def pinned_state_dict(net, x, d, seed):
    """A network of shape `net` in which every ReLU unit is on, or off, for all the samples (x, d) alike: built layer by
    layer in float64 (no operand rounding) from O.init_nerf_state_dict(seed).  Every pinned GEMM (hidden layers, branch)
    gets its weight scaled so that max |W h| over the samples is 0.5 - the scaled weight rounded to float32, and where
    that rounding lifts the maximum above 0.5 the factor is lowered by 2^-20 steps until it does not - and its bias set to
    +1 or -1 per unit (seeded, half each on average).  Every ReLU pre-activation then has 0.5 <= |z| <= 1.5 and max |h|
    <= 1.5: nothing near fp16's range, no saturated sigmoid.  The heads and the connection layer keep their
    initialisation.  -> float32 state dict."""
    L, D, skip, nf, nfd = net
    sd = O.init_nerf_state_dict(L, D, list(skip), nf, nfd, seed=seed)
    gen = torch.Generator().manual_seed(seed)

    def pin(name, h):
        W = sd[name + ".weight"].double()
        s = 0.5 / float((h @ W.T).abs().max())
        while True:
            W32 = (W * s).float()
            if float((h @ W32.double().T).abs().max()) <= 0.5:
                break
            s *= 1.0 - 2.0 ** -20
        n = W.shape[0]
        bias = torch.where(torch.rand(n, generator=gen) < 0.5, -torch.ones(n), torch.ones(n))
        sd[name + ".weight"], sd[name + ".bias"] = W32, bias
        return torch.relu(h @ W32.double().T + bias.double())

    x_in = O.posenc(x.double(), nf, True)
    h = x_in
    for i in range(L):
        h = pin(f"layers.{i}", h)
        if i in skip:
            h = torch.cat([h, x_in], dim=-1)
    f = h @ sd["connection.weight"].double().T + sd["connection.bias"].double()
    pin("branch", torch.cat([f, O.posenc(d.double(), nfd, True)], dim=-1))
    return sd


# ------------------------------------------------------------------------------------------------ metrics
def column_splits(net):
    """{weight name: ((label, column slice), ...)} of the weights whose columns come from different wgrad launches: a
    skip layer's successor and the branch layer (hidden columns: WG_BIG / WG_BR; encoding columns: WG_ENC / WG_BD).
    layers.0 is encoding columns only (WG_ENC): one block, listed so that the metrics name it."""
    L, D, skip, nf, nfd = net
    out = {"layers.0.weight": (("enc", slice(0, None)),),
           "branch.weight": (("hid", slice(0, D)), ("enc", slice(D, None)))}
    for i in skip:
        out[f"layers.{i + 1}.weight"] = (("hid", slice(0, D)), ("enc", slice(D, None)))
    return out


def rel_max(a, b, denom=None):
    """The project's _rel (tests/test_train_step.py): largest absolute error over the reference's largest entry."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    m = b.abs().max() if denom is None else denom
    return float((a - b).abs().max() / m.clamp(min=1e-12))


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


def entry_metrics(got, want, net):
    """(a)'s figures: {key: error}.  key = a tensor's name: rel_max of the whole tensor; "name[hid]" / "name[enc]": of a
    column block against that block's own largest entry; "name[rows r:r+16]" (weights, and their column blocks): of a
    block of 16 output rows against the whole tensor's (column block's) largest entry."""
    out = {}
    splits = column_splits(net)
    for k, w in want.items():
        g = got[k]
        assert tuple(g.shape) == tuple(w.shape), (k, tuple(g.shape), tuple(w.shape))
        out[k] = rel_max(g, w)
        if not k.endswith(".weight"):
            continue
        parts = [(k, slice(0, None))] + [(f"{k}[{lab}]", sl) for lab, sl in splits.get(k, ())]
        for key, sl in parts:
            gs, ws = g[:, sl], w[:, sl]
            out[key] = rel_max(gs, ws)
            m = ws.detach().double().abs().max()
            for r in range(0, w.shape[0], 16):
                out[f"{key}[rows {r}:{r + 16}]"] = rel_max(gs[r:r + 16], ws[r:r + 16], m)
    return out


def l2_metrics(got, want, net):
    """(b)'s figures: {key: (relative L2 error, norm of got, norm of want, all finite)} per tensor, per column block and
    per block of 16 output rows of a weight."""
    out = {}
    splits = column_splits(net)

    def put(key, g, w):
        g, w = g.detach().cpu().double(), w.detach().cpu().double()
        out[key] = (rel_l2(g, w), float(g.norm()), float(w.norm()), bool(torch.isfinite(g).all()))

    for k, w in want.items():
        g = got[k]
        assert tuple(g.shape) == tuple(w.shape), (k, tuple(g.shape), tuple(w.shape))
        put(k, g, w)
        if k.endswith(".weight"):
            for lab, sl in splits.get(k, ()):
                put(f"{k}[{lab}]", g[:, sl], w[:, sl])
            for r in range(0, w.shape[0], 16):
                put(f"{k}[rows {r}:{r + 16}]", g[r:r + 16], w[r:r + 16])
    return out


def base_key(key):
    """The key whose yardstick a 16-row block is held to: its tensor or column block."""
    i = key.find("[rows ")
    return key if i < 0 else key[:i]
