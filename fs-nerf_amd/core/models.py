"""Host-side mirror of the reference's `core/models.py` call surface, backed by HIP kernels.

  PositionalEncoder(d_input, n_freqs, log_space=False).forward(x)   (src/core/models.py:10-50)
  NeRF(d_pos, d_dir, n_layers, d_hidden, skip, pos_fn=..., dir_fn=...).forward(x, dirs=None)
                                                                      (src/core/models.py:53-143)
Parameters are ordinary nn.Linear modules under the reference's attribute names, so a reference
`state_dict()` loads unchanged (keys layers.N.*, sigma.*, connection.*, branch.*, rgb.*).
`forward` never touches them with torch ops: they are packed into the MFMA streaming layout
(re-packed whenever a parameter's version counter changes) and the whole network runs in the
fused kernel `fsn_mlp_fwd`.  In training mode with autograd enabled, `forward(x, dirs)` runs the training pair
instead (`_NerfTrainFn`: `fsn_nerf_train_fwd` / `_bwd`, hand-written MFMA forward-with-savers, dgrad chain and
split-K wgrad kernels in the same precision mode).  Additions over the reference: an optional frequency mask
(`set_freq_mask`) and the arithmetic mode `precision`:
  "fp16x3" (default) three fp16 MFMA passes on high / low parts, fp32 accumulate: fp32-class accuracy (the 1e-4 parity
            mode).  INFERENCE (round 4, `act_scaling = True`) runs the SCALED network in FSN_PREC_FP16X3U: a power of two
            per layer, calibrated from the layers' measured activation maxima on a probe batch (`calibrate`) and folded
            into the packed weights / biases / heads - an exact transformation - keeps every layer's activations at
            2^4 .. 2^10 whatever the network's own scale, so the plain split (unscaled low parts, one accumulator, no
            merge) is float32-grade and 6 % faster.  The kernels raise a device flag when the calibration no longer fits
            the data at either end (a value reached fp16 infinity; a wavefront's layer maximum below 2^-4): the host
            re-calibrates and re-runs the call (never silent, inf/NaN are never returned); only when that does not help
            it continues in "bf16x3" with a RuntimeWarning.  TRAINING (forward-with-savers / backward / weight
            gradients) keeps round 3's arithmetic (FSN_PREC_FP16X3: low parts scaled by 2^11, own correction accumulator:
            float32-grade from 2^-14 to 65504 with no calibration), as does inference with `act_scaling = False`;
  "bf16x3"  the same split on bf16 parts: no range limit, ~1e-5 per product;
  "fp16x2"  two passes (weights high part only): measured accuracy in DESIGN.md, not a parity mode;
  "bf16" / "fp16"  one pass (BASELINE config 5), tolerance stated in the tests.
What follows a range flag, and the state it keeps (`NeRF.act_state`, `NeRF.train_state`), is core/range_guard.py; this
file holds the encoder, `_NerfTrainFn`, `NeRF` (network, knobs, pack, forward) and `OccEvalFn`.
"""
import functools
import warnings
from typing import Optional, Tuple

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops
from .range_guard import (ActScaling, PackCache, TrainStatus, _warn_single_pass, choose_exponents, guarded_launch,
                          single_pass_launch)


def _freqs(n_freqs: int, log_space: bool) -> Tensor:
    # same expressions as the reference (models.py:31-34), evaluated by torch on the CPU once
    if log_space:
        return 2.0 ** torch.linspace(0.0, n_freqs - 1, n_freqs)
    return torch.linspace(2.0 ** 0.0, 2.0 ** (n_freqs - 1), n_freqs)


class PositionalEncoder(nn.Module):
    def __init__(self, d_input: int, n_freqs: int, log_space: bool = False):
        super().__init__()
        self.d_input, self.n_freqs, self.log_space = d_input, n_freqs, log_space
        self.d_output = d_input * (1 + 2 * n_freqs)
        self.freqs = [float(f) for f in _freqs(n_freqs, log_space)] if n_freqs > 0 else []

    def forward(self, x: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        return ops.posenc(x, self.freqs, mask)


class _NerfTrainFn(torch.autograd.Function):
    """NeRF.forward with gradients.  `fsn_nerf_train_fwd` runs the MFMA kernel of the inference
    path with the fp32 activations saved; `fsn_nerf_train_bwd` the dgrad chain + wgrad GEMMs on the matrix cores
    (csrc/train_fused.hip), in the model's precision mode.  Gradients flow to the parameters and - when they ask for
    them - to the inputs: sample positions and directions, or rays_o / rays_d in the ray form
    (`fsn_nerf_train_bwd_inputs`, csrc/input_grad.hip; a call whose inputs need none runs exactly the launches it ran
    before).  First order only (`once_differentiable`).  (The plain-fp32 library-GEMM formulation these kernels were
    first checked against lives entirely under tests/ref_fp32, binding included; nothing in this package can reach it.)"""

    @staticmethod
    def forward(ctx, model, packed, a, b, *params):
        """Point form: `packed` None, `a` / `b` = x / dirs [..., 3].  Ray form: `packed` = (ray_indices, t_starts,
        t_ends), `a` / `b` = rays_o / rays_d: the samples are the midpoints of the packed intervals, formed inside the
        launch (no gathered [N,3] tensors)."""
        n = len(params) // 2
        weights, biases = params[:n], params[n:]
        desc = model.desc
        ray_form = packed is not None
        dev = a.device
        prec = model.train_prec()
        # range-guard word of THIS call (one network, one step): the kernels of its forward and backward report into
        # it, and only they consult it - a flag raised by another network or by an inference launch must not zero
        # this network's gradients (the sticky per-device word of the inference path is not used here)
        word = torch.zeros(1, dtype=torch.int32, device=dev) if model.fp16_family(prec) else None
        pm, dm = model._mask(model.pos_mask, dev), model._mask(model.dir_mask, dev)
        if ray_form:
            out, work = ops.nerf_train_fwd_rays(desc, prec, weights, biases, a, b, *packed, pm, dm, status=word)
        else:
            out, work = ops.nerf_train_fwd(desc, prec, weights, biases, a, b, pm, dm, status=word)
        ctx.desc, ctx.prec, ctx.work, ctx.out, ctx.model, ctx.word = desc, prec, work, out, model, word
        ctx.weights = [w.detach() for w in weights]
        ctx.params = params  # (the leaf Parameters themselves: backward may accumulate into their .grad buffers)
        ctx.inputs = None
        need_a, need_b = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if need_a or need_b:  # the backward reads the inputs again
            # ray form: d rays_d = sum (m_i d_x_i + d_dirs_i), so EITHER ray tensor needs the per-sample position gradient
            ctx.inputs = {"pos_mask": pm, "dir_mask": dm, "want_x": need_a or (ray_form and need_b), "want_dirs": need_b}
            ctx.need = (need_a, need_b)
            if ray_form:
                ctx.inputs["rays"] = (a.detach(), b.detach(), *packed)
            else:
                ctx.inputs.update(x=a.detach(), dirs=b.detach())
            ctx.in_shapes = (a.shape, b.shape)
        return out if ray_form else out.reshape(*a.shape[:-1], 4)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        if ctx.work is None:
            raise RuntimeError("NeRF backward ran twice on one forward: the saved activations are released after the "
                               "first pass (retain_graph is not supported on this path)")
        # Gradient buffers owned by a flat bucket (shard.FlatGrads marks its parameters): the kernels ADD into p.grad on
        # the device - exactly what autograd's AccumulateGrad would do with returned tensors, minus 24 temporaries and 24
        # add launches per step - and autograd is handed None for them.  Anything else gets the gradients returned.
        n = len(ctx.params) // 2
        inputs = ctx.inputs
        # no parameter asks: a frozen network or a helper call (density_gradient) - the chain and the input gradient
        # only.  Such calls are no training steps: they keep per-stage factors and a range word of their own, so a
        # normals regulariser between two steps neither retunes the training backward's factors nor gates the optimizer.
        want_params = any(ctx.needs_input_grad[4:])
        sink = want_params and all(getattr(p, "_fsn_grad_sink", False) and p.requires_grad and p.grad is not None and p.grad.is_contiguous()
                   and p.grad.dtype == torch.float32 and p.grad.device == d_out.device for p in ctx.params)
        into = ([p.grad for p in ctx.params[:n]], [p.grad for p in ctx.params[n:]]) if sink else None
        model = ctx.model
        d_out = d_out.contiguous()
        kind = model.train_state.train if want_params else model.train_state.inputs
        stage = kind.stage_on(d_out.device, model.n_layers + 2) if model.fp16_family(ctx.prec) else None
        src = {} if inputs is None else {k: inputs[k] for k in ("x", "dirs", "rays", "pos_mask", "dir_mask") if k in inputs}
        if stage is not None and not kind.calibrated and d_out.shape[0] > 0:
            # first backward of this model in an fp16 mode: one throw-away pass to measure the per-stage gradient
            # magnitudes (delayed scaling needs a previous call; its own status word, scratch outputs).  A call without
            # samples - the all-background first batch of an empty occupancy grid - launches nothing and calibrates
            # nothing: the next one with samples does.
            scratch = torch.zeros_like(ctx.word) if ctx.word is not None else None
            if want_params:
                ops.nerf_train_bwd(ctx.desc, ctx.prec, ctx.weights, ctx.work, ctx.out, d_out, status=scratch, stage_state=stage)
            else:  # (the chain alone)
                ops.nerf_train_bwd_inputs(ctx.desc, ctx.prec, ctx.weights, ctx.work, ctx.out, d_out, **src, want_x=False,
                                          want_dirs=False, param_grads=False, status=scratch, stage_state=stage)
            kind.calibrated = True
        if inputs is None:
            dW, db = ops.nerf_train_bwd(ctx.desc, ctx.prec, ctx.weights, ctx.work, ctx.out, d_out, status=ctx.word,
                                        into=into, stage_state=stage)
            g_a = g_b = None
        else:
            dW, db, g_x, g_dirs = ops.nerf_train_bwd_inputs(ctx.desc, ctx.prec, ctx.weights, ctx.work, ctx.out, d_out, **src,
                                                            want_x=inputs["want_x"], want_dirs=inputs["want_dirs"],
                                                            param_grads=want_params, status=ctx.word, into=into,
                                                            stage_state=stage)
            if "rays" in inputs:  # per-sample gradients -> per-ray sums (one wave per ray, fixed order)
                o, _, ri, t0, t1 = inputs["rays"]
                g_a, g_b = ops.ray_grad_reduce(g_x, g_dirs, ri, t0, t1, o.shape[0], want_o=ctx.need[0], want_d=ctx.need[1])
            else:
                g_a, g_b = g_x, g_dirs
            g_a = None if g_a is None else g_a.reshape(ctx.in_shapes[0])
            g_b = None if g_b is None else g_b.reshape(ctx.in_shapes[1])
        ctx.work = None
        ctx.params = None
        ctx.inputs = None
        if ctx.word is not None:  # fp16 range guard without a per-step host sync
            model.train_state.after_backward(model, ctx.word, d_out.device, step=want_params)
        if sink or not want_params:
            return (None, None, g_a, g_b) + (None,) * (2 * n)
        db = [g.reshape(-1) for g in db]
        return (None, None, g_a, g_b, *dW, *db)


class NeRF(nn.Module):
    PRECISIONS = {"bf16x3": L.FSN_PREC_BF16X3, "bf16": L.FSN_PREC_BF16, "fp16x3": L.FSN_PREC_FP16X3,
                  "fp16": L.FSN_PREC_FP16, "fp16x2": L.FSN_PREC_FP16X2}
    FALLBACK = {"fp16x3": "bf16x3", "fp16x2": "bf16x3", "fp16": "bf16"}  # same pass structure, float32 range
    SINGLE_PASS = ("fp16", "bf16")  # modes of `packed_single`: cull_precision, autocast_precision, OccEvalFn

    def __init__(self, d_pos: int = 3, d_dir: int = 3, n_layers: int = 8, d_hidden: int = 256,
                 skip: Tuple[int, ...] = (4,), precision: str = "fp16x3", **kwargs) -> None:
        super().__init__()
        if d_pos != 3 or d_dir != 3:
            raise ValueError("the HIP path is built for 3-D positions and directions")
        self.d_pos, self.d_dir, self.n_layers, self.d_hidden = d_pos, d_dir, n_layers, d_hidden
        self.skip = tuple(skip)
        self.pos_encoder = PositionalEncoder(d_pos, kwargs["pos_fn"]["n_freqs"], kwargs["pos_fn"]["log_space"])
        self.dir_encoder = PositionalEncoder(d_dir, kwargs["dir_fn"]["n_freqs"], kwargs["dir_fn"]["log_space"])
        d_pe, d_de = self.pos_encoder.d_output, self.dir_encoder.d_output
        # construction order follows the reference (models.py:96-108) so that seeding
        # torch's RNG reproduces its initial parameters
        hidden = [nn.Linear(d_hidden + d_pe, d_hidden) if i in self.skip else nn.Linear(d_hidden, d_hidden)
                  for i in range(n_layers - 1)]
        self.layers = nn.ModuleList([nn.Linear(d_pe, d_hidden)] + hidden)
        self.sigma = nn.Linear(d_hidden, 1)
        self.connection = nn.Linear(d_hidden, d_hidden)
        self.branch = nn.Linear(d_hidden + d_de, d_hidden // 2)
        self.rgb = nn.Linear(d_hidden // 2, 3)
        self.precision = precision
        # fp16 modes: True = read the kernels' range flag back after each call (one host sync; a flagged call is re-run in
        # bf16x3 before it returns); "deferred" = asynchronous read-back, looked at by the NEXT call (batch rendering in
        # small launches: no wait per call; render_frame checks once per frame); False = never look
        self.range_check = True
        self.range_check_every = 16  # ... in training: every that many steps (gradients are guarded on the device)
        self._pack_calls = 0
        self.weight_check = True     # fp16 modes: look at the layers' largest weights when (re-)packing (_guard_weights)
        # accumulated range words, call counters and the backward's delayed per-stage gradient scaling (fp16 modes)
        self.train_state = TrainStatus()
        self.grad_overflow_looks = 0  # host looks that found a step skipped by the delayed gradient scaling
        self.train_precision: Optional[str] = None  # None: same mode as `precision`
        self.pos_mask: Optional[Tensor] = None
        self.dir_mask: Optional[Tensor] = None
        self._packed = PackCache()   # `packed`
        # OPT-IN, not a parity mode: arithmetic of the density pass behind the occupancy estimator's visibility cull when
        # it runs as the sampler in front of a training forward (None = the model's inference mode; "bf16" = one pass).
        # That pass only decides which marched samples are KEPT (transmittance >= early_stop_eps); the kept samples are
        # then evaluated, integrated and differentiated in the model's own mode.  See `packed_cull`.
        self.cull_precision: Optional[str] = None
        self._packed_single = {}  # mode -> PackCache: `packed_single`
        # OPT-IN, not a parity mode: this project's equivalent of running under autocast.  "fp16" / "bf16": a `forward`
        # made under torch.no_grad() AND inside an enabled CUDA autocast region (the reference's occupancy refresh,
        # run-nerf.py:288-295) runs in that single-pass mode, float32 tensor out.  None: autocast is ignored.  Training
        # forwards never look at it.  A flagged fp16 call is re-run in bf16 and the attribute stays "bf16" (RuntimeWarning).
        self.autocast_precision: Optional[str] = None
        # per-layer activation scaling of the fp16x3 inference path (module docstring)
        self.act_scaling = True
        self.act_target_exp = self.ACT_TARGET_EXP
        self.act_state = ActScaling()  # what `calibrate` measured, the target moves since
        self.calibrations = 0                   # statistics: calibration launches / range events (fall-backs and
        self.range_events = 0                   # re-calibrations) of this model

    # -- additions -----------------------------------------------------------------
    def set_freq_mask(self, pos_mask: Optional[Tensor], dir_mask: Optional[Tensor] = None) -> None:
        """Frequency mask multiplied onto the encoded features ([d_pos*(1+2n)], [d_dir*(1+2m)])."""
        self.pos_mask, self.dir_mask = pos_mask, dir_mask

    def train_prec(self) -> int:
        tp = self.train_precision or self.precision
        if tp == "fp16x2":
            tp = "fp16x3"  # the two-pass mode is inference only
        return self.PRECISIONS[tp]

    @staticmethod
    def fp16_family(prec: int) -> bool:
        return prec in (L.FSN_PREC_FP16X3, L.FSN_PREC_FP16, L.FSN_PREC_FP16X2)

    @property
    def fp16_mode(self) -> bool:
        """`precision` is one of the fp16 modes now (range-guarded; `fall_back` leaves them)."""
        return self.fp16_family(self.PRECISIONS[self.precision])

    @functools.cached_property
    def desc(self) -> L.MlpDesc:
        """Descriptor of every launch and blob (frequencies, depth, width and skips do not change after construction)."""
        return ops.make_desc(self.n_layers, self.d_hidden, self.skip, self.pos_encoder.freqs, self.dir_encoder.freqs)

    def fall_back(self, what: str, bits: int = L.FSN_STATUS_FP16_RANGE, probe=None, earlier_invalid: bool = False,
                  scaled: bool = True) -> None:
        """An fp16-mode launch reported values outside the mode's envelope; the caller re-runs the call afterwards.
        Scaled inference (`infer_prec() == FSN_PREC_FP16X3U`, and `scaled`: the report came from an inference launch):
        the calibration did not fit the data - re-calibrate on `probe` (`ActScaling.recalibrate`) and stay in fp16x3.  Otherwise,
        or when that does not help: continue in the bf16 mode of the same pass structure, which has float32's range,
        with a RuntimeWarning.  Never silent: `earlier_invalid` (deferred range checks) warns in the re-calibrated case
        too, because results already handed out were invalid."""
        self.range_events += 1
        if scaled and self.infer_prec() == L.FSN_PREC_FP16X3U and self.act_state.recalibrate(self, bits, probe):
            if earlier_invalid:
                warnings.warn(f"fs-nerf HIP path: {what}: the per-layer activation scales did not fit the data "
                              f"({ops.describe_flags(bits)}); re-calibrated", RuntimeWarning, stacklevel=3)
            return
        new = self.FALLBACK.get(self.precision, "bf16x3")
        warnings.warn(f"fs-nerf HIP path: {what}: hidden activations left the fp16 range envelope of precision "
                      f"'{self.precision}' ({ops.describe_flags(bits)}); re-running / continuing in '{new}'",
                      RuntimeWarning, stacklevel=3)
        self.precision = new
        if self.train_precision in self.FALLBACK:
            self.train_precision = None

    def _tensors(self):
        mods = list(self.layers) + [self.sigma, self.connection, self.branch, self.rgb]
        return [m.weight for m in mods], [m.bias for m in mods]

    # -- per-layer activation scaling (fp16x3 inference) ---------------------------------
    ACT_TARGET_EXP = 10  # a layer's largest probe activation is scaled into (2^9, 2^10]: 2^6 of headroom to 65504
    PROBE_MAX = 16384    # probe samples per calibration launch

    def infer_prec(self) -> int:
        """Arithmetic mode of the INFERENCE kernels (fsn_mlp_fwd, fsn_render_rays_fused, fsn_render_rays_occgrid)."""
        if self.precision == "fp16x3" and self.act_scaling:
            return L.FSN_PREC_FP16X3U
        return self.PRECISIONS[self.precision]

    def _param_key(self):
        ws, bs = self._tensors()
        return tuple((t.data_ptr(), t._version) for t in ws + bs)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.act_state.exps = None  # other weights: calibrate again on the next inference call
        self.act_state.forget_target_moves(self)
        return out

    def _default_probe(self, dev):
        g = torch.Generator(device="cpu").manual_seed(0)
        x = (torch.rand(4096, 3, generator=g) * 4.0 - 2.0).to(dev)
        d = torch.nn.functional.normalize(torch.randn(4096, 3, generator=g), dim=-1).to(dev)
        return x, d

    @torch.no_grad()
    def calibrate(self, probe=None, keep_if_close: bool = False) -> list:
        """Measure every layer's largest |activation| on a probe batch and choose the power-of-two scales of the
        fp16x3 inference path.  `probe`: (x [n,3], dirs [n,3]) tensors or a callable returning them - sample positions
        and directions like those the network is evaluated on (the call sites build them from their rays); None = a
        fixed default (uniform in [-2,2]^3, random unit directions).  One bf16x3 launch of the UNSCALED network on at
        most PROBE_MAX samples (`fsn_mlp_layer_maxima`) and one small read-back.  `keep_if_close`: an existing exponent
        is kept while it still puts the layer's maximum within [2^-3, 2^1] of the target (periodic re-calibration
        during training: no flapping between neighbouring powers of two).  -> the exponents."""
        ws, bs = self._tensors()
        dev = ws[0].device
        act = self.act_state
        if callable(probe):
            probe = probe()
        x, d = probe if probe is not None else self._default_probe(dev)
        x, d = x.reshape(-1, 3).to(dev, torch.float32), d.reshape(-1, 3).to(dev, torch.float32)
        if x.shape[0] == 0:
            x, d = self._default_probe(dev)
        if x.shape[0] > self.PROBE_MAX:
            idx = torch.linspace(0, x.shape[0] - 1, self.PROBE_MAX, device=dev).long()
            x, d = x[idx], d[idx]
        blob = act.blob.pack(self.desc, L.FSN_PREC_BF16X3, dev, None, ws, bs)  # (every probe launch packs afresh)
        maxima = ops.mlp_layer_maxima(blob, x.contiguous(), d.contiguous(), self._mask(self.pos_mask, dev),
                                      self._mask(self.dir_mask, dev))
        # largest |weight| per GEMM, activation columns and encoding columns separately (the scaled weights must stay
        # inside fp16 too): one stacked reduction, read back together with the maxima
        D, n = self.d_hidden, self.n_layers
        mods = list(self.layers) + [self.connection, self.branch]
        wmax = []
        for g, m in enumerate(mods):
            w = m.weight.detach().abs()
            na = 0 if g == 0 else D
            wmax.append(w[:, :na].amax() if na else w.new_zeros(()))
            wmax.append(w[:, na:].amax() if w.shape[1] > na else w.new_zeros(()))
        host = torch.cat([maxima, torch.stack(wmax).to(torch.float32)]).cpu().tolist()  # the one host sync
        act.exps = choose_exponents(host[:n + 2], host[n + 2:], int(self.act_target_exp), act.exps, keep_if_close, n)
        act.key = self._param_key()
        act.needs_calibration = False
        self.calibrations += 1
        return act.exps

    def _weights_below_envelope(self) -> bool:
        """fp16 modes: True when some layer's LARGEST weight is below 2^-20.  High parts under 2^-14 are fp16 subnormals
        and the scaled low parts resolve 2^-35: a layer whose largest weight is M keeps 2^-35 / M relative to it -
        2^-18 at the 6e-6 the envelope tests run (fine against the 1e-4 bar), 2^-15 at 2^-20, where this check draws the
        line.  (The kernels' low-end guard looks at activations; tiny weights under large activations would pass it.)
        One small reduction per layer and one 4-byte read-back: on the first pack and every `range_check_every`-th
        re-pack / training call."""
        mods = list(self.layers) + [self.connection, self.branch]  # (the sigma / rgb heads are float32 dot products)
        with torch.no_grad():
            m = torch.stack([mod.weight.detach().abs().amax() for mod in mods])
            return bool(((m > 0) & (m < 2.0 ** -20)).any())

    def _guard_weights(self, what: str, training: bool = False) -> None:
        # (scaled inference brings every layer's weights to the activations' scale: the check is about the unscaled
        # arithmetic of training and of `act_scaling = False`)
        if not training and self.infer_prec() == L.FSN_PREC_FP16X3U:
            return
        if self.range_check and self.weight_check and self.fp16_mode and self._weights_below_envelope():
            self.fall_back(what + " (a layer's largest weight is below 2^-20)", L.FSN_STATUS_FP16_SMALL, scaled=False)

    def packed(self, probe=None) -> ops.PackedMLP:
        """Weights in the MFMA streaming layout of the inference kernels; re-packed when any parameter changed.  Scaled
        fp16x3 inference: the first call (and the first one after `load_state_dict` or a request of the training
        loop's periodic look) calibrates the per-layer scales on `probe` (see `calibrate`) first."""
        ws, bs = self._tensors()
        act, dev, params = self.act_state, ws[0].device, self._param_key()
        if self.infer_prec() == L.FSN_PREC_FP16X3U and (act.exps is None or act.needs_calibration):
            self.calibrate(probe, keep_if_close=act.exps is not None)

        def mode():  # -> (exponents to pack with, key of the blob): the weight guard below may leave the fp16 modes
            exps = tuple(act.exps) if self.infer_prec() == L.FSN_PREC_FP16X3U else None
            return exps, (self.precision, dev, exps) + params

        exps, key = mode()
        if self._packed.stale(key):
            if self._pack_calls % max(1, int(self.range_check_every)) == 0:
                self._guard_weights("NeRF.packed")
                exps, key = mode()
            self._pack_calls += 1
            self._packed.pack(self.desc, self.infer_prec(), dev, key, ws, bs, exps)
        return self._packed.pm

    def packed_single(self, precision: str) -> ops.PackedMLP:
        """The weights packed for the single-pass mode `precision` ("fp16" / "bf16": no calibration), one cached blob
        per mode beside the model's own (`packed`), re-packed when a parameter changed."""
        if precision not in self.SINGLE_PASS:
            raise ValueError(f"single-pass precision: one of {self.SINGLE_PASS}, not {precision!r}")
        ws, bs = self._tensors()
        key = (ws[0].device,) + self._param_key()
        cache = self._packed_single.setdefault(precision, PackCache())
        if cache.stale(key):
            cache.pack(self.desc, self.PRECISIONS[precision], ws[0].device, key, ws, bs)
        return cache.pm

    def packed_cull(self) -> ops.PackedMLP:
        """The weights packed for the mode `cull_precision` names (single-pass bf16: float32's range, no calibration and
        no range flags), re-packed when a parameter changed."""
        if self.cull_precision != "bf16":
            raise ValueError("NeRF.cull_precision: None or 'bf16'")
        return self.packed_single(self.cull_precision)

    def occ_eval_fn(self, render_step_size: float, precision: str = "fp16") -> "OccEvalFn":
        """`occ_eval_fn` for `update_every_n_steps`: x -> self(x) * render_step_size in the single-pass mode `precision`
        (what the reference's closure computes under its autocast).  `OccGridEstimator` recognises the object and runs
        the whole refresh in one launch; any other estimator just calls it.  See `OccEvalFn`."""
        return OccEvalFn(self, render_step_size, precision)

    def _autocast_mode(self) -> Optional[str]:
        """The single-pass mode this inference forward runs in on account of `autocast_precision`, or None."""
        ap = self.autocast_precision
        if ap is None:
            return None
        if ap not in self.SINGLE_PASS:
            raise ValueError(f"NeRF.autocast_precision: None or one of {self.SINGLE_PASS}, not {ap!r}")
        return ap if not torch.is_grad_enabled() and torch.is_autocast_enabled("cuda") else None

    def _leave_fp16_autocast(self, what: str, bits: int) -> str:
        self.autocast_precision = "bf16"
        return _warn_single_pass(self, what, bits)

    def _mask(self, m: Optional[Tensor], dev) -> Optional[Tensor]:
        return None if m is None else m.to(dev, torch.float32)

    def forward_rays(self, rays_o: Tensor, rays_d: Tensor, ray_indices: Tensor, t_starts: Tensor, t_ends: Tensor,
                     full: bool = True) -> Tensor:
        """`self(x, d)` (full) or `self(x)` (density only) on the midpoints of packed intervals - what the reference's
        closures compute as `to = rays_o[ri]; td = rays_d[ri]; x = to + td * (t0 + t1)[:, None] / 2; model(x, td)`
        (rendering.py:58-64, 76-84) - with the gathers and the midpoint arithmetic inside the launch: no [N,3] tensor
        is materialised.  Same values bit for bit; gradients (full pass) flow to the parameters of a model in training
        mode and to `rays_o` / `rays_d` when they require grad (any mode; none to the interval edges)."""
        if full and self._differentiable(rays_o, rays_d):
            ws, bs = self._tensors()
            return _NerfTrainFn.apply(self, (ray_indices, t_starts, t_ends), rays_o, rays_d, *ws, *bs)
        dev = rays_o.device
        args = (rays_o, rays_d, ray_indices, t_starts, t_ends, full, self._mask(self.pos_mask, dev), self._mask(self.dir_mask, dev))

        def probe():
            n = ray_indices.numel()
            idx = torch.linspace(0, max(n - 1, 0), min(n, self.PROBE_MAX), device=dev).long()
            ri = ray_indices[idx].long()
            d = rays_d[ri]
            return rays_o[ri] + d * (t_starts[idx] + t_ends[idx])[:, None] / 2.0, d

        return guarded_launch([self], dev, "NeRF.forward_rays", probe, lambda: ops.mlp_fwd_rays(self.packed(probe), *args))

    # -- reference surface ---------------------------------------------------------
    def _differentiable(self, *inputs: Optional[Tensor]) -> bool:
        """This call runs the training pair (`_NerfTrainFn`): grad is enabled and either the model trains with
        parameters that require grad, or one of the inputs requires grad (training or eval mode)."""
        if not torch.is_grad_enabled():
            return False
        if self.training and any(p.requires_grad for p in self.parameters()):
            return True
        return any(t is not None and t.requires_grad for t in inputs)

    def density_gradient(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        """-> (sigma [N], d sigma / d x [N,3]) at positions x [N,3]: one full pass with the cotangent (0, 0, 0, 1) and a
        fixed direction (sigma does not depend on it), the network treated as frozen - no parameter gradient is computed
        or touched.  Surface normals are `-F.normalize(grad, dim=-1)`."""
        xg = x.detach().reshape(-1, 3).to(torch.float32).contiguous().requires_grad_(True)
        dirs = torch.tensor([0.0, 0.0, 1.0], device=xg.device).expand(xg.shape[0], 3).contiguous()
        ws, bs = self._tensors()
        with torch.enable_grad():
            out = _NerfTrainFn.apply(self, None, xg, dirs, *[t.detach() for t in ws + bs])
            cot = torch.zeros_like(out)
            cot[:, 3] = 1.0
            (grad,) = torch.autograd.grad(out, xg, cot)
        return out[:, 3].detach(), grad

    def forward(self, x: Tensor, dirs: Optional[Tensor] = None) -> Tensor:
        if self._differentiable(x, dirs):
            if dirs is None:
                if not self._differentiable():  # (only x asks: as before, the density-only pass carries no graph)
                    return self._forward_inference(x, dirs)
                raise NotImplementedError(
                    "NeRF.forward(x) with gradients: the density-only pass has no backward (the reference runs it "
                    "under torch.no_grad(), rendering.py:58-64); call it under torch.no_grad() (density_gradient(x) gives "
                    "sigma and its gradient with respect to x)")
            ws, bs = self._tensors()
            return _NerfTrainFn.apply(self, None, x, dirs, *ws, *bs)
        return self._forward_inference(x, dirs)

    def _forward_inference(self, x: Tensor, dirs: Optional[Tensor]) -> Tensor:
        dev = x.device
        mode = self._autocast_mode()
        if mode is not None:
            return single_pass_launch(self, mode, dev, "NeRF.forward (autocast_precision)", self._leave_fp16_autocast,
                                      lambda pm: ops.mlp_fwd(pm, x, dirs, self._mask(self.pos_mask, dev),
                                                             self._mask(self.dir_mask, dev)))

        def probe():
            xs = x.reshape(-1, 3)
            if dirs is not None:
                return xs, dirs.reshape(-1, 3)
            return xs, torch.tensor([0.0, 0.0, 1.0], device=dev).expand_as(xs)  # (density only: any direction)

        return guarded_launch([self], dev, "NeRF.forward", probe,
                              lambda: ops.mlp_fwd(self.packed(probe), x, dirs, self._mask(self.pos_mask, dev),
                                                  self._mask(self.dir_mask, dev)))


class OccEvalFn:
    """`NeRF.occ_eval_fn(render_step_size, precision)`: the callable for the `occ_eval_fn` slot of
    `update_every_n_steps` (run-nerf.py:288-295).  Called with points it returns `model(x) * render_step_size`, the density
    pass evaluated in the single-pass mode `precision` through `fsn_mlp_fwd` - this project's equivalent of the
    autocast region the reference wraps that call in, not a bit-for-bit copy of it.  `OccGridEstimator`
    does not call it: it reads `model`, `render_step_size` and `precision` and runs selection, density pass and maximum
    of all levels in one launch (`ops.occgrid_refresh`), with the same values bit for bit.  `precision` becomes "bf16"
    for good after an fp16 call that left the range envelope (RuntimeWarning; the flagged call is repeated)."""

    def __init__(self, model: NeRF, render_step_size: float, precision: str = "fp16") -> None:
        if precision not in NeRF.SINGLE_PASS:
            raise ValueError(f"OccEvalFn: precision is one of {NeRF.SINGLE_PASS}, not {precision!r}")
        self.model, self.render_step_size, self.precision = model, float(render_step_size), precision

    def _leave_fp16(self, what: str, bits: int) -> str:
        self.precision = "bf16"
        return _warn_single_pass(self.model, what, bits)

    def guarded(self, dev, what: str, launch, undo=None):
        """`launch(packed blob)` in this object's mode under the range guard (`single_pass_launch`)."""
        return single_pass_launch(self.model, self.precision, dev, what, self._leave_fp16, launch, undo)

    @torch.no_grad()
    def __call__(self, x: Tensor) -> Tensor:
        m, dev = self.model, x.device
        return self.guarded(dev, "OccEvalFn", lambda pm: ops.mlp_fwd(pm, x, None, m._mask(m.pos_mask, dev))) * self.render_step_size
